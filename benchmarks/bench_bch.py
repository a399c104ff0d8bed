#!/usr/bin/env python3
"""BCH encoder / decoder throughput (csrc/bch.hip): device-resident inputs, HIP-event timing on the launch stream after a warm-up that
covers the clock ramp, one JSON line per case, also written to profiles/bch_bench.jsonl.
    python benchmarks/bench_bch.py [--scale 1.0] [--steps 5] [--no-context]
Codes: (255, 239, t = 2), (1023, 923, t = 10) and the DVB-S2 short-frame code (3240, 3072, t = 12 over GF(2^14), prim_poly 16427).
Per code: the encoder, and the decoder ('bits' only) with exactly 0, ceil(t / 2), t and 2t errors per word at random positions -- the
decoder's time depends on the error count (a clean word leaves after the syndromes; 2t errors are mostly failures).  B is chosen so that
a launch moves n + k bytes per word, at least 1 GB in all (scale 1).  `frac_copy` is against the 6.29 TB/s of a streaming copy.  After
the timed region a sample of the timed output is compared with tests/bch_model.py (exactly).  For context the same run times the polar
SC decoder (1024, 512 + CRC-11) and the 802.11n (1944, 1296) LDPC min-sum decoder as benchmarks/bench_polar.py does."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bch_model as M  # noqa: E402
from commpy_amd import _lib  # noqa: E402
from commpy_amd.channelcoding import BCHCode  # noqa: E402
from benchmarks.bench_kernels import timeit  # noqa: E402
from benchmarks.other_configs import DESIGN_1944, Dev  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "bch_bench.jsonl")
COPY_CEILING = 6290.0   # GB/s, a measured streaming copy
CODES = ((255, 2, 8, None), (1023, 10, 10, None), (3240, 12, 14, 16427))


def emit(d, fh):
    d["build_id"] = _lib.build_id().get("full")
    line = json.dumps(d)
    print(line, flush=True)
    fh.write(line + "\n")


def sample(B, n=2):
    return sorted(set(list(range(min(n, B))) + list(range(B // 2, min(B // 2 + n, B))) + list(range(max(B - n, 0), B))))


def flip(words, e, rs):
    """words [B, n] with exactly e distinct random positions of every row flipped, in place."""
    B, n = words.shape
    if e == 0:
        return
    pos = rs.randint(0, n, (B, e))
    while True:
        srt = np.sort(pos, axis=1)
        again = np.flatnonzero((srt[:, 1:] == srt[:, :-1]).any(axis=1))
        if not len(again):
            break
        pos[again] = rs.randint(0, n, (len(again), e))
    words[np.arange(B)[:, None], pos] ^= 1


def line(kname, what, B, code, ms, ms_min, exact, words):
    gbs = B * (code.n + code.k) / (ms * 1e-3) / 1e9
    return {"kernel": kname, "workload": what, "B": B, "ms": ms, "ms_min": ms_min, "words_per_s": B / (ms * 1e-3),
            "value": B * code.k / (ms * 1e-3), "unit": "info-bits/s", "GB_per_s": gbs, "frac_copy": gbs / COPY_CEILING,
            "bytes_per_launch": B * (code.n + code.k), "dtype": "u8", "parity": {"vs": "tests/bch_model.py", "words": words, "ok": exact},
            "bound": "unmeasured (no counter pass)"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-context", action="store_true", help="skip the polar and LDPC lines")
    args = ap.parse_args()
    lib = _lib.load()
    _lib.require_device()
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    rs = np.random.RandomState(0)
    with open(OUT, "w") as fh:
        for n, t, m, prim in CODES:
            code, model = BCHCode(n, t, m=m, prim_poly=prim), M.Code(n, t, m, prim)
            B = max(int(args.scale * 1.0e9 / (code.n + code.k)) + 1, 64)
            name = "(%d, %d, t=%d)" % (code.n, code.k, t)
            msg = rs.randint(0, 2, (B, code.k), dtype=np.uint8)
            h = code._device_handle()
            dev = Dev(lib)
            try:
                d_msg, d_x, d_bits = dev.put(msg), dev.empty(B * code.n), dev.empty(B * code.k)
                ms, ms_min = timeit(lib, lambda: _lib.check(lib.cpx_bch_encode_dev(h, d_msg, B, d_x, None)), steps=args.steps,
                                    warmup=args.warmup)
                kname = _lib.last_kernel()
                _lib.check(lib.cpx_stream_sync(None))
                sent = dev.get(d_x, (B, code.n), np.uint8)
                idx = sample(B, 4)
                exact = bool(np.array_equal(sent[idx], M.encode_batch(msg[idx], model)))
                emit(line(kname, "bch_encode %s B=%d" % (name, B), B, code, ms, ms_min, exact, len(idx)), fh)
                assert exact, "bch_encode differs from the model"
                for e in (0, (t + 1) // 2, t, 2 * t):
                    rx = sent.copy()
                    flip(rx, e, rs)
                    _lib.check(lib.cpx_memcpy_h2d(d_x, _lib.ptr(rx), rx.nbytes))
                    ms, ms_min = timeit(lib, lambda: _lib.check(lib.cpx_bch_decode_dev(h, d_x, B, d_bits, None, None, None)), steps=args.steps,
                                        warmup=args.warmup)
                    kname = _lib.last_kernel()
                    _lib.check(lib.cpx_stream_sync(None))
                    bits = dev.get(d_bits, (B, code.k), np.uint8)
                    idx = sample(B, 4)
                    exact = bool(np.array_equal(bits[idx], M.decode_batch(rx[idx], model)["bits"]))
                    d = line(kname, "bch_decode %s, %d errors per word, B=%d" % (name, e, B), B, code, ms, ms_min, exact, len(idx))
                    d["errors_per_word"] = e
                    d["words_equal_to_sent"] = float(np.mean((bits == msg).all(axis=1)))
                    emit(d, fh)
                    assert exact, "bch_decode differs from the model"
                    del rx, bits
            finally:
                dev.free()
            del msg, sent
        if args.no_context:
            return
        # context: the polar SC decoder and the LDPC min-sum decoder, timed by the same run as benchmarks/bench_polar.py times them
        from commpy_amd.channelcoding import PolarCode, polar_encode
        N, K, B = 1024, 523, max(int(16384 * args.scale), 8)
        pcode = PolarCode(N, K, crc=0xE21)
        pmsg = rs.randint(0, 2, (B, pcode.A)).astype(np.uint8)
        sigma2 = 1.0 / (2.0 * (pcode.A / N) * 10.0 ** 0.3)
        llr = 2.0 * (1.0 - 2.0 * polar_encode(pmsg, pcode) + np.sqrt(sigma2) * rs.randn(B, N)) / sigma2
        dev = Dev(lib)
        try:
            d_llr, d_bits, d_ok = dev.put(llr), dev.empty(B * pcode.A), dev.empty(B)
            h = pcode._device_handle()
            ms, ms_min = timeit(lib, lambda: _lib.check(lib.cpx_polar_decode_dev(h, d_llr, B, 1, d_bits, d_ok, None, None, None, None, None, None)),
                                steps=args.steps, warmup=args.warmup)
            emit({"kernel": _lib.last_kernel(), "workload": "context: polar SC (1024, %d + CRC-11), Eb/N0=3 dB, B=%d" % (pcode.A, B), "B": B,
                  "ms": ms, "ms_min": ms_min, "value": B * pcode.A / (ms * 1e-3), "unit": "info-bits/s"}, fh)
        finally:
            dev.free()
        from commpy_amd.channelcoding.ldpc import _device_code, get_ldpc_code_params
        p = get_ldpc_code_params(DESIGN_1944, True)
        n, B = 1944, max(int(8192 * args.scale), 64)
        sigma = 1 / np.sqrt(10 ** 0.3 * (2.0 / 3) * 2)
        llr = 2.0 * (1.0 + sigma * rs.randn(B, n)) / sigma ** 2
        dev = Dev(lib)
        try:
            d_llr, d_dec, d_out, d_it = dev.put(llr), dev.empty(B * n), dev.empty(B * n * 8), dev.empty(B * 4)
            h = _device_code(p)
            ms, ms_min = timeit(lib, lambda: _lib.check(lib.cpx_ldpc_bp_decode_batch_bm_dev(h, d_llr, B, 1, 50, d_dec, d_out, d_it, None)),
                                steps=args.steps, warmup=args.warmup)
            emit({"kernel": _lib.last_kernel(), "workload": "context: LDPC 802.11n (1944, 1296) min-sum, <= 50 iterations, Eb/N0=3 dB, B=%d" % B,
                  "B": B, "ms": ms, "ms_min": ms_min, "value": B * 1296 / (ms * 1e-3), "unit": "info-bits/s"}, fh)
        finally:
            dev.free()


if __name__ == "__main__":
    main()
