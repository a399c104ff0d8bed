#!/usr/bin/env python3
"""Reed-Solomon encoder / decoder throughput (csrc/rs.hip): device-resident inputs, HIP-event timing on the launch stream after a warm-up
that covers the clock ramp, one JSON line per case, also written to profiles/rs_bench.jsonl.
    python benchmarks/bench_rs.py [--scale 1.0] [--steps 5] [--no-context]
Codes: (255, 223), (204, 188) shortened with fcr = 0, and (544, 514) over GF(2^10).  Per code: the encoder, and the decoder ('symbols'
only) with e = 0, t / 2 and t errors per word at random positions, with f = r erasures and no error (every flagged symbol replaced by
a random one), and with e = t + 1 errors (failures) -- the decoder's time depends on the case (a clean word leaves after the syndromes).
B is chosen so that a launch moves n + k symbols of 2 bytes per word, at least 1 GB in all (scale 1); the flags of the erasure case
(n bytes per word) are not counted.  `frac_copy` is against the 6.29 TB/s of a streaming copy.  After the timed region a sample of the
timed output is compared with tests/rs_model.py (exactly).  For context the same run times bch_decode on (255, 239, t = 2) as
benchmarks/bench_bch.py does."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bch_model  # noqa: E402
import rs_model as M  # noqa: E402
from commpy_amd import _lib  # noqa: E402
from commpy_amd.channelcoding import BCHCode, RSCode  # noqa: E402
from benchmarks.bench_bch import flip, sample  # noqa: E402
from benchmarks.bench_kernels import timeit  # noqa: E402
from benchmarks.other_configs import Dev  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "rs_bench.jsonl")
COPY_CEILING = 6290.0   # GB/s, a measured streaming copy
CODES = ((255, 223, 8, 1), (204, 188, 8, 0), (544, 514, 10, 1))


def emit(d, fh):
    d["build_id"] = _lib.build_id().get("full")
    line = json.dumps(d)
    print(line, flush=True)
    fh.write(line + "\n")


def positions(B, n, count, rs):
    """[B, count] distinct random positions per row."""
    pos = rs.randint(0, n, (B, count))
    while count > 1:
        srt = np.sort(pos, axis=1)
        again = np.flatnonzero((srt[:, 1:] == srt[:, :-1]).any(axis=1))
        if not len(again):
            break
        pos[again] = rs.randint(0, n, (len(again), count))
    return pos


def line(kname, what, B, code, ms, ms_min, exact, words):
    nbytes = 2 * B * (code.n + code.k)
    gbs = nbytes / (ms * 1e-3) / 1e9
    return {"kernel": kname, "workload": what, "B": B, "ms": ms, "ms_min": ms_min, "words_per_s": B / (ms * 1e-3),
            "value": B * code.k * code.m / (ms * 1e-3), "unit": "info-bits/s", "GB_per_s": gbs, "frac_copy": gbs / COPY_CEILING,
            "bytes_per_launch": nbytes, "dtype": "u16", "parity": {"vs": "tests/rs_model.py", "words": words, "ok": exact},
            "bound": "unmeasured (no counter pass)"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-context", action="store_true", help="skip the BCH lines")
    args = ap.parse_args()
    lib = _lib.load()
    _lib.require_device()
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    rs = np.random.RandomState(0)
    with open(OUT, "w") as fh:
        for n, k, m, fcr in CODES:
            code, model = RSCode(n, k, m=m, fcr=fcr), M.Code(n, k, m, fcr=fcr)
            r, t = n - k, (n - k) // 2
            B = max(int(args.scale * 1.0e9 / (2 * (n + k))) + 1, 64)
            name = "(%d, %d) over GF(2^%d), fcr=%d" % (n, k, m, fcr)
            msg = rs.randint(0, 1 << m, (B, k)).astype(np.uint16)
            h = code._device_handle()
            dev = Dev(lib)
            try:
                d_msg, d_x, d_fl, d_sym = dev.put(msg), dev.empty(2 * B * n), dev.empty(B * n), dev.empty(2 * B * k)
                ms, ms_min = timeit(lib, lambda: _lib.check(lib.cpx_rs_encode_dev(h, d_msg, B, d_x, None)), steps=args.steps,
                                    warmup=args.warmup)
                kname = _lib.last_kernel()
                _lib.check(lib.cpx_stream_sync(None))
                sent = dev.get(d_x, (B, n), np.uint16)
                idx = sample(B, 4)
                exact = bool(np.array_equal(sent[idx], M.encode_batch(msg[idx], model)))
                emit(line(kname, "rs_encode %s B=%d" % (name, B), B, code, ms, ms_min, exact, len(idx)), fh)
                assert exact, "rs_encode differs from the model"
                rows = np.arange(B)[:, None]
                for what, e, f in (("e=0", 0, 0), ("e=t/2", t // 2, 0), ("e=t", t, 0), ("f=r", 0, r), ("e=t+1", t + 1, 0)):
                    rx = sent.copy()
                    flags = None
                    if e:
                        rx[rows, positions(B, n, e, rs)] ^= rs.randint(1, 1 << m, (B, e)).astype(np.uint16)
                    if f:
                        pos = positions(B, n, f, rs)
                        flags = np.zeros((B, n), np.uint8)
                        flags[rows, pos] = 1
                        rx[rows, pos] = rs.randint(0, 1 << m, (B, f)).astype(np.uint16)
                        _lib.check(lib.cpx_memcpy_h2d(d_fl, _lib.ptr(flags), flags.nbytes))
                    _lib.check(lib.cpx_memcpy_h2d(d_x, _lib.ptr(rx), rx.nbytes))
                    d_er = d_fl if f else None
                    ms, ms_min = timeit(lib, lambda: _lib.check(lib.cpx_rs_decode_dev(h, d_x, d_er, B, d_sym, None, None, None)),
                                        steps=args.steps, warmup=args.warmup)
                    kname = _lib.last_kernel()
                    _lib.check(lib.cpx_stream_sync(None))
                    sym = dev.get(d_sym, (B, k), np.uint16)
                    idx = sample(B, 4)
                    exact = bool(np.array_equal(sym[idx], M.decode_batch(rx[idx], model, None if flags is None else flags[idx])["symbols"]))
                    d = line(kname, "rs_decode %s, %s (%d errors, %d erasures per word), B=%d" % (name, what, e, f, B), B, code, ms, ms_min,
                             exact, len(idx))
                    d.update({"case": what, "errors_per_word": e, "erasures_per_word": f,
                              "words_equal_to_sent": float(np.mean((sym == msg).all(axis=1)))})
                    emit(d, fh)
                    assert exact, "rs_decode differs from the model"
                    del rx, sym, flags
            finally:
                dev.free()
            del msg, sent
        if args.no_context:
            return
        # context: the BCH decoder of the parent commit on (255, 239, t = 2), as benchmarks/bench_bch.py times it
        bcode, bmodel = BCHCode(255, 2, m=8), bch_model.Code(255, 2, 8)
        B = max(int(args.scale * 1.0e9 / (bcode.n + bcode.k)) + 1, 64)
        sent = np.resize(bch_model.encode_batch(rs.randint(0, 2, (4096, bcode.k)), bmodel), (B, bcode.n))
        dev = Dev(lib)
        try:
            d_x, d_bits = dev.empty(B * bcode.n), dev.empty(B * bcode.k)
            h = bcode._device_handle()
            for e in (0, 2):
                rx = sent.copy()
                flip(rx, e, rs)
                _lib.check(lib.cpx_memcpy_h2d(d_x, _lib.ptr(rx), rx.nbytes))
                ms, ms_min = timeit(lib, lambda: _lib.check(lib.cpx_bch_decode_dev(h, d_x, B, d_bits, None, None, None)), steps=args.steps,
                                    warmup=args.warmup)
                emit({"kernel": _lib.last_kernel(), "workload": "context: bch_decode (255, 239, t=2), %d errors per word, B=%d" % (e, B), "B": B,
                      "ms": ms, "ms_min": ms_min, "words_per_s": B / (ms * 1e-3), "value": B * bcode.k / (ms * 1e-3), "unit": "info-bits/s",
                      "GB_per_s": B * (bcode.n + bcode.k) / (ms * 1e-3) / 1e9, "dtype": "u8"}, fh)
                del rx
        finally:
            dev.free()


if __name__ == "__main__":
    main()
