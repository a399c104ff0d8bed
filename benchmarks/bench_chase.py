#!/usr/bin/env python3
"""Chase-II BCH decoding and turbo-product-code throughput (csrc/bch_chase.hip): device-resident inputs, HIP-event timing on the launch
stream after a warm-up that covers the clock ramp, one JSON line per case, also written to profiles/chase_bench.jsonl.
    python benchmarks/bench_chase.py [--scale 1.0] [--steps 5]
chase_decode ('bits' and 'extrinsic'): (255, 239, t = 2) at p = 4 and 6, (1023, 923, t = 10) and the DVB-S2 short-frame code
(3240, 3072, t = 12) at p = 4; 1 GB of LLRs per launch (scale 1), code words over BPSK and AWGN at the noise level where a word holds t
hard errors on average.  The same run times bch_decode ('bits') on the same hard decisions and on words with exactly t errors; the
figure of merit is `ratio_per_pattern` = (chase time per word and test pattern) / (bch_decode time per word at t errors): a test
pattern's syndromes are incremental, so it should not cost more than a whole hard decode (house rule: <= 1.25).
tpc_decode: (63, 57)^2 and (127, 113)^2, four iterations (eight launches), p = 4, with the bit and block error rates beside those of
one hard-decision pass of bch_decode over the rows, then the columns.  `frac_copy` is against the 6.29 TB/s of a streaming copy.  After
the timed region a sample of the output is compared with the NumPy models (exactly)."""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bch_model as M  # noqa: E402
import chase_model as CM  # noqa: E402
import tpc_model as TM  # noqa: E402
from commpy_amd import _lib  # noqa: E402
from commpy_amd.channelcoding import BCHCode, ProductCode, bch_decode, bch_encode, tpc_encode  # noqa: E402
from commpy_amd.channelcoding.productcode import ALPHA, BETA  # noqa: E402
from benchmarks.bench_bch import COPY_CEILING, flip, sample  # noqa: E402
from benchmarks.bench_kernels import timeit  # noqa: E402
from benchmarks.other_configs import Dev  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "chase_bench.jsonl")
CHASE = ((255, 2, 8, None, 4), (255, 2, 8, None, 6), (1023, 10, 10, None, 4), (3240, 12, 14, 16427, 4))
TPC = ((63, 1, 6, 4.0), (127, 2, 7, 3.5))                         # (n, t, m) of both components, Eb/N0 in dB
BOUND = "unmeasured (no counter pass)"


def emit(d, fh):
    d["build_id"] = _lib.build_id().get("full")
    line = json.dumps(d)
    print(line, flush=True)
    fh.write(line + "\n")


def sigma_for(rate):
    """The noise deviation at which a BPSK hard decision is wrong with probability `rate` (Q(1 / sigma) = rate), by bisection."""
    lo, hi = 0.05, 5.0
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if 0.5 * math.erfc(1.0 / (mid * math.sqrt(2.0))) < rate else (lo, mid)
    return lo


def chase_case(lib, fh, rs, n, t, m, prim, p, args):
    code, model = BCHCode(n, t, m=m, prim_poly=prim), M.Code(n, t, m, prim)
    B = max(int(args.scale * 1.0e9 / (8 * n)) + 1, 64)
    name = "(%d, %d, t=%d)" % (n, code.k, t)
    sigma = sigma_for(t / n)
    msg = rs.randint(0, 2, (B, code.k), dtype=np.uint8)
    sent = bch_encode(msg, code)
    llr = (2.0 / sigma ** 2) * (1.0 - 2.0 * sent + sigma * rs.standard_normal((B, n)))
    hard = (llr < 0).astype(np.uint8)
    h = code._device_handle()
    dev = Dev(lib)
    try:
        d_llr, d_bits, d_ext, d_hard = dev.put(llr), dev.empty(B * code.k), dev.empty(8 * B * n), dev.put(hard)
        ms, ms_min = timeit(lib, lambda: _lib.check(lib.cpx_chase_bch_dev(h, d_llr, None, 1.0, 2.0 / sigma ** 2, p, B, 1, n, 0, 1, d_bits, None, d_ext,
                                                                          None, None, None)), steps=args.steps, warmup=args.warmup)
        kname = _lib.last_kernel()
        _lib.check(lib.cpx_stream_sync(None))
        bits, ext = dev.get(d_bits, (B, code.k), np.uint8), dev.get(d_ext, (B, n), np.float64)
        idx = sample(B, 2)
        ref = CM.decode_batch(llr[idx], model, p, 2.0 / sigma ** 2)
        exact = bool(np.array_equal(bits[idx], ref["bits"]) and np.array_equal(ext[idx].view(np.int64), ref["extrinsic"].view(np.int64)))
        chase_wer = float(np.mean((bits != msg).any(axis=1)))
        del ext
        # bch_decode on the same hard decisions, then on words with exactly t errors
        hard_ms, _ = timeit(lib, lambda: _lib.check(lib.cpx_bch_decode_dev(h, d_hard, B, d_bits, None, None, None)), steps=args.steps, warmup=args.warmup)
        _lib.check(lib.cpx_stream_sync(None))
        hard_wer = float(np.mean((dev.get(d_bits, (B, code.k), np.uint8) != msg).any(axis=1)))
        rx = sent.copy()
        flip(rx, t, rs)
        _lib.check(lib.cpx_memcpy_h2d(d_hard, _lib.ptr(rx), rx.nbytes))
        t_ms, _ = timeit(lib, lambda: _lib.check(lib.cpx_bch_decode_dev(h, d_hard, B, d_bits, None, None, None)), steps=args.steps, warmup=args.warmup)
        _lib.check(lib.cpx_stream_sync(None))
        nbytes = B * (16 * n + code.k)
        gbs = nbytes / (ms * 1e-3) / 1e9
        emit({"kernel": kname, "workload": "chase_decode %s p=%d, bits + extrinsic, %.2f hard errors per word, B=%d" % (name, p, (hard != sent).sum() / B, B),
              "B": B, "p": p, "ms": ms, "ms_min": ms_min, "words_per_s": B / (ms * 1e-3), "value": B * code.k / (ms * 1e-3), "unit": "info-bits/s",
              "GB_per_s": gbs, "frac_copy": gbs / COPY_CEILING, "bytes_per_launch": nbytes, "dtype": "f64",
              "ns_per_word_and_pattern": ms * 1e6 / (B * (1 << p)), "bch_decode_ns_per_word_at_t_errors": t_ms * 1e6 / B,
              "bch_decode_ns_per_word_same_hard_decisions": hard_ms * 1e6 / B, "ratio_per_pattern": (ms / (1 << p)) / t_ms,
              "ratio_rule": 1.25, "word_error_rate": chase_wer, "word_error_rate_bch_decode": hard_wer,
              "parity": {"vs": "tests/chase_model.py", "words": len(idx), "ok": exact}, "bound": BOUND}, fh)
        assert exact, "chase_decode differs from the model"
    finally:
        dev.free()


def tpc_case(lib, fh, rs, n, t, m, ebn0_db, args, iters=4, p=4):
    comp, model = BCHCode(n, t, m=m), M.Code(n, t, m)
    code = ProductCode(comp, comp)
    B = max(int(args.scale * 1.0e9 / (8 * code.n)) + 1, 4)
    sigma = math.sqrt(1.0 / (2.0 * (code.k / code.n) * 10.0 ** (ebn0_db / 10.0)))
    scale = 2.0 / sigma ** 2
    msg = rs.randint(0, 2, (B, code.k_c, code.k_r), dtype=np.uint8)
    sent = tpc_encode(msg, code)
    llr = scale * (1.0 - 2.0 * sent + sigma * rs.standard_normal(sent.shape))
    del sent
    h = comp._device_handle()
    dev = Dev(lib)
    try:
        d_llr, d_w, d_word = dev.put(llr), dev.empty(8 * B * code.n), dev.empty(B * code.n)

        def decode():
            _lib.check(lib.cpx_memset(d_w, 0, 8 * B * code.n))
            for hi in range(2 * iters):
                J, sj, si = (n, n, 1) if hi % 2 == 0 else (n, 1, n)
                _lib.check(lib.cpx_chase_bch_dev(h, d_llr, d_w, ALPHA[min(hi, 7)], scale * BETA[min(hi, 7)], p, B, J, n * n, sj, si, None,
                                                 d_word if hi == 2 * iters - 1 else None, d_w, None, None, None))

        ms, ms_min = timeit(lib, decode, steps=args.steps, warmup=args.warmup)
        kname = _lib.last_kernel()
        _lib.check(lib.cpx_stream_sync(None))
        word = dev.get(d_word, (B, n, n), np.uint8)
        idx = sample(B, 1)[:2]
        exact = bool(np.array_equal(word[idx], TM.decode(llr[idx], model, model, iters, p, llr_scale=scale)["codeword"]))
        wrong = word[:, :code.k_c, :code.k_r] != msg
        # one hard-decision pass: the rows, then the columns
        hard = bch_decode((llr < 0).astype(np.uint8).reshape(B * n, n), comp, want="codeword").reshape(B, n, n)
        hard = bch_decode(np.ascontiguousarray(hard.transpose(0, 2, 1)).reshape(B * n, n), comp, want="codeword").reshape(B, n, n).transpose(0, 2, 1)
        hard_wrong = hard[:, :code.k_c, :code.k_r] != msg
        nbytes = 2 * iters * B * code.n * 24                      # per launch: llr and prior read, extrinsic written
        gbs = nbytes / (ms * 1e-3) / 1e9
        emit({"kernel": kname, "workload": "tpc_decode (%d, %d)^2, %d iterations, p=%d, Eb/N0=%.1f dB, B=%d" % (n, comp.k, iters, p, ebn0_db, B),
              "B": B, "p": p, "iters": iters, "launches": 2 * iters, "ms": ms, "ms_min": ms_min, "blocks_per_s": B / (ms * 1e-3),
              "value": B * code.k / (ms * 1e-3), "unit": "info-bits/s", "GB_per_s": gbs, "frac_copy": gbs / COPY_CEILING,
              "bytes_per_call": nbytes, "dtype": "f64", "ns_per_word_and_pattern": ms * 1e6 / (2 * iters * B * n * (1 << p)),
              "ber": float(wrong.mean()), "bler": float(wrong.any(axis=(1, 2)).mean()), "ber_hard_rows_then_columns": float(hard_wrong.mean()),
              "bler_hard_rows_then_columns": float(hard_wrong.any(axis=(1, 2)).mean()), "ebn0_db": ebn0_db,
              "parity": {"vs": "tests/tpc_model.py", "blocks": len(idx), "ok": exact}, "bound": BOUND}, fh)
        assert exact, "tpc_decode differs from the model"
    finally:
        dev.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    lib = _lib.load()
    _lib.require_device()
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    rs = np.random.RandomState(0)
    with open(OUT, "w") as fh:
        for n, t, m, prim, p in CHASE:
            chase_case(lib, fh, rs, n, t, m, prim, p, args)
        for n, t, m, ebn0_db in TPC:
            tpc_case(lib, fh, rs, n, t, m, ebn0_db, args)


if __name__ == "__main__":
    main()
