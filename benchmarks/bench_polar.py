#!/usr/bin/env python3
"""Polar encoder / decoder throughput (csrc/polar.hip): device-resident inputs, HIP-event timing on the launch stream after a warm-up,
one JSON line per case, also appended to profiles/polar_bench.jsonl.
    python benchmarks/bench_polar.py [--scale 1.0] [--steps 5] [--no-context]
Cases: (1024, 512 + CRC-11) at L = 1 and L = 8, (128, 64 + CRC-11) at L = 8, the (1024, 512 + CRC-11) encoder; BPSK over AWGN at
Eb/N0 = 3 dB, code words from the device encoder.  B is chosen so that one launch lasts milliseconds and is part of every line.  After
the timed region the first, middle and last words of the timed output are compared with tests/polar_model.py (exactly).  For context
the same run times the turbo decoder of config 3 (rate 1/3, N = 1024, 6 iterations) and the 802.11n (1944, 1296) LDPC min-sum decoder
(50 iterations at most); their lines carry no parity check of their own (bench.py and benchmarks/other_configs.py hold those)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import polar_model as M  # noqa: E402
from commpy_amd import _lib  # noqa: E402
from commpy_amd.channelcoding import PolarCode, polar_encode  # noqa: E402
from benchmarks.bench_kernels import timeit  # noqa: E402
from benchmarks.other_configs import DESIGN_1944, Dev, turbo_workload  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "polar_bench.jsonl")
CRC11 = 0xE21


def emit(d, fh):
    d["build_id"] = _lib.build_id().get("full")
    line = json.dumps(d)
    print(line, flush=True)
    fh.write(line + "\n")


def sample(B, n=2):
    return sorted(set(list(range(min(n, B))) + list(range(B // 2, min(B // 2 + n, B))) + list(range(max(B - n, 0), B))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-context", action="store_true", help="skip the turbo and LDPC lines")
    args = ap.parse_args()
    lib = _lib.load()
    _lib.require_device()
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    rs = np.random.RandomState(0)
    with open(OUT, "w") as fh:
        for N, K, L, B in ((1024, 523, 1, 16384), (1024, 523, 8, 2048), (128, 75, 8, 16384)):
            B = max(int(B * args.scale), 8)
            code = PolarCode(N, K, crc=CRC11)
            msg = rs.randint(0, 2, (B, code.A)).astype(np.uint8)
            sigma2 = 1.0 / (2.0 * (code.A / N) * 10.0 ** 0.3)
            llr = 2.0 * (1.0 - 2.0 * polar_encode(msg, code) + np.sqrt(sigma2) * rs.randn(B, N)) / sigma2
            dev = Dev(lib)
            try:
                d_llr, d_bits, d_ok = dev.put(llr), dev.empty(B * code.A), dev.empty(B)
                h = code._device_handle()
                ms, ms_min = timeit(lib, lambda: _lib.check(lib.cpx_polar_decode_dev(h, d_llr, B, L, d_bits, d_ok, None, None, None, None, None,
                                                                                    None)), steps=args.steps, warmup=args.warmup)
                kname = _lib.last_kernel()
                _lib.check(lib.cpx_stream_sync(None))
                bits, ok = dev.get(d_bits, (B, code.A), np.uint8), dev.get(d_ok, (B,), np.uint8)
            finally:
                dev.free()
            idx = sample(B)
            ref = M.decode_batch(llr[idx], code.frozen, L, CRC11)
            exact = bool(np.array_equal(bits[idx], ref["bits"]) and np.array_equal(ok[idx], ref["crc_ok"]))
            emit({"kernel": kname, "workload": "polar_decode (%d, %d + CRC-11) L=%d Eb/N0=3 dB B=%d" % (N, code.A, L, B), "B": B, "ms": ms,
                  "ms_min": ms_min, "value": B * code.A / (ms * 1e-3), "unit": "info-bits/s", "dtype": "f64", "block_error_rate": float(np.mean((bits != msg).any(axis=1))), "crc_pass_rate": float(ok.mean()),
                  "parity": {"vs": "tests/polar_model.py", "words": len(idx), "ok": exact}, "bound": "unmeasured (no counter pass)"}, fh)
            assert exact, "polar_decode differs from the model"
        # the encoder
        code = PolarCode(1024, 523, crc=CRC11)
        B = max(int((1 << 20) * args.scale), 8)
        msg = rs.randint(0, 2, (B, code.A)).astype(np.uint8)
        dev = Dev(lib)
        try:
            d_msg, d_x = dev.put(msg), dev.empty(B * 1024)
            h = code._device_handle()
            ms, ms_min = timeit(lib, lambda: _lib.check(lib.cpx_polar_encode_dev(h, d_msg, B, d_x, None)), steps=args.steps, warmup=args.warmup)
            kname = _lib.last_kernel()
            _lib.check(lib.cpx_stream_sync(None))
            x = dev.get(d_x, (B, 1024), np.uint8)
        finally:
            dev.free()
        idx = sample(B, 8)
        exact = bool(np.array_equal(x[idx], np.stack([M.encode(m, code.frozen, CRC11) for m in msg[idx]])))
        gbs = B * (code.A + 1024) / (ms * 1e-3) / 1e9
        emit({"kernel": kname, "workload": "polar_encode (1024, %d + CRC-11) B=%d" % (code.A, B), "B": B, "ms": ms, "ms_min": ms_min,
              "value": B * code.A / (ms * 1e-3), "unit": "info-bits/s", "GB_per_s": gbs, "dtype": "u8",
              "parity": {"vs": "tests/polar_model.py", "words": len(idx), "ok": exact}, "bound": "unmeasured (no counter pass)"}, fh)
        assert exact, "polar_encode differs from the model"
        if args.no_context:
            return
        # context: the turbo decoder of config 3 and the LDPC min-sum decoder, timed by the same run
        B, Nt, n_iter = max(int(16384 * args.scale), 64), 1024, 6
        tr, il, _, s, p1, p2, nv = turbo_workload(B, Nt)
        dev = Dev(lib)
        try:
            d_s, d_p1, d_p2, d_perm, d_bits = dev.put(s), dev.put(p1), dev.put(p2), dev.put(np.asarray(il.p_array, dtype=np.int32)), dev.empty(B * Nt)
            h = tr._device_handle()
            ms, ms_min = timeit(lib, lambda: _lib.check(lib.cpx_turbo_decode_batch_dev(h, d_s, d_p1, d_p2, None, d_perm, B, Nt, nv, n_iter, d_bits,
                                                                                      None)), steps=args.steps, warmup=args.warmup)
            emit({"kernel": _lib.last_kernel(), "workload": "context: turbo config 3, rate 1/3, N=1024, 6 iterations, Eb/N0=1.5 dB, B=%d" % B,
                  "B": B, "ms": ms, "ms_min": ms_min, "value": B * Nt / (ms * 1e-3), "unit": "info-bits/s"}, fh)
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
