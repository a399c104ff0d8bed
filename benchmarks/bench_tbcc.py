#!/usr/bin/env python3
"""Tail-biting Viterbi throughput (csrc/tbcc.hip): device-resident inputs, HIP-event timing on the launch stream after a warm-up that
covers the clock ramp, one JSON line per case, also written to profiles/tbcc_bench.jsonl.
    python benchmarks/bench_tbcc.py [--scale 1.0] [--steps 5]
Codes: (133, 171, 165) at T = 40 and 140, (133, 171) at T = 288; 'soft', max_wraps = 4, all four outputs.  B is chosen so that a launch
reads about 1 GB of LLRs (scale 1): a base of 16384 noisy tail-biting words, repeated.  Rows at Eb/N0 = 6 dB (one trip on average) and at
1 dB (mixed); the trip histogram is the device's own 'wraps'.  Reported: time per code word, and per trellis step per trip
(ms / (T * sum of wraps): with 64 states a wave holds one code word and runs exactly its trips).  After the timed region the first,
middle and last rows of the timed output are compared with tests/tbcc_model.py (exactly).

Yardstick, same run: viterbi_decode's state-per-lane kernel (path 'wave') on terminated blocks of the same trellis and T steps' worth of
input (T - 6 message bits and the tail), 'soft', default traceback depth, as many rows; its time per step is ms / (B * steps run).
`step_ratio` = tail-biting time per step per trip over that; the project's 1.25x rule applies to it."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import tbcc_model as M  # noqa: E402
from commpy_amd import _lib  # noqa: E402
from commpy_amd.channelcoding import Trellis, conv_encode_batch  # noqa: E402
from commpy_amd.channelcoding.convcode import _viterbi_sizes, device_trellis  # noqa: E402
from benchmarks.bench_bch import sample  # noqa: E402
from benchmarks.bench_kernels import timeit  # noqa: E402
from benchmarks.other_configs import Dev  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "tbcc_bench.jsonl")
CASES = (((0o133, 0o171, 0o165), 40), ((0o133, 0o171, 0o165), 140), ((0o133, 0o171), 288))
BASE_ROWS, MAX_WRAPS, SOFT = 16384, 4, 1


def emit(d, fh):
    d["build_id"] = _lib.build_id().get("full")
    line = json.dumps(d)
    print(line, flush=True)
    fh.write(line + "\n")


def llrs(words, ebn0_db, rate, rs):
    sigma = np.sqrt(1.0 / (2.0 * rate * 10.0 ** (ebn0_db / 10.0)))
    return 2.0 * ((2.0 * words - 1.0) + sigma * rs.randn(*words.shape)) / sigma ** 2


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
        for gens, T in CASES:
            tr = Trellis(np.array([6]), np.array([list(gens)]))
            n, mem = tr.n, tr.total_memory
            B = max(int(args.scale * 1.0e9 / (8 * T * n)), 64)
            base = min(BASE_ROWS, B)
            name = "(%s) T=%d" % (", ".join("%o" % g for g in gens), T)
            h = device_trellis(tr)
            sent, closed = M.encode_batch(rs.randint(0, 2, (base, T)), tr)
            assert closed.all()
            term = conv_encode_batch(rs.randint(0, 2, (base, T - mem)), tr)          # T steps with the tail
            assert term.shape[1] == T * n
            L, steps_run, tb = _viterbi_sizes(T * n, tr, None)
            for ebn0 in (6.0, 1.0):
                dev = Dev(lib)
                try:
                    # ---- the yardstick: terminated blocks through the state-per-lane Viterbi kernel
                    rx = np.resize(llrs(term, ebn0, 1.0 / n, rs), (B, T * n))
                    d_rx, d_bits = dev.put(rx), dev.empty(B * T)
                    _lib.viterbi_set_path("wave")
                    try:
                        y_ms, y_min = timeit(lib, lambda: _lib.check(lib.cpx_viterbi_decode_batch_dev(h, d_rx, B, T * n, L, steps_run, tb, SOFT,
                                                                                                      d_bits, None)),
                                             steps=args.steps, warmup=args.warmup)
                        y_kernel = _lib.last_kernel()
                    finally:
                        _lib.viterbi_set_path(None)
                    assert "viterbi_wave_kernel" in y_kernel, y_kernel
                    y_step_ns = y_ms * 1e6 / (B * steps_run)
                    emit({"kernel": y_kernel, "workload": "yardstick: viterbi_decode 'wave', terminated %s, %g dB, B=%d" % (name, ebn0, B), "B": B,
                          "T": T, "ebn0_db": ebn0, "ms": y_ms, "ms_min": y_min, "steps_run": steps_run, "tb_depth": tb,
                          "ns_per_codeword": y_ms * 1e6 / B, "ns_per_step": y_step_ns, "dtype": "f64", "bytes_per_launch": rx.nbytes}, fh)
                    # ---- the tail-biting decoder
                    rx = np.resize(llrs(sent, ebn0, 1.0 / n, rs), (B, T * n))
                    _lib.check(lib.cpx_memcpy_h2d(d_rx, _lib.ptr(rx), rx.nbytes))
                    d_wraps, d_tb, d_metric = dev.empty(4 * B), dev.empty(B), dev.empty(8 * B)
                    ms, ms_min = timeit(lib, lambda: _lib.check(lib.cpx_tbcc_decode_dev(h, d_rx, B, T, SOFT, MAX_WRAPS, d_bits, d_wraps, d_tb,
                                                                                        d_metric, None)),
                                        steps=args.steps, warmup=args.warmup)
                    kernel = _lib.last_kernel()
                    _lib.check(lib.cpx_stream_sync(None))
                    got = {"bits": dev.get(d_bits, (B, T), np.uint8), "wraps": dev.get(d_wraps, (B,), np.int32),
                           "tailbiting": dev.get(d_tb, (B,), np.uint8), "metric": dev.get(d_metric, (B,), np.float64)}
                    idx = sample(B, 4)
                    ref = M.decode_batch(rx[idx], tr, 'soft', MAX_WRAPS)
                    exact = all(np.array_equal(got[key][idx].view(np.int64) if key == "metric" else got[key][idx],
                                               ref[key].view(np.int64) if key == "metric" else ref[key]) for key in got)
                    trips = int(got["wraps"].sum())
                    step_ns = ms * 1e6 / (T * trips)
                    ratio = step_ns / y_step_ns
                    emit({"kernel": kernel, "workload": "tailbiting_decode %s, 'soft', %g dB, max_wraps=%d, B=%d" % (name, ebn0, MAX_WRAPS, B),
                          "B": B, "T": T, "ebn0_db": ebn0, "ms": ms, "ms_min": ms_min, "ns_per_codeword": ms * 1e6 / B,
                          "ns_per_step_per_trip": step_ns, "mean_trips": trips / B,
                          "trip_histogram": np.bincount(got["wraps"], minlength=MAX_WRAPS + 1).tolist(),
                          "tailbiting_share": float(got["tailbiting"].mean()), "value": B * T / (ms * 1e-3), "unit": "info-bits/s",
                          "yardstick_ns_per_step": y_step_ns, "step_ratio": ratio, "within_1.25x": bool(ratio <= 1.25), "dtype": "f64",
                          "bytes_per_launch": rx.nbytes, "parity": {"vs": "tests/tbcc_model.py", "rows": len(idx), "ok": bool(exact)}}, fh)
                    assert exact, "tailbiting_decode differs from the model"
                    del rx, got
                finally:
                    dev.free()


if __name__ == "__main__":
    main()
