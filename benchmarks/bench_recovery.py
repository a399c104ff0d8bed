#!/usr/bin/env python3
"""Timing / carrier recovery throughput (csrc/recovery.hip): device-resident inputs, HIP-event timing on the launch stream after a
warm-up that covers the clock ramp, one JSON line per case, also written to profiles/recovery_bench.jsonl.
    python benchmarks/bench_recovery.py [--scale 1.0] [--steps 5]
Cases: QPSK and 64-QAM raised-cosine rows (roll-off 0.35, timing offset 0.3 symbol, sample clock 1.0004, phase 0.03 turn, 5e-4 cycle
per symbol, noise 0.02 sqrt(Es) per part), n = 1024 strobes, sps = 2 and 4, the Gardner and the Mueller-Mueller detector, 64
training labels, the cubic interpolator, the carrier loop on, gains k1 = 0.02 sps / Es, k2 = 2e-4 sps / Es,
carrier = (0.05 / Es, 0.002 / Es); 'symbols' only, plus one case that also asks for 'indices'.
B is chosen so that a launch reads about 1 GB of y (scale 1).  Rows are a base of up to 256 bursts, repeated.  After the timed region
the first, middle and last rows of the timed output are compared with tests/recovery_model.py (exactly).

Yardstick, same run, never the code under test: cpx_adaptive_equalize_dev, LMS, linear, nf = 8, 64 training labels, on the same rows
and sps -- ad_lms_kernel is the closest existing serial per-row recursion with a slicer in it.  `ratio` is ns per symbol of the
recovery loop over ns per symbol of the yardstick.  The allowance comes from the instruction counts of the two compiled step loops
(gfx950, hipcc -S, the blocks of one step on the path the benchmark takes, the slicer's loop counted per point):
  ad_lms_kernel   251 + 36 sps outside the tap loops, 32 (filter) + 28 (update) = 60 per feed-forward tap, 15 per constellation point;
  tr_loop_kernel  <gardner, cubic, carrier> 430 and <mm, cubic, carrier> 355 outside the slicer, 15 per constellation point, and the
                  ring's refill, 282 instructions (16 loads and 32 LDS writes with their addresses) once every 16 / sps steps.
`allowance` = (tr + 282 sps / 16 + 15 M) / (251 + 36 sps + 60 nf + 15 M), and `within_1.25x` is ratio <= 1.25 * allowance.  To
regenerate the constants after a change to either kernel: `hipcc --offload-arch=gfx950 -O3 -ffp-contract=off --cuda-device-only -S`
on csrc/recovery.hip and csrc/adaptive.hip, then add up the instructions of the basic blocks between the head of the step loop and
its back edge (the output blocks of results that are not asked for left out); they are not derived at run time, so every line carries
the counts it was judged with (`instruction_counts`) next to the build id."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import recovery_model as R  # noqa: E402
from commpy_amd import _lib  # noqa: E402
from commpy_amd.modulation import QAMModem  # noqa: E402
from benchmarks.bench_kernels import timeit  # noqa: E402
from benchmarks.other_configs import Dev  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "recovery_bench.jsonl")
N, NT, BASE_ROWS, NF = 1024, 64, 256, 8
LMS_FIXED, LMS_PER_SPS, LMS_PER_TAP, PER_POINT = 251.0, 36.0, 60.0, 15.0          # instructions of the compiled loops, see above
TR_FIXED, TR_REFILL = {"gardner": 430.0, "mm": 355.0}, 282.0
# (ted, also 'indices')
RUNS = [("gardner", False), ("mm", False), ("gardner", True)]


def emit(d, fh):
    d["build_id"] = _lib.build_id().get("full")
    line = json.dumps(d)
    print(line, flush=True)
    fh.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    lib = _lib.load()
    _lib.require_device()
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as fh:
        for name, M_ in (("QPSK", 4), ("64-QAM", 64)):
            modem = QAMModem(M_)
            handle, es = modem._device_handle(), float(modem.Es)
            for sps in (2, 4):
                n_y = (N + 8) * sps
                B = max(int(args.scale * 1.0e9 / (16 * n_y)), 64)
                base = min(BASE_ROWS, B)
                bursts = [R.rc_burst(modem.constellation, N + 16, sps, 1000 * M_ + 10 * sps + b, sigma=0.02 * np.sqrt(es), n_y=n_y)
                          for b in range(base)]
                idx0, y0 = np.stack([b[0] for b in bursts]), np.stack([b[1] for b in bursts])
                y, tr = np.resize(y0, (B, n_y)), np.ascontiguousarray(np.resize(idx0[:, :NT], (B, NT)), dtype=np.int32)
                rows = sorted({0, 1, B // 2, B // 2 + 1, B - 2, B - 1})
                k1, k2, kc = 0.02 * sps / es, 2e-4 * sps / es, (0.05 / es, 0.002 / es)
                dev = Dev(lib)
                try:
                    d_y, d_tr = dev.put(y.view(np.float64)), dev.put(tr)
                    d_sym, d_idx = dev.empty(16 * B * N), dev.empty(4 * B * N)
                    # ---- the yardstick: the linear LMS equaliser on the same rows
                    d_step = dev.put(np.array([0.01 / es]))
                    fn = lambda: _lib.check(lib.cpx_adaptive_equalize_dev(handle, d_y, B, n_y, N, sps, d_tr, 1, NT, NF, 0, (NF - 1) // 2, 0, d_step,
                                                                          0, None, 0, None, 0, 1e-6, None, 0, None, 0, d_idx, None, None, None,
                                                                          None, None, None))
                    ms, ms_min = timeit(lib, fn, steps=args.steps, warmup=args.warmup)
                    lms_ns = ms * 1e6 / (B * N)
                    emit({"kernel": _lib.last_kernel(), "workload": "yardstick: adaptive_equalize %s lms nf=%d nb=0 n=%d nt=%d sps=%d, hard, B=%d"
                          % (name, NF, N, NT, sps, B), "B": B, "n": N, "nf": NF, "sps": sps, "M": M_, "ms": ms, "ms_min": ms_min,
                          "ns_per_symbol": lms_ns, "dtype": "f64", "bytes_per_launch": y.nbytes}, fh)
                    d_par = {key: dev.put(np.array([v])) for key, v in (("k1", k1), ("k2", k2), ("kc1", kc[0]), ("kc2", kc[1]), ("mu0", 0.0),
                                                                        ("phase0", 0.0))}
                    d_m0 = dev.put(np.zeros(1, dtype=np.int64))
                    for ted, with_indices in RUNS:
                        if with_indices and (M_, sps) != (4, 2):
                            continue
                        fn = lambda: _lib.check(lib.cpx_timing_recover_dev(handle, d_y, B, n_y, N, sps, R.TEDS.index(ted), 1, d_par["k1"], 0,
                                                                           d_par["k2"], 0, d_par["kc1"], 0, d_par["kc2"], 0, d_tr,
                                                                           1, NT, d_m0, 0, d_par["mu0"], 0, d_par["phase0"], 0, d_sym,
                                                                           d_idx if with_indices else None, None, None, None, None, None,
                                                                           None))
                        ms, ms_min = timeit(lib, fn, steps=args.steps, warmup=args.warmup)
                        kernel = _lib.last_kernel()
                        _lib.check(lib.cpx_stream_sync(None))
                        ref = R.recover(y[rows], sps, modem.constellation, ted, "cubic", k1, k2, kc, tr[rows], N)
                        got = np.stack([dev.get(d_sym, (N,), np.complex128, offset=16 * N * r) for r in rows])
                        exact = bool(np.array_equal(got.view(np.int64), ref["symbols"].view(np.int64))) and not ref["bad"].any()
                        if with_indices:
                            labels = np.stack([dev.get(d_idx, (N,), np.int32, offset=4 * N * r) for r in rows])
                            exact = exact and bool(np.array_equal(labels, ref["indices"]))
                        errors = int((ref["indices"][:, 500:N] != idx0[[r % base for r in rows]][:, 500:N]).sum())
                        ns = ms * 1e6 / (B * N)
                        allowance = ((TR_FIXED[ted] + TR_REFILL * sps / 16 + PER_POINT * M_)
                                     / (LMS_FIXED + LMS_PER_SPS * sps + LMS_PER_TAP * NF + PER_POINT * M_))
                        emit({"kernel": kernel, "workload": "timing_recover %s %s cubic carrier n=%d nt=%d sps=%d, %s, B=%d"
                              % (name, ted, N, NT, sps, "symbols + indices" if with_indices else "symbols", B), "B": B, "n": N, "nt": NT,
                              "sps": sps, "M": M_, "ted": ted, "ms": ms, "ms_min": ms_min, "ns_per_row": ms * 1e6 / B, "ns_per_symbol": ns,
                              "value": B * N / (ms * 1e-3), "unit": "symbols/s", "symbol_errors_after_500_in_checked_rows": errors,
                              "dtype": "f64", "bytes_per_launch": y.nbytes, "read_GBps": y.nbytes / (ms * 1e-3) / 1e9,
                              "bounding_unit": "unmeasured", "yardstick_ns_per_symbol": lms_ns, "ratio": ns / lms_ns, "allowance": allowance,
                              "within_1.25x": bool(ns / lms_ns <= 1.25 * allowance),
                              "instruction_counts": {"lms_fixed": LMS_FIXED, "lms_per_sps": LMS_PER_SPS, "lms_per_tap": LMS_PER_TAP,
                                                     "per_point": PER_POINT, "tr_fixed": TR_FIXED[ted], "tr_refill": TR_REFILL},
                              "parity": {"vs": "tests/recovery_model.py", "rows": len(rows), "ok": exact}}, fh)
                        assert exact, "timing_recover differs from the model"
                finally:
                    dev.free()


if __name__ == "__main__":
    main()
