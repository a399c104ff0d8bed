#!/usr/bin/env python3
"""Adaptive equaliser throughput (csrc/adaptive.hip): device-resident inputs, HIP-event timing on the launch stream after a warm-up that
covers the clock ramp, one JSON line per case, also written to profiles/adaptive_bench.jsonl.
    python benchmarks/bench_adaptive.py [--scale 1.0] [--steps 5]
Cases: QPSK and 64-QAM through three taps at 20 dB, n = 256 symbols of which nt = 64 train, sps = 1 and 2 (zero-stuffed); the linear
equaliser (nf = 32) and the feedback equaliser (nf = 32, nb = 7) with 'lms' (mu = 0.01 / Es) and 'nlms' (mu = 0.2), and 'rls' at
nf = 16, nb = 4 (lambda = 0.99); the default delays; 'indices' only.
B is chosen so that a launch reads about 1 GB of y (scale 1).  Rows are a base of up to 4096 noisy blocks, repeated.  After the timed
region the first, middle and last rows of the timed output are compared with tests/adaptive_model.py (exactly).

Yardstick, same run, never the code under test: cpx_mmse_equalize_dev as a feedback equaliser (nf = 32, nb = 7, delay 26, shared taps, hard) on the
rows of the sps = 1 case -- eq_dfe_kernel is the closest existing serial per-row recursion.  Its time per symbol and feedback tap,
ms / (B n nb), stands against the LMS time per symbol and tap, ms / (B n (nf + nb)): `tap_ratio`.  The allowance comes from the
instruction counts of the compiled loops (gfx950, hipcc -S): eq_dfe_kernel<0> issues 23 instructions per feedback tap (8 float64
operations, 4 LDS reads); ad_lms_kernel issues 32 (filter, 12 float64 with the regressor energy, 4 LDS reads) + 28 (update, 8 float64,
4 LDS reads and 2 LDS writes) = 60 per feed-forward tap and 24 + 20 = 44 per feedback tap (the blocks that hold the float64 work of the
feedback loops; the selection of x = 0.0 for t - j < 0 sits in further blocks, so 44 is a lower bound and the allowance errs low).  To
regenerate the three constants after a change to either kernel: `hipcc --offload-arch=gfx950 -O3 -ffp-contract=off --cuda-device-only -S`
on csrc/adaptive.hip and csrc/equalize.hip, then count the instructions of the loop blocks (those ending in s_cbranch that hold
v_*_f64) of ad_lms_kernel and eq_dfe_kernel<0>; they are not derived at run time.  `allowance` is the case's mean over its
taps divided by 23 (2.61 for nf = 32, 2.48 with nb = 7), and `within_1.25x` is tap_ratio <= 1.25 * allowance.  The yardstick's numerator
also holds the scan of y, the feed-forward pass and the slicer, spread over only 7 taps, so the ratio flatters the LMS kernel;
`ns_per_symbol` is given for both to compare whole calls."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import adaptive_model as A  # noqa: E402
from commpy_amd import _lib  # noqa: E402
from commpy_amd.modulation import QAMModem  # noqa: E402
from benchmarks.bench_kernels import timeit  # noqa: E402
from benchmarks.other_configs import Dev  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "adaptive_bench.jsonl")
TAPS = np.array([1.0, 0.3 + 0.2j, -0.1j])
N, NT, BASE_ROWS, SNR_DB = 256, 64, 4096, 20.0
DFE_PER_TAP, LMS_PER_FF_TAP, LMS_PER_FB_TAP = 23.0, 60.0, 44.0          # instructions of the compiled loops, see above
# (algorithm, nf, nb, parameters); the LMS step is divided by the mean symbol energy
RUNS = [("lms", 32, 0, dict(step=0.01)), ("lms", 32, 7, dict(step=0.01)), ("nlms", 32, 0, dict(step=0.2)), ("nlms", 32, 7, dict(step=0.2)),
        ("rls", 16, 4, dict(forgetting=0.99, delta=0.01))]


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
            handle = modem._device_handle()
            dfe_tap_ps = None
            for sps in (1, 2):
                rs = np.random.RandomState(40 + M_ + sps)
                n_y = N * sps + len(TAPS) - 1
                B = max(int(args.scale * 1.0e9 / (16 * n_y)), 64)
                base = min(BASE_ROWS, B)
                idx0 = rs.randint(0, M_, (base, N))
                up = np.zeros((base, N * sps), dtype=np.complex128)
                up[:, ::sps] = modem.constellation[idx0]
                y0 = np.stack([np.convolve(row, TAPS) for row in up])
                y0 = y0 + np.sqrt(modem.Es / 10 ** (SNR_DB / 10) / 2) * (rs.randn(*y0.shape) + 1j * rs.randn(*y0.shape))
                y, tr = np.resize(y0, (B, n_y)), np.ascontiguousarray(np.resize(idx0[:, :NT], (B, NT)), dtype=np.int32)
                rows = sorted({0, 1, B // 2, B // 2 + 1, B - 2, B - 1})
                dev = Dev(lib)
                try:
                    d_y, d_tr, d_idx = dev.put(y.view(np.float64)), dev.put(tr), dev.empty(4 * B * N)
                    if sps == 1:
                        # ---- the yardstick: the MMSE feedback equaliser with shared taps on the same rows
                        nv = np.array([modem.Es / 10 ** (SNR_DB / 10)])
                        d_h, d_nv = dev.put(np.ascontiguousarray(TAPS).view(np.float64)), dev.put(nv)
                        fn = lambda: _lib.check(lib.cpx_mmse_equalize_dev(handle, float(modem.Es), d_y, d_h, 0, B, N, len(TAPS), 1, d_nv, 0, 32, 7,
                                                                          26, d_idx, *((None,) * 7), None))
                        ms, ms_min = timeit(lib, fn, steps=args.steps, warmup=args.warmup)
                        dfe_tap_ps = ms * 1e9 / (B * N * 7)
                        emit({"kernel": _lib.last_kernel(), "workload": "yardstick: mmse_equalize %s L=3 nf=32 nb=7 n=%d, hard, shared taps, B=%d"
                              % (name, N, B), "B": B, "n": N, "nf": 32, "nb": 7, "M": M_, "ms": ms, "ms_min": ms_min,
                              "ns_per_symbol": ms * 1e6 / (B * N), "ps_per_symbol_and_feedback_tap": dfe_tap_ps, "dtype": "f64",
                              "bytes_per_launch": y.nbytes}, fh)
                    for algorithm, nf, nb, par in RUNS:
                        code = A.ALGORITHMS.index(algorithm)
                        par = {key: (v / modem.Es if algorithm == "lms" else v) for key, v in par.items()}
                        d_par = {key: dev.put(np.array([v])) for key, v in par.items()}
                        delay = A.default_delay(nf, nb)                # in samples, whatever sps
                        fn = lambda: _lib.check(lib.cpx_adaptive_equalize_dev(handle, d_y, B, n_y, N, sps, d_tr, 1, NT, nf, nb, delay, code,
                                                                              d_par.get("step"), 0, d_par.get("forgetting"), 0, d_par.get("delta"), 0,
                                                                              1e-6, None, 0, None, 0, d_idx, None, None, None, None, None, None))
                        ms, ms_min = timeit(lib, fn, steps=args.steps, warmup=args.warmup)
                        kernel = _lib.last_kernel()
                        _lib.check(lib.cpx_stream_sync(None))
                        ref = A.equalize(y[rows], modem.constellation, tr[rows], nf, nb, algorithm, delay=delay, sps=sps, n=N, **par)
                        got = np.stack([dev.get(d_idx, (N,), np.int32, offset=4 * N * r) for r in rows])
                        exact = bool(np.array_equal(got, ref["indices"]))
                        errors = int((got[:, NT:] != idx0[[r % base for r in rows]][:, NT:]).sum())
                        tap_ps = ms * 1e9 / (B * N * (nf + nb))
                        line = {"kernel": kernel, "workload": "adaptive_equalize %s %s nf=%d nb=%d n=%d nt=%d sps=%d, hard, B=%d"
                                % (name, algorithm, nf, nb, N, NT, sps, B), "B": B, "n": N, "nt": NT, "nf": nf, "nb": nb, "sps": sps, "M": M_,
                                "algorithm": algorithm, "ms": ms, "ms_min": ms_min, "ns_per_row": ms * 1e6 / B, "ns_per_symbol": ms * 1e6 / (B * N),
                                "ps_per_symbol_and_tap": tap_ps, "value": B * N * modem.num_bits_symbol / (ms * 1e-3), "unit": "bits/s",
                                "symbol_errors_after_training_in_checked_rows": errors, "dtype": "f64", "bytes_per_launch": y.nbytes,
                                "bounding_unit": "unmeasured", "parity": {"vs": "tests/adaptive_model.py", "rows": len(rows), "ok": exact}}
                        if algorithm != "rls":
                            allowance = (nf * LMS_PER_FF_TAP + nb * LMS_PER_FB_TAP) / (nf + nb) / DFE_PER_TAP
                            line.update({"yardstick_ps_per_symbol_and_feedback_tap": dfe_tap_ps, "tap_ratio": tap_ps / dfe_tap_ps,
                                         "allowance": allowance, "within_1.25x": bool(tap_ps / dfe_tap_ps <= 1.25 * allowance)})
                        emit(line, fh)
                        assert exact, "adaptive_equalize differs from the model"
                finally:
                    dev.free()


if __name__ == "__main__":
    main()
