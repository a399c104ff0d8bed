#!/usr/bin/env python3
"""MIMO detection throughput (csrc/mimo.hip): device-resident inputs, HIP-event timing on the launch stream, after a warm-up
that covers the clock ramp; results are checked against the single-vector API after the timed region.  One JSON line each.
    python benchmarks/bench_mimo.py [--scale 1.0]
  kbest_hard / kbest_soft  4x4 16-QAM, K = 16, B = 2^20 vectors, one H per vector
  ml_qpsk / ml_qam16       4x4 QPSK (B = 2^20) and 4x4 16-QAM (B = 16384: 1.07e9 hypotheses)
  best_first               4x4 16-QAM, stack sizes (1, 3, 5), llr_max 500, B = 2^20 vectors, one H per vector; also the mean and
                           maximum number of search iterations per vector (a second, untimed launch with the iteration counter)
For ML and K-best the bound is the float64 VALU rate: `flop` counts the float64 operations of the search (per ML hypothesis nr complex
subtractions, squares and sums: 6 nr; per K-best child one complex multiply-subtract, a square and a sum: 12; the QR and the
selection are not counted) against the spec vector FP64 peak.  Best-first is a serial search of one wave per vector: its
`flop` is an upper bound (every pop evaluating m children twice at 8 depth + 6 float64 operations each), quoted only to show
how far it is from that bound.  The counters of a rocprofv3 --pmc run of their own are
quoted from profiles/ (profiles/README.md)."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from commpy_amd import _lib  # noqa: E402
from benchmarks.bench_kernels import timeit  # noqa: E402
from benchmarks.other_configs import Dev  # noqa: E402

FP64_PEAK = 78.6e12          # vector FP64, spec (FLOP/s)


def emit(name, workload, vectors, hyps, ms, flop, extra=None):
    d = {"kernel": name, "workload": workload, "value": vectors / (ms * 1e-3), "unit": "vectors/s", "ms": ms, "dtype": "f64",
         "hypotheses_per_s": hyps / (ms * 1e-3),
         "roofline": {"bound": "fp64 VALU", "achieved": flop / (ms * 1e-3) / 1e12, "peak": FP64_PEAK / 1e12, "unit": "TFLOP/s",
                      "frac": flop / (ms * 1e-3) / FP64_PEAK, "counted_flop_per_launch": flop},
         "build_id": _lib.build_id().get("full")}
    if extra:
        d.update(extra)
    print(json.dumps(d), flush=True)


def _problem(rs, B, nr, nt, md, noise):
    h = (rs.randn(B, nr, nt) + 1j * rs.randn(B, nr, nt)) / np.sqrt(2)
    x = md.constellation[rs.randint(0, md.m, (B, nt))]
    y = np.einsum('bij,bj->bi', h, x) + noise * (rs.randn(B, nr) + 1j * rs.randn(B, nr)) / np.sqrt(2)
    return np.ascontiguousarray(y), np.ascontiguousarray(h)


def bench_kbest(lib, scale, rs):
    from commpy_amd.modulation import QAMModem, kbest
    md = QAMModem(16)
    dem = lambda s: md.demodulate(s, 'hard')  # noqa: E731
    B, nr, nt, K = int((1 << 20) * scale), 4, 4, 16
    y, h = _problem(rs, B, nr, nt, md, 0.5)
    dev = Dev(lib)
    dy, dh = dev.put(y), dev.put(h)
    didx, dllr = dev.empty(4 * B * nt), dev.empty(8 * B * nt * 4)
    mh = md._device_handle()
    # children evaluated: 16 + 16*16 * 3 per vector
    children = 16 + 3 * 16 * 16
    for mode in ("hard", "soft"):
        if mode == "hard":
            def run():
                _lib.check(lib.cpx_kbest_hard_dev(mh, dy, dh, 1, B, nr, nt, K, didx, None))
        else:
            def run():
                _lib.check(lib.cpx_kbest_soft_dev(mh, dy, dh, 1, B, nr, nt, K, 0.25, dllr, None))
        ms, _ = timeit(lib, run, steps=5, warmup=2)
        kernel = _lib.last_kernel()
        pick = rs.choice(B, 24, replace=False)
        if mode == "hard":
            got = md.constellation[dev.get(didx, (B, nt), np.int32)[pick]]
            ok = all(np.array_equal(kbest(y[b], h[b], md.constellation, K), got[i]) for i, b in enumerate(pick))
        else:
            got = dev.get(dllr, (B, nt * 4), np.float64)[pick]
            with np.errstate(divide="ignore", invalid="ignore"):
                ref = np.array([kbest(y[b], h[b], md.constellation, K, 0.25, 'soft', dem) for b in pick])
            fin = np.isfinite(ref)
            ok = bool(np.array_equal(np.isinf(ref), np.isinf(got)) and np.allclose(got[fin], ref[fin], rtol=1e-9, atol=1e-9))
        flop = B * (12 * children + (nt * nr * 8 + nr * 4) * K * (mode == "soft"))
        emit("kbest_%s" % mode, "4x4 16-QAM K=16, B=%d, H per vector" % B, B, B * children, ms, flop,
             {"checked_vectors": len(pick), "check_ok": ok, "kernel_path": kernel})
    dev.free()


def bench_ml(lib, scale, rs):
    from commpy_amd.modulation import QAMModem, mimo_ml
    for m, B in ((4, int((1 << 20) * scale)), (16, int(16384 * scale))):
        md = QAMModem(m)
        nr = nt = 4
        y, h = _problem(rs, B, nr, nt, md, 0.6)
        dev = Dev(lib)
        dy, dh, didx = dev.put(y), dev.put(h), dev.empty(4 * B * nt)
        mh = md._device_handle()

        def run():
            _lib.check(lib.cpx_mimo_ml_dev(mh, dy, dh, 1, B, nr, nt, didx, None))
        ms, _ = timeit(lib, run, steps=3 if m == 16 else 5, warmup=1)
        kernel = _lib.last_kernel()
        got = md.constellation[dev.get(didx, (B, nt), np.int32)]
        pick = rs.choice(B, 8 if m == 16 else 32, replace=False)
        ok = all(np.array_equal(mimo_ml(y[b], h[b], md.constellation), got[b]) for b in pick)
        hyps = B * m ** nt
        emit("ml_%s" % ("qpsk" if m == 4 else "qam16"), "4x4 %d-QAM, B=%d, H per vector" % (m, B), B, hyps, ms,
             hyps * 6 * nr, {"checked_vectors": len(pick), "check_ok": ok, "kernel_path": kernel})
        dev.free()


def bench_best_first(lib, scale, rs):
    from commpy_amd.modulation import QAMModem, best_first_detector
    md = QAMModem(16)
    dem = lambda s: md.demodulate(s, 'hard')  # noqa: E731
    B, nr, nt, stacks = int((1 << 20) * scale), 4, 4, (1, 3, 5)
    y, h = _problem(rs, B, nr, nt, md, 0.5)
    dev = Dev(lib)
    dy, dh = dev.put(y), dev.put(h)
    dllr, diters = dev.empty(8 * B * nr * 4), dev.empty(4 * B)
    sizes = np.array(stacks, dtype=np.int32)
    mh = md._device_handle()

    def run(iters=None):
        _lib.check(lib.cpx_best_first_dev(mh, dy, dh, 1, B, nr, nt, _lib.ptr(sizes), 500.0, None, dllr, iters, None))
    ms, _ = timeit(lib, run, steps=5, warmup=2)
    kernel = _lib.last_kernel()
    got = dev.get(dllr, (B, nr * 4), np.float64)
    run(diters)
    it = dev.get(diters, (B,), np.int32)
    pick = rs.choice(B, 24, replace=False)
    ok = bool(all(np.array_equal(best_first_detector(y[b], h[b], md.constellation, stacks, 0.25, dem, 500), got[b]) for b in pick))
    ok = ok and bool(np.all(it > 0)) and bool(np.array_equal(dev.get(dllr, (B, nr * 4), np.float64), got))
    children = float(it.sum()) * (nr - 1) * 2 * 16            # upper bound: every stack popped in every iteration
    flop = children * (8 * nr + 6)
    emit("best_first", "4x4 16-QAM stacks (1,3,5) llr_max 500, B=%d, H per vector" % B, B, children, ms, flop,
         {"checked_vectors": len(pick), "check_ok": ok, "kernel_path": kernel, "iterations_mean": float(it.mean()),
          "iterations_max": int(it.max()), "us_per_vector_per_wave": ms * 1e3 / B})
    dev.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--which", default="kbest,ml,best_first")
    a = ap.parse_args()
    lib = _lib.load()
    _lib.require_device()
    rs = np.random.RandomState(11)
    if "kbest" in a.which:
        bench_kbest(lib, a.scale, rs)
    if "ml" in a.which.split(","):
        bench_ml(lib, a.scale, rs)
    if "best_first" in a.which:
        bench_best_first(lib, a.scale, rs)


if __name__ == "__main__":
    main()
