#!/usr/bin/env python3
"""Pulse shaping, matched filtering and frequency offset throughput (csrc/fir.hip): device-resident inputs (random bits -> QPSK on
the device), HIP-event timing on the launch stream after a warm-up, one JSON line per case, then a CPU line per case.
    python benchmarks/bench_fir.py [--scale 1.0] [--steps 5]
Cases: RRC alpha = 0.22 over 12 symbols at sps 4 and 8 (49 / 97 real taps), interpolator and decimator, long rows (B = 64) and short
rows (64 symbols per row); an 839-tap complex (Zadoff-Chu) correlator at sps = 1; the frequency offset.  Each launch moves at least
1 GB (scale 1).  Algorithmic bytes per row: interpolator (n + n sps + ntaps - 1) 16, decimator (n + outputs) 16, offset 2 n 16.
`frac` is against the 8.0 TB/s HBM peak, `frac_copy` against the 6.29 TB/s of a streaming copy.  The correlator is bound by float64
FMA issue: its line reports the fraction of the 39.3 T FMA/s the vector units issue (256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz).
The CPU lines are numpy.convolve / numpy.exp over the same rows on the host, on fewer rows."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from commpy_amd import _lib  # noqa: E402
from commpy_amd.filters import _fir_plan, rrcosfilter  # noqa: E402
from commpy_amd.modulation import QAMModem  # noqa: E402
from commpy_amd.sequences import zcsequence  # noqa: E402
from commpy_amd.utilities import upsample  # noqa: E402
from benchmarks.bench_kernels import timeit  # noqa: E402
from benchmarks.other_configs import Dev  # noqa: E402

HBM_PEAK = 8000.0       # GB/s, spec
COPY_CEILING = 6290.0   # GB/s, a measured streaming copy
FMA_PEAK = 256 * 4 * 16 * 2.4e9   # float64 FMAs per second the vector units can issue


def emit(d):
    print(json.dumps(d), flush=True)


def best_of(fn, reps=3):
    best = float("inf")
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        best = min(best, time.perf_counter() - t0)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-cpu", action="store_true", help="skip the host lines (counter passes)")
    args = ap.parse_args()
    lib = _lib.load()
    _lib.require_device()
    md = QAMModem(4)
    target = 1e9 * args.scale
    cases = []
    for sps in (4, 8):
        _, h = rrcosfilter(12 * sps + 1, 0.22, 1.0, sps)
        for rows in ("long", "short"):
            cases.append(("rrc", sps, np.ascontiguousarray(h), False, rows))
    cases.append(("zc839", 1, np.ascontiguousarray(np.conj(zcsequence(25, 839)[::-1])), True, "long"))
    rs = np.random.RandomState(0)
    for name, sps, h, cx, rows in cases:
        ntaps = h.size
        plan = _fir_plan(h, cx).handle()
        if rows == "short":
            n = 64
            B = int(np.ceil(target / ((n + n * sps + ntaps - 1) * 16)))
        else:
            B = 64
            n = int(np.ceil(target / (B * (1 + sps) * 16)))
        lw = n * sps + ntaps - 1
        off = ntaps - 1
        ld = -(-(lw + ntaps - 1 - off) // sps)
        dev = Dev(lib)
        try:
            bits = dev.empty(B * n * 2)
            x = dev.empty(B * n * 16)
            w = dev.empty(B * lw * 16)
            r = dev.empty(B * ld * 16)
            _lib.check(lib.cpx_random_bits_dev(bits, B * n * 2, 1, 0, None))
            _lib.check(lib.cpx_modulate_dev(md._device_handle(), bits, B * n, x, None))
            calls = [("interp", lambda: _lib.check(lib.cpx_fir_interp_dev(plan, x, B, n, sps, w, None)), (n + lw) * 16 * B,
                      2 * (2 if cx else 1) * -(-ntaps // sps) * lw * B),
                     ("decim", lambda: _lib.check(lib.cpx_fir_decim_dev(plan, w, B, lw, sps, off, r, None)), (lw + ld) * 16 * B,
                      2 * (2 if cx else 1) * ntaps * ld * B)]
            for what, call, nbytes, fmas in calls:
                ms, ms_min = timeit(lib, call, steps=args.steps, warmup=args.warmup)
                gbs = nbytes / (ms * 1e-3) / 1e9
                if name == "zc839":
                    roof = {"bound": "valu", "achieved": fmas / (ms * 1e-3), "peak": FMA_PEAK, "unit": "float64 FMA/s",
                            "frac": fmas / (ms * 1e-3) / FMA_PEAK, "GB_per_s": gbs}
                else:
                    roof = {"bound": "HBM", "achieved": gbs, "peak": HBM_PEAK, "unit": "GB/s", "frac": gbs / HBM_PEAK,
                            "frac_copy": gbs / COPY_CEILING, "algorithmic_bytes_per_launch": nbytes}
                emit({"kernel": _lib.last_kernel(), "workload": "fir_%s %s sps=%d ntaps=%d %s rows B=%d n=%d" %
                      (what, name, sps, ntaps, rows, B, n if what == "interp" else lw), "ms": ms, "ms_min": ms_min,
                      "value": (lw if what == "interp" else ld) * B / (ms * 1e-3), "unit": "output samples/s", "dtype": "complex128",
                      "roofline": roof, "build_id": _lib.build_id().get("full")})
            _lib.check(lib.cpx_stream_sync(None))
            # what was timed, against numpy on the first row
            x0 = dev.get(x, (n,), complex)[:2000]
            w0 = dev.get(w, (lw,), complex)[:2000 * sps]
            assert np.max(np.abs(w0 - np.convolve(upsample(x0, sps), h)[:2000 * sps])) < 1e-9, "interpolator mismatch"
            nd = min(ld, 2000)                                  # the decimator's first outputs from the waveform it read
            wd = dev.get(w, (min(lw, off + nd * sps),), complex)
            r0 = dev.get(r, (nd,), complex)
            assert np.max(np.abs(r0 - np.convolve(wd, h)[off::sps][:nd])) < 1e-9 * np.sum(np.abs(h)), "decimator mismatch"
        finally:
            dev.free()
        if args.no_cpu:
            continue
        nc = min(n, 50000)                                      # the CPU lines: rows cut to 50 000 symbols, about 3e8 multiply-adds
        ncpu = max(1, min(B, int(3e8 / (nc * sps * ntaps))))
        xc = rs.randn(ncpu, nc) + 1j * rs.randn(ncpu, nc)
        wc = [np.convolve(upsample(row, sps), h) for row in xc]
        ti = best_of(lambda: [np.convolve(upsample(row, sps), h) for row in xc])
        td = best_of(lambda: [np.convolve(row, h)[off::sps] for row in wc])
        for what, tt, nb in (("interp", ti, (nc + nc * sps + ntaps - 1) * 16 * ncpu), ("decim", td, (nc * sps + ntaps - 1 + nc + 1) * 16 * ncpu)):
            emit({"kernel": "cpu_baseline (numpy.convolve on the host, %d rows of %d symbols)" % (ncpu, nc), "workload": "fir_%s %s sps=%d ntaps=%d %s rows"
                  % (what, name, sps, ntaps, rows), "ms": tt * 1e3, "GB_per_s": nb / tt / 1e9})
    # frequency offset
    B, n = 64, int(np.ceil(target / (64 * 32)))
    dev = Dev(lib)
    try:
        bits = dev.empty(B * n * 2)
        x = dev.empty(B * n * 16)
        y = dev.empty(B * n * 16)
        st = dev.empty(8)
        step = np.array([(2 * np.pi) * (1.234e3 / 1e6)])
        _lib.check(lib.cpx_memcpy_h2d(st, _lib.ptr(step), 8))
        _lib.check(lib.cpx_random_bits_dev(bits, B * n * 2, 1, 0, None))
        _lib.check(lib.cpx_modulate_dev(md._device_handle(), bits, B * n, x, None))
        ms, ms_min = timeit(lib, lambda: _lib.check(lib.cpx_freq_offset_dev(x, B, n, st, 0, y, None)), steps=args.steps, warmup=args.warmup)
        nbytes = 2 * n * 16 * B
        gbs = nbytes / (ms * 1e-3) / 1e9
        emit({"kernel": _lib.last_kernel(), "workload": "freq_offset B=%d n=%d" % (B, n), "ms": ms, "ms_min": ms_min,
              "value": B * n / (ms * 1e-3), "unit": "samples/s", "dtype": "complex128",
              "roofline": {"bound": "HBM", "achieved": gbs, "peak": HBM_PEAK, "unit": "GB/s", "frac": gbs / HBM_PEAK,
                           "frac_copy": gbs / COPY_CEILING, "algorithmic_bytes_per_launch": nbytes},
              "build_id": _lib.build_id().get("full")})
        _lib.check(lib.cpx_stream_sync(None))
        x0, y0 = dev.get(x, (4000,), complex), dev.get(y, (4000,), complex)
        assert np.max(np.abs(y0 - x0 * np.exp(1j * (step[0] * np.arange(4000))))) < 1e-12, "frequency offset mismatch"
    finally:
        dev.free()
    if args.no_cpu:
        return
    xc = rs.randn(10 ** 6) + 1j * rs.randn(10 ** 6)
    tt = best_of(lambda: xc * np.exp(1j * 2 * np.pi * (1.234e3 / 1e6) * np.arange(len(xc))))
    emit({"kernel": "cpu_baseline (numpy.exp on the host, 1e6 samples)", "workload": "freq_offset", "ms": tt * 1e3,
          "GB_per_s": 32 * len(xc) / tt / 1e9})


if __name__ == "__main__":
    main()
