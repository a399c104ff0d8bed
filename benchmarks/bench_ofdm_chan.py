#!/usr/bin/env python3
"""Multipath channel, resource mapping and pilot-aided channel estimation (csrc/ofdm_chan.hip): device-resident inputs (random bits
-> QAM points on the device), HIP-event timing of each CALL on the launch stream after a warm-up, one JSON line per case.
    python benchmarks/bench_ofdm_chan.py [--scale 1.0] [--steps 5] [--out profiles/ofdm_chan_bench.jsonl] [--only frame1]
Cases: frames of 14 symbols of (nfft, nsc, cp) = (64, 52, 16) at 2x2 with comb pilots every 4 subcarriers ('linear'), and of
(2048, 1200, 144) at 4x4 with comb pilots every 8 (('taps', 144, 2048)); the multipath channel with L = 16 at 1x1 and 4x4.  Each
launch moves at least 1 GB (scale 1).  Algorithmic bytes per frame: map (ndata nt + nt nsym nsc) 16; estimate (nr nsym nsc +
ndata nr + ndata nr nt) 16 (read Y, write y_data and h_data; H^ per subcarrier stays an intermediate); multipath
(nt n + nr (n + L - 1)) 16 per row and 4 nr nt L (n + L - 1) FMAs.  `frac` is against the 8.0 TB/s HBM peak, `frac_copy` against the
6.29 TB/s of a streaming copy, `frac_fma` against the 39.3 T FMA/s float64 issue rate.  An estimate call is three or four kernels
(cpx_last_kernel names them): its figures are the call's, not one kernel's."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from commpy_amd import _lib  # noqa: E402
from commpy_amd.modulation import OfdmPilots, QAMModem  # noqa: E402
from benchmarks.bench_kernels import timeit  # noqa: E402
from benchmarks.other_configs import Dev  # noqa: E402

HBM_PEAK = 8000.0       # GB/s, spec
COPY_CEILING = 6290.0   # GB/s, a measured streaming copy
FMA_PEAK = 39.3e12      # float64 FMA/s
FRAMES = [((64, 52, 16), 2, 2, 4, [0, 7], 'linear'), ((2048, 1200, 144), 4, 4, 8, [0, 4, 7, 11], ('taps', 144, 2048))]
NSYM = 14
MULTIPATH = [(1, 1, 1 << 22, 16), (4, 4, 1 << 20, 16)]


def qam(lib, dev, md, n, seed):
    """n random 64-QAM points on the device."""
    bits, x = dev.empty(n * 6), dev.empty(n * 16)
    _lib.check(lib.cpx_random_bits_dev(bits, n * 6, seed, 0, None))
    _lib.check(lib.cpx_modulate_dev(md._device_handle(), bits, n, x, None))
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    ap.add_argument("--only", default=None, help="comma-separated subset of frame0, frame1, multipath0, multipath1 (a profiler run of one case)")
    args = ap.parse_args()
    lib = _lib.load()
    _lib.require_device()
    md = QAMModem(64)
    sink = open(args.out, "a") if args.out else None
    only = set(args.only.split(",")) if args.only else None

    def emit(d):
        d["build_id"] = _lib.build_id().get("full")
        line = json.dumps(d)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    def roof(nbytes, ms, fma=None):
        gbs = nbytes / (ms * 1e-3) / 1e9
        r = {"achieved": gbs, "peak": HBM_PEAK, "unit": "GB/s", "frac": gbs / HBM_PEAK, "frac_copy": gbs / COPY_CEILING,
             "algorithmic_bytes_per_launch": nbytes}
        if fma is not None:
            r.update({"fma_per_launch": fma, "fma_per_s": fma / (ms * 1e-3), "frac_fma": fma / (ms * 1e-3) / FMA_PEAK})
        return r

    for case, ((nfft, nsc, cp), nt, nr, spacing, psym, interp) in enumerate(FRAMES):
        if only and "frame%d" % case not in only:
            continue
        p = OfdmPilots.comb(nsc, NSYM, nt, spacing, psym, interp)
        F, nd = NSYM * nsc, p.ndata
        per_map = (nd * nt + nt * F) * 16
        per_est = (nr * F + nd * nr + nd * nr * nt) * 16
        B = int(np.ceil(1e9 * args.scale / min(per_map, per_est)))
        what = "nfft=%d nsc=%d nsym=%d %dx%d comb/%d %s" % (nfft, nsc, NSYM, nr, nt, spacing, interp if isinstance(interp, str) else interp[0])
        dev = Dev(lib)
        try:
            data, Y = qam(lib, dev, md, B * nd * nt, 1), qam(lib, dev, md, B * nr * F, 2)
            grid, y, h = dev.empty(B * nt * F * 16), dev.empty(B * nd * nr * 16), dev.empty(B * nd * nr * nt * 16)
            calls = {"ofdm_map": (lambda: _lib.check(lib.cpx_pilots_map_dev(p.handle(), data, B, grid, None)), per_map),
                     "ofdm_estimate": (lambda: _lib.check(lib.cpx_pilots_estimate_dev(p.handle(), Y, B, nr, None, y, h, None)), per_est)}
            for name, (fn, per) in calls.items():
                ms, ms_min = timeit(lib, fn, steps=args.steps, warmup=args.warmup)
                emit({"kernel": _lib.last_kernel(), "workload": "%s %s" % (name, what), "frames": B, "ms": ms, "ms_min": ms_min,
                      "value": B / (ms * 1e-3), "unit": "frames/s", "dtype": "complex128", "roofline": dict(roof(per * B, ms), bound="HBM")})
            # what was timed, checked on the first frame: the grid against its data, y_data against Y
            _lib.check(lib.cpx_stream_sync(None))
            g0 = dev.get(grid, (nt, NSYM, nsc), complex)
            d0 = dev.get(data, (nd, nt), complex)
            assert np.array_equal(g0[:, p.data_sym, p.data_sc].T, d0), "map mismatch"
            Y0, y0 = dev.get(Y, (nr, NSYM, nsc), complex), dev.get(y, (nd, nr), complex)
            assert np.array_equal(Y0[:, p.data_sym, p.data_sc].T, y0), "demap mismatch"
        finally:
            dev.free()

    for case, (nt, nr, n, L) in enumerate(MULTIPATH):
        if only and "multipath%d" % case not in only:
            continue
        per = (nt * n + nr * (n + L - 1)) * 16
        B = int(np.ceil(1e9 * args.scale / per))
        rs = np.random.RandomState(0)
        g = (rs.randn(nr, nt, L) + 1j * rs.randn(nr, nt, L)) * np.exp(-0.3 * np.arange(L))
        dev = Dev(lib)
        try:
            x, dg, out = qam(lib, dev, md, B * nt * n, 3), dev.put(g), dev.empty(B * nr * (n + L - 1) * 16)
            fn = lambda: _lib.check(lib.cpx_multipath_dev(x, dg, 0, B, nt, nr, n, L, out, None))
            ms, ms_min = timeit(lib, fn, steps=args.steps, warmup=args.warmup)
            fma = 4 * nr * nt * L * (n + L - 1) * B
            emit({"kernel": _lib.last_kernel(), "workload": "multipath %dx%d n=%d L=%d" % (nr, nt, n, L), "rows": B, "ms": ms,
                  "ms_min": ms_min, "value": B * nr * (n + L - 1) / (ms * 1e-3), "unit": "output samples/s", "dtype": "complex128",
                  "roofline": dict(roof(per * B, ms, fma), bound="float64 FMA issue" if fma / FMA_PEAK > per * B / (HBM_PEAK * 1e9) else "HBM")})
            _lib.check(lib.cpx_stream_sync(None))
            x0 = np.stack([dev.get(x, (4096,), complex, offset=t * n * 16) for t in range(nt)])       # row 0: x [B][nt][n]
            want = sum(np.convolve(x0[t], g[1 % nr, t]) for t in range(nt))[:4096]
            got = dev.get(out, (4096,), complex, offset=(1 % nr) * (n + L - 1) * 16)
            assert np.max(np.abs(got - want)) < 1e-9, "multipath mismatch"
        finally:
            dev.free()
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
