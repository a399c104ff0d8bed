#!/usr/bin/env python3
"""Time-tracking pilot-aided channel estimation (cpx_pilots_estimate_tv_dev) beside the per-frame estimator
(cpx_pilots_estimate_dev) on the same Y in the same run: device-resident inputs (random bits -> QAM points on the device), HIP-event
timing of each CALL on the launch stream after a warm-up, the two calls alternating; one JSON line per call and case.
    python benchmarks/bench_ofdm_tv.py [--scale 1.0] [--steps 8] [--out profiles/ofdm_tv_bench.jsonl] [--only frame1]
Cases: the two frame shapes of bench_ofdm_chan.py, 14 symbols of (nfft, nsc, cp) = (64, 52, 16) at 2x2 with comb pilots every 4
subcarriers ('linear' in frequency) and of (2048, 1200, 144) at 4x4 with comb pilots every 8 (('taps', 144, 2048)), pilot symbols
(0, 4, 9, 13), 'linear' in time.  Both calls write y_data and h_data.  Algorithmic bytes per frame, the same for both: (nr nsym nsc +
ndata nr + ndata nr nt) 16 (read Y, write y_data and h_data; LSp, Hp and H^ per symbol are intermediates); each launch moves at
least 1 GB (scale 1).  `frac` is against the 8.0 TB/s HBM peak, `frac_copy` against the 6.29 TB/s of a streaming copy; `ratio` is
the time-tracking call's time over the per-frame call's.  A call is four kernels (cpx_last_kernel names them): the figures are the
call's, not one kernel's."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from commpy_amd import _lib  # noqa: E402
from commpy_amd.modulation import OfdmPilots, QAMModem  # noqa: E402
from benchmarks.bench_ofdm_chan import COPY_CEILING, HBM_PEAK, qam  # noqa: E402
from benchmarks.other_configs import Dev, warm  # noqa: E402

FRAMES = [((64, 52, 16), 2, 2, 4, 'linear'), ((2048, 1200, 144), 4, 4, 8, ('taps', 144, 2048))]
NSYM, PILOT_SYMBOLS = 14, [0, 4, 9, 13]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    ap.add_argument("--only", default=None, help="comma-separated subset of frame0, frame1 (a profiler run of one case)")
    args = ap.parse_args()
    lib = _lib.load()
    _lib.require_device()
    md = QAMModem(64)
    sink = open(args.out, "a") if args.out else None
    only = set(args.only.split(",")) if args.only else None
    tm = ctypes.c_void_p()
    _lib.check(lib.cpx_timer_create(ctypes.byref(tm)))

    def timed(fn):
        _lib.check(lib.cpx_timer_start(tm, None))
        fn()
        _lib.check(lib.cpx_timer_stop(tm, None))
        v = ctypes.c_float()
        _lib.check(lib.cpx_timer_elapsed_ms(tm, ctypes.byref(v)))
        return v.value

    for case, ((nfft, nsc, cp), nt, nr, spacing, interp) in enumerate(FRAMES):
        if only and "frame%d" % case not in only:
            continue
        p = OfdmPilots.comb(nsc, NSYM, nt, spacing, PILOT_SYMBOLS, interp, time_interp='linear')
        F, nd = NSYM * nsc, p.ndata
        per = (nr * F + nd * nr + nd * nr * nt) * 16
        B = int(np.ceil(1e9 * args.scale / per))
        what = "nfft=%d nsc=%d nsym=%d %dx%d comb/%d %s pilot symbols %s" % (nfft, nsc, NSYM, nr, nt, spacing,
                                                                              interp if isinstance(interp, str) else interp[0], PILOT_SYMBOLS)
        dev = Dev(lib)
        try:
            Y = qam(lib, dev, md, B * nr * F, 2)
            y, h = dev.empty(B * nd * nr * 16), dev.empty(B * nd * nr * nt * 16)
            y0, h0 = dev.empty(B * nd * nr * 16), dev.empty(B * nd * nr * nt * 16)
            calls = {"ofdm_estimate_tv": lambda: _lib.check(lib.cpx_pilots_estimate_tv_dev(p.handle(), Y, B, nr, None, y, h, None)),
                     "ofdm_estimate": lambda: _lib.check(lib.cpx_pilots_estimate_dev(p.handle(), Y, B, nr, None, y0, h0, None))}
            ms, kernels = {k: [] for k in calls}, {}
            for name, fn in calls.items():
                warm(lib, fn, args.warmup)
                kernels[name] = _lib.last_kernel()
            for _ in range(args.steps):                     # alternating, so that a drift of the clocks meets both alike
                for name, fn in calls.items():
                    ms[name].append(timed(fn))
            mean = {k: float(np.mean(v)) for k, v in ms.items()}
            for name in calls:
                gbs = per * B / (mean[name] * 1e-3) / 1e9
                d = {"kernel": kernels[name], "workload": "%s %s" % (name, what), "frames": B, "ms": mean[name], "ms_min": float(np.min(ms[name])),
                     "ms_max": float(np.max(ms[name])), "value": B / (mean[name] * 1e-3), "unit": "frames/s", "dtype": "complex128",
                     "roofline": {"bound": "HBM", "achieved": gbs, "peak": HBM_PEAK, "unit": "GB/s", "frac": gbs / HBM_PEAK,
                                  "frac_copy": gbs / COPY_CEILING, "algorithmic_bytes_per_launch": per * B},
                     "build_id": _lib.build_id().get("full")}
                if name == "ofdm_estimate_tv":
                    d["ratio_to_per_frame_estimate"] = mean["ofdm_estimate_tv"] / mean["ofdm_estimate"]
                line = json.dumps(d)
                print(line, flush=True)
                if sink:
                    sink.write(line + "\n")
                    sink.flush()
            # what was timed, checked on the first frame: both calls demap Y alike, and h_data was written (its values are the tests' business)
            _lib.check(lib.cpx_stream_sync(None))
            Y0 = dev.get(Y, (nr, NSYM, nsc), complex)
            for buf in (y, y0):
                assert np.array_equal(Y0[:, p.data_sym, p.data_sc].T, dev.get(buf, (nd, nr), complex)), "demap mismatch"
            assert np.all(np.isfinite(dev.get(h, (nd, nr, nt), complex))), "h_data not finite"
        finally:
            dev.free()
    lib.cpx_timer_destroy(tm)
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
