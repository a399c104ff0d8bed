#!/usr/bin/env python3
"""Doppler-fading multipath channel (csrc/fading.hip): device-resident rows (random bits -> QAM points on the device), HIP-event timing
of each CALL on the launch stream after a warm-up, one JSON line per measurement.
    python benchmarks/bench_fading.py [--scale 1.0] [--steps 5] [--warmup 3] [--out profiles/fading_bench.jsonl] [--only small1x1]
Cases: rows of 14 OFDM symbols of (nfft, cp) = (64, 16) ("small", n = 1120) and (2048, 144) ("large", n = 30688), 1x1 and 4x4, L = 16,
Ns = 16, hold = 1, one symbol (nfft + cp) and the whole row (n + L).  Per case:
  gains      cpx_fading_gains_dev for as many rows as make 10^9 sinusoid evaluations (B nblk nr nt L Ns).  `value` = sinusoids/s;
             `slots_per_sinusoid` = float64 lane-issue slots the device offers per sinusoid at that rate (256 CUs x 64 lanes per clock x
             2.4 GHz = 3.93e13 per second: the float64 vector rate behind the 78.6 TFLOPS of the data sheet); the instructions a
             sinusoid really takes were not counted, so no share of that rate is claimed.
  convolve   cpx_fading_convolve_dev with the caller's G, for as many rows as make 1 GB of algorithmic bytes: x + y + G, each once.
             `frac` is against the 8.0 TB/s HBM peak, `frac_copy` against the 6.29 TB/s of a streaming copy.
  multipath  cpx_multipath_dev (the static channel) on the same rows in the same run: the reference point.  `vs_multipath` = the
             convolve call's time over its time; for hold >= the row the two do the same arithmetic on the same bytes.
  channel    cpx_fading_channel_dev without a caller's G (gains in the scratch arena, chunked): the whole call.
What was timed is checked on the host against the model of tests/fading_model.py on the first row."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import fading_model as M  # noqa: E402
from commpy_amd import _lib  # noqa: E402
from commpy_amd.modulation import QAMModem  # noqa: E402
from benchmarks.bench_kernels import timeit  # noqa: E402
from benchmarks.other_configs import Dev  # noqa: E402

HBM_PEAK = 8000.0       # GB/s, spec
COPY_CEILING = 6290.0   # GB/s, a measured streaming copy
F64_SLOTS = 256 * 64 * 2.4e9
ROWS = [("small", 64, 16), ("large", 2048, 144)]
NSYM, L, NS, FD = 14, 16, 16, 0.001
SEED, SID = 5, 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    ap.add_argument("--only", default=None, help="comma-separated subset of small1x1, small4x4, large1x1, large4x4")
    args = ap.parse_args()
    lib = _lib.load()
    _lib.require_device()
    md = QAMModem(64)
    sink = open(args.out, "a") if args.out else None
    only = set(args.only.split(",")) if args.only else None
    pdp = np.exp(-0.25 * np.arange(L))
    pdp /= pdp.sum()
    P_ = _lib.ptr

    def emit(d):
        d["build_id"] = _lib.build_id().get("full")
        line = json.dumps(d)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    def roof(nbytes, ms):
        gbs = nbytes / (ms * 1e-3) / 1e9
        return {"achieved": gbs, "peak": HBM_PEAK, "unit": "GB/s", "frac": gbs / HBM_PEAK, "frac_copy": gbs / COPY_CEILING,
                "algorithmic_bytes_per_launch": nbytes, "bound": "unmeasured (no counter pass)"}

    def gains(B, na, hold, nblk, out):
        _lib.check(lib.cpx_fading_gains_dev(B, na, na, L, P_(pdp), None, NS, FD, 0.0, hold, 0, nblk, SEED, SID, 0, out, None))

    for rname, nfft, cp in ROWS:
        for na in (1, 4):
            case = "%s%dx%d" % (rname, na, na)
            if only and case not in only:
                continue
            n = NSYM * (nfft + cp)
            lout, ntaps = n + L - 1, na * na * L
            for hold in (n + L, nfft + cp, 1):                                   # the whole row first: its time is the others' yardstick
                nblk = -(-lout // hold)
                what = "%s n=%d %dx%d L=%d Ns=%d hold=%d (%d blocks)" % (rname, n, na, na, L, NS, hold, nblk)
                dev = Dev(lib)
                try:
                    # ---- gains: 10^9 sinusoids ----
                    Bg = int(np.ceil(1e9 * args.scale / (nblk * ntaps * NS)))
                    G = dev.empty(Bg * nblk * ntaps * 16)
                    ms, ms_min = timeit(lib, lambda: gains(Bg, na, hold, nblk, G), steps=args.steps, warmup=args.warmup)
                    rate = Bg * nblk * ntaps * NS / (ms * 1e-3)
                    emit({"kernel": _lib.last_kernel(), "workload": "fading_gains " + what, "rows": Bg, "ms": ms, "ms_min": ms_min, "value": rate,
                          "unit": "sinusoids/s", "dtype": "complex128", "slots_per_sinusoid": F64_SLOTS / rate,
                          "roofline": roof(16 * Bg * nblk * ntaps, ms)})
                    _lib.check(lib.cpx_stream_sync(None))
                    prm = dev.empty(ntaps * (NS + 1) * 16)
                    _lib.check(lib.cpx_fading_params_dev(1, na, na, L, NS, FD, 0.0, SEED, SID, 0, prm, None))
                    _lib.check(lib.cpx_stream_sync(None))
                    jb = min(nblk, 64)                                           # the first blocks of row 0, and its last one
                    taus = M.block_times(0, hold, nblk)[np.r_[0:jb, nblk - 1]]
                    got = np.concatenate([dev.get(G, (jb, na, na, L), complex), dev.get(G, (1, na, na, L), complex, offset=(nblk - 1) * ntaps * 16)])
                    want = M.gains_from_params(dev.get(prm, (1, na, na, L, NS + 1, 2), np.float64), pdp, None, taus)[0]
                    bound = M.gain_bound(pdp, None, NS, FD, 0.0, taus, M.FADING_SINCOS_ULP)[:, None, None, :]
                    assert np.all(np.maximum(np.abs(got.real - want.real), np.abs(got.imag - want.imag)) <= bound), "gains mismatch"
                    dev.free()
                    # ---- convolution: 1 GB ----
                    per_row = 16 * (na * n + na * lout + nblk * ntaps)
                    B = int(np.ceil(1e9 * args.scale / per_row))
                    bits, x = dev.empty(B * na * n * 6), dev.empty(B * na * n * 16)
                    _lib.check(lib.cpx_random_bits_dev(bits, B * na * n * 6, 1, 0, None))
                    _lib.check(lib.cpx_modulate_dev(md._device_handle(), bits, B * na * n, x, None))
                    G, y = dev.empty(B * nblk * ntaps * 16), dev.empty(B * na * lout * 16)
                    gains(B, na, hold, nblk, G)
                    if nblk == 1:
                        g0 = G
                    else:
                        g0 = dev.empty(B * ntaps * 16)
                        gains(B, na, n + L, 1, g0)
                    mp = lambda: _lib.check(lib.cpx_multipath_dev(x, g0, 1, B, na, na, n, L, y, None))
                    ms, ms_min = timeit(lib, mp, steps=args.steps, warmup=args.warmup)
                    mp_ms = ms
                    emit({"kernel": _lib.last_kernel(), "workload": "multipath (reference point) " + what, "rows": B, "ms": ms, "ms_min": ms_min,
                          "dtype": "complex128", "roofline": roof(16 * B * (na * n + na * lout + ntaps), ms)})
                    cv = lambda: _lib.check(lib.cpx_fading_convolve_dev(x, G, 1, B, na, na, n, L, hold, y, None))
                    ms, ms_min = timeit(lib, cv, steps=args.steps, warmup=args.warmup)
                    emit({"kernel": _lib.last_kernel(), "workload": "fading_convolve " + what, "rows": B, "ms": ms, "ms_min": ms_min,
                          "value": B * na * lout / (ms * 1e-3), "unit": "output samples/s", "dtype": "complex128", "vs_multipath": ms / mp_ms,
                          "roofline": roof(B * per_row, ms)})
                    _lib.check(lib.cpx_stream_sync(None))
                    x0 = dev.get(x, (1, na, n), complex)
                    G0 = dev.get(G, (1, nblk, na, na, L), complex)
                    err = np.abs(dev.get(y, (1, na, lout), complex) - M.convolve(x0, G0, hold))
                    assert np.all(err <= M.convolve_bound(x0, G0, hold)), "convolve mismatch"
                    ch = lambda: _lib.check(lib.cpx_fading_channel_dev(x, B, na, na, n, L, P_(pdp), None, NS, FD, 0.0, hold, 0, SEED, SID, 0, y, None,
                                                                       None))
                    ms, ms_min = timeit(lib, ch, steps=args.steps, warmup=args.warmup)
                    emit({"kernel": _lib.last_kernel(), "workload": "fading_channel (gains in scratch) " + what, "rows": B, "ms": ms, "ms_min": ms_min,
                          "value": B * na * lout / (ms * 1e-3), "unit": "output samples/s", "dtype": "complex128",
                          "roofline": roof(16 * B * (na * n + na * lout), ms)})
                    _lib.check(lib.cpx_stream_sync(None))
                    assert np.all(np.abs(dev.get(y, (1, na, lout), complex) - M.convolve(x0, G0, hold)) <= M.convolve_bound(x0, G0, hold)), "channel mismatch"
                finally:
                    dev.free()
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
