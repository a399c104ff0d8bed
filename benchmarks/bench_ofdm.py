#!/usr/bin/env python3
"""OFDM transmit / receive throughput (csrc/ofdm.hip): device-resident inputs (random bits -> 64-QAM on the device), HIP-event
timing on the launch stream after a warm-up, one JSON line per (direction, shape), then a CPU baseline line per shape.
    python benchmarks/bench_ofdm.py [--scale 1.0] [--steps 5]
Shapes (nfft, nsc, cp): (64, 52, 16), (2048, 1200, 144), (4096, 3276, 288) on the LDS-resident FFT, (1536, 900, 108) on the direct
DFT.  Each launch moves at least 1 GB (scale 1).  Algorithmic bytes per symbol: TX (nsc + P + nfft) 16 (read the subcarriers, write
prefix and symbol), RX (nfft + nsc) 16 (read the symbol without its prefix, write the used bins).  `frac` is against the 8.0 TB/s
HBM peak, `frac_copy` against the 6.29 TB/s a streaming copy reaches on the MI355X.
The CPU baseline is vectorised numpy.fft (bin map, ifft / fft, prefix) over the same shapes on this machine's host cores, timed
on fewer symbols; the reference's own ofdm_tx / ofdm_rx do not run on Python 3."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from commpy_amd import _lib  # noqa: E402
from commpy_amd.modulation import QAMModem, _ofdm_plan, ofdm_prefix_length  # noqa: E402
from benchmarks.bench_kernels import timeit  # noqa: E402
from benchmarks.other_configs import Dev  # noqa: E402

HBM_PEAK = 8000.0       # GB/s, spec
COPY_CEILING = 6290.0   # GB/s, a measured streaming copy
SHAPES = [(64, 52, 16), (2048, 1200, 144), (4096, 3276, 288), (1536, 900, 108)]


def alg_bytes(nfft, nsc, cp):
    P = ofdm_prefix_length(nfft, cp)
    return {"tx": (nsc + P + nfft) * 16, "rx": (nfft + nsc) * 16}


def emit(d):
    print(json.dumps(d), flush=True)


def cpu_baseline(nfft, nsc, cp, nsym):
    """numpy.fft on the host: TX and RX of nsym symbols, best of three."""
    h, P = nsc // 2, ofdm_prefix_length(nfft, cp)
    rs = np.random.RandomState(0)
    x = rs.randn(nsym, nsc) + 1j * rs.randn(nsym, nsc)
    bins = np.concatenate([np.arange(1, h + 1), np.arange(nfft - h, nfft)])
    src = np.concatenate([np.arange(h, 2 * h), np.arange(h)])

    def tx():
        F = np.zeros((nsym, nfft), complex)
        F[:, bins] = x[:, src]
        t = np.fft.ifft(F, axis=1)
        return np.concatenate([t[:, nfft - P:], t], axis=1)

    y = np.concatenate([np.zeros((nsym, cp), complex), tx()[:, P:]], axis=1)

    def rx():
        X = np.fft.fft(y[:, cp:], axis=1)
        return np.concatenate([X[:, nfft - h:], X[:, 1:h + 1]], axis=1)

    out = {}
    for name, fn in (("tx", tx), ("rx", rx)):
        best = float("inf")
        for _ in range(3):
            t0 = time.perf_counter()
            fn()
            best = min(best, time.perf_counter() - t0)
        out[name] = best
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    lib = _lib.load()
    _lib.require_device()
    md = QAMModem(64)
    for nfft, nsc, cp in SHAPES:
        P = ofdm_prefix_length(nfft, cp)
        per = alg_bytes(nfft, nsc, cp)
        nsym = int(np.ceil(1e9 * args.scale / min(per.values())))
        plan = _ofdm_plan(nfft, nsc, cp).handle()
        dev = Dev(lib)
        try:
            bits = dev.empty(nsym * nsc * 6)
            x = dev.empty(nsym * nsc * 16)
            t = dev.empty(nsym * (P + nfft) * 16)
            xr = dev.empty(nsym * nsc * 16)
            _lib.check(lib.cpx_random_bits_dev(bits, nsym * nsc * 6, 1, 0, None))
            _lib.check(lib.cpx_modulate_dev(md._device_handle(), bits, nsym * nsc, x, None))
            calls = {"tx": lambda: _lib.check(lib.cpx_ofdm_tx_dev(plan, x, 1, nsym, t, None)),
                     "rx": lambda: _lib.check(lib.cpx_ofdm_rx_dev(plan, t, 1, nsym * (P + nfft), xr, None))}
            for name in ("tx", "rx"):
                ms, ms_min = timeit(lib, calls[name], steps=args.steps, warmup=args.warmup)
                kernel = _lib.last_kernel()
                nbytes = per[name] * nsym
                gbs = nbytes / (ms * 1e-3) / 1e9
                emit({"kernel": kernel, "workload": "ofdm_%s nfft=%d nsc=%d cp=%d" % (name, nfft, nsc, cp), "symbols": nsym,
                      "ms": ms, "ms_min": ms_min, "value": nsym / (ms * 1e-3), "unit": "OFDM symbols/s", "dtype": "complex128",
                      "roofline": {"bound": "HBM", "achieved": gbs, "peak": HBM_PEAK, "unit": "GB/s", "frac": gbs / HBM_PEAK,
                                   "frac_copy": gbs / COPY_CEILING, "algorithmic_bytes_per_launch": nbytes},
                      "build_id": _lib.build_id().get("full")})
            # the round trip of a few symbols as a sanity check of what was timed
            _lib.check(lib.cpx_stream_sync(None))
            got = dev.get(xr, (min(nsym, 64), nsc), complex)
            want = dev.get(x, (min(nsym, 64), nsc), complex)
            assert np.max(np.abs(got - want)) < 1e-9, "ofdm round trip mismatch"
        finally:
            dev.free()
        ncpu = max(1, min(nsym, int(2e8 / min(per.values()))))
        cpu = cpu_baseline(nfft, nsc, cp, ncpu)
        for name in ("tx", "rx"):
            emit({"kernel": "cpu_baseline (numpy.fft on the host, not the reference)", "workload": "ofdm_%s nfft=%d nsc=%d cp=%d" %
                  (name, nfft, nsc, cp), "symbols": ncpu, "ms": cpu[name] * 1e3, "value": ncpu / cpu[name], "unit": "OFDM symbols/s",
                  "GB_per_s": per[name] * ncpu / cpu[name] / 1e9})


if __name__ == "__main__":
    main()
