#!/usr/bin/env python3
"""Timing / frequency-offset synchronisation (csrc/sync.hip): device-resident rows (random bits -> QAM points on the device), HIP-event
timing of each CALL on the launch stream after a warm-up, one JSON line per case.
    python benchmarks/bench_sync.py [--scale 1.0] [--steps 5] [--warmup 3] [--out profiles/sync_bench.jsonl] [--only sc2048x1]
Cases: the Schmidl-Cox search (D = W = nfft / 2) at (nfft, cp) = (64, 16), (2048, 144), (8192, 576) and the cyclic-prefix correlator
(D = nfft, W = cp) at (2048, 144), each with nr = 1 and 4, on rows of 16 OFDM symbols; per case cpx_sync_estimate_dev, then
cpx_sync_align_dev fed by its outputs (offset = -cp, nout = 15 symbols), and as reference points of the same run cpx_freq_offset_dev
on the same rows and the NumPy running-sum (cumsum) evaluation of the search on the host.  Every call moves at least 1 GB (scale 1).
Algorithmic bytes per row: estimate nr n 16 (read; its outputs are 24 bytes); align and freq_offset 2 x 16 per output sample.
`frac` is against the 8.0 TB/s HBM peak, `frac_copy` against the 6.29 TB/s of a streaming copy, `vs_freq_offset` the call's
bytes per second over cpx_freq_offset_dev's.  An estimate call is two or three kernels (cpx_last_kernel names them): its figures
are the call's, not one kernel's."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from commpy_amd import _lib  # noqa: E402
from commpy_amd.modulation import QAMModem  # noqa: E402
from benchmarks.bench_kernels import timeit  # noqa: E402
from benchmarks.other_configs import Dev  # noqa: E402

HBM_PEAK = 8000.0       # GB/s, spec
COPY_CEILING = 6290.0   # GB/s, a measured streaming copy
I64MAX = (1 << 63) - 1
# name, nfft, cp, lag, window
FORMS = [("sc64", 64, 16, 32, 32), ("sc2048", 2048, 144, 1024, 1024), ("sc8192", 8192, 576, 4096, 4096), ("cp2048", 2048, 144, 2048, 144)]
NSYM = 16


def host_search(row, D, W):
    """The search of one row [nr, n] as NumPy running sums (cumsum and a difference): (d, M[d], step)."""
    n = row.shape[1]
    q = np.sum(np.conj(row[:, :n - D]) * row[:, D:], axis=0)
    e = 0.5 * np.sum(np.abs(row[:, :n - D]) ** 2 + np.abs(row[:, D:]) ** 2, axis=0)
    cq, ce = np.concatenate([[0], np.cumsum(q)]), np.concatenate([[0], np.cumsum(e)])
    P, E = cq[W:] - cq[:-W], ce[W:] - ce[:-W]
    m = np.where(E > 0, np.abs(P) ** 2 / np.where(E > 0, E, 1) ** 2, 0.0)
    d = int(np.argmax(m))
    return d, m, -np.angle(P[d]) / D


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    ap.add_argument("--only", default=None, help="comma-separated subset of the cases, e.g. sc2048x1,cp2048x4 (a profiler run of one case)")
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

    def roof(nbytes, ms, ref_gbs=None):
        gbs = nbytes / (ms * 1e-3) / 1e9
        r = {"achieved": gbs, "peak": HBM_PEAK, "unit": "GB/s", "frac": gbs / HBM_PEAK, "frac_copy": gbs / COPY_CEILING,
             "algorithmic_bytes_per_launch": nbytes, "bound": "HBM"}
        if ref_gbs:
            r["vs_freq_offset"] = gbs / ref_gbs
        return r

    for name, nfft, cp, D, W in FORMS:
        for nr in (1, 4):
            case = "%sx%d" % (name, nr)
            if only and case not in only:
                continue
            n = NSYM * (nfft + cp)
            nout = (NSYM - 1) * (nfft + cp)
            B = int(np.ceil(1e9 * args.scale / (nr * n * 16)))
            what = "%s nfft=%d cp=%d D=%d W=%d nr=%d n=%d" % (name, nfft, cp, D, W, nr, n)
            dev = Dev(lib)
            try:
                bits, y = dev.empty(B * nr * n * 6), dev.empty(B * nr * n * 16)
                _lib.check(lib.cpx_random_bits_dev(bits, B * nr * n * 6, 1, 0, None))
                _lib.check(lib.cpx_modulate_dev(md._device_handle(), bits, B * nr * n, y, None))
                d_hat, peak, step = dev.empty(B * 8), dev.empty(B * 8), dev.empty(B * 8)
                out = dev.empty(B * nr * nout * 16)
                st_in = dev.put(np.full(B * nr, 2 * np.pi * 1e-4))
                rot = dev.empty(B * nr * n * 16)
                # the reference point first: the rotation of the same rows
                fo = lambda: _lib.check(lib.cpx_freq_offset_dev(y, B * nr, n, st_in, 1, rot, None))
                ms, ms_min = timeit(lib, fo, steps=args.steps, warmup=args.warmup)
                fo_bytes = 2 * 16 * B * nr * n
                fo_gbs = fo_bytes / (ms * 1e-3) / 1e9
                emit({"kernel": _lib.last_kernel(), "workload": "freq_offset (reference point) " + what, "rows": B, "ms": ms, "ms_min": ms_min,
                      "dtype": "complex128", "roofline": roof(fo_bytes, ms)})
                est = lambda: _lib.check(lib.cpx_sync_estimate_dev(y, B, nr, n, D, W, 0, I64MAX, d_hat, peak, step, None))
                ms, ms_min = timeit(lib, est, steps=args.steps, warmup=args.warmup)
                emit({"kernel": _lib.last_kernel(), "workload": "sync_estimate " + what, "rows": B, "ms": ms, "ms_min": ms_min,
                      "value": B * nr * n / (ms * 1e-3), "unit": "samples/s", "dtype": "complex128", "roofline": roof(16 * B * nr * n, ms, fo_gbs)})
                ali = lambda: _lib.check(lib.cpx_sync_align_dev(y, B, nr, n, d_hat, step, -cp, nout, out, None))
                ms, ms_min = timeit(lib, ali, steps=args.steps, warmup=args.warmup)
                emit({"kernel": _lib.last_kernel(), "workload": "sync_align " + what, "rows": B, "ms": ms, "ms_min": ms_min,
                      "value": B * nr * nout / (ms * 1e-3), "unit": "output samples/s", "dtype": "complex128",
                      "roofline": roof(2 * 16 * B * nr * nout, ms, fo_gbs)})
                # what was timed, checked on the first row against the host's running-sum evaluation, itself timed
                _lib.check(lib.cpx_stream_sync(None))
                row = dev.get(y, (nr, n), complex)
                t0 = time.perf_counter()
                d_ref, m_ref, _ = host_search(row, D, W)
                host_s = time.perf_counter() - t0
                d0 = int(dev.get(d_hat, (1,), np.int64)[0])
                pk0, st0 = float(dev.get(peak, (1,), np.float64)[0]), float(dev.get(step, (1,), np.float64)[0])
                assert 0 <= d0 < len(m_ref) and abs(m_ref[d0] - pk0) < 1e-9 and m_ref[d_ref] - pk0 < 1e-9, "estimate mismatch"
                k = np.arange(nout)
                src = d0 - cp + k
                want = np.where((src >= 0) & (src < n), row[:, np.clip(src, 0, n - 1)], 0) * np.exp(1j * st0 * k)
                assert np.max(np.abs(dev.get(out, (nr, nout), complex) - want)) < 1e-9, "align mismatch"
                emit({"kernel": "cpu_baseline (numpy cumsum evaluation of one row on the host)", "workload": "sync_estimate " + what, "rows": 1,
                      "ms": host_s * 1e3, "value": nr * n / host_s, "unit": "samples/s", "dtype": "complex128",
                      "roofline": {"achieved": 16 * nr * n / host_s / 1e9, "unit": "GB/s"}})
            finally:
                dev.free()
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
