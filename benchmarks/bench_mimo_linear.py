#!/usr/bin/env python3
"""Linear MIMO detection throughput (csrc/mimo_linear.hip): device-resident inputs, HIP-event timing on the launch stream after a
warm-up that covers the clock ramp, at least 1 GB moved per launch.  One JSON line per case, also appended to --out.
    python benchmarks/bench_mimo_linear.py [--scale 1.0] [--out profiles/mimo_linear_bench.jsonl]
  4x4 (B = 2^22 vectors, 2^24 with a shared H) and 8x8 (2^20, 2^23), QPSK / 16-QAM / 64-QAM, hard and soft output, one H per
  vector and one shared H.
  Per case: time, vectors/s and the fraction of the HBM peak on ALGORITHMIC bytes, (nr nt + nr) 16 + output bytes per vector (a shared
  H counted once).  In the same run, on the same device buffers, cpx_kbest_hard_dev / cpx_kbest_soft_dev at K = 16 for every case
  with one H per vector, so that the ratio has one provenance; then DeviceMimoLink with 'mmse' beside 'kbest' (uncoded 4x4 16-QAM).
  --pmc-case runs the 4x4 16-QAM soft case alone, a few launches: the target of a rocprofv3 --pmc pass of its own.
The detector's outputs are checked against the single-vector API after the timed region."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from commpy_amd import _lib  # noqa: E402
from benchmarks.bench_kernels import timeit  # noqa: E402
from benchmarks.other_configs import Dev  # noqa: E402

HBM_PEAK = 8.0e12            # bytes/s, spec; the project's target is half of it
_out = None


def emit(d):
    d["build_id"] = _lib.build_id().get("full")
    line = json.dumps(d)
    print(line, flush=True)
    if _out:
        with open(_out, "a") as f:
            f.write(line + "\n")


_draws = {}


def problem(rs, B, nr, nt, md, shared):
    """y = H x + noise; the Gaussian draws of one (shape, B, shared) are made once and reused for every constellation."""
    key = (B, nr, nt, shared)
    if key not in _draws:
        _draws.clear()
        n = 1 if shared else B
        h = (rs.standard_normal((n, nr, nt)) + 1j * rs.standard_normal((n, nr, nt))) / np.sqrt(2)
        noise = (rs.standard_normal((B, nr)) + 1j * rs.standard_normal((B, nr))) / np.sqrt(2)
        _draws[key] = (h, noise)
    h, noise = _draws[key]
    x = md.constellation[rs.randint(0, md.m, (B, nt))]
    y = np.matmul(h, x[:, :, None])[:, :, 0] + 0.3 * np.sqrt(md.Es) * noise
    return np.ascontiguousarray(y), np.ascontiguousarray(h[0] if shared else h)


def check(md, y, h, reg, noise_var, got_idx, got_llr, rs):
    from commpy_amd.modulation import mmse_detector
    pick = rs.choice(len(got_idx if got_idx is not None else got_llr), 16, replace=False)     # among the downloaded head of the batch
    ok = True
    for b in pick:
        hb = h if h.ndim == 2 else h[b]
        if got_idx is not None:
            ok &= bool(np.array_equal(mmse_detector(y[b], hb, md.constellation, noise_var), md.constellation[got_idx[b]]))
        if got_llr is not None:
            ok &= bool(np.array_equal(mmse_detector(y[b], hb, md.constellation, noise_var, 'soft'), got_llr[b]))
    return ok


def bench_case(lib, rs, nr, nt, m, B, shared, modes, steps, warmup, with_kbest):
    from commpy_amd.modulation import QAMModem
    md = QAMModem(m)
    nb = md.num_bits_symbol
    y, h = problem(rs, B, nr, nt, md, shared)
    noise_var = 0.09 * md.Es
    reg = noise_var / md.Es                      # mmse_detector's regulariser, so that the check can use it
    dev = Dev(lib)
    dy, dh = dev.put(y), dev.put(h)
    didx, dllr = dev.empty(4 * B * nt), dev.empty(8 * B * nt * nb)
    mh = md._device_handle()
    in_bytes = 16 * (B * nr + (1 if shared else B) * nr * nt)
    times = {}
    for mode in modes:
        out_bytes = 4 * B * nt if mode == "hard" else 8 * B * nt * nb

        def run():
            _lib.check(lib.cpx_mimo_linear_dev(mh, dy, dh, int(not shared), B, nr, nt, reg, noise_var,
                                               didx if mode == "hard" else None, dllr if mode == "soft" else None, None, None, None))
        ms, ms_min = timeit(lib, run, steps=steps, warmup=warmup)
        kernel = _lib.last_kernel()
        head = min(B, 1 << 16)
        got_idx = dev.get(didx, (head, nt), np.int32) if mode == "hard" else None
        got_llr = dev.get(dllr, (head, nt * nb), np.float64) if mode == "soft" else None
        ok = check(md, y, h, reg, noise_var, got_idx, got_llr, rs)
        nbytes = in_bytes + out_bytes
        times[mode] = ms
        emit({"kernel": "mimo_linear_%s" % mode, "workload": "%dx%d %d-QAM MMSE, B=%d, %s" % (nr, nt, m, B, "shared H" if shared else "H per vector"),
              "value": B / (ms * 1e-3), "unit": "vectors/s", "ms": ms, "ms_min": ms_min, "dtype": "f64",
              "roofline": {"bound": "HBM", "algorithmic_bytes": nbytes, "achieved": nbytes / (ms * 1e-3) / 1e12, "peak": HBM_PEAK / 1e12,
                           "unit": "TB/s", "frac": nbytes / (ms * 1e-3) / HBM_PEAK, "target_frac": 0.5},
              "check_ok": ok, "kernel_path": kernel})
    if with_kbest:
        for mode in modes:
            if mode == "hard":
                def run():
                    _lib.check(lib.cpx_kbest_hard_dev(mh, dy, dh, 1, B, nr, nt, 16, didx, None))
            else:
                def run():
                    _lib.check(lib.cpx_kbest_soft_dev(mh, dy, dh, 1, B, nr, nt, 16, noise_var, dllr, None))
            ms, ms_min = timeit(lib, run, steps=2, warmup=1)
            emit({"kernel": "kbest_%s" % mode, "workload": "%dx%d %d-QAM K=16, B=%d, H per vector (the linear case's inputs)" % (nr, nt, m, B),
                  "value": B / (ms * 1e-3), "unit": "vectors/s", "ms": ms, "ms_min": ms_min, "dtype": "f64",
                  "kernel_path": _lib.last_kernel(), "linear_ms": times[mode], "kbest_over_linear": ms / times[mode]})
    dev.free()


def bench_link(steps):
    from commpy_amd.channels import MIMOFlatChannel
    from commpy_amd.devicelink import DeviceMimoLink
    from commpy_amd.modulation import QAMModem
    md = QAMModem(16)
    for detector in ("kbest", "mmse"):
        ch = MIMOFlatChannel(4, 4)
        ch.uncorr_rayleigh_fading(complex)
        link = DeviceMimoLink(md, ch, detector=detector, K=16, send_chunk=720)
        T = link.tx_batch
        link.run_batch(12.0, T)
        link.run_batch(12.0, T)
        t = []
        for _ in range(steps):
            t0 = time.perf_counter()
            errs = link.run_batch(12.0, T)              # ends in a stream synchronise
            t.append(time.perf_counter() - t0)
        ms = 1e3 * float(np.mean(t))
        emit({"kernel": "DeviceMimoLink_%s" % detector, "workload": "uncoded 4x4 16-QAM at 12 dB, %d transmissions of 720 bits" % T,
              "value": T * link.vectors_per_tx / (ms * 1e-3), "unit": "vectors/s", "ms": ms, "ms_min": 1e3 * min(t),
              "timing": "host clock around run_batch (whole batch: source, channel, detector, count)",
              "ber": float(errs.sum()) / (T * link.send_chunk)})


def main():
    global _out
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    ap.add_argument("--pmc-case", action="store_true", help="only the 4x4 16-QAM soft case, H per vector (the counter run's target)")
    ap.add_argument("--no-kbest", action="store_true")
    ap.add_argument("--no-link", action="store_true")
    a = ap.parse_args()
    _out = a.out
    lib = _lib.load()
    _lib.require_device()
    rs = np.random.RandomState(12)
    if a.pmc_case:
        bench_case(lib, rs, 4, 4, 16, int((1 << 22) * a.scale), False, ("soft",), 2, 1, False)
        return
    # batch sizes that move at least 1 GB per launch in every case: a shared H leaves 16 nr bytes of input per vector
    for nr, nt, B_own, B_shared in ((4, 4, 1 << 22, 1 << 24), (8, 8, 1 << 20, 1 << 23)):
        for shared in (False, True):
            for m in (4, 16, 64):
                bench_case(lib, rs, nr, nt, m, int((B_shared if shared else B_own) * a.scale), shared, ("hard", "soft"), a.steps,
                           a.warmup, not shared and not a.no_kbest)
    if not a.no_link:
        bench_link(3)


if __name__ == "__main__":
    main()
