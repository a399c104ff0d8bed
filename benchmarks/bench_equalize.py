#!/usr/bin/env python3
"""MMSE linear / decision-feedback equaliser throughput (csrc/equalize.hip): device-resident inputs, HIP-event timing on the launch
stream after a warm-up that covers the clock ramp, one JSON line per case, also written to profiles/equalize_bench.jsonl.
    python benchmarks/bench_equalize.py [--scale 1.0] [--steps 5]
Cases: QPSK and 64-QAM through L = 8 taps, nf = 32, n = 256, 12 dB, with the tail; the linear equaliser (nb = 0) and the feedback
equaliser with nb = 7; per-row taps, hard ('indices') and soft ('indices', 'bits', 'llr'); the design alone
(want = 'ff', 'fb', 'gain', 'noise'); and shared taps once per constellation (one design, hard).  B is chosen so that a launch reads about 1 GB of y
(scale 1).  Rows are a base of up to 4096 noisy blocks, repeated.  After the timed region the first, middle and last rows of the timed
output are compared with tests/equalize_model.py (exactly).

Yardsticks, same run, never the code under test:
  cpx_multipath_dev at 1x1 with L = nf taps on as many rows of n symbols: its time per complex multiply-add, ms / (B n nf).  The
      equaliser's filtering time is the hard linear call with shared taps, where the design is one row's: `mac_ratio` is its time per
      complex multiply-add over the yardstick's (the scan of y for NaN and the slicer's M points per symbol ride in the numerator).
      The hard per-row call minus the design-alone call of the same rows is given beside it (`..._by_difference`).
  cpx_mimo_linear_dev (MMSE, hard) at nr = nt = 32, the wave kernel, on about 1 GB of H: its time per row and nt^3.  `design_ratio` is
      the design-alone time per row and nf^3 over that.
The feedback pass has no sibling: what a call takes beyond the design-alone call of the same rows (feed-forward sums through the
arena plus the recursion) is reported per symbol, and per symbol and feedback tap, beside the linear equaliser's."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import equalize_model as E  # noqa: E402
from mlse_model import draw  # noqa: E402
from commpy_amd import _lib  # noqa: E402
from commpy_amd.equalizers import MMSE_WANT  # noqa: E402
from commpy_amd.modulation import QAMModem  # noqa: E402
from benchmarks.bench_kernels import timeit  # noqa: E402
from benchmarks.other_configs import Dev  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "equalize_bench.jsonl")
L, NF, NB, N, BASE_ROWS, SNR_DB = 8, 32, 7, 256, 4096, 12.0
MIMO_NT = 32
MODES = {"hard": ("indices",), "soft": ("indices", "bits", "llr"), "design": ("ff", "fb", "gain", "noise")}


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
    rs = np.random.RandomState(0)
    n_y = N + L - 1
    B = max(int(args.scale * 1.0e9 / (16 * n_y)), 64)
    with open(OUT, "w") as fh:
        # ---- yardstick 1: the multipath channel, 1x1, nf taps per row
        dev = Dev(lib)
        try:
            x = np.resize(rs.randn(BASE_ROWS, N) + 1j * rs.randn(BASE_ROWS, N), (B, N))
            g = np.resize(rs.randn(BASE_ROWS, NF) + 1j * rs.randn(BASE_ROWS, NF), (B, NF))
            d_x, d_g, d_o = dev.put(x.view(np.float64)), dev.put(g.view(np.float64)), dev.empty(16 * B * (N + NF - 1))
            mp_ms, mp_min = timeit(lib, lambda: _lib.check(lib.cpx_multipath_dev(d_x, d_g, 1, B, 1, 1, N, NF, d_o, None)), steps=args.steps,
                                   warmup=args.warmup)
            mp_ps = mp_ms * 1e9 / (B * N * NF)
            emit({"kernel": _lib.last_kernel(), "workload": "yardstick: multipath 1x1, L=%d, n=%d, B=%d" % (NF, N, B), "B": B, "n": N,
                  "L": NF, "ms": mp_ms, "ms_min": mp_min, "ps_per_complex_mac": mp_ps, "dtype": "f64", "bytes_per_launch": x.nbytes}, fh)
            del x, g
        finally:
            dev.free()
        # ---- yardstick 2: the linear MIMO detector's wave kernel, one 32 x 32 solve per row
        dev = Dev(lib)
        try:
            qpsk = QAMModem(4)
            Bm = max(int(args.scale * 1.0e9 / (16 * MIMO_NT * MIMO_NT)), 64)
            base = min(BASE_ROWS, Bm)
            H = np.resize((rs.randn(base, MIMO_NT, MIMO_NT) + 1j * rs.randn(base, MIMO_NT, MIMO_NT)) / np.sqrt(2), (Bm, MIMO_NT, MIMO_NT))
            ym = np.resize(rs.randn(base, MIMO_NT) + 1j * rs.randn(base, MIMO_NT), (Bm, MIMO_NT))
            d_ym, d_H, d_i = dev.put(ym.view(np.float64)), dev.put(H.view(np.float64)), dev.empty(4 * Bm * MIMO_NT)
            ml_ms, ml_min = timeit(lib, lambda: _lib.check(lib.cpx_mimo_linear_dev(qpsk._device_handle(), d_ym, d_H, 1, Bm, MIMO_NT, MIMO_NT,
                                                                                   0.05, 0.1, d_i, None, None, None, None)),
                                   steps=args.steps, warmup=args.warmup)
            ml_ps = ml_ms * 1e9 / (Bm * MIMO_NT ** 3)
            emit({"kernel": _lib.last_kernel(), "workload": "yardstick: mimo_linear MMSE hard %dx%d QPSK, B=%d" % (MIMO_NT, MIMO_NT, Bm),
                  "B": Bm, "nt": MIMO_NT, "ms": ml_ms, "ms_min": ml_min, "ns_per_row": ml_ms * 1e6 / Bm, "ps_per_row_nt3": ml_ps,
                  "dtype": "f64", "bytes_per_launch": H.nbytes}, fh)
            del H, ym
        finally:
            dev.free()
        # ---- the equalisers
        for name, M_ in (("QPSK", 4), ("64-QAM", 64)):
            modem = QAMModem(M_)
            m = modem.num_bits_symbol
            dev = Dev(lib)
            try:
                base = min(BASE_ROWS, B)
                _, y0, h0 = draw(modem, L, N, base, 23 + M_, True, snr_db=SNR_DB)
                h0[:, 0] += 1.0
                y0 = np.stack([np.convolve(modem.constellation[rs.randint(0, M_, N)], hb) for hb in h0])
                nv = np.array([modem.Es / 10 ** (SNR_DB / 10)])
                y0 = y0 + np.sqrt(nv[0] / 2) * (rs.randn(*y0.shape) + 1j * rs.randn(*y0.shape))
                y, h = np.resize(y0, (B, n_y)), np.resize(h0, (B, L))
                d_y, d_h, d_nv = dev.put(y.view(np.float64)), dev.put(h.view(np.float64)), dev.put(nv)
                sizes = {"indices": 4 * B * N, "bits": B * N * m, "llr": 8 * B * N * m, "ff": 16 * B * NF, "fb": 16 * B * NB, "gain": 8 * B,
                         "noise": 8 * B}
                shapes = {"indices": ((B, N), np.int32), "bits": ((B, N * m), np.uint8), "llr": ((B, N * m), np.float64),
                          "ff": ((B, NF), np.complex128), "gain": ((B,), np.float64), "noise": ((B,), np.float64)}
                bufs = {key: dev.empty(v) for key, v in sizes.items()}
                handle = modem._device_handle()
                rows = sorted({0, 1, B // 2, B // 2 + 1, B - 2, B - 1})
                times = {}
                runs = [(nb, mode, 1) for nb in (0, NB) for mode in ("design", "hard", "soft")]
                runs.append((0, "hard", 0))
                for nb, mode, per_row in runs:
                    want = MODES[mode]
                    outs = [bufs[key] if key in want else None for key in MMSE_WANT]
                    fn = lambda: _lib.check(lib.cpx_mmse_equalize_dev(handle, float(modem.Es), d_y, d_h, per_row, B, N, L, 1, d_nv, 0, NF, nb,
                                                                      (NF + L - 2) // 2 if nb == 0 else NF - 1, *outs, None))
                    ms, ms_min = timeit(lib, fn, steps=args.steps, warmup=args.warmup)
                    kernel = _lib.last_kernel()
                    _lib.check(lib.cpx_stream_sync(None))
                    ref = E.equalize(y[rows], h[rows] if per_row else h[0], modem.constellation, modem.Es, nv[0], NF, nb)
                    shapes["fb"] = ((B, nb), np.complex128)
                    exact = True
                    for key in want:
                        if key == "fb" and nb == 0:
                            continue
                        got = dev.get(bufs[key], *shapes[key])[rows]
                        exact &= bool(np.array_equal(got.view(np.int64) if got.dtype.kind in "fc" else got,
                                                     ref[key].view(np.int64) if got.dtype.kind in "fc" else ref[key]))
                    times[(nb, mode, per_row)] = ms
                    line = {"kernel": kernel, "workload": "mmse_equalize %s L=%d nf=%d nb=%d n=%d, %s, %s taps, B=%d"
                            % (name, L, NF, nb, N, mode, "per-row" if per_row else "shared", B), "B": B, "n": N, "L": L, "nf": NF, "nb": nb,
                            "M": M_, "mode": mode, "per_row_taps": bool(per_row), "ms": ms, "ms_min": ms_min, "ns_per_row": ms * 1e6 / B,
                            "dtype": "f64", "bytes_per_launch": y.nbytes,
                            "parity": {"vs": "tests/equalize_model.py", "rows": len(rows), "ok": exact}}
                    if mode == "design":
                        ps = ms * 1e9 / (B * NF ** 3)
                        line.update({"ps_per_row_nf3": ps, "yardstick_ps_per_row_nt3": ml_ps, "design_ratio": ps / ml_ps,
                                     "within_1.25x": bool(ps / ml_ps <= 1.25)})
                    else:
                        line.update({"value": B * N * m / (ms * 1e-3), "unit": "bits/s", "ns_per_symbol": ms * 1e6 / (B * N)})
                        if not per_row:
                            ps = ms * 1e9 / (B * N * NF)
                            line.update({"ps_per_complex_mac": ps, "yardstick_ps_per_complex_mac": mp_ps, "mac_ratio": ps / mp_ps,
                                         "within_1.25x": bool(ps / mp_ps <= 1.25),
                                         "ps_per_complex_mac_by_difference": (times[(0, "hard", 1)] - times[(0, "design", 1)]) * 1e9 / (B * N * NF)})
                        else:
                            rest = ms - times[(nb, "design", 1)]
                            line.update({"ms_beyond_design": rest, "ns_per_symbol_beyond_design": rest * 1e6 / (B * N)})
                            if nb:
                                line["ns_per_symbol_and_feedback_tap_beyond_design"] = rest * 1e6 / (B * N * nb)
                    emit(line, fh)
                    assert exact, "mmse_equalize differs from the model"
            finally:
                dev.free()


if __name__ == "__main__":
    main()
