#!/usr/bin/env python3
"""Trellis-equaliser throughput (csrc/mlse.hip): device-resident inputs, HIP-event timing on the launch stream after a warm-up that
covers the clock ramp, one JSON line per case, also written to profiles/mlse_bench.jsonl.
    python benchmarks/bench_mlse.py [--scale 1.0] [--steps 5]
Cases: BPSK L = 5 with n = 148 (GSM-like), QPSK L = 4 with n = 256, 8-PSK L = 3 with n = 256, 16-QAM L = 3 with n = 256; per-row taps,
12 dB, with the tail; each hard ('indices' + 'metric') and soft (all four outputs, with a prior).  B is chosen so that a launch reads
about 1 GB of y (scale 1), or fewer rows where that would pass EVALS_PER_LAUNCH branch evaluations (a launch of about 100 ms): the
line states the bytes it read.  Rows are a base of up to 4096 noisy blocks, repeated.  Reported: time per branch evaluation,
ms / (B n S M).  After the timed region the first, middle and last rows of the timed output are compared with tests/mlse_model.py
(exactly).

Yardstick, same run: tailbiting_decode on a rate-1/2 shift-register trellis of the same state count (64 states where the equaliser
has 256: the tail-biting kernel stops there), T = n, 'unquantized', max_wraps = 1 (every row runs exactly one trip); its time per
state and candidate is ms / (B T S 2).  `candidate_ratio` = the equaliser's time per branch evaluation over that."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mlse_model as M  # noqa: E402
import tbcc_model  # noqa: E402
from commpy_amd import _lib  # noqa: E402
from commpy_amd.channelcoding import Trellis  # noqa: E402
from commpy_amd.channelcoding.convcode import device_trellis  # noqa: E402
from commpy_amd.modulation import PSKModem, QAMModem  # noqa: E402
from benchmarks.bench_kernels import timeit  # noqa: E402
from benchmarks.other_configs import Dev  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "mlse_bench.jsonl")
CASES = (("BPSK", lambda: PSKModem(2), 5, 148), ("QPSK", lambda: QAMModem(4), 4, 256), ("8-PSK", lambda: PSKModem(8), 3, 256),
         ("16-QAM", lambda: QAMModem(16), 3, 256))
YARD_GENS = {16: (0o25, 0o37), 64: (0o133, 0o171)}
BASE_ROWS, EVALS_PER_LAUNCH, NOISE_VAR = 4096, 4.0e10, 0.1


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
    with open(OUT, "w") as fh:
        for name, make, L, n in CASES:
            modem = make()
            m, Mp = modem.num_bits_symbol, modem.m
            S, n_y = Mp ** (L - 1), n + L - 1
            B = max(int(min(args.scale * 1.0e9 / (16 * n_y), args.scale * EVALS_PER_LAUNCH / (n * S * Mp))), 64)
            base = min(BASE_ROWS, B)
            dev = Dev(lib)
            try:
                # ---- the yardstick: one trip of the tail-biting decoder over a trellis of as many states (at most 64)
                Sy = min(S, 64)
                tr = Trellis(np.array([Sy.bit_length() - 1]), np.array([list(YARD_GENS[Sy])]))
                By = max(int(min(args.scale * 1.0e9 / (16 * n), args.scale * EVALS_PER_LAUNCH / (n * Sy * 2))), 64)
                words, _ = tbcc_model.encode_batch(rs.randint(0, 2, (min(BASE_ROWS, By), n)), tr)
                rx = np.resize((2.0 * words - 1.0) + 0.3 * rs.randn(*words.shape), (By, 2 * n))
                d_rx, d_bits, d_wraps = dev.put(rx), dev.empty(By * n), dev.empty(4 * By)
                y_ms, y_min = timeit(lib, lambda: _lib.check(lib.cpx_tbcc_decode_dev(device_trellis(tr), d_rx, By, n, 2, 1, d_bits, d_wraps, None,
                                                                                     None, None)),
                                     steps=args.steps, warmup=args.warmup)
                y_kernel = _lib.last_kernel()
                y_ps = y_ms * 1e9 / (By * n * Sy * 2)
                emit({"kernel": y_kernel, "workload": "yardstick: tailbiting_decode %d states, T=%d, one trip, B=%d" % (Sy, n, By), "B": By,
                      "T": n, "states": Sy, "ms": y_ms, "ms_min": y_min, "ps_per_state_candidate": y_ps, "dtype": "f64",
                      "bytes_per_launch": rx.nbytes}, fh)
                del rx
                # ---- the equaliser, hard and soft
                _, y0, h0 = M.draw(modem, L, n, base, 17 + L, True, snr_db=12.0)
                prior0 = 1.5 * rs.randn(base, n * m)
                y, h, prior = np.resize(y0, (B, n_y)), np.resize(h0, (B, L)), np.resize(prior0, (B, n * m))
                nv = np.array([NOISE_VAR])
                d_y, d_h, d_nv, d_pr = dev.put(y.view(np.float64)), dev.put(h.view(np.float64)), dev.put(nv), dev.put(prior)
                d_idx, d_bit, d_met, d_llr = dev.empty(4 * B * n), dev.empty(B * n * m), dev.empty(8 * B), dev.empty(8 * B * n * m)
                handle = modem._device_handle()
                for mode in ("hard", "soft"):
                    if mode == "hard":
                        fn = lambda: _lib.check(lib.cpx_mlse_dev(handle, d_y, d_h, 1, B, n, L, 1, None, 0, None, d_idx, None, d_met, None, None))
                    else:
                        fn = lambda: _lib.check(lib.cpx_mlse_dev(handle, d_y, d_h, 1, B, n, L, 1, d_nv, 0, d_pr, d_idx, d_bit, d_met, d_llr,
                                                                 None))
                    ms, ms_min = timeit(lib, fn, steps=args.steps, warmup=args.warmup)
                    kernel = _lib.last_kernel()
                    _lib.check(lib.cpx_stream_sync(None))
                    rows = sorted({0, 1, B // 2, B // 2 + 1, B - 2, B - 1})
                    soft = mode == "soft"
                    ref = M.equalize(y[rows], h[rows], modem.constellation, NOISE_VAR if soft else None, prior[rows] if soft else None, True,
                                     soft=soft)
                    got = {"indices": dev.get(d_idx, (B, n), np.int32)[rows], "metric": dev.get(d_met, (B,), np.float64)[rows]}
                    if soft:
                        got["bits"] = dev.get(d_bit, (B, n * m), np.uint8)[rows]
                        got["llr"] = dev.get(d_llr, (B, n * m), np.float64)[rows]
                    exact = all(np.array_equal(v.view(np.int64) if v.dtype == np.float64 else v,
                                               ref[key].view(np.int64) if v.dtype == np.float64 else ref[key]) for key, v in got.items())
                    ps = ms * 1e9 / (B * n * S * Mp)
                    ratio = ps / y_ps
                    emit({"kernel": kernel, "workload": "mlse_equalize %s L=%d n=%d, %s, B=%d" % (name, L, n, mode, B), "B": B, "n": n, "L": L,
                          "M": Mp, "states": S, "mode": mode, "ms": ms, "ms_min": ms_min, "ns_per_row": ms * 1e6 / B,
                          "ps_per_branch_evaluation": ps, "value": B * n * m / (ms * 1e-3), "unit": "bits/s",
                          "yardstick_ps_per_state_candidate": y_ps, "yardstick_states": Sy, "candidate_ratio": ratio,
                          "within_1.25x": bool(ratio <= 1.25), "dtype": "f64", "bytes_per_launch": y.nbytes,
                          "parity": {"vs": "tests/mlse_model.py", "rows": len(rows), "ok": bool(exact)}}, fh)
                    assert exact, "mlse_equalize differs from the model"
            finally:
                dev.free()


if __name__ == "__main__":
    main()
