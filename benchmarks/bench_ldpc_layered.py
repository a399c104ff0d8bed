#!/usr/bin/env python3
"""Layered min-sum LDPC decoding (csrc/ldpc_layered.hip) against the flooding min-sum decoder: device-resident inputs, HIP-event timing on
the launch stream after a warm-up that covers the clock ramp, one JSON line per case, also written to profiles/ldpc_layered_bench.jsonl.
    python benchmarks/bench_ldpc_layered.py [--scale 1.0] [--steps 5]
Code: (1944,1296), B = 32 768 random code words (systematic, GF(2) generator) over BPSK / AWGN at Eb/N0 = 3.0 and 2.2 dB.

Yardstick, same run, same LLRs: ``ldpc_bp_decode``'s min-sum on its 'resident' path (cpx_ldpc_bp_decode_batch_bm_dev, forced).
1. Time per block-iteration: layered with early_stop off and 20 iterations, ms / (20 B); flooding capped at 20 iterations (it always
   stops early), ms / (sum of executed iterations), on the 2.2 dB LLRs.  `iteration_ratio` = layered / flooding; above 1.25 is a defect.
2. Decode time, mean iterations, bit and block error rates with at most 50 iterations at both SNRs: flooding min-sum, layered alpha = 1,
   layered alpha = 0.75.  `time_ratio` = layered / flooding; not below 1 is a defect.
After each timed region rows of the layered output are compared with tests/ldpc_layered_model.py (exactly)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ldpc_layered_model as M  # noqa: E402
from commpy_amd import _lib, deviceops  # noqa: E402
from commpy_amd.channelcoding import get_ldpc_code_params, ldpc_layers  # noqa: E402
from commpy_amd.channelcoding import ldpc as ldpc_mod  # noqa: E402
from commpy_amd.channelcoding import ldpc_layered as LL  # noqa: E402
from benchmarks.bench_bch import sample  # noqa: E402
from benchmarks.bench_kernels import timeit  # noqa: E402
from benchmarks.other_configs import Dev  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "ldpc_layered_bench.jsonl")
DESIGN = os.path.join(ROOT, "commpy_amd", "channelcoding", "designs", "ldpc", "ieee80211n", "1944.1296.txt")
MSA, CAP_ITERS, FIXED_ITERS = 1, 50, 20


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
    p = get_ldpc_code_params(DESIGN)
    n_v, n_c = p["n_vnodes"], p["n_cnodes"]
    k = n_v - n_c
    B = max(int(32768 * args.scale), 64)
    P = deviceops.gf2_generator(p).astype(np.int64)                              # [m, k]
    base = rs.randint(0, 2, (min(B, 4096), k))
    words = np.resize(np.concatenate([base, base.dot(P.T) % 2], axis=1).astype(np.int8), (B, n_v))
    code = M.code_from_params(p)
    layers = ldpc_layers(p)
    assert not M.syndrome(code, words[:64].astype(bool)).any()
    plan = LL.plan(p)
    h_lay, h_flood = plan.handle(), ldpc_mod._device_code(p)
    what = "(1944,1296), B=%d" % B
    dev = Dev(lib)
    with open(OUT, "w") as fh:
        try:
            d_llr = dev.empty(8 * B * n_v)
            d_bits, d_out, d_it, d_cv = dev.empty(B * n_v), dev.empty(8 * B * n_v), dev.empty(4 * B), dev.empty(B)

            def errors(bits):
                wrong = bits != words
                return float(wrong.mean()), float(wrong.any(axis=1).mean())

            def flooding(n_iters, ebn0):
                # the flooding decoder clips its input in place, to +-500: these LLRs stay far inside (asserted below), so that it rewrites
                # nothing and both decoders read the very same buffer
                with _lib.forced_path("ldpc", "resident"):
                    ms, ms_min = timeit(lib, lambda: _lib.check(lib.cpx_ldpc_bp_decode_batch_bm_dev(h_flood, d_llr, B, MSA, n_iters, d_bits, d_out,
                                                                                                    d_it, None)),
                                        steps=args.steps, warmup=args.warmup)
                    kernel = _lib.last_kernel()
                _lib.check(lib.cpx_stream_sync(None))
                assert "ldpc_resident_kernel" in kernel, kernel
                its = dev.get(d_it, (B,), np.int32)
                ber, bler = errors(dev.get(d_bits, (B, n_v), np.int8))
                d = {"kernel": kernel, "workload": "yardstick: ldpc_bp_decode min-sum 'resident', %s, %g dB, at most %d iterations" % (what, ebn0, n_iters),
                     "B": B, "ebn0_db": ebn0, "max_iters": n_iters, "ms": ms, "ms_min": ms_min, "mean_iters": float(its.mean()),
                     "sum_iters": int(its.sum()), "ns_per_block_iteration": ms * 1e6 / int(its.sum()), "ber": ber, "bler": bler, "dtype": "f64"}
                emit(d, fh)
                return d

            def layered(n_iters, ebn0, alpha, early_stop):
                ms, ms_min = timeit(lib, lambda: _lib.check(lib.cpx_ldpc_layered_decode_dev(h_lay, d_llr, B, n_iters, alpha, 0.0, 1 if early_stop else 0,
                                                                                            500.0, d_bits, d_out, d_it, d_cv, None)),
                                    steps=args.steps, warmup=args.warmup)
                kernel = _lib.last_kernel()
                _lib.check(lib.cpx_stream_sync(None))
                got = {"bits": dev.get(d_bits, (B, n_v), np.int8), "llr": dev.get(d_out, (B, n_v), np.float64), "iters": dev.get(d_it, (B,), np.int32),
                       "converged": dev.get(d_cv, (B,), np.uint8)}
                idx = sample(B, 3)
                ref = M.decode(llr[idx], code, layers, n_iters, alpha, 0.0, early_stop)
                exact = all(np.array_equal(got[key][idx].view(np.int64) if key == "llr" else got[key][idx],
                                           ref[key].view(np.int64) if key == "llr" else ref[key]) for key in got)
                ber, bler = errors(got["bits"])
                total = int(got["iters"].sum())
                d = {"kernel": kernel, "workload": "ldpc_layered_decode alpha=%g, %s, %g dB, %s %d iterations" %
                     (alpha, what, ebn0, "at most" if early_stop else "exactly", n_iters), "B": B, "ebn0_db": ebn0, "alpha": alpha, "beta": 0.0,
                     "early_stop": bool(early_stop), "max_iters": n_iters, "ms": ms, "ms_min": ms_min, "mean_iters": total / B, "sum_iters": total,
                     "ns_per_block_iteration": ms * 1e6 / total, "converged_share": float(got["converged"].mean()), "ber": ber, "bler": bler,
                     "value": B * k / (ms * 1e-3), "unit": "info-bits/s", "dtype": "f64",
                     "parity": {"vs": "tests/ldpc_layered_model.py", "rows": len(idx), "ok": bool(exact)}}
                emit(d, fh)
                assert exact, "ldpc_layered_decode differs from the model"
                return d

            for ebn0 in (3.0, 2.2):
                sigma2 = 1.0 / (2.0 * (k / n_v) * 10.0 ** (ebn0 / 10.0))
                llr = 2.0 * (1.0 - 2.0 * words + np.sqrt(sigma2) * rs.randn(B, n_v)) / sigma2
                assert np.abs(llr).max() < 500.0
                _lib.check(lib.cpx_memcpy_h2d(d_llr, _lib.ptr(llr), llr.nbytes))
                if ebn0 == 2.2:
                    f = flooding(FIXED_ITERS, ebn0)
                    l = layered(FIXED_ITERS, ebn0, 1.0, False)
                    ratio = l["ns_per_block_iteration"] / f["ns_per_block_iteration"]
                    emit({"summary": "time per block-iteration, %s, 2.2 dB, %d iterations" % (what, FIXED_ITERS),
                          "layered_ns": l["ns_per_block_iteration"], "flooding_ns": f["ns_per_block_iteration"], "iteration_ratio": ratio,
                          "within_1.25x": bool(ratio <= 1.25)}, fh)
                f = flooding(CAP_ITERS, ebn0)
                for alpha in (1.0, 0.75):
                    l = layered(CAP_ITERS, ebn0, alpha, True)
                    emit({"summary": "decode, %s, %g dB, at most %d iterations, layered alpha=%g against flooding" % (what, ebn0, CAP_ITERS, alpha),
                          "ebn0_db": ebn0, "alpha": alpha, "layered_ms": l["ms"], "flooding_ms": f["ms"], "time_ratio": l["ms"] / f["ms"],
                          "faster": bool(l["ms"] < f["ms"]), "iters_ratio": l["mean_iters"] / f["mean_iters"],
                          "bler_layered": l["bler"], "bler_flooding": f["bler"], "ber_layered": l["ber"], "ber_flooding": f["ber"],
                          "bound": "inferred, no counter pass"}, fh)
        finally:
            dev.free()


if __name__ == "__main__":
    main()
