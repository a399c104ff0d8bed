#!/usr/bin/env python3
"""A/B of the fused Viterbi kernel's OTHER 64-state 'soft' float64 flavours over two builds of the library, on the headline geometry
(65 536 codewords of 1024 bits, (133,171), 3 dB): bench.py times the Mirrored32 flavour only, and every flavour that shares cw_step
(csrc/viterbi_cw.hip) inherits a change of the step.

    python scripts/micro/argmin_flavour_ab.py --other <libcommpy_amd.so of the other build> [--rounds 5]

Each round starts one fresh process per build, the other build first (CPX_LIB_PATH), then the in-tree one, so that clock drift hits both
alike.  A process times, with HIP events on the launch stream after a warm-up, 20 launches of each flavour and prints the median:

  mirrored   tb_depth 30 (the default), B = 65 536: the headline flavour, as a cross-check against bench.py
  hops       tb_depth 15: the same ring, run-time hop count
  deep       tb_depth 40: the 64-slot ring (Deep64)
  lean       tb_depth 30, B = 65 536 + 192: the ring stored once (Lean32), with the remainder's state-per-lane kernel beside it
             (the time is the whole call's)

The parent process never touches the GPU.  Last line: per flavour the medians of both builds over the rounds, and their spreads."""
import argparse
import ctypes
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
FLAVOURS = (("mirrored", 30, 0), ("hops", 15, 0), ("deep", 40, 0), ("lean", 30, 192))


def child():
    from commpy_amd import _lib
    from commpy_amd.channelcoding import Trellis, conv_encode_batch
    from benchmarks.other_configs import Dev, warm
    lib = _lib.load()
    _lib.require_device()
    tr = Trellis(np.array([6]), np.array([[0o133, 0o171]]))
    rs = np.random.RandomState(4)
    B0 = 65536 + 192
    coded = conv_encode_batch(rs.randint(0, 2, (B0, 1024)).astype(np.uint8), tr).astype(np.float64)
    sigma2 = 1.0 / (2.0 * 0.5 * 10.0 ** 0.3)                             # 3 dB, rate 1/2: LLR = 2 y / sigma^2
    llr = np.ascontiguousarray(2.0 * ((2.0 * coded - 1.0) + rs.standard_normal(coded.shape) * np.sqrt(sigma2)) / sigma2)
    dev = Dev(lib)
    d_in, d_out = dev.put(llr), dev.empty(B0 * 1030)
    h = tr._device_handle()
    tm = ctypes.c_void_p()
    _lib.check(lib.cpx_timer_create(ctypes.byref(tm)))
    res = {}
    for name, tb, extra in FLAVOURS:
        B = 65536 + extra

        def fn():
            _lib.check(lib.cpx_viterbi_decode_batch_dev(h, d_in, B, 2060, 1030, 1030, tb, 1, d_out, None))
        warm(lib, fn, 3)
        ms = []
        for _ in range(20):
            _lib.check(lib.cpx_timer_start(tm, None))
            fn()
            _lib.check(lib.cpx_timer_stop(tm, None))
            v = ctypes.c_float()
            _lib.check(lib.cpx_timer_elapsed_ms(tm, ctypes.byref(v)))
            ms.append(v.value)
        res[name] = {"ms_median": round(float(np.median(ms)), 4), "kernel": _lib.last_kernel()}
    lib.cpx_timer_destroy(tm)
    dev.free()
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--other", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child()
    arms = (("other", os.path.abspath(a.other)), ("tree", None)) if a.other else (("tree", None),)
    runs = {arm: {f[0]: [] for f in FLAVOURS} for arm, _ in arms}
    for r in range(a.rounds):
        for arm, path in arms:
            env = dict(os.environ)
            env.pop("CPX_LIB_PATH", None)
            if path:
                env["CPX_LIB_PATH"] = path
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, capture_output=True, text=True, timeout=240)
            if out.returncode != 0:                                      # nothing more is started on the GPU after a failure
                sys.exit("round %d, %s: exit %d\n%s" % (r + 1, arm, out.returncode, out.stderr[-2000:]))
            j = json.loads(out.stdout.strip().split("\n")[-1])
            print(json.dumps({"round": r + 1, "lib": arm, **{k: v["ms_median"] for k, v in j.items()}}), flush=True)
            if r == 0:
                print(json.dumps({"lib": arm, "kernels": {k: v["kernel"] for k, v in j.items()}}), flush=True)
            for k, v in j.items():
                runs[arm][k].append(v["ms_median"])
    print(json.dumps({arm: {k: {"median": round(float(np.median(v)), 4), "spread": round(max(v) - min(v), 4)} for k, v in fl.items()}
                      for arm, fl in runs.items()}))


if __name__ == "__main__":
    main()
