#!/usr/bin/env python3
"""A/B over two builds of the library of the fused Viterbi kernel's flavours that bench.py and argmin_flavour_ab.py do not time: the ones
WITHOUT the 32-bit first-argmin ('hard', 'unquantized', the table-driven form, the small rings), whose traceback hops run in four batches
between the phases of the step (csrc/viterbi_cw.hip, WalkHook, LATE = false).  65 536 codewords of 1024 bits, 3 dB, forced codeword path.

    python scripts/micro/walk_flavour_ab.py --other <libcommpy_amd.so of the other build> [--rounds 5]

Each round starts one fresh process per build, the other build first (CPX_LIB_PATH), then the in-tree one.  A process times, with HIP
events after a warm-up, 20 launches of each flavour and prints the median.  Flavours: name = code, decoding type, tb_depth
(default depth = compile-time hops; below it = run-time hops; K = 7 above 30 = 64-slot ring).
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
K7, T135, K3, K5 = (6, (0o133, 0o171)), (6, (0o135, 0o147)), (2, (5, 7)), (4, (0o23, 0o35))
# name, (memory, generators), decoding type (0 hard, 1 soft, 2 unquantized), tb_depth
FLAVOURS = (("k7_hard", K7, 0, 30), ("k7_hard_hops", K7, 0, 15), ("k7_hard_deep", K7, 0, 40), ("k7_unq", K7, 2, 30), ("k7_unq_deep", K7, 2, 40),
            ("table_soft", T135, 1, 30), ("table_soft_hops", T135, 1, 15), ("table_hard", T135, 0, 30),
            ("k3_hard", K3, 0, 10), ("k3_hard_hops", K3, 0, 6), ("k5_soft", K5, 1, 20), ("k5_soft_hops", K5, 1, 12))


def child():
    from commpy_amd import _lib
    from commpy_amd.channelcoding import Trellis, conv_encode_batch
    from benchmarks.other_configs import Dev, warm
    lib = _lib.load()
    _lib.require_device()
    B = 65536
    sigma2 = 1.0 / (2.0 * 0.5 * 10.0 ** 0.3)                             # 3 dB, rate 1/2: LLR = 2 y / sigma^2
    tm = ctypes.c_void_p()
    _lib.check(lib.cpx_timer_create(ctypes.byref(tm)))
    res, data = {}, {}
    for name, (mem, gen), vtype, tb in FLAVOURS:
        tr = Trellis(np.array([mem]), np.array([list(gen)]))
        if (mem, gen) not in data:
            rs = np.random.RandomState(4 + mem)
            coded = conv_encode_batch(rs.randint(0, 2, (B, 1024)).astype(np.uint8), tr).astype(np.float64)
            data[(mem, gen)] = (2.0 * coded - 1.0) + rs.standard_normal(coded.shape) * np.sqrt(sigma2)
        y = data[(mem, gen)]
        rx = np.ascontiguousarray((y > 0).astype(np.float64) if vtype == 0 else 2.0 * y / sigma2 if vtype == 1 else y)
        L = 1024 + mem
        dev = Dev(lib)
        d_in, d_out = dev.put(rx), dev.empty(B * L)
        h = tr._device_handle()

        def fn():
            _lib.check(lib.cpx_viterbi_decode_batch_dev(h, d_in, B, 2 * L, L, L, tb, vtype, d_out, None))
        with _lib.forced_path("viterbi", "cw!"):
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
        dev.free()
    lib.cpx_timer_destroy(tm)
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
