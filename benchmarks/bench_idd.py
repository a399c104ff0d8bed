#!/usr/bin/env python3
"""Iterative detection and decoding on the device (DeviceMimoLink(idd_iters=...), csrc/mimo_idd.hip).  One JSON line per case,
also appended to profiles/idd_bench.jsonl:
    python benchmarks/bench_idd.py [--steps 3] [--host-tx 2] [--snr 18]
  link      4x4 16-QAM, K = 16, WiMAX (1440,720) LDPC, MSA 15 iterations, 720 bits per transmission, idd_iters in 0..3 ('decode'
            decision): info-bit/s of whole run_batch calls of the default tx_batch (HIP events, after a warm-up batch),
            `stages_ms` by events around each stage ('list' = search, distances and first pass; 'idd' = the rounds)
  exchange  idd_exchange_kernel alone over 2^22 vectors (3.2 GB of algorithmic traffic per launch): cand (int32) and dist read, the
            decoder's input and output read, the input rewritten -- `alg_bytes`, achieved GB/s and the fraction of the HBM peak
  list_llr, list_dist  the other two kernels on the same batch
  host      one transmission through links.idd_decoder + apriori_detector + the engine's ldpc_bp_decode (wall clock), and its
            ratio to the device link's time per transmission at the same idd_iters; the first transmission runs once untimed before."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))      # helpers.ldpc_params: the WiMAX design, as benchmarks/bench_mimo_link.py

from commpy_amd import _lib  # noqa: E402

HBM_PEAK = 8000.0            # GB/s, MI355X spec
OUT = os.path.join(ROOT, "profiles", "idd_bench.jsonl")


def emit(d):
    d["build_id"] = _lib.build_id().get("full")
    line = json.dumps(d)
    print(line, flush=True)
    with open(OUT, "a") as f:
        f.write(line + "\n")


class Timers:
    """HIP event pairs by name (DeviceMimoLink's `mark` hook, or around a single launch)."""

    def __init__(self, lib):
        self.lib, self.t, self.used = lib, {}, []

    def __call__(self, name, start):
        if name not in self.t:
            h = ctypes.c_void_p()
            _lib.check(self.lib.cpx_timer_create(ctypes.byref(h)))
            self.t[name] = h
        _lib.check((self.lib.cpx_timer_start if start else self.lib.cpx_timer_stop)(self.t[name], None))
        if start:
            self.used.append(name)

    def read(self):
        _lib.check(self.lib.cpx_stream_sync(None))
        out = {}
        for name in self.used:
            v = ctypes.c_float()
            _lib.check(self.lib.cpx_timer_elapsed_ms(self.t[name], ctypes.byref(v)))
            out[name] = v.value
        self.used = []
        return out


def _chan():
    from commpy_amd.channels import MIMOFlatChannel
    c = MIMOFlatChannel(4, 4)
    c.uncorr_rayleigh_fading(complex)
    return c


def kernels(lib, steps):
    """The three kernels alone on 2^22 4x4 16-QAM vectors with K = 16 lists."""
    from commpy_amd.devicelink import DeviceBuf
    from commpy_amd.modulation import QAMModem
    md = QAMModem(16)
    hd = md._device_handle()
    nr = nt = 4
    V, Ke, nbt, nv, clip = 1 << 22, 16, 16, 0.3, 500.0
    rs = np.random.RandomState(0)
    h = (rs.randn(V, nr, nt) + 1j * rs.randn(V, nr, nt)) / np.sqrt(2)
    x = md.constellation[rs.randint(0, 16, (V, nt))]
    y = np.einsum('vrt,vt->vr', h, x) + 0.4 * (rs.randn(V, nr) + 1j * rs.randn(V, nr))
    d_y, d_h = DeviceBuf.from_array(y), DeviceBuf.from_array(h)
    del h, x, y
    d_cand, d_count, d_dist = DeviceBuf(V * Ke * nt * 4), DeviceBuf(V * 4), DeviceBuf(V * Ke * 8)
    d_a, d_out = DeviceBuf(V * nbt * 8), DeviceBuf.from_array(rs.randn(V, nbt) * 5)
    _lib.check(lib.cpx_kbest_list_dev(hd, d_y.ptr, d_h.ptr, 1, V, nr, nt, 16, d_cand.ptr, d_count.ptr, None))
    common = V * (Ke * nt * 4 + 4 + Ke * 8)                         # cand, count, dist
    runs = (
        ("list_dist_kernel", V * (nr * 16 + nr * nt * 16 + Ke * nt * 4 + 4 + Ke * 8), lambda: lib.cpx_mimo_list_dist_dev(
            hd, d_y.ptr, d_h.ptr, 1, V, nr, nt, d_cand.ptr, d_count.ptr, Ke, d_dist.ptr, None)),
        ("list_llr_kernel", common + V * nbt * 8, lambda: lib.cpx_mimo_list_llr_dev(
            hd, d_cand.ptr, d_count.ptr, d_dist.ptr, V, nt, Ke, None, nv, clip, d_a.ptr, None)),
        ("idd_exchange_kernel", common + V * nbt * 8 * 3, lambda: lib.cpx_mimo_idd_exchange_dev(
            hd, d_cand.ptr, d_count.ptr, d_dist.ptr, V, nt, Ke, d_a.ptr, d_out.ptr, nv, clip, 0, None)))
    tm = Timers(lib)
    for name, nbytes, run in runs:
        for _ in range(20):                                          # past the clock ramp
            _lib.check(run())
        ms = []
        for _ in range(max(steps, 10)):
            tm(name, True)
            _lib.check(run())
            tm(name, False)
            ms.append(tm.read()[name])
        med = float(np.median(ms))
        emit({"kernel": name, "workload": "4x4 16-QAM, K = 16 lists, 2^22 vectors", "value": V / (med * 1e-3), "unit": "vectors/s",
              "ms": med, "ms_min": float(np.min(ms)), "dispatch": _lib.last_kernel(),
              "roofline": {"bound": "HBM", "alg_bytes": nbytes, "achieved": nbytes / (med * 1e-3) / 1e9, "peak": HBM_PEAK,
                           "unit": "GB/s", "frac": nbytes / (med * 1e-3) / 1e9 / HBM_PEAK}})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--host-tx", type=int, default=2)
    ap.add_argument("--snr", type=float, default=18.0)
    args = ap.parse_args()
    lib = _lib.load()
    _lib.require_device()
    from helpers import ldpc_params
    from commpy_amd.channelcoding.ldpc import ldpc_bp_decode
    from commpy_amd.devicelink import DeviceMimoLink
    from commpy_amd.links import idd_decoder
    from commpy_amd.modulation import QAMModem, apriori_detector, list_apriori_batch
    md, ldpc = QAMModem(16), ldpc_params("wimax1440")
    kernels(lib, args.steps)
    per_tx = {}
    for n_it in (0, 1, 2, 3):
        link = DeviceMimoLink(md, _chan(), detector='kbest', K=16, output_type='soft', ldpc_params=ldpc, ldpc_alg='MSA', ldpc_iters=15,
                              send_chunk=720, idd_iters=n_it, idd_decision='decode')
        T = link.tx_batch
        link.run_batch(args.snr, T)                                   # warm-up: clocks, allocations, handles
        tm = Timers(lib)
        ms, per_stage, errs = [], [], 0
        for _ in range(args.steps):
            tm("batch", True)
            e = link.run_batch(args.snr, T, mark=tm)
            tm("batch", False)
            r = tm.read()
            ms.append(r.pop("batch"))
            per_stage.append(r)
            errs += int(e.sum())
        batch_ms, bits = float(np.mean(ms)), T * link.send_chunk
        per_tx[n_it] = batch_ms / T
        emit({"kernel": "mimo_idd_link", "idd_iters": n_it, "snr_db": args.snr, "value": bits / (batch_ms * 1e-3), "unit": "info-bit/s",
              "workload": "4x4 16-QAM K-best(16) soft + WiMAX (1440,720) MSA x15, 720 bits/tx, 'decode' decision",
              "ms": batch_ms, "ms_min": float(np.min(ms)), "tx_per_batch": T, "vectors_per_batch": T * link.vectors_per_tx,
              "ber": errs / (bits * args.steps), "stages_ms": {s: float(np.mean([p[s] for p in per_stage])) for s in per_stage[0]},
              "device_ms_per_tx": per_tx[n_it]})
        del link
    # the host path: one transmission at a time through links.idd_decoder, a device call per vector and round
    link = DeviceMimoLink(md, _chan(), detector='kbest', K=16, output_type='soft', ldpc_params=ldpc, send_chunk=720)
    link.keep_rx = True
    link.run_batch(args.snr, args.host_tx)
    rx = link.last_rx
    nv, vpt = rx['noise_std'] ** 2, link.vectors_per_tx
    det = apriori_detector(md, 16)
    for n_it in (1, 3):
        for i, t in enumerate([0] + list(range(args.host_tx))):       # transmission 0 once untimed: first-call overheads
            if i == 1:
                t0 = time.perf_counter()
            y, h = rx['y'][t * vpt:(t + 1) * vpt], rx['h'][t * vpt:(t + 1) * vpt]
            first = list_apriori_batch(y, h, md, 16, nv, None, 500.0).reshape(-1)
            idd_decoder(det, lambda l: ldpc_bp_decode(l, ldpc, 'MSA', 15)[1].reshape(-1, order='F'),
                        lambda l: ldpc_bp_decode(l, ldpc, 'MSA', 15)[0], n_it)(y, h, md.constellation, nv, first, 16)
        host_ms = (time.perf_counter() - t0) * 1e3 / args.host_tx
        emit({"kernel": "host_idd_decoder", "idd_iters": n_it, "host_ms_per_tx": host_ms, "host_tx_timed": args.host_tx,
              "device_ms_per_tx": per_tx[n_it], "speedup_vs_host": host_ms / per_tx[n_it]})


if __name__ == "__main__":
    main()
