#!/usr/bin/env python3
"""MIMO link throughput on the device (DeviceMimoLink, csrc/mimo_channel.hip) against the host LinkModel path, in one run.
One JSON line per link:
    python benchmarks/bench_mimo_link.py [--steps 3] [--host-tx 30] [--channel-only]
  kbest_hard   4x4 16-QAM, uncoded, K = 16, 720 bits per transmission, SNR 10 log10(4) + 10 dB
  best_first   4x4 16-QAM, WiMAX (1440,720) LDPC, MSA 15 iterations, stack sizes (1, 3, 5), 720 bits per transmission, SNR 18 dB
  (the second and third links of the reference's test_links.py)
`value` is message bits per second of whole run_batch calls of the link's default tx_batch (about 2^20 vectors per detector launch),
HIP events on the launch stream, after a warm-up batch.  `stages_ms` splits one batch into source (random bits, encoder), channel,
detector, decoder and count by events around each stage.  The channel kernel's roofline is HBM: it writes H and y and reads the
bits, `alg_bytes` per launch.  `host_ms_per_tx` is the wall clock per transmission of LinkModel.link_performance with the batched
GPU receiver (mimo_receiver) and the NumPy channel, timed in the same process over --host-tx transmissions."""
import argparse
import ctypes
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from commpy_amd import _lib  # noqa: E402

HBM_PEAK = 8000.0            # GB/s, MI355X spec
STAGES = ("source", "channel", "detector", "decoder", "count")


class StageTimer:
    """HIP event pairs around the stages of one run_batch (DeviceMimoLink's `mark` hook)."""

    def __init__(self, lib):
        self.lib, self.t = lib, {}
        for s in STAGES:
            h = ctypes.c_void_p()
            _lib.check(lib.cpx_timer_create(ctypes.byref(h)))
            self.t[s] = h
        self.used = set()

    def __call__(self, stage, start):
        _lib.check((self.lib.cpx_timer_start if start else self.lib.cpx_timer_stop)(self.t[stage], None))
        self.used.add(stage)

    def read(self):
        out = {}
        for s in STAGES:
            if s in self.used:
                v = ctypes.c_float()
                _lib.check(self.lib.cpx_timer_elapsed_ms(self.t[s], ctypes.byref(v)))
                out[s] = v.value
        self.used = set()
        return out


def _links():
    from helpers import ldpc_params
    from commpy_amd.channelcoding.ldpc import ldpc_bp_decode, triang_ldpc_systematic_encode
    from commpy_amd.channels import MIMOFlatChannel
    from commpy_amd.devicelink import DeviceMimoLink
    from commpy_amd.links import LinkModel, mimo_receiver
    from commpy_amd.modulation import QAMModem
    md = QAMModem(16)

    def chan():
        c = MIMOFlatChannel(4, 4)
        c.uncorr_rayleigh_fading(complex)
        return c
    dev = DeviceMimoLink(md, chan(), detector='kbest', K=16, send_chunk=720)
    host = LinkModel(md.modulate, chan(), mimo_receiver(md, 'kbest', 16), md.num_bits_symbol, md.constellation, md.Es)
    yield "kbest_hard", "4x4 16-QAM K-best(16) hard, uncoded, 720 bits/tx", 10 * math.log10(4) + 10, dev, host, 1

    ldpc = ldpc_params("wimax1440")
    dev = DeviceMimoLink(md, chan(), detector='best_first', stack_size=(1, 3, 5), llr_max=500, ldpc_params=ldpc, ldpc_alg='MSA',
                         ldpc_iters=15, send_chunk=720)

    def modulate(bits):
        return md.modulate(triang_ldpc_systematic_encode(bits, ldpc, False).reshape(-1, order='F'))

    def decoder(llrs):
        return ldpc_bp_decode(llrs, ldpc, 'MSA', 15)[0][:720].reshape(-1, order='F')
    host = LinkModel(modulate, chan(), mimo_receiver(md, 'best_first'), md.num_bits_symbol, md.constellation, md.Es, decoder, 0.5)
    yield "best_first_ldpc", "4x4 16-QAM best-first (1,3,5) + WiMAX (1440,720) MSA x15, 720 bits/tx", 18.0, dev, host, 0.5


def channel_only(lib, steps):
    """The channel kernel alone over 2^20 4x4 16-QAM vectors, uncorrelated Rayleigh and correlated Rician (both products): the
    launches a counter run (rocprofv3 --pmc) of its own is pointed at."""
    from benchmarks.bench_kernels import timeit
    from commpy_amd.channels import MIMOFlatChannel
    from commpy_amd.devicelink import DeviceBuf, _channel_handles
    from commpy_amd.modulation import QAMModem
    md = QAMModem(16)
    nr = nt = 4
    V = 1 << 20
    rs = np.random.RandomState(0)
    d_bits = DeviceBuf.from_array(rs.randint(0, 2, V * nt * 4).astype(np.uint8))
    d_y, d_h = DeviceBuf(V * nr * 16), DeviceBuf(V * nr * nt * 16)
    for fading in ("rayleigh", "rician_corr"):
        ch = MIMOFlatChannel(nt, nr)
        if fading == "rayleigh":
            ch.uncorr_rayleigh_fading(complex)
        else:
            ch.expo_corr_rician_fading(np.ones((nr, nt), complex), 2.0, np.exp(0.3j), np.exp(-0.5j), 0.2, 0.4)
        hs = _channel_handles(ch)

        def run():
            _lib.check(lib.cpx_mimo_channel_run_dev(hs.get(), md._device_handle(), d_bits.ptr, V, 0, 0.3, 1, 2, 3, d_y.ptr, d_h.ptr,
                                                    None))
        ms, ms_min = timeit(lib, run, steps=steps, warmup=3)
        kernel = _lib.last_kernel()
        nbytes = V * (nr * nt * 16 + nr * 16 + nt * 4)
        print(json.dumps({"kernel": "mimo_channel_kernel", "workload": "4x4 16-QAM, %s, 2^20 vectors" % fading, "value": V / (ms * 1e-3),
                          "unit": "vectors/s", "ms": ms, "ms_min": ms_min, "dispatch": kernel,
                          "roofline": {"bound": "HBM", "alg_bytes": nbytes, "achieved": nbytes / (ms * 1e-3) / 1e9, "peak": HBM_PEAK,
                                       "unit": "GB/s", "frac": nbytes / (ms * 1e-3) / 1e9 / HBM_PEAK},
                          "build_id": _lib.build_id().get("full")}), flush=True)
        hs.drop()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--host-tx", type=int, default=30)
    ap.add_argument("--channel-only", action="store_true", help="time the channel kernel alone (the counter run's target)")
    args = ap.parse_args()
    lib = _lib.load()
    _lib.require_device()
    if args.channel_only:
        channel_only(lib, max(args.steps, 5))
        return
    for name, workload, snr, dev, host, rate in _links():
        T = dev.tx_batch
        V = T * dev.vectors_per_tx
        dev.run_batch(snr, T)                                             # warm-up: clocks, allocations, handles
        tm = ctypes.c_void_p()
        _lib.check(lib.cpx_timer_create(ctypes.byref(tm)))
        stages = StageTimer(lib)
        ms, per_stage, errs = [], [], 0
        for _ in range(args.steps):
            _lib.check(lib.cpx_timer_start(tm, None))
            e = dev.run_batch(snr, T, mark=stages)
            _lib.check(lib.cpx_timer_stop(tm, None))
            _lib.check(lib.cpx_stream_sync(None))
            v = ctypes.c_float()
            _lib.check(lib.cpx_timer_elapsed_ms(tm, ctypes.byref(v)))
            ms.append(v.value)
            per_stage.append(stages.read())
            errs += int(e.sum())
        lib.cpx_timer_destroy(tm)
        batch_ms = float(np.mean(ms))
        st = {s: float(np.mean([p[s] for p in per_stage])) for s in per_stage[0]}
        bits = T * dev.send_chunk
        chan_bytes = V * (dev.nr * dev.nt * 16 + dev.nr * 16) + V * dev.nt * dev.nb
        # the host path, same process: LinkModel.link_performance over host_tx transmissions (err_min never reached)
        np.random.seed(1)
        t0 = time.perf_counter()
        host.link_performance([snr], args.host_tx * dev.send_chunk, 10 ** 12, dev.send_chunk, rate)
        host_ms = (time.perf_counter() - t0) * 1e3 / args.host_tx
        dev_ms_per_tx = batch_ms / T
        d = {"kernel": "mimo_link", "link": name, "workload": workload, "snr_db": snr, "value": bits / (batch_ms * 1e-3),
             "unit": "info-bit/s", "ms": batch_ms, "ms_min": float(np.min(ms)), "tx_per_batch": T, "vectors_per_batch": V,
             "ber": errs / (bits * args.steps), "stages_ms": st, "channel_share": st["channel"] / batch_ms,
             "channel_roofline": {"bound": "HBM", "alg_bytes": chan_bytes, "achieved": chan_bytes / (st["channel"] * 1e-3) / 1e9,
                                  "peak": HBM_PEAK, "unit": "GB/s", "frac": chan_bytes / (st["channel"] * 1e-3) / 1e9 / HBM_PEAK},
             "device_ms_per_tx": dev_ms_per_tx, "host_ms_per_tx": host_ms, "host_tx_timed": args.host_tx,
             "speedup_vs_host": host_ms / dev_ms_per_tx, "kernels_last": _lib.last_kernel(),
             "build_id": _lib.build_id().get("full")}
        print(json.dumps(d), flush=True)


if __name__ == "__main__":
    main()
