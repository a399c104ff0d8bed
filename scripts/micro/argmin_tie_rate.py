#!/usr/bin/env python3
"""How often does the first-argmin of a trellis step NOT follow from the high dwords of the 64 path metrics alone?

The fused Viterbi kernel ('soft', 64 states, float64) finds the first-argmin state of a step on the upper 32 bits of the metrics and
falls back to the float64 minimum tree + first-equal scan for a whole wave of 64 codewords when any of its lanes has two or more
states whose high dword equals the minimum high dword (csrc/viterbi_cw.hip, cw_step).  The kernel reads that condition off the minima
of an 8 x 8 grid of the high dwords (state s = 8 j + i: more than one row minimum or more than one column minimum equals the overall
minimum); the script counts the lanes where that flag and the hit count disagree, and where the grid's index is not the single hit
(both 0 by construction).  This script measures that rate on the CPU, on
the input of `bench.py --synth host`: the same messages, noise seeds, QPSK mapping and Eb/N0 (bench.synth_inputs' arithmetic), the
reference's soft-demodulator formula and a NumPy float64 add-compare-select written after oracle/np_viterbi.py.

    python scripts/micro/argmin_tie_rate.py [--batch 4096] > profiles/viterbi_argmin32_tie_rate.txt
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

MSG_BITS, EBN0_DB = 1024, 3.0                                      # bench.py


def host_llrs(B, seed_msg=10, seed_noise=11):
    from commpy_amd.channelcoding import Trellis
    from commpy_amd.modulation import QAMModem
    tr = Trellis(np.array([6]), np.array([[0o133, 0o171]]))
    md = QAMModem(4)
    nxt, out = np.asarray(tr.next_state_table), np.asarray(tr.output_table)
    msgs = np.random.RandomState(seed_msg).randint(0, 2, (B, MSG_BITS))
    bits = np.concatenate([msgs, np.zeros((B, 6), msgs.dtype)], axis=1)       # termination 'term'
    st = np.zeros(B, np.int64)
    coded = np.zeros((B, bits.shape[1], 2), np.int64)
    for t in range(bits.shape[1]):
        o = out[st, bits[:, t]]
        coded[:, t, 0], coded[:, t, 1] = o >> 1, o & 1
        st = nxt[st, bits[:, t]]
    sym = md.modulate(coded.reshape(-1)).reshape(B, -1)
    N0 = md.Es / (0.5 * 2 * 10 ** (EBN0_DB / 10.0))
    noise = np.random.RandomState(seed_noise).randn(B, sym.shape[1], 2).view(np.complex128)[..., 0]
    y = sym + np.sqrt(N0 / 2) * noise
    # the soft demodulator's formula: log(sum over points with bit = 1 / sum over points with bit = 0) of exp(-|y - s|^2 / N0)
    c = np.asarray(md.constellation)
    e = np.exp(-np.abs(y[..., None] - c) ** 2 / N0)                           # [B, nsym, 4]
    lab = np.arange(4)
    llr = np.stack([np.log(e[..., (lab >> 1) & 1 == 1].sum(-1) / e[..., (lab >> 1) & 1 == 0].sum(-1)),
                    np.log(e[..., lab & 1 == 1].sum(-1) / e[..., lab & 1 == 0].sum(-1))], axis=-1)
    return tr, llr.reshape(B, -1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    a = ap.parse_args()
    B = a.batch
    tr, x = host_llrs(B)
    x = np.clip(x, -500, 500)
    nxt, out = np.asarray(tr.next_state_table), np.asarray(tr.output_table)
    S = 64
    ps, pc = np.zeros((S, 2), np.int64), np.zeros((S, 2), np.int64)
    cnt = np.zeros(S, np.int64)
    for p in range(S):
        for i in range(2):
            s = nxt[p, i]
            ps[s, cnt[s]], pc[s, cnt[s]] = p, out[p, i]
            cnt[s] += 1
    L = x.shape[1] // 2
    T = L + 6 - 1
    pm = np.full((B, S), np.inf)
    pm[:, 0] = 0.0
    cw_steps = cw_hi_tie = cw_f64_tie = cw_wrong = wave_steps = wave_fb = grid_flag_differs = grid_index_differs = 0
    per_wave_lanes = []
    for t in range(1, T + 1):
        r = x[:, 2 * (t - 1):2 * t] if t <= L else np.zeros((B, 2))
        nll0 = np.log(np.exp(r) + 1)
        nll1 = nll0 - r
        bm = np.stack([(0.0 + (nll1 if c >> 1 else nll0)[:, 0]) + (nll1 if c & 1 else nll0)[:, 1] for c in range(4)], axis=1)
        cand = pm[:, ps] + bm[:, pc.reshape(-1)].reshape(B, S, 2)
        pm = cand.min(axis=2)
        hi = pm.view(np.uint64) >> np.uint64(32)
        hit = hi == hi.min(axis=1, keepdims=True)
        n_hit = hit.sum(axis=1)
        tie = n_hit >= 2
        grid = (hi == hi.min(axis=1, keepdims=True)).reshape(B, 8, 8)      # row / column minimum == minimum <=> a hit in that row / column
        rows, cols = grid.any(axis=2), grid.any(axis=1)
        grid_flag_differs += int(((rows.sum(axis=1) + cols.sum(axis=1) != 2) != tie).sum())
        grid_index_differs += int(((8 * rows.argmax(axis=1) + cols.argmax(axis=1) != hit.argmax(axis=1)) & ~tie).sum())
        cw_steps += B
        cw_hi_tie += int(tie.sum())
        cw_f64_tie += int(((pm == pm.min(axis=1, keepdims=True)).sum(axis=1) >= 2).sum())
        cw_wrong += int((hit.argmax(axis=1) != pm.argmin(axis=1)).sum())
        w = tie.reshape(-1, 64)
        wave_steps += w.shape[0]
        wave_fb += int(w.any(axis=1).sum())
        per_wave_lanes.append(w.sum(axis=1))
    lanes = np.concatenate(per_wave_lanes)
    print("input: bench.py --synth host arithmetic, %d codewords, Eb/N0 %.1f dB, %d trellis steps each" % (B, EBN0_DB, T))
    print("codeword-steps                                              %d" % cw_steps)
    print("  >= 2 states share the minimum high dword                  %d  (%.3e)" % (cw_hi_tie, cw_hi_tie / cw_steps))
    print("  exact float64 tie of the minimum                          %d  (%.3e)" % (cw_f64_tie, cw_f64_tie / cw_steps))
    print("  first high-dword hit is NOT the first-argmin              %d  (%.3e)" % (cw_wrong, cw_wrong / cw_steps))
    print("  row/column flag differs from (hits >= 2)                  %d" % grid_flag_differs)
    print("  one hit, and 8 j* + i* is not that state                  %d" % grid_index_differs)
    print("wave-steps (64 consecutive codewords)                       %d" % wave_steps)
    print("  any lane ties on the high dword = the fallback runs       %d  (%.3e)" % (wave_fb, wave_fb / wave_steps))
    print("  tying lanes per falling-back wave-step: mean %.2f, max %d" % (lanes[lanes > 0].mean() if wave_fb else 0.0, lanes.max()))


if __name__ == "__main__":
    main()
