#!/usr/bin/env python3
"""Generate tests/golden/idd.npz from the LIVE reference: the anchors of the list detector with a-priori LLRs and of the
iterative detection and decoding loop (csrc/mimo_idd.hip, DeviceMimoLink(idd_iters=...)).

Run in the build container only (the GPU box has no reference checkout):

    python tests/golden/make_golden_idd.py

Reference entry points exercised (file:line in the reference checkout):
  kbest(..., 'soft')      commpy/modulation.py:325   its final candidate list is captured through the `demode` callback
  max_log_approx          commpy/modulation.py:599
  idd_decoder             commpy/links.py:345
  ldpc_bp_decode (MSA)    commpy/channelcoding/ldpc.py:144

The detector with priors has no counterpart in the reference (its idd_decoder takes any callback): `list_model` below IS its
definition, restated in tests/test_idd_host.py and tests/test_idd_gpu.py.

Detector anchor, per case `det_<name>`: y [n, nr], h [n, nr, nt], const, labels [m, nb], K, noise_var, the reference's final list
cand [n, Ke, nt] (uint8, rows past count hold 255) and count [n], the reference's max_log_approx LLRs `ref`, and for random
priors `prior` (some beyond +-clip) the model's LLRs `post` at `clip`.
Loop anchor `loop_*`: T = 4 transmissions of one (1440, 720) WiMAX codeword over 4x4 16-QAM at 20 dB; the chain is the
reference's idd_decoder with list_model on the reference's K = 64 list as `detector` and the reference's ldpc_bp_decode (MSA, 15
iterations) out_llrs as `decoder`, started from the prior-free detector pass; stored per n_it in (1, 2, 3): the final LLRs (what
`decision` receives).  Every chain is run again with every detector output scaled by 1 + 1e-9 u, u uniform in +-1 (the size of
the detector contract); the largest change of a final LLR is `idd_llr_sensitivity`.  The script takes the first seed (1, 2, ...
up to MAX_SEEDS) at which every stored final LLR exceeds 100 times that in magnitude -- no decision on a knife edge -- and
asserts that it found one.

Why K = 64 at 20 dB and not the link benchmark's K = 16 at 15 dB: a K = 16 list leaves about 45 % of the bits without a
counter-hypothesis, their LLRs are exactly +-clip, min-sum messages of exactly +-500 cancel to exactly 0.0 inside a decoder that
does not converge, and a 1e-9 perturbation flips the sign of such a zero and with it the early-termination test of ldpc.py:205
(sensitivities of 2 to 60 LLR units on every seed tried, at K = 16, 64 and 256 alike, whenever a codeword failed to converge).
Where the decoder converges the chain is smooth: sensitivities of 5e-7 to 3e-6 against smallest final LLRs of 0.1 to 1.  The K = 64
list still leaves about 20 % of the bits at exactly +-clip, so that path stays in the anchor.
"""
import os
import sys
import warnings

os.environ.setdefault("MPLBACKEND", "Agg")
sys.dont_write_bytecode = True
REF = os.environ.get("COMMPY_REFERENCE", "/root/reference")
sys.path.insert(0, REF)

import numpy as np  # noqa: E402

warnings.simplefilter("ignore")

from commpy.channelcoding.ldpc import get_ldpc_code_params, ldpc_bp_decode, triang_ldpc_systematic_encode  # noqa: E402
from commpy.links import idd_decoder  # noqa: E402
from commpy.modulation import QAMModem, kbest  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = {}
MAX_SEEDS = 20


def list_model(y, h, const, labels, cand, prior, noise_var, clip):
    """The max-log list detector with priors: `cand` [count, nt] constellation indices, `labels` [m, nb] the bits of each point
    (MSB first), `prior` [nt * nb] (positive: bit 0).  cost_c = |y - h x_c|^2 / (2 noise_var) + sum_k b_k(c) La_k with La the prior
    clipped to +-clip; L_k = min_{b_k = 1} cost - min_{b_k = 0} cost, an empty side +inf, clipped to +-clip; any NaN in y, h or the
    prior makes every LLR NaN."""
    la = np.clip(np.asarray(prior, dtype=float), -clip, clip)
    bits = labels[cand].reshape(len(cand), -1).astype(bool)
    if np.isnan(y).any() or np.isnan(h).any() or np.isnan(la).any():
        return np.full(bits.shape[1], np.nan)
    dist = np.linalg.norm(y[:, None] - h.dot(const[cand].T), axis=0) ** 2
    cost = dist / (2 * noise_var) + np.where(bits, la[None, :], 0.0).sum(axis=1)
    out = np.empty(bits.shape[1])
    with np.errstate(invalid="ignore"):
        for k in range(bits.shape[1]):
            one = np.min(np.append(cost[bits[:, k]], np.inf))
            zero = np.min(np.append(cost[~bits[:, k]], np.inf))
            out[k] = one - zero
    return np.clip(out, -clip, clip)


def rnd_c(rs, *shape):
    return (rs.randn(*shape) + 1j * rs.randn(*shape)) / np.sqrt(2)


def reference_list(y, h, md, K, noise_var):
    """(candidate indices [count, nt], the reference's soft K-best LLRs) of one vector."""
    const = md.constellation
    seen = []

    def demode(pts):
        seen.append(np.array(pts))
        return md.demodulate(pts, 'hard')
    llr = kbest(y, h, const, K, noise_var, 'soft', demode)
    pts = seen[0].reshape(-1, h.shape[1])                      # candidate after candidate (order='F' of [nt, n])
    idx = np.argmax(pts[:, :, None] == const[None, None, :], axis=2)
    assert np.array_equal(const[idx], pts)
    return idx, llr


def detector_case(name, rs, md, nr, nt, K, n, noise, noise_var, clip):
    const = md.constellation
    m, nb = len(const), md.num_bits_symbol
    labels = md.demodulate(const, 'hard').reshape(m, nb).astype(np.uint8)
    ke = min(K, m ** nt)
    ys, hs = np.empty((n, nr), complex), np.empty((n, nr, nt), complex)
    cand, count = np.full((n, ke, nt), 255, np.uint8), np.zeros(n, np.int32)
    ref, prior, post = (np.empty((n, nt * nb)) for _ in range(3))
    for i in range(n):
        hs[i] = rnd_c(rs, nr, nt)
        ys[i] = hs[i].dot(const[rs.randint(0, m, nt)]) + noise * rnd_c(rs, nr)
        idx, ref[i] = reference_list(ys[i], hs[i], md, K, noise_var)
        count[i] = len(idx)
        cand[i, :len(idx)] = idx
        prior[i] = rs.randn(nt * nb) * rs.choice([2.0, 30.0, 400.0])
        post[i] = list_model(ys[i], hs[i], const, labels, idx, prior[i], noise_var, clip)
        zero = list_model(ys[i], hs[i], const, labels, idx, np.zeros(nt * nb), noise_var, np.inf)
        assert np.allclose(zero, ref[i], rtol=1e-9, atol=1e-9, equal_nan=True), (name, i)     # La = 0, clip = inf: max_log_approx
    for key, val in (("y", ys), ("h", hs), ("const", const), ("labels", labels), ("K", np.array(K)), ("noise_var", np.array(noise_var)),
                     ("clip", np.array(clip)), ("cand", cand), ("count", count), ("ref", ref), ("prior", prior), ("post", post)):
        OUT["det_%s_%s" % (name, key)] = val
    print("%-16s n %3d Ke %3d  |prior| > clip: %d  |post| = clip: %d" % (name, n, ke, int((np.abs(prior) > clip).sum()),
                                                                          int((np.abs(post) == clip).sum())))


def loop_case(seed):
    """The loop anchor for one seed: (arrays, smallest |final LLR|, sensitivity)."""
    rs = np.random.RandomState(seed)
    md = QAMModem(16)
    const, nb, nt, nr, K, clip = md.constellation, 4, 4, 4, 64, 500.0
    labels = md.demodulate(const, 'hard').reshape(16, nb).astype(np.uint8)
    ldpc = get_ldpc_code_params(os.path.join(REF, 'commpy/channelcoding/designs/ldpc/wimax/1440.720.txt'), True)
    T, n, k, snr_db = 4, 1440, 720, 20.0
    bps, V = nt * nb, n // (nt * nb)
    noise_std = np.sqrt(2 * nt * md.Es / (0.5 * 10 ** (snr_db / 10)))               # channels.py:74
    noise_var = noise_std ** 2                                                      # what the detector is told (quirk B7)
    out = {"y": np.empty((T, V, nr), complex), "h": np.empty((T, V, nr, nt), complex), "msg": np.empty((T, k), np.uint8),
           "noise_var": np.array(noise_var), "K": np.array(K), "clip": np.array(clip), "ldpc_iters": np.array(15)}
    finals = {n_it: np.empty((T, n)) for n_it in (1, 2, 3)}
    sens, smallest = 0.0, np.inf
    for t in range(T):
        msg = rs.randint(0, 2, k)
        code = triang_ldpc_systematic_encode(msg, ldpc, False).reshape(-1, order='F')
        x = md.modulate(code).reshape(V, nt)
        h = rnd_c(rs, V, nr, nt)
        y = np.einsum('vrt,vt->vr', h, x) + noise_std * 0.5 * (rs.randn(V, nr) + 1j * rs.randn(V, nr))
        out["y"][t], out["h"][t], out["msg"][t] = y, h, msg
        lists = [reference_list(y[v], h[v], md, K, noise_var)[0] for v in range(V)]
        by_key = {y[v].tobytes(): lists[v] for v in range(V)}

        def decoder(llrs):
            return ldpc_bp_decode(llrs, ldpc, 'MSA', 15)[1].reshape(-1, order='F')

        def make_detector(jitter):
            def detector(yv, hv, constellation, nv, a_priori):
                llr = list_model(yv, hv, const, labels, by_key[yv.tobytes()], a_priori, nv, clip)
                return llr * (1 + 1e-9 * jitter.uniform(-1, 1, llr.shape)) if jitter is not None else llr
            return detector
        for n_it in (1, 2, 3):
            got = []
            for jitter in (None, np.random.RandomState(seed + 1000 * t + n_it)):
                det = make_detector(jitter)
                first = np.concatenate([det(y[v], h[v], const, noise_var, np.zeros(bps)) for v in range(V)])
                got.append(idd_decoder(det, decoder, lambda llrs: llrs.copy(), n_it)(y, h, const, noise_var, first, bps))
            finals[n_it][t] = got[0]
            sens = max(sens, float(np.max(np.abs(got[1] - got[0]))))
            smallest = min(smallest, float(np.min(np.abs(got[0]))))
    for n_it in (1, 2, 3):
        out["final_it%d" % n_it] = finals[n_it]
    out["snr_db"] = np.array(snr_db)
    return out, smallest, sens


def main():
    rs = np.random.RandomState(20261017)
    qpsk, q16 = QAMModem(4), QAMModem(16)
    detector_case("qpsk_2x2", rs, qpsk, 2, 2, 4, 80, 0.5, 0.25, 500.0)
    detector_case("qpsk_4x4_full", rs, qpsk, 4, 4, 256, 60, 0.6, 0.36, 500.0)
    detector_case("qam16_4x4", rs, q16, 4, 4, 16, 100, 0.5, 0.25, 500.0)
    detector_case("qam16_3x2", rs, q16, 3, 2, 16, 80, 0.5, 0.25, 50.0)
    for seed in range(1, MAX_SEEDS + 1):
        loop, smallest, sens = loop_case(seed)
        print("loop seed %d: smallest |final LLR| %.3e, sensitivity %.3e" % (seed, smallest, sens))
        if smallest > 100 * sens:
            break
    assert smallest > 100 * sens, "no seed up to %d with every |final LLR| above 100 x the sensitivity" % MAX_SEEDS
    for key, val in loop.items():
        OUT["loop_" + key] = val
    OUT["loop_seed"] = np.array(seed)
    OUT["idd_llr_sensitivity"] = np.array(sens)
    for n_it in (1, 2, 3):
        errs = (np.signbit(loop["final_it%d" % n_it][:, :720]) != loop["msg"].astype(bool)).sum(axis=1)
        print("n_it %d: hard-decision bit errors per transmission %s" % (n_it, errs.tolist()))
    path = os.path.join(HERE, "idd.npz")
    np.savez_compressed(path, **OUT)
    print("wrote %s (%.1f kB, %d arrays)" % (path, os.path.getsize(path) / 1e3, len(OUT)))


if __name__ == "__main__":
    main()
