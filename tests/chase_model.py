"""A NumPy model of Chase-II soft-decision BCH decoding with Pyndiah's soft output, on top of bch_model.decode_batch; no engine import.

Per word of n float64 values (positive = bit 0):
1. x_i = llr_i, or fl(llr_i + fl(alpha prior_i)) with a prior (two roundings).  A word holding a non-finite x_i is rejected on its own:
   candidates = -1, metric = +inf, the hard decisions (a NaN counts as bit 0), extrinsic 0.
2. h_i = (x_i < 0), r_i = |x_i|.
3. The p positions of least (r_i, i), ascending.
4. tau = 0 .. 2^p - 1: bit j of tau flips the j-th of them; the result is decoded by bch_model (its failures included); a success is a
   candidate c_tau.
5. M_tau = sum of r_i over c_tau != h, added one by one in ascending position order (not np.sum, which adds pairwise).
6. D = the candidate of least metric, ties to the lowest tau; none: D = h, metric = +inf, extrinsic 0.
7. s_i = +1 for d_i = 0, else -1.  extrinsic_i = fl(s_i fl(M_C - M_D) - x_i), M_C the least metric of the candidates with c_i != d_i;
   s_i beta where there is none.
"""
import numpy as np

import bch_model as M

INF = np.float64(np.inf)


def soft_input(llr, prior=None, alpha=1.0):
    llr = np.asarray(llr, dtype=np.float64)
    if prior is None:
        return llr.copy()
    with np.errstate(invalid="ignore", over="ignore"):
        scaled = np.float64(alpha) * np.asarray(prior, dtype=np.float64)
        return llr + scaled


def least_reliable(r, p):
    """The p positions of least (r_i, i), ascending."""
    return np.lexsort((np.arange(len(r)), r))[:p]


def serial_sum(values):
    acc = np.float64(0.0)
    for v in values:
        acc = acc + np.float64(v)
    return acc


def candidates(x, code, p):
    """The successful test patterns of one word x [n] (finite): (h, list of (tau, code word [n] uint8, metric))."""
    h = (x < 0).astype(np.uint8)
    r = np.abs(x)
    lrp = least_reliable(r, p)
    tests = np.repeat(h[None, :], 1 << p, axis=0)
    for j, pos in enumerate(lrp):
        tests[((np.arange(1 << p) >> j) & 1) == 1, pos] ^= 1
    dec = M.decode_batch(tests, code)
    out = []
    for tau in range(1 << p):
        if dec["errors"][tau] >= 0:
            cw = dec["codeword"][tau]
            out.append((tau, cw, serial_sum(r[np.flatnonzero(cw != h)])))
    return h, out


def decode_word(x, code, p, beta):
    """One word x [n] -> dict of 'codeword' [n] uint8, 'extrinsic' [n] float64, 'metric', 'candidates'."""
    n = code.n
    if not np.isfinite(x).all():
        return {"codeword": (x < 0).astype(np.uint8), "extrinsic": np.zeros(n), "metric": INF, "candidates": -1}
    h, cands = candidates(x, code, p)
    if not cands:
        return {"codeword": h, "extrinsic": np.zeros(n), "metric": INF, "candidates": 0}
    best = 0
    for c in range(1, len(cands)):
        if cands[c][2] < cands[best][2]:
            best = c
    d, md = cands[best][1], cands[best][2]
    words = np.stack([c[1] for c in cands])
    metrics = np.array([c[2] for c in cands], dtype=np.float64)
    mc = np.where(words != d[None, :], metrics[:, None], INF).min(axis=0)
    s = np.where(d == 0, 1.0, -1.0)
    with np.errstate(invalid="ignore"):
        gap = mc - md
        soft = s * gap - x
    ext = np.where(mc < INF, soft, s * np.float64(beta))
    return {"codeword": d.copy(), "extrinsic": ext, "metric": md, "candidates": len(cands)}


def decode_batch(llr, code, p, beta, prior=None, alpha=1.0):
    """llr [B, n] -> {'bits' [B, k] uint8, 'codeword' [B, n] uint8, 'extrinsic' [B, n] float64, 'metric' [B] float64,
    'candidates' [B] int32}."""
    x = np.atleast_2d(soft_input(llr, None if prior is None else np.atleast_2d(prior), alpha))
    B, n = x.shape
    assert n == code.n and 1 <= p <= min(8, n)
    out = {"codeword": np.zeros((B, n), np.uint8), "extrinsic": np.zeros((B, n)), "metric": np.zeros(B), "candidates": np.zeros(B, np.int32)}
    for b in range(B):
        res = decode_word(x[b], code, p, beta)
        for key in out:
            out[key][b] = res[key]
    out["bits"] = out["codeword"][:, :code.k].copy()
    return out


# ---- layouts: the words of a strided call as a flat batch and back --------------------------------------------------------------------
def words_of(block, axis):
    """block [B, n_c, n_r] -> the flat batch of its words along ``axis`` (2: rows [B n_c, n_r], 1: columns [B n_r, n_c])."""
    a = np.asarray(block)
    return (a if axis == 2 else a.transpose(0, 2, 1)).reshape(-1, a.shape[axis])


def block_of(words, shape, axis):
    """The inverse of words_of for a block of ``shape`` [B, n_c, n_r]."""
    B, nc, nr = shape
    return words.reshape(B, nc, nr) if axis == 2 else np.ascontiguousarray(words.reshape(B, nr, nc).transpose(0, 2, 1))
