"""Plain NumPy float64 models of the MIMO detectors of csrc/mimo.hip, the inputs they are compared on, and an exact-rational
second evaluation for inputs with metric ties.  No GPU, no engine import.

Shared by tests/test_mimo_model_host.py (which pins the models on the reference's goldens and proves them exact on the tie
inputs) and tests/test_mimo_model_gpu.py (which holds the kernels to them).

The rules modelled:

* ``ml_model``: all ``m^nt`` hypotheses, antenna 0 the most significant digit, metric ``sum_r |y_r - (H x)_r|^2``, the choice
  is ``np.argmin`` -- the first minimum, a NaN metric before every number.
* ``kbest_model``: the reference's breadth-first search on ``np.linalg.qr(h)`` and ``Q^H y``, antenna ``nt - 1`` down to 0,
  children at position ``point * nb + parent``, ``np.argsort(kind='stable')`` (equal metrics by the lowest position, NaN
  last), the ``min(N, K)`` smallest kept in ascending order.
* ``kbest_llr_model``: max-log LLRs over a candidate list on the ORIGINAL ``y`` and ``H``: metric ``norm(y - H x) ** 2``, bit
  labels are the index bits MSB first, ``-(min0 - min1) / (2 noise_var)`` with an empty set counting as +inf, NumPy's ``min``.

Squares of complex numbers are taken as ``re^2 + im^2`` (not ``abs() ** 2``: a hypot is not exact on dyadic inputs, and the
tie inputs below rely on every operation being exact in float64).

``gap`` is the models' own measure of how close an input is to a tie, relative to the larger of the two metrics compared.  A
vector whose gap is at most ``GAP_MIN`` is not a fair exact-equality case: a Householder QR on the device and LAPACK's differ
around 1e-14 in the metrics.  The threshold is a condition on the input, never a tolerance on an output.
"""
from fractions import Fraction

import numpy as np

GAP_MIN = 1e-9
SCREEN_CAP = 0.02          # at most this share of a random case may be screened out
BPSK = np.array([-1.0, 1.0])


def _sq(z):
    z = np.asarray(z, dtype=np.complex128)
    return z.real * z.real + z.imag * z.imag


def _rel_gaps(s):
    """(s[i+1] - s[i]) / s[i+1] of an ascending float array; NaN where it cannot be formed (a NaN or 0 / 0)."""
    with np.errstate(all="ignore"):
        return (s[1:] - s[:-1]) / s[1:]


def _min_gap(g, gaps):
    """min(g, min(gaps)) in which a NaN sticks: such a vector never passes ``gap > GAP_MIN``."""
    if gaps.size == 0 or g != g:
        return g
    with np.errstate(all="ignore"):
        v = float(np.min(gaps))
    return v if v != v or v < g else g


# ---- ML ----------------------------------------------------------------------------------------------------------------------
def ml_metrics(y, h, const):
    """Metrics of all m^nt hypotheses [m^nt], hypothesis index = sum_t digit_t * m^(nt-1-t)."""
    y = np.asarray(y, dtype=np.complex128)
    h = np.asarray(h, dtype=np.complex128)
    c = np.asarray(const, dtype=np.complex128)
    nr, nt = h.shape
    with np.errstate(all="ignore"):
        hx = np.zeros((1, nr), dtype=np.complex128)
        for t in range(nt):
            hx = (hx[:, None, :] + c[None, :, None] * h[None, None, :, t]).reshape(-1, nr)
        np.subtract(y[None, :], hx, out=hx)
        parts = hx.view(np.float64)                       # [m^nt, 2 nr]: re, im of every receive antenna
        return np.einsum('ij,ij->i', parts, parts)


def digits_of(index, m, nt):
    """Per-antenna constellation indices [..., nt] of hypothesis numbers, antenna 0 the most significant digit."""
    index = np.asarray(index, dtype=np.int64)
    return (index[..., None] // (m ** np.arange(nt - 1, -1, -1, dtype=np.int64))) % m


def ml_model(y, h, const):
    """(indices [nt], gap): gap = (second best - best) / second best."""
    met = ml_metrics(y, h, const)
    best = int(np.argmin(met))
    nt = np.asarray(h).shape[1]
    if met.size == 1:
        return digits_of(best, len(const), nt), np.inf
    two = np.partition(met, 1)[:2] if not np.isnan(met).any() else np.array([np.nan, np.nan])
    return digits_of(best, len(const), nt), float(_rel_gaps(np.sort(two))[0])


# ---- K-best ------------------------------------------------------------------------------------------------------------------
def kbest_search(yt, r, const, K, levels=None):
    """The breadth-first search on an upper-triangular ``r`` [nt, nt] and ``yt`` [nt].  Returns (cand [n, nt], n, gap); where
    ``levels`` is a list, (children metrics in position order, number kept) of every level is appended to it."""
    c = np.asarray(const, dtype=np.complex128)
    r = np.asarray(r, dtype=np.complex128)
    nt, m = r.shape[1], c.size
    d = np.array(yt, dtype=np.complex128)[:nt, None]          # [nt, nb] what is left of yt per candidate
    idx = np.zeros((nt, 1), dtype=np.int64)
    tot = np.zeros(1)
    nb, gap = 1, np.inf
    with np.errstate(all="ignore"):
        for coor in range(nt - 1, -1, -1):
            N = nb * m
            p, q = np.repeat(np.arange(m), nb), np.tile(np.arange(nb), m)     # child j = p * nb + q
            e = d[coor, q] - r[coor, coor] * c[p]
            child = tot[q] + _sq(e)
            order = np.argsort(child, kind="stable")
            nk = min(N, K)
            gap = _min_gap(gap, _rel_gaps(child[order[:min(N, nk + 1)]]))
            if levels is not None:
                levels.append((child.copy(), nk))
            keep = order[:nk]
            d, idx = d[:, q[keep]], idx[:, q[keep]]
            d[coor] = e[keep]
            d[:coor] -= r[:coor, coor, None] * c[p[keep]]
            idx[coor] = p[keep]
            tot = child[keep]
            nb = nk
    return idx.T.copy(), nb, float(gap)


def kbest_model(y, h, const, K, levels=None):
    """(candidate indices [n, nt] in ascending metric order, n, gap) for one received vector."""
    y = np.asarray(y, dtype=np.complex128)
    h = np.asarray(h, dtype=np.complex128)
    q, r = np.linalg.qr(h)                   # a NaN in h reaches every later column of R and Q, hence the first level
    with np.errstate(all="ignore"):
        yt = q.conj().T.dot(y)
    return kbest_search(yt, r, const, K, levels)


def kbest_llr_model(y, h, const, cand, noise_var):
    """Max-log LLRs [nt * nbits] over the candidate index list ``cand`` [n, nt]."""
    y = np.asarray(y, dtype=np.complex128)
    h = np.asarray(h, dtype=np.complex128)
    c = np.asarray(const, dtype=np.complex128)
    cand = np.asarray(cand, dtype=np.int64)
    nt = h.shape[1]
    nbits = int(np.log2(c.size))
    out = np.empty(nt * nbits)
    with np.errstate(all="ignore"):
        met = np.linalg.norm(y[:, None] - h.dot(c[cand].T), axis=0) ** 2
        for t in range(nt):
            for b in range(nbits):
                bit = (cand[:, t] >> (nbits - 1 - b)) & 1
                mn0 = np.min(np.append(met[bit == 0], np.inf))
                mn1 = np.min(np.append(met[bit == 1], np.inf))
                out[t * nbits + b] = -(mn0 - mn1) / (2 * np.float64(noise_var))
    return out


def pad_list(cand, width):
    """A candidate list [n, nt] as the engine returns it: [width, nt] int32 with -1 past the count."""
    out = np.full((width, cand.shape[1]), -1, dtype=np.int32)
    out[:len(cand)] = cand
    return out


# ---- exact rational evaluation (upper-triangular H with dyadic entries, no QR) --------------------------------------------------
def _fc(z):
    z = complex(z)
    return Fraction(z.real), Fraction(z.imag)


def _fmul(a, b):
    return a[0] * b[0] - a[1] * b[1], a[0] * b[1] + a[1] * b[0]


def _fsub(a, b):
    return a[0] - b[0], a[1] - b[1]


def _fsq(a):
    return a[0] * a[0] + a[1] * a[1]


def ml_exact(y, h, const):
    """(first minimum's indices [nt], metrics of all hypotheses as Fractions) in exact arithmetic."""
    nr, nt = np.asarray(h).shape
    m = len(const)
    H = [[_fc(h[r][t]) for t in range(nt)] for r in range(nr)]
    Y, C = [_fc(v) for v in y], [_fc(v) for v in const]
    mets = []
    for i in range(m ** nt):
        dg = [(i // m ** (nt - 1 - t)) % m for t in range(nt)]
        tot = Fraction(0)
        for r in range(nr):
            e = Y[r]
            for t in range(nt):
                e = _fsub(e, _fmul(H[r][t], C[dg[t]]))
            tot += _fsq(e)
        mets.append(tot)
    best = min(range(len(mets)), key=mets.__getitem__)          # min() returns the first minimum
    return np.array([(best // m ** (nt - 1 - t)) % m for t in range(nt)]), mets


def kbest_exact(y, h, const, K):
    """The search of ``kbest_model`` on R = h, Q = I in exact arithmetic: (cand [n, nt], n, levels) with ``levels`` a list of
    (children metrics as Fractions in position order, number kept).  ``h`` must be square and upper triangular."""
    h = np.asarray(h)
    nt = h.shape[1]
    assert h.shape[0] == nt and not np.any(np.tril(h, -1)), "kbest_exact: h must be square upper triangular"
    m = len(const)
    R = [[_fc(h[r][t]) for t in range(nt)] for r in range(nt)]
    C = [_fc(v) for v in const]
    par = [([_fc(v) for v in y], [0] * nt, Fraction(0))]         # (d [nt], indices [nt], total)
    levels = []
    for coor in range(nt - 1, -1, -1):
        nb = len(par)
        N = nb * m
        es, child = [], []
        for j in range(N):
            p, q = divmod(j, nb)
            e = _fsub(par[q][0][coor], _fmul(R[coor][coor], C[p]))
            es.append(e)
            child.append(par[q][2] + _fsq(e))
        order = sorted(range(N), key=child.__getitem__)          # stable
        nk = min(N, K)
        levels.append((child, nk))
        nxt = []
        for j in order[:nk]:
            p, q = divmod(j, nb)
            d, ix = list(par[q][0]), list(par[q][1])
            d[coor], ix[coor] = es[j], p
            for t in range(coor):
                d[t] = _fsub(d[t], _fmul(R[t][coor], C[p]))
            nxt.append((d, ix, child[j]))
        par = nxt
    return np.array([ix for _, ix, _ in par]), len(par), levels


# ---- inputs ------------------------------------------------------------------------------------------------------------------
def rnd_c(rs, *shape):
    return (rs.randn(*shape) + 1j * rs.randn(*shape)) / np.sqrt(2)


def random_inputs(seed, B, nr, nt, const, shared, real=False, noise=0.6):
    """(y [B, nr], h [nr, nt] or [B, nr, nt]): Gaussian H, random points of ``const``, Gaussian noise."""
    rs = np.random.RandomState(seed)
    const = np.asarray(const)
    hshape = (nr, nt) if shared else (B, nr, nt)
    h = rs.randn(*hshape) if real else rnd_c(rs, *hshape)
    x = const[rs.randint(0, const.size, (B, nt))]
    n = rs.randn(B, nr) if real else rnd_c(rs, B, nr)
    y = (np.einsum('ij,bj->bi', h, x) if shared else np.einsum('bij,bj->bi', h, x)) + noise * n
    return y, h


def h_of(h, b):
    return h if h.ndim == 2 else h[b]


# (nr, nt, m, B, real): one ML launch each; the kernel note each must leave is the last entry
ML_CASES = [
    (8, 2, 256, 128, False, "mimo_ml_kernel<direct>"),      # 16 * 2 * 256 * 8 B of products do not fit next to the base
    (1, 1, 16, 200, False, "mimo_ml_kernel<table>"),        # P = 1: only lane 0 has a prefix
    (2, 2, 4, 200, False, "mimo_ml_kernel<table>"),         # P = 4: fewer prefixes than lanes
    (6, 3, 64, 128, False, "mimo_ml_kernel<table>"),        # 2^18 hypotheses
    (5, 5, 4, 200, False, "mimo_ml_kernel<table>"),         # 256 prefixes: four passes of the lanes
    (4, 4, 2, 200, True, "mimo_ml_kernel<table>"),          # BPSK, real y and H
]

# (nr, nt, m, K, B, path): path is the kernel storage the arguments take unforced
KB_CASES = [
    (4, 4, 16, 16, 200, "lds"),
    (6, 4, 16, 8, 200, "lds"),
    (8, 8, 4, 7, 200, "lds"),
    (12, 11, 4, 5, 200, "lds"),        # nr (nt + 1) = 144: the [H | y] load and the QR column loop take a second pass
    (12, 11, 64, 7, 128, "lds"),       # nt nbits = 66 LLRs, nk nt = 77 survivor entries
    (5, 3, 64, 70, 200, "lds"),
    (1, 1, 16, 4, 200, "lds"),
    (3, 3, 4, 64, 200, "lds"),         # K is the full width m^nt
    (4, 4, 2, 1, 200, "lds"),          # BPSK: nbits = 1, K = 1
    (4, 4, 16, 1, 200, "lds"),         # one survivor: every bit misses a value, every LLR is +-inf
    (3, 2, 256, 20, 128, "lds"),       # m = 256 within LDS
    (3, 2, 256, 300, 128, "global"),   # 76 800 children: above 64 KB without forcing
    (4, 4, 16, 1024, 64, "global"),    # 16 384 children per level
]
NOISE_VARS = (0.3, 0.0)


def case_seed(kind, i, shared):
    return 20261018 + 1000 * (0 if kind == "ml" else 1) + 10 * i + int(shared)


def ml_case_id(c):
    return "%dx%d_m%d%s" % (c[0], c[1], c[2], "_real" if c[4] else "")


def kb_case_id(c):
    return "%dx%d_m%d_K%d" % c[:4]


# ---- exact ties --------------------------------------------------------------------------------------------------------------
# H: positive powers of two on the diagonal, small dyadic entries above it.  Every product, difference and sum of squares of
# the searches is then an integer multiple of 2^-4 far below 2^53: exact in float64, on LAPACK's QR (which returns R = H, Q = I
# for such a matrix) and on a Householder QR that negates rows (its reflectors are exact here: v = 2 x0 e_k, f = a / x0).
TIE_H3 = np.array([[2.0, 0.5 - 1.0j, 1.5j],
                   [0.0, 4.0, -1.0 + 0.25j],
                   [0.0, 0.0, 1.0]], dtype=np.complex128)
TIE_H2 = np.array([[4.0, 1.0 - 0.5j],
                   [0.0, 2.0]], dtype=np.complex128)


def tie_inputs(qam4, qam16):
    """[(name, y [n, nt], h, const, K)]: the tie cases, one H and several received vectors each.

    ``y = H (x0 + delta)`` with delta moving one or more antennas from an odd-integer point onto an even integer: the midpoint of
    two points; y = 0 is the midpoint of all."""
    q4, q16 = np.asarray(qam4, dtype=np.complex128), np.asarray(qam16, dtype=np.complex128)
    out = []
    # QPSK 3x3: the origin, then one antenna at a time on a one-axis midpoint, then all of them on two-axis midpoints
    x0 = np.array([1 + 1j, -1 + 1j, 1 - 1j])
    xs = np.array([np.zeros(3), x0 + [0, 0, -1], x0 + [0, 1, 0], x0 + [-1, 0, 0], x0 + [-1j, 0, 0], [0, 2j, 0],
                   x0 + [-1 - 1j, 0, 1j]], dtype=np.complex128)
    out.append(("qpsk_3x3_K3", xs.dot(TIE_H3.T), TIE_H3, q4, 3))
    out.append(("qpsk_3x3_K2", xs.dot(TIE_H3.T), TIE_H3, q4, 2))
    out.append(("qpsk_3x3_K5", xs.dot(TIE_H3.T), TIE_H3, q4, 5))
    # 16-QAM 2x2
    x0 = np.array([3 - 1j, -1 + 3j])
    xs = np.array([np.zeros(2), x0 + [0, 1], x0 + [1j, 0], x0 + [-1, 0], x0 + [1 + 1j, -1 - 1j], [2, 2j], [0, -2 + 2j]],
                  dtype=np.complex128)
    out.append(("qam16_2x2_K4", xs.dot(TIE_H2.T), TIE_H2, q16, 4))
    out.append(("qam16_2x2_K6", xs.dot(TIE_H2.T), TIE_H2, q16, 6))
    # a power-of-two multiple of the identity: every antenna decides alone
    xs = np.array([np.zeros(3), [2, 1 + 1j, -1 - 1j], [1 + 1j, 2j, -1 + 1j], [1 - 1j, -1 - 1j, 0]], dtype=np.complex128)
    out.append(("qpsk_2I_K3", 2.0 * xs, 2.0 * np.eye(3, dtype=np.complex128), q4, 3))
    return out


# ---- the random cases with their model answers, computed once per process ---------------------------------------------------------
_cache = {}


def ml_case(i, shared, const):
    """(y, h, want indices [B, nt], keep [B] bool) of ML_CASES[i]; ``keep`` is False where the model's gap is at most GAP_MIN."""
    key = ("ml", i, shared)
    if key not in _cache:
        nr, nt, m, B, real, _ = ML_CASES[i]
        assert len(const) == m
        y, h = random_inputs(case_seed("ml", i, shared), B, nr, nt, const, shared, real)
        res = [ml_model(y[b], h_of(h, b), const) for b in range(B)]
        _cache[key] = (y, h, np.array([r[0] for r in res]), np.array([r[1] > GAP_MIN for r in res]))
    return _cache[key]


def kb_case(i, shared, const):
    """(y, h, lists [B, Ke, nt] padded with -1, counts [B], keep [B] bool, {noise_var: LLRs [B, nt nbits]}) of KB_CASES[i]."""
    key = ("kb", i, shared)
    if key not in _cache:
        nr, nt, m, K, B, _ = KB_CASES[i]
        assert len(const) == m
        y, h = random_inputs(case_seed("kb", i, shared), B, nr, nt, const, shared)
        ke = min(K, m ** nt)
        res = [kbest_model(y[b], h_of(h, b), const, K) for b in range(B)]
        llr = {nv: np.array([kbest_llr_model(y[b], h_of(h, b), const, res[b][0], nv) for b in range(B)]) for nv in NOISE_VARS}
        _cache[key] = (y, h, np.array([pad_list(r[0], ke) for r in res]), np.array([r[1] for r in res], dtype=np.int32),
                       np.array([r[2] > GAP_MIN for r in res]), llr)
    return _cache[key]


def assert_llr(got, want):
    """The LLR rule of tests/test_mimo_gpu.py: the same NaN / +-inf pattern, finite values within 1e-9 relative (absolute below 1)."""
    got, want = np.asarray(got), np.asarray(want)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.array_equal(np.where(np.isfinite(want), 0, got), np.where(np.isfinite(want), 0, want), equal_nan=True)
    fin = np.isfinite(want)
    assert np.all(np.abs(got[fin] - want[fin]) <= 1e-9 * np.maximum(1, np.abs(want[fin])))


# ---- the grid wrap: 2x2 QPSK, 2^20 + 70 vectors so that workgroups 0..69 of the LDS paths take a second vector ------------------
WRAP_B = (1 << 20) + 70
WRAP_SEL = np.concatenate((np.arange(70), np.arange(1 << 20, WRAP_B)))
WRAP_NAN = 3               # a NaN vector whose successor in the same workgroup, 2^20 + 3, must come out clean
WRAP_K = 2
WRAP_NOISE_VAR = 0.3


def wrap_case(const):
    """(y [WRAP_B, 2], h [WRAP_B, 2, 2], {output: model answer on WRAP_SEL}, keep [140] bool)."""
    key = ("wrap",)
    if key not in _cache:
        y, h = random_inputs(20261019, WRAP_B, 2, 2, const, False)
        y[WRAP_NAN, 1] = np.nan
        ml = [ml_model(y[b], h[b], const) for b in WRAP_SEL]
        kb = [kbest_model(y[b], h[b], const, WRAP_K) for b in WRAP_SEL]
        want = {"ml": np.array([r[0] for r in ml]), "hard": np.array([r[0][0] for r in kb]),
                "soft": np.array([kbest_llr_model(y[b], h[b], const, r[0], WRAP_NOISE_VAR) for b, r in zip(WRAP_SEL, kb)])}
        keep = np.array([(a[1] > GAP_MIN and k[2] > GAP_MIN) or b == WRAP_NAN for a, k, b in zip(ml, kb, WRAP_SEL)])
        _cache[key] = (y, h, want, keep)
    return _cache[key]


# ---- NaN and inf inside an ordinary batch: 4x3 16-QAM, one H per vector ----------------------------------------------------------
SPECIAL_B, SPECIAL_K = 130, 8
SPECIAL = {"nan_y": 5, "inf_y": 64, "nan_h": 129}


def special_inputs(const):
    """(clean y, clean h, y, h): a batch of 130 ordinary vectors and the same with a NaN in one y, +inf in another and a NaN
    entry in the H of a third -- below the diagonal of column 0, where only a QR that lets the NaN through notices it."""
    y0, h0 = random_inputs(20261020, SPECIAL_B, 4, 3, const, False)
    y, h = y0.copy(), h0.copy()
    y[SPECIAL["nan_y"], 2] = np.nan
    y[SPECIAL["inf_y"], 1] = np.inf
    h[SPECIAL["nan_h"], 2, 0] = np.nan
    return y0, h0, y, h
