"""Edge-case received symbols for the demodulators, and the contract their hard decisions are held to.

Shared by tests/test_demod_edges_gpu.py, tests/test_demod_edges_host.py and scripts/fuzz_gpu.py.

The reference rule is ``abs(y - c[:, None]).argmin(0)``: the first minimum of ``hypot(fl(y.re - c.re), fl(y.im - c.im))``.
``hard_contract`` sorts every symbol into one of three classes by exact rational arithmetic on the same rounded differences
the rule takes the hypot of (float64 values are dyadic rationals: their squares are summed exactly as integers over a common
power of two, the order ``fractions.Fraction`` would give):

* ``EXACT``: every float64 distance is the same non-finite value (all inf, or all NaN), or only one label lies within the
  2-ulp band of the exact minimum -- the kernel must return what the reference returns;
* ``TIE``: several labels lie in the band and their exact distances are equal (so their float64 distances are bit-identical)
  -- the kernel must return the lowest of them, as the first-minimum rule does;
* ``ROUND``: several labels lie in the band only because the distances are within rounding of each other -- the kernel's
  label must lie in the band.  The device ``hypot`` is not guaranteed to round like the host's, so bit equality with the
  reference cannot be promised there.

The band is every label whose exact distance exceeds the exact minimum by at most 2 ulps, an ulp taken as its upper bound
2^-52 of the distance: ``D_m <= D_min (1 + 2^-51)^2`` on the squared distances.
"""
from fractions import Fraction

import numpy as np

EXACT, TIE, ROUND = 0, 1, 2
BIG = (1e3, 1e5, 1e8, 1e150, 1e300)
_BAND = (1 + Fraction(1, 2 ** 51)) ** 2
_BAND_NUM, _BAND_DEN = _BAND.numerator, _BAND.denominator


def _exact_sq(diffs):
    """Exact |d|^2 of float64 complex values, as integers over one common power of two (the same scale for every entry)."""
    parts = [float(v) for z in diffs for v in (z.real, z.imag)]
    ratios = [v.as_integer_ratio() for v in parts]
    K = max(den.bit_length() for _, den in ratios)
    ints = [num << (K - den.bit_length()) for num, den in ratios]
    return [ints[2 * j] ** 2 + ints[2 * j + 1] ** 2 for j in range(len(diffs))]


def labels_of(bits, nb):
    """MSB-first int8 bits [n * nb] -> labels [n]."""
    b = np.asarray(bits, dtype=np.int64).reshape(-1, nb)
    return b.dot(1 << np.arange(nb - 1, -1, -1))


def _ulps(v, k):
    out = v
    for _ in range(k):
        out = np.nextafter(out, np.inf)
    lo = v
    for _ in range(k):
        lo = np.nextafter(lo, -np.inf)
    return [out, lo]


def edge_symbols(c, rs, big=BIG):
    """Edge-case symbols for constellation ``c`` (complex [M]) and a class name per symbol: exact points, midpoints between
    adjacent grid levels (one axis, both axes, the origin), the boundaries +-1, 2 and 64 ulps, boundaries with the other
    component at each magnitude of ``big``, every combination of {finite, +inf, -inf, NaN} in the two components, both
    components beyond the overflow of hypot, subnormal offsets and -0.0."""
    c = np.asarray(c, dtype=np.complex128)
    M = c.size
    xs, ys = np.unique(c.real), np.unique(c.imag)
    if xs.size > 16:
        xs = np.sort(rs.choice(xs, 16, replace=False))
    if ys.size > 16:
        ys = np.sort(rs.choice(ys, 16, replace=False))
    xb = (xs[:-1] + xs[1:]) / 2 if xs.size > 1 else xs.copy()
    yb = (ys[:-1] + ys[1:]) / 2 if ys.size > 1 else ys.copy()
    out = []

    def add(cls, re, im):
        out.append((cls, complex(float(re), float(im))))

    pts = c if M <= 256 else c[rs.choice(M, 64, replace=False)]
    for p in pts:
        add("point", p.real, p.imag)
    for b in xb:
        add("mid1", b, rs.choice(ys))
    for b in yb:
        add("mid1", rs.choice(xs), b)
    for bx in xb:
        for by in yb[:8]:
            add("mid2", bx, by)
    for re, im in ((0.0, 0.0), (-0.0, 0.0), (0.0, -0.0), (-0.0, -0.0)):
        add("origin", re, im)
    for i in rs.choice(M, min(M, 16), replace=False):        # midpoints of nearest pairs (PSK, custom tables)
        dd = np.abs(c - c[i])
        dd[i] = np.inf
        j = int(np.argmin(dd))
        mid = (c[i] + c[j]) / 2
        add("pairmid", mid.real, mid.imag)
    for k in (1, 2, 64):
        for b in xb:
            for v in _ulps(b, k):
                add("ulp", v, rs.choice(ys))
        for b in yb:
            for v in _ulps(b, k):
                add("ulp", rs.choice(xs), v)
    offs = (0.0, 5e-324, 1e-300, 1e-12, 1e-7, 5e-7)
    for B in big:
        for s in (1.0, -1.0):
            for b in xb[:4]:
                for o in offs:
                    add("big", b + o * rs.choice((-1, 1)), s * B)
                for v in _ulps(b, 1):
                    add("big", v, s * B)
            for b in yb[:4]:
                for o in offs:
                    add("big", s * B, b + o * rs.choice((-1, 1)))
            add("big", rs.choice(xs), s * B)
            add("big", s * B, rs.choice(ys))
            add("big", s * B, s * B * 0.5)
    fin = [0.3, -2.0, 5.1, float(xs[0]), float(xb[0])]
    spec = [np.inf, -np.inf, np.nan]
    for f in fin:
        for s in spec:
            add("nonfinite", f, s)
            add("nonfinite", s, f)
    for s1 in spec:
        for s2 in spec:
            add("nonfinite", s1, s2)
    for s1 in (1.0, -1.0):
        for s2 in (1.0, -1.0):
            add("overflow", s1 * 1.3e308, s2 * 1.5e308)
            add("overflow", s1 * 1.7e308, s2 * 1.0e308)
            add("overflow", s1 * np.finfo(float).max, s2 * np.finfo(float).max)
    for t in (5e-324, -5e-324, 2.2e-310, -2.2e-310, -0.0):
        add("subnormal", t, rs.choice(ys))
        add("subnormal", rs.choice(xs), t)
        add("subnormal", t, t)
        for b in xb[:2]:
            add("subnormal", b + t, rs.choice(ys))
    cls = np.array([o[0] for o in out])
    y = np.array([o[1] for o in out], dtype=np.complex128)
    return y, cls


def scatter(c, edges, n, rs, noise=0.3):
    """``n`` noisy constellation points with edge symbols at random positions: all of them (or as many as fit), at least one.
    Returns (y, positions of the edge symbols)."""
    c = np.asarray(c, dtype=np.complex128)
    y = c[rs.randint(0, c.size, n)] + noise * (rs.randn(n) + 1j * rs.randn(n))
    k = max(1, min(n // 2 if n > 1 else 1, edges.size)) if n < 2 * edges.size else edges.size
    pos = rs.choice(n, k, replace=False)
    y[pos] = edges[rs.choice(edges.size, k, replace=False)] if k < edges.size else edges
    return y, pos


def hard_contract(c, y):
    """(kind [n], band [n] of label lists or None, ref [n]): the class of every symbol (EXACT / TIE / ROUND, see the module
    docstring), its 2-ulp band where it has more than one label, and the reference rule's label (literal NumPy)."""
    c = np.asarray(c, dtype=np.complex128)
    y = np.asarray(y, dtype=np.complex128).reshape(-1)
    n = y.size
    kind = np.full(n, EXACT, dtype=np.int64)
    band = [None] * n
    with np.errstate(all="ignore"):
        diff = y[:, None] - c[None, :]
        d = np.abs(diff)
        ref = d.argmin(1)
        fin = np.isfinite(d)
        dmin = np.where(fin, d, np.inf).min(1)
        cand = fin & (d <= dmin[:, None] * (1 + 2.0 ** -45))
    ncand = cand.sum(1)
    for i in np.nonzero(ncand > 1)[0]:
        ms = np.nonzero(cand[i])[0]
        D = _exact_sq(diff[i, ms])
        Dmin = min(D)
        inb = [int(m) for m, v in zip(ms, D) if v * _BAND_DEN <= Dmin * _BAND_NUM]
        if len(inb) == 1:
            continue
        vals = {v for m, v in zip(ms, D) if int(m) in inb}
        kind[i] = TIE if len(vals) == 1 else ROUND
        band[i] = inb
    return kind, band, ref


def hard_violations(c, y, got):
    """Indices of the symbols whose label ``got`` breaks the contract, and the number of ROUND symbols."""
    kind, band, ref = hard_contract(c, y)
    got = np.asarray(got).reshape(-1)
    bad = []
    for i in range(len(got)):
        if kind[i] == EXACT:
            ok = got[i] == ref[i]
        elif kind[i] == TIE:
            ok = got[i] == min(band[i])
        else:
            ok = int(got[i]) in band[i]
        if not ok:
            bad.append(i)
    return bad, int(np.sum(kind == ROUND))


def soft_literal(c, y, noise_var):
    """The reference's soft rule as literal NumPy: per bit, sums of exp(-|y - c_m|^2 / noise_var) in constellation order,
    LLR = log(num / den), MSB first."""
    c = np.asarray(c, dtype=np.complex128)
    y = np.asarray(y, dtype=np.complex128).reshape(-1)
    M = c.size
    nb = int(np.log2(M))
    out = np.zeros(y.size * nb)
    with np.errstate(all="ignore"):
        e = np.exp((-np.abs(y[:, None] - c[None, :]) ** 2) / noise_var)     # [n, M]
        for b in range(nb):
            num = np.zeros(y.size)
            den = np.zeros(y.size)
            for m in range(M):                                              # sequential, in constellation order
                if (m >> b) & 1:
                    num = num + e[:, m]
                else:
                    den = den + e[:, m]
            out[nb - 1 - b::nb] = np.log(num / den)
    return out


def same_soft(got, want, tol=1e-9):
    """NaN / +inf / -inf patterns identical and finite values within ``tol``; returns the indices that break it."""
    got, want = np.asarray(got), np.asarray(want)
    pat = (np.isnan(got) != np.isnan(want)) | (np.isposinf(got) != np.isposinf(want)) | (np.isneginf(got) != np.isneginf(want))
    fin = np.isfinite(want) & np.isfinite(got)
    far = np.zeros(got.shape, bool)
    far[fin] = np.abs(got[fin] - want[fin]) > tol
    return np.nonzero(pat | far)[0]
