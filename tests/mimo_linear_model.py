"""Plain NumPy float64 model of the linear MIMO detectors of csrc/mimo_linear.hip (zero forcing / MMSE, hard and soft), an
exact-rational second evaluation of the equaliser, and the inputs both are compared on.  No GPU, no engine import.

Shared by tests/test_mimo_linear_host.py (which checks the model against the exact solve and against the textbook identities)
and tests/test_mimo_linear_gpu.py (which holds the kernels to the model).

The contract modelled, per received vector, with m = 2^nb points, a regulariser reg >= 0 and an LLR scale noise_var:

* ``A = H^H H + reg I`` (Hermitian), ``b = H^H y``; ``A = L L^H`` by ``np.linalg.cholesky``, ``z = np.linalg.solve(A, b)``,
  ``a_i = (A^-1)_ii = sum_j |(L^-1)_ji|^2``; ``g_i = 1 - reg a_i``.
* unbiased estimate ``xhat_i = z_i / g_i``, effective noise variance ``nu_i = noise_var a_i / g_i``; reg = 0 is zero forcing
  (``xhat = pinv(H) y``, ``nu_i = noise_var a_i``), reg = N0 / Es unbiased MMSE.
* hard: the first minimum of ``|xhat_i - s|^2`` over the points in index order (strict ``<`` from index 0: ties to the lowest
  index).  soft: ``llr[i nb + k] = (min over the points whose bit k is 1 - min over those whose bit k is 0) / (2 nu_i)``, the bits
  being the MSB-first bits of the point's index; positive means bit 0.
* a vector FAILS when a Cholesky pivot is not a positive finite number (singular H under ZF, nt > nr with reg = 0, NaN / inf in
  H; positive in float64's terms: rounding leaves an exactly singular A a pivot of either sign of the order of
  ``(nr + nt) 2^-52 A_jj``, so the pivot ``L_jj^2`` of column j must exceed ``PIVOT_TOL(nr, nt) A_jj = 4 (nr + nt) 2^-52 A_jj``), when b is not finite (NaN / inf in y) or when some g_i is not positive: xhat, nu and the LLRs are NaN, the indices 0.

Squares of complex numbers are taken as ``re^2 + im^2``.

``margin`` is the model's own measure of how close a vector is to a tie: the second-smallest minus the smallest distance, the
minimum over its streams.  A vector whose margin is below ``MARGIN_MIN * Es`` is not a fair exact-equality case for the indices;
that is a condition on the input, never a tolerance on an output.

The bound on xhat and nu.  Kernel and model are both backward-stable solves of the same system, so each differs from the exact
answer by a small multiple of ``nt nr 2^-52 kappa_2(A)`` in the 2-norm, relative.  The model's own worst ratio against the exact
rational solve (``exact_equalize``) over the 64 seeded vectors of ``ACCURACY_CASES`` -- ``measure_model_ratio()``, run by
tests/test_mimo_linear_host.py -- is 1.25 (xhat: 0.496, nu: 1.248; the ratio is error / (nt nr 2^-52 kappa_2(A)), and the
worst cases are the 1 x 1 ones, where kappa = 1 and the error is a rounding or two).  Four times that, rounded up to a power of
two: ``K_BOUND = 8``.  The kernel sums in another order than LAPACK and
multiplies by reciprocals of the pivots; two stable algorithms differ by such a small constant.
"""
from fractions import Fraction

import numpy as np

from mimo_model import BPSK, rnd_c

MARGIN_MIN = 1e-9
MARGIN_CAP = 0.001          # at most this share of a batch may be left out as a near-tie
EPS = 2.0 ** -52
MODEL_RATIO = 1.25          # measure_model_ratio() on ACCURACY_CASES, rounded up in the last digit
K_BOUND = 8.0               # 4 * MODEL_RATIO rounded up to a power of two
KAPPA_XHAT = 1e4            # inputs of the xhat / nu comparison have kappa_2(A) <= this
KAPPA_LLR = 1e2             # ... of the LLR comparison


def _sq(z):
    z = np.asarray(z, dtype=np.complex128)
    return z.real * z.real + z.imag * z.imag


def h_all(h, B):
    h = np.asarray(h, dtype=np.complex128)
    return np.broadcast_to(h, (B,) + h.shape[-2:]) if h.ndim == 2 else h


def gram(h, reg):
    """A = H^H H + reg I of every vector [B, nt, nt] (h already [B, nr, nt])."""
    with np.errstate(all="ignore"):
        return np.matmul(h.conj().transpose(0, 2, 1), h) + reg * np.eye(h.shape[2])


def kappa(h, reg, B=None):
    """kappa_2(A) of every vector (inf where A is singular or not finite)."""
    A = gram(h_all(h, B if B is not None else len(h)), reg)
    out = np.full(len(A), np.inf)
    ok = np.isfinite(A).all(axis=(1, 2))
    if ok.any():
        ev = np.linalg.eigvalsh(A[ok])
        with np.errstate(all="ignore"):
            out[ok] = np.where(ev[:, 0] > 0, ev[:, -1] / ev[:, 0], np.inf)
    return out


def pivot_tol(nr, nt):
    return 4.0 * (nr + nt) * EPS


def equalize_model(y, h, reg, noise_var):
    """(xhat [B, nt], nu [B, nt], bad [B]) of ``y [B, nr]`` and ``h`` [nr, nt] or [B, nr, nt]."""
    y = np.atleast_2d(np.asarray(y, dtype=np.complex128))
    B = len(y)
    H = h_all(h, B)
    nt = H.shape[2]
    xhat = np.full((B, nt), np.nan + 1j * np.nan)
    nu = np.full((B, nt), np.nan)
    bad = np.ones(B, dtype=bool)
    with np.errstate(all="ignore"):
        A = gram(H, reg)
        bv = np.matmul(H.conj().transpose(0, 2, 1), y[:, :, None])[:, :, 0]
    eye = np.eye(nt)
    for v in np.flatnonzero(np.isfinite(A).all(axis=(1, 2)) & np.isfinite(bv).all(axis=1)):
        try:
            L = np.linalg.cholesky(A[v])
        except np.linalg.LinAlgError:
            continue
        piv = L.diagonal().real ** 2
        if not np.all((piv > pivot_tol(H.shape[1], nt) * A[v].diagonal().real) & np.isfinite(piv)):
            continue
        z = np.linalg.solve(A[v], bv[v])
        a = _sq(np.linalg.solve(L, eye)).sum(axis=0)
        g = 1.0 - reg * a
        if not np.all(g > 0):
            continue
        xhat[v], nu[v], bad[v] = z / g, noise_var * a / g, False
    return xhat, nu, bad


def index_bits(m):
    nb = int(np.log2(m))
    return (np.arange(m)[:, None] >> np.arange(nb - 1, -1, -1)) & 1


def slice_model(xhat, nu, bad, const):
    """(idx [B, nt] int32, llr [B, nt nb], margin [B]) from the equaliser's outputs."""
    c = np.asarray(const, dtype=np.complex128)
    B, nt = xhat.shape
    nb = int(np.log2(c.size))
    with np.errstate(all="ignore"):
        d = _sq(xhat[:, :, None] - c[None, None, :])                  # [B, nt, m]
        idx = np.zeros((B, nt), dtype=np.int32)
        for s in range(1, c.size):                                     # strict <, from index 0
            best = np.take_along_axis(d, idx[:, :, None].astype(np.int64), axis=2)[:, :, 0]
            idx = np.where(d[:, :, s] < best, s, idx).astype(np.int32)
        two = np.sort(d, axis=2)[:, :, :2]
        margin = (two[:, :, 1] - two[:, :, 0]).min(axis=1)
        bits = index_bits(c.size)
        llr = np.empty((B, nt, nb))
        for k in range(nb):
            one = bits[:, k] == 1
            llr[:, :, k] = (d[:, :, one].min(axis=2) - d[:, :, ~one].min(axis=2)) / (2.0 * nu)
    idx[bad] = 0
    llr[bad] = np.nan
    margin = np.where(bad, np.inf, margin)
    return idx, llr.reshape(B, nt * nb), margin


def linear_model(y, h, const, reg, noise_var):
    """dict(xhat, nu, bad, idx, llr, margin) of one batch."""
    xhat, nu, bad = equalize_model(y, h, reg, noise_var)
    idx, llr, margin = slice_model(xhat, nu, bad, const)
    return dict(xhat=xhat, nu=nu, bad=bad, idx=idx, llr=llr, margin=margin)


# ---- exact rational evaluation ---------------------------------------------------------------------------------------------------
def _fc(z):
    z = complex(z)
    return Fraction(z.real), Fraction(z.imag)


def _fmul(a, b):
    return a[0] * b[0] - a[1] * b[1], a[0] * b[1] + a[1] * b[0]


def _fsub(a, b):
    return a[0] - b[0], a[1] - b[1]


def _fdiv(a, b):
    n = b[0] * b[0] + b[1] * b[1]
    return (a[0] * b[0] + a[1] * b[1]) / n, (a[1] * b[0] - a[0] * b[1]) / n


def exact_equalize(y, h, reg, noise_var):
    """(xhat [nt] complex, nu [nt]) of ONE vector: A = H^H H + reg I and b = H^H y formed and the complex systems A z = b and
    A X = I solved by Gaussian elimination, all in exact rational arithmetic on the float64 inputs; rounded once at the end."""
    nr, nt = np.asarray(h).shape
    H = [[_fc(h[r][t]) for t in range(nt)] for r in range(nr)]
    Y = [_fc(v) for v in y]
    rg, nv = Fraction(float(reg)), Fraction(float(noise_var))
    zero, one = (Fraction(0), Fraction(0)), (Fraction(1), Fraction(0))
    rows = []
    for i in range(nt):
        row = []
        for j in range(nt):
            s = zero
            for r in range(nr):
                p = _fmul((H[r][i][0], -H[r][i][1]), H[r][j])
                s = (s[0] + p[0], s[1] + p[1])
            row.append((s[0] + rg, s[1]) if i == j else s)
        s = zero
        for r in range(nr):
            p = _fmul((H[r][i][0], -H[r][i][1]), Y[r])
            s = (s[0] + p[0], s[1] + p[1])
        rows.append(row + [s] + [one if k == i else zero for k in range(nt)])
    w = 2 * nt + 1
    for col in range(nt):                                  # Gauss-Jordan; A is positive definite, so no pivot is zero
        piv = rows[col][col]
        rows[col] = [_fdiv(v, piv) for v in rows[col]]
        for i in range(nt):
            if i != col and rows[i][col] != zero:
                f = rows[i][col]
                rows[i] = [_fsub(rows[i][k], _fmul(f, rows[col][k])) for k in range(w)]
    xhat, nu = np.empty(nt, dtype=np.complex128), np.empty(nt)
    for i in range(nt):
        a = rows[i][nt + 1 + i][0]
        g = 1 - rg * a
        xhat[i] = complex(float(rows[i][nt][0] / g), float(rows[i][nt][1] / g))
        nu[i] = float(nv * a / g)
    return xhat, nu


# ---- inputs --------------------------------------------------------------------------------------------------------------------
def conditioned_inputs(seed, B, nr, nt, const, shared, smax, noise=0.3, real=False):
    """(y [B, nr], h [nr, nt] or [B, nr, nt]): H = U diag(s) V^H with U, V from the QR of Gaussian matrices and singular values
    uniform in [1, smax], so that kappa_2(H^H H) <= smax^2 wherever nr >= nt; random points of ``const`` plus Gaussian noise."""
    rs = np.random.RandomState(seed)
    const = np.asarray(const)
    n = 1 if shared else B
    k = min(nr, nt)
    draw = (lambda *s: rs.randn(*s)) if real else (lambda *s: rnd_c(rs, *s))
    U = np.linalg.qr(draw(n, nr, nr))[0][:, :, :k]
    V = np.linalg.qr(draw(n, nt, nt))[0][:, :, :k]
    s = 1.0 + (smax - 1.0) * rs.rand(n, k)
    h = np.matmul(U * s[:, None, :], np.conj(V).transpose(0, 2, 1))
    x = const[rs.randint(0, const.size, (B, nt))]
    y = np.matmul(h, x[:, :, None])[:, :, 0] + noise * draw(B, nr)
    return y, (h[0] if shared else h)


def const_of(m):
    """The points the GPU tests use for m: real BPSK for 2, else the reference's Gray-indexed square QAM."""
    if m == 2:
        return BPSK.copy()
    side = int(np.sqrt(m))
    pam = np.arange(-side + 1, side, 2)
    pts = np.tile(np.hstack((pam, pam[::-1])), side // 2) * 1j + pam.repeat(side)
    idx = np.arange(m)
    return pts[(idx ^ (idx >> 1)).argsort()]


# (nr, nt, m, B, shared): the shapes of the kernel comparison.  nt <= 8: one vector per lane; nt >= 9: one wave per vector.
# nr = nt, nt + 3 and nt - 1 (MMSE only), every m, B around one workgroup of 64 vectors
CASES = [
    (1, 1, 16, 65, False), (4, 1, 2, 64, True),
    (2, 2, 4, 63, False), (5, 2, 64, 65, True), (1, 2, 16, 64, False),
    (3, 3, 2, 65, True), (6, 3, 16, 1, False), (2, 3, 4, 63, False),
    (4, 4, 16, 200, False), (4, 4, 64, 65, True), (7, 4, 4, 64, False), (3, 4, 16, 65, False),
    (8, 8, 4, 65, False), (8, 8, 16, 63, True), (11, 8, 64, 64, False), (7, 8, 2, 65, False),
    (9, 9, 4, 65, False), (12, 9, 16, 63, True), (8, 9, 2, 64, False),
    (12, 12, 16, 65, False), (15, 12, 4, 1, True), (11, 12, 64, 63, False),
]
SMAX_LLR = 8.0              # kappa_2(A) <= 64 under ZF
SMAX_XHAT = 60.0            # kappa_2(A) <= 3600 under ZF: the ill-conditioned set of the xhat / nu comparison
NOISE_VAR = 0.3
# the 64 vectors that are also solved exactly, to measure the model's own error: (case, condition set, method, vectors) -- vector 0 of
# every case under both condition sets, the method alternating, and ten more of the 4x4 16-QAM case under each
ACCURACY_CASES = [(i, smax, i % 2, (0,)) for i in range(len(CASES)) for smax in (SMAX_LLR, SMAX_XHAT)] + \
                 [(8, smax, j, tuple(range(1, 11))) for j, smax in enumerate((SMAX_LLR, SMAX_XHAT))]


def case_id(c):
    return "%dx%d_m%d_B%d_%s" % (c[0], c[1], c[2], c[3], "shared" if c[4] else "own")


def case_seed(i, smax):
    return 20261101 + 10 * i + int(smax > 10)


def case_reg(c, method, const):
    """The regulariser of a case: 0 for ZF, noise_var / Es for MMSE; 1 where nt > nr (nt - nr eigenvalues of A are reg itself, and
    kappa_2(A) = (smax^2 + reg) / reg has to stay within the comparison's range)."""
    if method == "zf":
        return 0.0
    return 1.0 if c[1] > c[0] else NOISE_VAR / float(np.mean(_sq(const)))


def methods_of(c):
    return ("zf", "mmse") if c[0] >= c[1] else ("mmse",)


_cache = {}


def case(i, smax=SMAX_LLR):
    """(y, h, const, {method: model dict}) of CASES[i], computed once per process and never modified."""
    key = (i, smax)
    if key not in _cache:
        nr, nt, m, B, shared = CASES[i]
        const = const_of(m)
        y, h = conditioned_inputs(case_seed(i, smax), B, nr, nt, const, shared, smax, real=(m == 2))
        want = {me: linear_model(y, h, const, case_reg(CASES[i], me, const), NOISE_VAR) for me in methods_of(CASES[i])}
        _cache[key] = (y, h, const, want)
    return _cache[key]


def rel_err(got, want):
    """Per-vector relative error in the 2-norm, [B]."""
    with np.errstate(all="ignore"):
        return np.linalg.norm(got - want, axis=1) / np.linalg.norm(want, axis=1)


def measure_model_ratio():
    """(worst xhat ratio, worst nu ratio, vectors) of the float64 model against the exact solve over ACCURACY_CASES:
    error / (nt nr 2^-52 kappa_2(A))."""
    worst, count = [0.0, 0.0], 0
    for i, smax, which, vectors in ACCURACY_CASES:
        nr, nt = CASES[i][:2]
        y, h, const, want = case(i, smax)
        me = methods_of(CASES[i])[which % len(methods_of(CASES[i]))]
        reg = case_reg(CASES[i], me, const)
        vs = [v for v in vectors if v < len(y)]
        kap = kappa(h, reg, len(y))[vs]
        ex = [exact_equalize(y[b], h if h.ndim == 2 else h[b], reg, NOISE_VAR) for b in vs]
        unit = nt * nr * EPS * kap
        worst[0] = max(worst[0], float(np.max(rel_err(want[me]["xhat"][vs], np.array([e[0] for e in ex])) / unit)))
        worst[1] = max(worst[1], float(np.max(rel_err(want[me]["nu"][vs], np.array([e[1] for e in ex])) / unit)))
        count += len(vs)
    return worst[0], worst[1], count


# ---- the grid wrap ---------------------------------------------------------------------------------------------------------------
REG_GRID, WAVE_GRID = 2048, 4096         # workgroups of a launch of the two kernels (mimo_linear.hip)
WRAP_REG_B = 64 * REG_GRID + 65          # one vector per lane: workgroups 0 and 1 take a second tile, the second one partial
WRAP_WAVE_B = WAVE_GRID + 70             # one wave per vector: workgroups 0..69 take a second vector
