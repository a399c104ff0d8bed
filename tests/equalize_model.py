"""NumPy model of the MMSE linear and decision-feedback equalisers (csrc/equalize.hip) -- TEST INFRASTRUCTURE ONLY.

``y_t = sum_l h_l x_{t-l} + w_t`` with ``x_t = c[a_t]`` for ``0 <= t < n`` and 0 elsewhere; ``Es`` the mean symbol energy, ``N0`` the
noise variance, ``d`` the delay, ``nf`` feed-forward and ``nb`` feedback taps.  The rule, as the header, the kernel and
``mmse_equalize_batch`` state it (float64, real and imaginary parts separate doubles, every product rounded before it is added, every
sum from 0.0 in ascending index order; ``a b = (ar br - ai bi, ar bi + ai br)``, ``a conj(b) = (ar br + ai bi, ai br - ar bi)``):

    design      H[i][k] = h_{k-i} for 0 <= k-i < L (i < nf); K = all columns but d+1 .. d+nb.  For j <= i:
                S[i][j] = sum over k in K, i <= k < j+L, of h_{k-i} conj(h_{k-j}); R[i][j] = Es S[i][j], and + N0 on the diagonal, whose
                imaginary part is never computed.  p_i = Es h_{d-i} (0 outside the taps).
    L D L^H     column j: g_k = (D_k Lr[j][k], -(D_k Li[j][k])) for k < j; v_i = R[i][j] - sum_{k<j} L[i][k] g_k for i >= j;
                D_j = Re v_j; L[i][j] = (vr / D_j, vi / D_j) for i > j.
    solve       a_i = p_i - sum_{k<i} L[i][k] a_k; b_i = (ar / D_i, ai / D_i); u_i = b_i - sum_{k>i} u_k conj(L[k][i]), i descending,
                every sum over k ascending.
    taps        ff_i = conj(u_i); fb_j = sum_i ff_i h_{d+j-i} over the i with 0 <= d+j-i < L, j = 1 .. nb;
                gain = sum_i (ffr hr - ffi hi) of h_{d-i} over the i with 0 <= d-i < L; nu = (Es (1 - gain)) / gain.
    equalise    z_t = sum_{i<nf} ff_i y_{t+d-i} - sum_{j=1..nb, t-j>=0} fb_j c[a^_{t-j}], a sample outside the row read as 0.0 and
                multiplied like any other; x^_t = (zr / gain, zi / gain); a^_t = the first minimum over a ascending of
                e = x^_t - c[a], er er + ei ei, a later point winning only if strictly smaller.
    soft        llr[t m + i] = (min over the a with bit i = 1 - min over the a with bit i = 0 of that distance) / nu, bits MSB first,
                each minimum from +inf over a ascending, replaced only by a strictly smaller value.
    rejection   a row whose y, h or noise_var holds a NaN or +-inf (or a noise_var <= 0), one of whose pivots D_j is not positive and
                finite, or whose gain is not a finite number in (0, 1): zero indices and bits, NaN everything else.

Loops over taps, columns, steps and points are Python loops; every operation inside them is one NumPy call on real arrays over the rows.
"""
import numpy as np


def _mul(ar, ai, br, bi):
    return ar * br - ai * bi, ar * bi + ai * br


def _mulc(ar, ai, br, bi):
    """a conj(b)"""
    return ar * br + ai * bi, ai * br - ar * bi


def _complex(re, im):
    """The complex array of two real ones, part by part (``re + 1j * im`` would lose the sign of a zero)."""
    out = np.empty(np.shape(re), dtype=np.complex128)
    out.real, out.imag = re, im
    return out


def default_delay(nf, nb, L):
    return (nf + L - 2) // 2 if nb == 0 else nf - 1


def matrix(hr, hi, Es, N0, nf, nb, d):
    """``(Rr, Ri, pr, pi)``: the lower triangle ``R[i][j]`` (``j <= i``; ``Ri[i][i]`` stays 0) as ``[nf, nf, B]`` and ``p`` ``[nf, B]``."""
    B, L = hr.shape
    Rr, Ri = np.zeros((nf, nf, B)), np.zeros((nf, nf, B))
    pr, pi = np.zeros((nf, B)), np.zeros((nf, B))
    for j in range(nf):
        for i in range(j, nf):
            sr, si = np.zeros(B), np.zeros(B)
            for k in range(i, j + L):
                if d + 1 <= k <= d + nb:
                    continue
                if i == j:
                    sr = sr + (hr[:, k - i] * hr[:, k - j] + hi[:, k - i] * hi[:, k - j])
                else:
                    qr, qi = _mulc(hr[:, k - i], hi[:, k - i], hr[:, k - j], hi[:, k - j])
                    sr, si = sr + qr, si + qi
            if i == j:
                Rr[i, j] = Es * sr + N0
            else:
                Rr[i, j], Ri[i, j] = Es * sr, Es * si
    for i in range(nf):
        if 0 <= d - i < L:
            pr[i], pi[i] = Es * hr[:, d - i], Es * hi[:, d - i]
    return Rr, Ri, pr, pi


def design(h, Es, noise_var, nf, nb=0, delay=None):
    """``{'ff' [B, nf], 'fb' [B, nb], 'gain' [B], 'noise' [B], 'bad' [B]}`` of taps ``h [B, L]`` and ``noise_var [B]`` (no row replaced)."""
    h = np.atleast_2d(np.asarray(h, dtype=np.complex128))
    B, L = h.shape
    d = default_delay(nf, nb, L) if delay is None else delay
    N0 = np.broadcast_to(np.asarray(noise_var, dtype=np.float64), (B,))
    hr, hi = np.ascontiguousarray(h.real), np.ascontiguousarray(h.imag)
    with np.errstate(all='ignore'):
        Rr, Ri, pr, pi = matrix(hr, hi, Es, N0, nf, nb, d)
        Lr, Li, D = np.zeros((nf, nf, B)), np.zeros((nf, nf, B)), np.zeros((nf, B))
        bad = np.zeros(B, dtype=bool)
        for j in range(nf):
            g = [(D[k] * Lr[j, k], -(D[k] * Li[j, k])) for k in range(j)]
            for i in range(j, nf):
                sr, si = np.zeros(B), np.zeros(B)
                for k in range(j):
                    if i == j:
                        sr = sr + (Lr[i, k] * g[k][0] - Li[i, k] * g[k][1])
                    else:
                        qr, qi = _mul(Lr[i, k], Li[i, k], g[k][0], g[k][1])
                        sr, si = sr + qr, si + qi
                if i == j:
                    D[j] = Rr[j, j] - sr
                    bad |= ~((D[j] > 0) & np.isfinite(D[j]))
                else:
                    Lr[i, j], Li[i, j] = (Rr[i, j] - sr) / D[j], (Ri[i, j] - si) / D[j]
        ar, ai = np.zeros((nf, B)), np.zeros((nf, B))
        for i in range(nf):
            sr, si = np.zeros(B), np.zeros(B)
            for k in range(i):
                qr, qi = _mul(Lr[i, k], Li[i, k], ar[k], ai[k])
                sr, si = sr + qr, si + qi
            ar[i], ai[i] = pr[i] - sr, pi[i] - si
        br, bi = ar / D, ai / D
        ur, ui = np.zeros((nf, B)), np.zeros((nf, B))
        for i in range(nf - 1, -1, -1):
            sr, si = np.zeros(B), np.zeros(B)
            for k in range(i + 1, nf):
                qr, qi = _mulc(ur[k], ui[k], Lr[k, i], Li[k, i])
                sr, si = sr + qr, si + qi
            ur[i], ui[i] = br[i] - sr, bi[i] - si
        fr, fi = ur, -ui
        fbr, fbi = np.zeros((nb, B)), np.zeros((nb, B))
        for j in range(1, nb + 1):
            sr, si = np.zeros(B), np.zeros(B)
            for i in range(max(0, d + j - L + 1), min(nf - 1, d + j) + 1):
                qr, qi = _mul(fr[i], fi[i], hr[:, d + j - i], hi[:, d + j - i])
                sr, si = sr + qr, si + qi
            fbr[j - 1], fbi[j - 1] = sr, si
        gain = np.zeros(B)
        for i in range(max(0, d - L + 1), min(nf - 1, d) + 1):
            gain = gain + (fr[i] * hr[:, d - i] - fi[i] * hi[:, d - i])
        nu = (Es * (1.0 - gain)) / gain
        bad |= ~(np.isfinite(gain) & (gain > 0) & (gain < 1))
    return {'ff': _complex(fr.T, fi.T), 'fb': _complex(fbr.T, fbi.T), 'gain': gain, 'noise': nu, 'bad': bad,
            'R': (Rr, Ri), 'p': (pr, pi), 'u': (ur, ui)}


def equalize(y, h, const, Es, noise_var, nf, nb=0, delay=None, tail=True):
    """Every result of ``mmse_equalize_batch`` by name ('bits' and 'llr' only for a power-of-two constellation) for rows ``y [B, n_y]``
    through taps ``h [L]`` or ``[B, L]`` over the points ``const [M]`` (label = position) of mean energy ``Es``."""
    y = np.atleast_2d(np.asarray(y, dtype=np.complex128))
    B, n_y = y.shape
    h = np.asarray(h, dtype=np.complex128)
    h = np.broadcast_to(h, (B, h.shape[-1])) if h.ndim == 1 else h
    L = h.shape[1]
    n = n_y - (L - 1) if tail else n_y
    d = default_delay(nf, nb, L) if delay is None else delay
    const = np.asarray(const, dtype=np.complex128).reshape(-1)
    M = const.size
    m = M.bit_length() - 1 if M & (M - 1) == 0 else None
    cr, ci = np.ascontiguousarray(const.real), np.ascontiguousarray(const.imag)
    nv = np.broadcast_to(np.asarray(noise_var, dtype=np.float64), (B,)).copy()
    bad = ~np.isfinite(y.real).all(1) | ~np.isfinite(y.imag).all(1) | ~np.isfinite(h.real).all(1) | ~np.isfinite(h.imag).all(1)
    bad |= ~np.isfinite(nv) | ~(nv > 0)
    y, h = y.copy(), h.copy()
    y[bad], h[bad], nv[bad] = 0.0, 0.0, 1.0
    des = design(h, Es, nv, nf, nb, d)
    bad |= des['bad']
    fr, fi = np.ascontiguousarray(des['ff'].real.T), np.ascontiguousarray(des['ff'].imag.T)
    fbr, fbi = np.ascontiguousarray(des['fb'].real.T), np.ascontiguousarray(des['fb'].imag.T)
    gain, nu = des['gain'], des['noise']
    right = max(0, n + d - n_y)
    yr = np.concatenate([np.zeros((B, nf - 1)), y.real, np.zeros((B, right))], axis=1)
    yi = np.concatenate([np.zeros((B, nf - 1)), y.imag, np.zeros((B, right))], axis=1)
    idx = np.zeros((B, n), dtype=np.int32)
    est = np.zeros((B, n), dtype=np.complex128)
    llr = None if m is None else np.zeros((B, n * m))
    rows = np.arange(B)
    with np.errstate(all='ignore'):
        for t in range(n):
            sr, si = np.zeros(B), np.zeros(B)
            for i in range(nf):
                qr, qi = _mul(fr[i], fi[i], yr[:, t + d - i + nf - 1], yi[:, t + d - i + nf - 1])
                sr, si = sr + qr, si + qi
            br, bi = np.zeros(B), np.zeros(B)
            for j in range(1, min(nb, t) + 1):
                a = idx[:, t - j]
                qr, qi = _mul(fbr[j - 1], fbi[j - 1], cr[a], ci[a])
                br, bi = br + qr, bi + qi
            xr, xi = (sr - br) / gain, (si - bi) / gain
            est[:, t] = _complex(xr, xi)
            best, sel = None, np.zeros(B, dtype=np.int32)
            if m is not None:
                m0 = [np.full(B, np.inf) for _ in range(m)]
                m1 = [np.full(B, np.inf) for _ in range(m)]
            for a in range(M):
                er, ei = xr - cr[a], xi - ci[a]
                dd = er * er + ei * ei
                if a == 0:
                    best = dd
                else:
                    upd = dd < best
                    best = np.where(upd, dd, best)
                    sel = np.where(upd, a, sel).astype(np.int32)
                if m is not None:
                    for i in range(m):
                        if (a >> (m - 1 - i)) & 1:
                            m1[i] = np.where(dd < m1[i], dd, m1[i])
                        else:
                            m0[i] = np.where(dd < m0[i], dd, m0[i])
            idx[:, t] = sel
            if m is not None:
                for i in range(m):
                    llr[:, t * m + i] = (m1[i] - m0[i]) / nu
    out = {'indices': idx, 'estimate': est, 'noise': nu.copy(), 'ff': des['ff'], 'fb': des['fb'], 'gain': gain.copy()}
    idx[bad] = 0
    for key in ('estimate', 'noise', 'ff', 'fb', 'gain'):
        out[key][bad] = complex(np.nan, np.nan) if out[key].dtype.kind == 'c' else np.nan       # both parts
    if m is not None:
        llr[bad] = np.nan
        out['llr'] = llr
        out['bits'] = ((idx[:, :, None] >> np.arange(m - 1, -1, -1)) & 1).astype(np.uint8).reshape(B, n * m)
    return out
