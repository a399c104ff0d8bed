"""NumPy model of the adaptive equalisers (csrc/adaptive.hip): LMS, normalised LMS and RLS, linear and decision-feedback -- TEST
INFRASTRUCTURE ONLY.

``y`` holds ``sps`` samples per symbol; ``nf`` feed-forward taps one sample apart, ``nb`` feedback taps one symbol apart, ``d`` the
delay in samples, ``N = nf + nb``, ``c`` the constellation, ``theta = (ff, fb)``.  The rule, as the header, the kernel and
``adaptive_equalize_batch`` state it (float64, real and imaginary parts separate doubles, every product rounded before it is added,
every sum from 0.0 in ascending index order; ``a b = (ar br - ai bi, ar bi + ai br)``, ``a conj(b) = (ar br + ai bi, ai br - ar bi)``),
for ``t = 0 .. n-1``:

    regressor   x[i] = y[t sps + d - i] for i < nf, a sample outside the row read as 0.0 and multiplied like any other;
                x[nf + j - 1] = -r_{t-j} (each part negated) for j = 1 .. nb, and 0.0 where t - j < 0, multiplied like any other.
    output      z_t = (sum_{k<nf} theta_k x_k) + (sum_{nf<=k<N} theta_k x_k), no conjugate, the two sums formed separately.
    decision    a^_t = the first minimum over a ascending of e = z_t - c[a], er er + ei ei, a later point winning only if strictly
                smaller.  It is the 'indices' output at every t, training included.
    reference   r_t = c[training[t]] for t < nt, else c[a^_t]; e_t = r_t - z_t.
    lms         w = (mu er, mu ei); theta_k <- theta_k + w conj(x_k).
    nlms        the same with mu_t = mu / (eps + sum_{k<N} (xr xr + xi xi)) in place of mu.
    rls         P = I / delta = (1.0 / delta) on the diagonal before the first step.  g_i = sum_{j<N} P[i][j] conj(x_j);
                den = lambda + sum_{k<N} (xr gr - xi gi); kappa_i = (gr_i / den, gi_i / den); theta_i <- theta_i + kappa_i e_t;
                P[i][j] <- ((Pr - qr) / lambda, (Pi - qi) / lambda) with q = kappa_i conj(g_j).
    rejection   a row whose y (all n_y samples), ff0, fb0, step, forgetting, delta or eps holds a NaN or +-inf or lies outside its
                range (step > 0, 0 < forgetting <= 1, delta > 0, eps >= 0), one of whose training labels is negative or >= M, one of
                whose z_t is not finite, or one of whose den is not positive and finite: zero indices and bits, NaN everything else.

Loops over steps, over the terms of a sum and over the points are Python loops; every operation inside them is one NumPy call on real
arrays over the rows (and, where no sum is formed, over the taps).
"""
import numpy as np

ALGORITHMS = ('lms', 'nlms', 'rls')


def _complex(re, im):
    """The complex array of two real ones, part by part (``re + 1j * im`` would lose the sign of a zero)."""
    out = np.empty(np.shape(re), dtype=np.complex128)
    out.real, out.imag = re, im
    return out


def default_delay(nf, nb):
    return (nf - 1) // 2 if nb == 0 else nf - 1


def _per_row(v, B):
    return np.broadcast_to(np.asarray(v, dtype=np.float64), (B,)).copy()


def _taps(t0, B, count):
    if t0 is None:
        return np.zeros((B, count), dtype=np.complex128)
    t0 = np.asarray(t0, dtype=np.complex128)
    return np.broadcast_to(t0, (B, count)).copy()


def equalize(y, const, training, nf, nb=0, algorithm='lms', step=None, forgetting=1.0, delta=0.01, eps=1e-6, delay=None, sps=1, n=None,
             ff0=None, fb0=None):
    """Every result of ``adaptive_equalize_batch`` by name ('bits' only for a power-of-two constellation), and 'bad' ``[B]``, for rows
    ``y [B, n_y]`` over the points ``const [M]`` (label = position)."""
    assert algorithm in ALGORITHMS
    y = np.atleast_2d(np.asarray(y, dtype=np.complex128)).copy()
    B, n_y = y.shape
    n = n_y // sps if n is None else n
    d = default_delay(nf, nb) if delay is None else delay
    N = nf + nb
    const = np.asarray(const, dtype=np.complex128).reshape(-1)
    M = const.size
    m = M.bit_length() - 1 if M & (M - 1) == 0 else None
    cr, ci = np.ascontiguousarray(const.real), np.ascontiguousarray(const.imag)
    tr = np.asarray(training, dtype=np.int64)
    tr = np.broadcast_to(tr, (B, tr.shape[-1])).copy()
    nt = tr.shape[1]
    ff, fb = _taps(ff0, B, nf), _taps(fb0, B, nb)
    rls, nlms = algorithm == 'rls', algorithm == 'nlms'

    bad = ~np.isfinite(y.real).all(1) | ~np.isfinite(y.imag).all(1)
    for taps in (ff, fb):
        bad |= ~np.isfinite(taps.real).all(1) | ~np.isfinite(taps.imag).all(1)
    if rls:
        lam, dl = _per_row(forgetting, B), _per_row(delta, B)
        bad |= ~np.isfinite(lam) | ~(lam > 0) | ~(lam <= 1) | ~np.isfinite(dl) | ~(dl > 0)
        lam[bad], dl[bad] = 1.0, 1.0
    else:
        mu = _per_row(step, B)
        bad |= ~np.isfinite(mu) | ~(mu > 0)
        bad |= not (np.isfinite(eps) and eps >= 0)
        mu[bad] = 1.0
        eps = eps if np.isfinite(eps) else 0.0
    y[bad], ff[bad], fb[bad] = 0.0, 0.0, 0.0

    left, right = nf - 1, max(0, (n - 1) * sps + d + 1 - n_y)
    yr = np.concatenate([np.zeros((B, left)), y.real, np.zeros((B, right))], axis=1)
    yi = np.concatenate([np.zeros((B, left)), y.imag, np.zeros((B, right))], axis=1)
    thr = np.ascontiguousarray(np.concatenate([ff.real, fb.real], axis=1).T)        # [N, B]
    thi = np.ascontiguousarray(np.concatenate([ff.imag, fb.imag], axis=1).T)
    if rls:
        Pr, Pi = np.zeros((N, N, B)), np.zeros((N, N, B))                           # P[i][j] at [i, j]
        for i in range(N):
            Pr[i, i] = 1.0 / dl
    refr, refi = np.zeros((n, B)), np.zeros((n, B))
    idx = np.zeros((B, n), dtype=np.int32)
    est, err = np.zeros((B, n), dtype=np.complex128), np.zeros((B, n), dtype=np.complex128)
    xr, xi = np.zeros((N, B)), np.zeros((N, B))
    with np.errstate(all='ignore'):
        for t in range(n):
            for i in range(nf):
                s = t * sps + d - i + left
                xr[i], xi[i] = yr[:, s], yi[:, s]
            for j in range(1, nb + 1):
                if t - j >= 0:
                    xr[nf + j - 1], xi[nf + j - 1] = -refr[t - j], -refi[t - j]
                else:
                    xr[nf + j - 1], xi[nf + j - 1] = 0.0, 0.0
            fr, fi, br, bi, pw = np.zeros(B), np.zeros(B), np.zeros(B), np.zeros(B), np.zeros(B)
            for k in range(nf):
                fr = fr + (thr[k] * xr[k] - thi[k] * xi[k])
                fi = fi + (thr[k] * xi[k] + thi[k] * xr[k])
            for k in range(nf, N):
                br = br + (thr[k] * xr[k] - thi[k] * xi[k])
                bi = bi + (thr[k] * xi[k] + thi[k] * xr[k])
            if nlms:
                for k in range(N):
                    pw = pw + (xr[k] * xr[k] + xi[k] * xi[k])
            zr, zi = fr + br, fi + bi
            bad |= ~np.isfinite(zr) | ~np.isfinite(zi)
            best, sel = None, np.zeros(B, dtype=np.int64)
            for a in range(M):
                er, ei = zr - cr[a], zi - ci[a]
                dd = er * er + ei * ei
                if a == 0:
                    best = dd
                else:
                    upd = dd < best
                    best = np.where(upd, dd, best)
                    sel = np.where(upd, a, sel)
            lab = sel
            if t < nt:
                lab = tr[:, t]
                out_of_range = (lab < 0) | (lab >= M)
                bad |= out_of_range
                lab = np.where(out_of_range, 0, lab)
            refr[t], refi[t] = cr[lab], ci[lab]
            er, ei = refr[t] - zr, refi[t] - zi
            idx[:, t] = sel
            est[:, t], err[:, t] = _complex(zr, zi), _complex(er, ei)
            if not rls:
                mt = mu / (eps + pw) if nlms else mu
                ur, ui = mt * er, mt * ei
                thr, thi = thr + (ur * xr + ui * xi), thi + (ui * xr - ur * xi)
                continue
            gr, gi = np.zeros((N, B)), np.zeros((N, B))
            for j in range(N):
                gr = gr + (Pr[:, j] * xr[j] + Pi[:, j] * xi[j])
                gi = gi + (Pi[:, j] * xr[j] - Pr[:, j] * xi[j])
            acc = np.zeros(B)
            for k in range(N):
                acc = acc + (xr[k] * gr[k] - xi[k] * gi[k])
            den = lam + acc
            bad |= ~np.isfinite(den) | ~(den > 0)
            kr, ki = gr / den, gi / den
            thr, thi = thr + (kr * er - ki * ei), thi + (kr * ei + ki * er)
            qr = kr[:, None] * gr[None, :] + ki[:, None] * gi[None, :]
            qi = ki[:, None] * gr[None, :] - kr[:, None] * gi[None, :]
            Pr, Pi = (Pr - qr) / lam, (Pi - qi) / lam
    out = {'indices': idx, 'estimate': est, 'error': err, 'ff': _complex(thr[:nf].T, thi[:nf].T), 'fb': _complex(thr[nf:].T, thi[nf:].T),
           'bad': bad}
    idx[bad] = 0
    for key in ('estimate', 'error', 'ff', 'fb'):
        out[key][bad] = complex(np.nan, np.nan)
    if m is not None:
        out['bits'] = ((idx[:, :, None] >> np.arange(m - 1, -1, -1)) & 1).astype(np.uint8).reshape(B, n * m)
    return out
