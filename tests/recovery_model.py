"""NumPy model of the symbol-timing and carrier recovery loop (csrc/recovery.hip) -- TEST INFRASTRUCTURE ONLY.  It is the definition.

``y`` holds nominally ``sps`` samples per symbol; ``c`` is the constellation (label = position).  The rule, as the header, the kernel
and ``timing_recover_batch`` state it (float64, real and imaginary parts separate doubles, every product rounded before it is added,
no fused multiply-add; a sample index outside ``[0, n_y)`` reads 0.0 and is used like any other sample).  Per-row state: the sampling
position ``m`` (int64) and ``mu``, from ``m0`` and ``mu0``; the timing integrator ``v = 0.0``; the period ``w = (double)sps``; the
carrier phase ``phi = phase0`` and its integrator ``f = 0.0``; the previous strobe and the previous reference.  For ``k = 0 .. n-1``:

    interpolate   z_k = I(m, mu), each part on its own.  'linear': x0 + mu (x1 - x0) with x0 = y[m], x1 = y[m+1].  'cubic' (4-sample
                  Lagrange in Farrow form), with xm = y[m-1], x0 = y[m], x1 = y[m+1], x2 = y[m+2] and S = 0.16666666666666666 (the
                  double nearest 1/6; the divisions are multiplications by S and by 0.5):
                      v3 = ((x2 - xm) + 3.0 (x0 - x1)) S
                      v2 = ((x1 + xm) 0.5) - x0
                      v1 = ((6.0 x1 - x2) - (3.0 x0 + 2.0 xm)) S
                      I  = ((v3 mu + v2) mu + v1) mu + x0
    derotate      with a carrier loop (c, s) = unit_phasor(phi) and z'_k = (zr c + zi s, zi c - zr s); without one z' = z.
    decide        with a constellation, a^_k = the first minimum over a ascending of e = z'_k - c[a], er er + ei ei, a later point
                  winning only if strictly smaller (cpx_slice.h).  Reference r_k = c[training[k]] for k < nt, else c[a^_k].
    timing error  e_0 = 0.0 and no midpoint is read at k = 0.  'gardner': t = mu - 0.5 w, fl = floor(t), zm = I(m + fl, t - fl),
                  e_k = (zr_{k-1} - zr_k) zmr + (zi_{k-1} - zi_k) zmi on the UNrotated strobes.
                  'mm': e_k = (rr_{k-1} z'r_k + ri_{k-1} z'i_k) - (rr_k z'r_{k-1} + ri_k z'i_{k-1}).
    carrier       ep = z'i_k rr_k - z'r_k ri_k; f <- f + kc2 ep; phi <- phi + (f + kc1 ep); phi <- phi - rint(phi).  The row is
                  rejected unless |phi| <= 0.5 (a NaN fails).
    loop filter   v <- v + k2 e_k; w = sps + (v + k1 e_k).  The row is rejected unless 0.5 sps < w < 1.5 sps.
    controller    t = mu + w, fl = floor(t), m <- m + fl, mu <- t - fl.
    outputs       symbols[k] = z'_k; indices[k] = a^_k; position[k] = (double)m + mu and count (below) before the controller;
                  error[k] = e_k; phase[k] = phi after its update.  count = the strobes all of whose interpolator reads (the window of
                  z_k and, for 'gardner' and k >= 1, that of zm) had their indices in [0, n_y).
    rejection     a row whose y (all n_y samples), k1, k2, kc1, kc2, mu0 or phase0 holds a NaN or +-inf or lies outside its range
                  (k1, k2, kc1, kc2 >= 0; 0 <= mu0 < 1; |phase0| <= 0.5; 0 <= m0 < n_y), one of whose training labels is negative
                  or >= M, or one of whose w or phi fails its test: zero integers, NaN floats.

unit_phasor(u) for |u| <= 0.5: q = rint(4 u), r = u - 0.25 q (exact), x = r 6.283185307179586, x2 = x x, sin = x P(x2) and
cos = Q(x2) by Horner's rule from the highest coefficient, P and Q the Taylor polynomials through x^17 and x^16 with the nearest
doubles as coefficients; q = 0: (cos, sin), 1: (-sin, cos), 2 and -2: (-cos, -sin), -1: (sin, -cos).

Loops over strobes, polynomial terms and constellation points are Python loops; every operation inside them is one NumPy call on real
arrays over the rows.
"""
import numpy as np

TEDS = ('gardner', 'mm')
INTERPS = ('linear', 'cubic')
SIXTH = 0.16666666666666666
TWO_PI = 6.283185307179586
SIN_COEF = (1.0, -0.16666666666666666, 0.008333333333333333, -0.0001984126984126984, 2.7557319223985893e-06, -2.505210838544172e-08,
            1.6059043836821613e-10, -7.647163731819816e-13, 2.8114572543455206e-15)
COS_COEF = (1.0, -0.5, 0.041666666666666664, -0.001388888888888889, 2.48015873015873e-05, -2.755731922398589e-07,
            2.08767569878681e-09, -1.1470745597729725e-11, 4.779477332387385e-14)


def _complex(re, im):
    """The complex array of two real ones, part by part (``re + 1j * im`` would lose the sign of a zero)."""
    out = np.empty(np.shape(re), dtype=np.complex128)
    out.real, out.imag = re, im
    return out


def unit_phasor(u):
    """``(cos 2 pi u, sin 2 pi u)`` of float64 ``u`` with ``|u| <= 0.5``, in the fixed operation order of csrc/cpx_phasor.h."""
    u = np.asarray(u, dtype=np.float64)
    q = np.rint(4.0 * u)
    r = u - 0.25 * q
    x = r * TWO_PI
    x2 = x * x
    p = np.full(u.shape, SIN_COEF[8])
    g = np.full(u.shape, COS_COEF[8])
    for k in range(7, -1, -1):
        p = p * x2 + SIN_COEF[k]
        g = g * x2 + COS_COEF[k]
    sn = x * p
    c = np.where(q == 0, g, np.where(q == 1, -sn, np.where(q == -1, sn, -g)))
    s = np.where(q == 0, sn, np.where(q == 1, g, np.where(q == -1, -g, -sn)))
    return c, s


def farrow(xm, x0, x1, x2, mu):
    """The cubic interpolator on one part."""
    v3 = ((x2 - xm) + 3.0 * (x0 - x1)) * SIXTH
    v2 = ((x1 + xm) * 0.5) - x0
    v1 = ((6.0 * x1 - x2) - (3.0 * x0 + 2.0 * xm)) * SIXTH
    return ((v3 * mu + v2) * mu + v1) * mu + x0


def linear(x0, x1, mu):
    return x0 + mu * (x1 - x0)


def interpolate(yr, yi, m, mu, cubic):
    """``(zr, zi, inside)`` at the positions ``m + mu`` of the rows ``yr, yi [B, n_y]``; ``inside``: every index read was in the row."""
    B, n_y = yr.shape
    rows = np.arange(B)

    def read(idx):
        ok = (idx >= 0) & (idx < n_y)
        j = np.clip(idx, 0, max(n_y - 1, 0))
        return np.where(ok, yr[rows, j], 0.0), np.where(ok, yi[rows, j], 0.0), ok
    r0, i0, ok0 = read(m)
    r1, i1, ok1 = read(m + 1)
    if not cubic:
        return linear(r0, r1, mu), linear(i0, i1, mu), ok0 & ok1
    rm, im, okm = read(m - 1)
    r2, i2, ok2 = read(m + 2)
    return farrow(rm, r0, r1, r2, mu), farrow(im, i0, i1, i2, mu), okm & ok0 & ok1 & ok2


def _per_row(v, B, dtype=np.float64):
    return np.broadcast_to(np.asarray(v, dtype=dtype), (B,)).copy()


def recover(y, sps, const=None, ted='gardner', interp='cubic', k1=0.0, k2=0.0, carrier=None, training=None, n=None, m0=0, mu0=0.0,
            phase0=0.0):
    """Every result of ``timing_recover_batch`` by name ('indices' only with a constellation, 'bits' only for a power of two, 'phase'
    only with a carrier loop), and 'bad' ``[B]`` and 'm' ``[B, n]`` (the integer part of the position at each strobe), for rows
    ``y [B, n_y]``."""
    assert ted in TEDS and interp in INTERPS
    y = np.atleast_2d(np.asarray(y, dtype=np.complex128)).copy()
    B, n_y = y.shape
    n = n_y // sps if n is None else n
    cubic, mm, pll = interp == 'cubic', ted == 'mm', carrier is not None
    M = 0
    if const is not None:
        const = np.asarray(const, dtype=np.complex128).reshape(-1)
        M = const.size
        cr, ci = np.ascontiguousarray(const.real), np.ascontiguousarray(const.imag)
    assert M or not (mm or pll or training is not None)
    tr = np.zeros((B, 0), dtype=np.int64)
    if training is not None:
        tr = np.asarray(training, dtype=np.int64)
        tr = np.broadcast_to(tr, (B, tr.shape[-1])).copy()
    nt = tr.shape[1]
    k1, k2, mu, phi = _per_row(k1, B), _per_row(k2, B), _per_row(mu0, B), _per_row(phase0, B)
    kc1, kc2 = (_per_row(carrier[0], B), _per_row(carrier[1], B)) if pll else (np.zeros(B), np.zeros(B))
    m = _per_row(m0, B, np.int64)

    bad = ~np.isfinite(y.real).all(1) | ~np.isfinite(y.imag).all(1)
    for gain in (k1, k2, kc1, kc2):
        bad |= ~np.isfinite(gain) | ~(gain >= 0)
        gain[bad] = 0.0
    bad |= ~np.isfinite(mu) | ~(mu >= 0) | ~(mu < 1)
    bad |= ~np.isfinite(phi) | ~(np.abs(phi) <= 0.5)
    bad |= (m < 0) | (m >= n_y)
    y[bad], mu[bad], phi[bad], m[bad] = 0.0, 0.0, 0.0, 0
    yr, yi = np.ascontiguousarray(y.real), np.ascontiguousarray(y.imag)

    fsps = float(sps)
    v, w, f = np.zeros(B), np.full(B, fsps), np.zeros(B)
    pzr, pzi, prr, pri = np.zeros(B), np.zeros(B), np.zeros(B), np.zeros(B)
    sym = np.zeros((B, n), dtype=np.complex128)
    idx = np.zeros((B, n), dtype=np.int32)
    pos, err, phase = np.zeros((B, n)), np.zeros((B, n)), np.zeros((B, n))
    ms = np.zeros((B, n), dtype=np.int64)
    count = np.zeros(B, dtype=np.int32)
    with np.errstate(all='ignore'):
        for k in range(n):
            zr, zi, inside = interpolate(yr, yi, m, mu, cubic)
            if pll:
                c, s = unit_phasor(phi)
                dr, di = zr * c + zi * s, zi * c - zr * s
            else:
                dr, di = zr, zi
            sel = np.zeros(B, dtype=np.int64)
            if M:
                best = None
                for a in range(M):
                    er, ei = dr - cr[a], di - ci[a]
                    dd = er * er + ei * ei
                    if a == 0:
                        best = dd
                    else:
                        upd = dd < best
                        best = np.where(upd, dd, best)
                        sel = np.where(upd, a, sel)
                lab = sel
                if k < nt:
                    lab = tr[:, k]
                    out_of_range = (lab < 0) | (lab >= M)
                    bad |= out_of_range
                    lab = np.where(out_of_range, 0, lab)
                rr, ri = cr[lab], ci[lab]
            e = np.zeros(B)
            if k > 0 and not mm:
                t = mu - 0.5 * w
                fl = np.floor(t)
                mr, mi, mid_inside = interpolate(yr, yi, m + fl.astype(np.int64), t - fl, cubic)
                inside = inside & mid_inside
                e = (pzr - zr) * mr + (pzi - zi) * mi
            elif k > 0:
                e = (prr * dr + pri * di) - (rr * pzr + ri * pzi)
            sym[:, k], idx[:, k], pos[:, k], err[:, k] = _complex(dr, di), sel, m.astype(np.float64) + mu, e
            ms[:, k] = m
            count += inside
            if pll:
                ep = di * rr - dr * ri
                f = f + kc2 * ep
                phi = phi + (f + kc1 * ep)
                phi = phi - np.rint(phi)
                bad |= ~(np.abs(phi) <= 0.5)
                phi = np.where(bad, 0.0, phi)
                phase[:, k] = phi
            v = v + k2 * e
            w = fsps + (v + k1 * e)
            bad |= ~((0.5 * fsps < w) & (w < 1.5 * fsps))
            w = np.where(bad, fsps, w)
            t = mu + w
            fl = np.floor(t)
            m = m + fl.astype(np.int64)
            mu = t - fl
            if mm:
                pzr, pzi, prr, pri = dr, di, rr, ri
            else:
                pzr, pzi = zr, zi
    out = {'symbols': sym, 'position': pos, 'error': err, 'count': count, 'bad': bad, 'm': ms}
    if M:
        out['indices'] = idx
        if M & (M - 1) == 0:
            nbits = M.bit_length() - 1
            out['bits'] = ((idx[:, :, None] >> np.arange(nbits - 1, -1, -1)) & 1).astype(np.uint8).reshape(B, n * nbits)
    if pll:
        out['phase'] = phase
    idx[bad], count[bad] = 0, 0
    if 'bits' in out:
        out['bits'][bad] = 0
    sym[bad] = complex(np.nan, np.nan)
    pos[bad], err[bad], phase[bad] = np.nan, np.nan, np.nan
    return out


# ---- test signals ---------------------------------------------------------------------------------------------------------------------
def raised_cosine(t, beta):
    """The raised-cosine pulse at ``t`` symbols."""
    t = np.asarray(t, dtype=np.float64)
    den = 1.0 - (2.0 * beta * t) ** 2
    flat = np.abs(den) < 1e-9
    return np.where(flat, np.pi / 4 * np.sinc(1.0 / (2 * beta)), np.sinc(t) * np.cos(np.pi * beta * t) / np.where(flat, 1.0, den))


def rc_burst(const, nsym, sps, seed, tau=0.3, clock=1.0004, phase=0.03, cfo=5e-4, sigma=0.02, beta=0.35, span=10, n_y=None):
    """``(labels [nsym], y [n_y])``: random symbols of ``const`` with a raised-cosine pulse (what a matched filter hands on), sampled at
    ``t_i = i clock / sps - tau`` symbols -- a timing offset of ``tau`` symbols and a symbol period of ``sps / clock`` samples --
    rotated by ``phase + cfo t_i`` turns, plus Gaussian noise of ``sigma`` per part."""
    rs = np.random.RandomState(seed)
    idx = rs.randint(0, len(const), nsym)
    a = np.asarray(const, dtype=np.complex128)[idx]
    n_y = int(nsym * sps / clock) if n_y is None else n_y
    ts = np.arange(n_y) * clock / sps - tau
    j0 = np.floor(ts).astype(np.int64)
    y = np.zeros(n_y, dtype=np.complex128)
    for d in range(-span, span + 1):
        j = j0 + d
        ok = (j >= 0) & (j < nsym)
        y += np.where(ok, a[np.clip(j, 0, nsym - 1)], 0.0) * raised_cosine(ts - j, beta)
    y *= np.exp(2j * np.pi * (phase + cfo * ts))
    return idx, y + sigma * (rs.randn(n_y) + 1j * rs.randn(n_y))
