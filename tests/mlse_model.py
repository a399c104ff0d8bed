"""NumPy model of the trellis equaliser (csrc/mlse.hip) -- TEST INFRASTRUCTURE ONLY.

A block of n symbols with labels a_0 .. a_{n-1} and values c[a] goes in silence through L taps: y_t = sum_l h_l c[a_{t-l}] + w_t, the
terms with t - l < 0 or t - l >= n absent.  The rule, as the header, the kernel and ``mlse_equalize_batch`` state it (float64, real and
imaginary parts separate doubles, every product rounded before it is added, sums in the order written):

    state after step t   s' = a_t M^(L-2) + ... + a_{t-L+2}, the newest symbol most significant
    candidates into s'   old = 0 .. M-1 in this order, pred = (s' mod M^(L-2)) M + old
    branch metric        xh = sum_{l=0}^{L-1} h_l c[a_{t-l}], l ascending from 0.0, each product (hr cr - hi ci, hr ci + hi cr), the terms
                         with t - l < 0 skipped; e = y_t - xh; d = er er + ei ei
    prior cost           P_t[a] = noise_var (sum of La over the bits 1 of a, MSB first, from 0.0); zero without a prior
    forward              alpha_0 = 0; alpha_{t+1}[s'] = (first minimum over old of alpha_t[pred] + d) + P_t[a_t]; a later candidate wins
                         only if strictly smaller; the winning old is the decision
    tail                 beta_n[s] = sum_{j=0}^{L-2} |y_{n+j} - xh_j(s)|^2, j ascending from 0.0, xh_j(s) over l = j+1 .. L-1 (and
                         n + j - l >= 0); beta_n = 0 without the tail
    hard output          s* = first minimum of alpha_n + beta_n, that minimum is the metric; indices from s* and the decisions
    soft output          beta_t[s] = min over a of (d_t(s, a) + (P_t[a] + beta_{t+1}[s'])); Lambda_t[s'] = alpha_{t+1}[s'] + beta_{t+1}[s'];
                         llr[t m + i] = (min over the s' whose a_t has bit i = 1 of Lambda_t - the same with bit i = 0) / noise_var
    A row whose y, h, prior or noise_var holds a NaN or +-inf is rejected: zero indices and bits, NaN metric and LLRs.

Loops over steps, candidates and taps are Python loops; every operation inside them is one NumPy call on REAL arrays over the rows and
states (no complex128 multiply or abs: NumPy's SIMD complex loops may fuse).  Minima with a winner are comparison loops (strictly
smaller replaces), never ``argmin``.
"""
import numpy as np


def _mul(hr, hi, cr, ci):
    return hr * cr - hi * ci, hr * ci + hi * cr


class _Row:
    """The arrays of one call, rejected rows replaced by zeros."""

    def __init__(self, y, h, const, noise_var, a_priori, tail):
        y = np.atleast_2d(np.asarray(y, dtype=np.complex128))
        B = y.shape[0]
        h = np.asarray(h, dtype=np.complex128)
        h = np.broadcast_to(h, (B, h.shape[-1])) if h.ndim == 1 else h
        const = np.asarray(const, dtype=np.complex128).reshape(-1)
        self.B, self.L, self.M = B, h.shape[1], const.size
        self.m = self.M.bit_length() - 1
        self.n = y.shape[1] - (self.L - 1 if tail else 0)
        self.tail = tail
        self.S = self.M ** (self.L - 1)
        bad = ~np.isfinite(y.real).all(1) | ~np.isfinite(y.imag).all(1) | ~np.isfinite(h.real).all(1) | ~np.isfinite(h.imag).all(1)
        if noise_var is None:
            nv = np.ones(B)
        else:
            nv = np.broadcast_to(np.asarray(noise_var, dtype=np.float64), (B,)).copy()
            bad |= ~np.isfinite(nv) | (nv <= 0)
        if a_priori is None:
            la = np.zeros((B, self.n * self.m))
            self.prior = False
        else:
            la = np.atleast_2d(np.asarray(a_priori, dtype=np.float64)).copy()
            bad |= ~np.isfinite(la).all(1)
            self.prior = True
        y, h = y.copy(), h.copy()
        y[bad], h[bad], nv[bad], la[bad] = 0.0, 0.0, 1.0, 0.0
        self.bad, self.nv, self.la = bad, nv, la
        self.yr, self.yi = np.ascontiguousarray(y.real), np.ascontiguousarray(y.imag)
        self.hr, self.hi = np.ascontiguousarray(h.real), np.ascontiguousarray(h.imag)
        self.cr, self.ci = np.ascontiguousarray(const.real), np.ascontiguousarray(const.imag)
        self.kept = {}

    def digit(self, s, i):
        """Digit i of state s, 0 = the most significant = the newest symbol."""
        return (s // self.M ** (self.L - 2 - i)) % self.M

    def prefix(self, t, sp, key):
        """The sum over l <= min(t, L-2) of the branch into sp[k]; from step L-2 on it no longer depends on t and is kept under ``key``."""
        full = t >= self.L - 2
        if full and key in self.kept:
            return self.kept[key]
        xr = np.zeros((self.B, sp.size))
        xi = np.zeros((self.B, sp.size))
        for l in range(min(t, self.L - 2) + 1):
            sym = self.digit(sp, l)
            pr, pi = _mul(self.hr[:, l, None], self.hi[:, l, None], self.cr[sym][None, :], self.ci[sym][None, :])
            xr = xr + pr
            xi = xi + pi
        if full:
            self.kept[key] = (xr, xi)
        return xr, xi

    def branch(self, t, sp, old, key):
        """d_t of the branch into state sp[k] from the predecessor whose oldest symbol is old[k]: [B, K]."""
        xr, xi = self.prefix(t, sp, key)
        if t >= self.L - 1:
            l = self.L - 1
            pr, pi = _mul(self.hr[:, l, None], self.hi[:, l, None], self.cr[old][None, :], self.ci[old][None, :])
            xr = xr + pr
            xi = xi + pi
        er = self.yr[:, t, None] - xr
        ei = self.yi[:, t, None] - xi
        return er * er + ei * ei

    def prior_cost(self, t):
        """P_t[a]: [B, M]."""
        acc = np.zeros((self.B, self.M))
        for i in range(self.m):
            one = ((np.arange(self.M) >> (self.m - 1 - i)) & 1).astype(bool)
            acc[:, one] = acc[:, one] + self.la[:, t * self.m + i, None]
        return self.nv[:, None] * acc

    def tail_cost(self):
        """beta_n[s]: [B, S]."""
        beta = np.zeros((self.B, self.S))
        if not self.tail:
            return beta
        s = np.arange(self.S)
        for j in range(self.L - 1):
            xr = np.zeros((self.B, self.S))
            xi = np.zeros((self.B, self.S))
            for l in range(j + 1, min(self.L - 1, self.n + j) + 1):
                sym = self.digit(s, l - j - 1)
                pr, pi = _mul(self.hr[:, l, None], self.hi[:, l, None], self.cr[sym][None, :], self.ci[sym][None, :])
                xr = xr + pr
                xi = xi + pi
            er = self.yr[:, self.n + j, None] - xr
            ei = self.yi[:, self.n + j, None] - xi
            beta = beta + (er * er + ei * ei)
        return beta


def equalize(y, h, const, noise_var=None, a_priori=None, tail=True, soft=False):
    """``{'indices' [B, n] int32, 'bits' [B, n m] uint8, 'metric' [B], 'llr' [B, n m] (``soft`` only)}`` of rows ``y [B, n_y]`` through
    taps ``h [L]`` or ``[B, L]`` over the points ``const [M]`` (label = position)."""
    r = _Row(y, h, const, noise_var, a_priori, tail)
    B, S, M, L, n, m = r.B, r.S, r.M, r.L, r.n, r.m
    s = np.arange(S)
    newest = r.digit(s, 0)
    pred0 = (s % (S // M)) * M
    rows = np.arange(B)[:, None]
    alpha = np.zeros((B, S))
    alphas, decs = [alpha], []
    for t in range(n):
        best, dec = None, np.zeros((B, S), dtype=np.int64)
        for old in range(M):
            cand = alpha[:, pred0 + old] + r.branch(t, s, np.full(S, old), 'into')
            if old == 0:
                best = cand
            else:
                upd = cand < best
                best = np.where(upd, cand, best)
                dec = np.where(upd, old, dec)
        alpha = best + r.prior_cost(t)[:, newest]
        alphas.append(alpha)
        decs.append(dec)
    beta = r.tail_cost()
    tot = alpha + beta
    metric, star = tot[:, 0].copy(), np.zeros(B, dtype=np.int64)
    for k in range(1, S):
        upd = tot[:, k] < metric
        metric = np.where(upd, tot[:, k], metric)
        star = np.where(upd, k, star)
    idx = np.zeros((B, n), dtype=np.int32)
    st = star
    for t in range(n - 1, -1, -1):
        idx[:, t] = r.digit(st, 0)
        st = (st % (S // M)) * M + decs[t][rows[:, 0], st]
    out = {}
    if soft:
        llr = np.zeros((B, n * m))
        for t in range(n - 1, -1, -1):
            lam = alphas[t + 1] + beta
            for i in range(m):
                one = ((newest >> (m - 1 - i)) & 1).astype(bool)
                llr[:, t * m + i] = (lam[:, one].min(1) - lam[:, ~one].min(1)) / r.nv
            if t:
                P = r.prior_cost(t)
                nxt = None
                for a in range(M):
                    sp = a * (S // M) + s // M
                    cand = r.branch(t, sp, s % M, a) + (P[:, a, None] + beta[:, sp])
                    nxt = cand if nxt is None else np.minimum(nxt, cand)
                beta = nxt
        llr[r.bad] = np.nan
        out['llr'] = llr
    idx[r.bad] = 0
    metric[r.bad] = np.nan
    out['indices'] = idx
    out['bits'] = ((idx[:, :, None] >> np.arange(m - 1, -1, -1)) & 1).astype(np.uint8).reshape(B, n * m)
    out['metric'] = metric
    return out


def draw(modem, L, n, B, seed, tail=True, snr_db=8.0, per_row_h=True):
    """``(idx, y, h)``: B rows of n random labels through random taps of unit energy, with noise."""
    rs = np.random.RandomState(seed)
    idx = rs.randint(0, modem.m, (B, n))
    h = (rs.randn(B if per_row_h else 1, L) + 1j * rs.randn(B if per_row_h else 1, L)) / np.sqrt(2 * L)
    x = modem.constellation[idx]
    full = np.stack([np.convolve(x[b], h[b if per_row_h else 0]) for b in range(B)])
    sigma = np.sqrt(modem.Es / 10 ** (snr_db / 10) / 2)
    y = full + sigma * (rs.randn(*full.shape) + 1j * rs.randn(*full.shape))
    return idx, (y if tail else y[:, :n]), (h if per_row_h else h[0])


def brute_force(y, h, const, noise_var=None, a_priori=None, tail=True):
    """One row by enumeration of all M^n sequences: ``(cost [M] * n, llr [n m] or None)``; the cost includes the prior's."""
    y, h, const = (np.asarray(v, dtype=np.complex128).reshape(-1) for v in (y, h, const))
    L, M = h.size, const.size
    m = M.bit_length() - 1
    n = y.size - (L - 1 if tail else 0)
    cost = np.zeros((M,) * n)
    axis = lambda t: tuple(M if k == t else 1 for k in range(n))
    for t in range(y.size):
        xh = np.zeros((1,) * n, dtype=np.complex128)
        for l in range(L):
            if 0 <= t - l < n:
                xh = xh + h[l] * const.reshape(axis(t - l))
        e = y[t] - xh
        cost = cost + (e.real * e.real + e.imag * e.imag)
    if a_priori is not None:
        la = np.asarray(a_priori, dtype=np.float64)
        for t in range(n):
            p = np.array([sum(la[t * m + i] for i in range(m) if (a >> (m - 1 - i)) & 1) for a in range(M)], dtype=np.float64)
            cost = cost + noise_var * p.reshape(axis(t))
    llr = None
    if noise_var is not None:
        llr = np.zeros(n * m)
        for t in range(n):
            per = cost.min(axis=tuple(k for k in range(n) if k != t)) if n > 1 else cost
            for i in range(m):
                one = ((np.arange(M) >> (m - 1 - i)) & 1).astype(bool)
                llr[t * m + i] = (per[one].min() - per[~one].min()) / noise_var
    return cost, llr
