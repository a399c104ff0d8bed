"""NumPy models of the ``fp32-fast`` kernels (``cpx_set_precision``) in ``np.float32`` -- TEST INFRASTRUCTURE ONLY.

Every array that stands for a kernel register is ``np.float32`` and every operation on it is one NumPy call over the batch, so each
result is rounded to float32 exactly where the kernel rounds it (the library is compiled without contraction: no fused multiply-add).

VITERBI -- ``cw_step(float ...)`` and ``viterbi_cw_fused_kernel<..., float>`` (csrc/viterbi_cw.hip), rate 1/2, k = 1:

    sizes       L = len / 2, T = L + m - 1 steps, tb = tb_depth or min(5 m, L), H = tb - 2 hops (as oracle/np_viterbi.py).
    start       pm[0] = 0, every other state +inf.
    input       step t <= L reads (r0, r1) = x[2 t - 2], x[2 t - 1]; the padded tail t > L reads the pad, -1 for 'unquantized', else 0.
    bit metric  hard         m0 = (float)((long long)r ^ 0), m1 = (float)((long long)r ^ 1)
                soft         r clipped to [-500, 500] in float64; m0 = 0, m1 = -(float)r
                unquantized  x = (float)r; m0 = (x + 1)^2, m1 = (x - 1)^2, sum and product each rounded
    branch      bm[c] = (0 + m_first[bit 1 of c]) + m_second[bit 0 of c], c the two output bits, first one the more significant.
    select      cand_j = pm[pred_j] + bm[output of that branch], predecessors in ascending order; the second one wins only if it is
                STRICTLY smaller (v_cmp_lt_f32); the new metric is fmin(cand_0, cand_1) (v_min_f32: of a NaN and a number, the number).
    best        the FIRST state whose metric equals the minimum (fmin over the states); state 0 if none does (all NaN).
    output      bit of step s = the input bit of the branch into the state at step s on the path traced back from best[min(s + H, T)].

  Domain.  'unquantized': every float64 input, NaN, +-inf and values whose square overflows float32 included (a NaN or an infinite
  metric reaches every state of its step at once, since every branch metric contains both received values; from there on every
  decision is "first predecessor" and every best state 0).  'soft': every input but NaN -- +-inf is clipped; a codeword with a NaN is
  flagged by the kernel and decoded again by the float64 NaN-exact kernel, so such rows follow the float64 oracle, not this model.
  'hard': finite values of magnitude below 2^63 (the conversion to ``long long`` of anything else is undefined in C++; such rows
  are outside the model).

LDPC -- ``ldpc_resident_f32_kernel`` with ``check_msa_f32`` / ``check_spa_f32`` and ``var_node_f32`` (csrc/ldpc_resident.hip):

    tables      edges sorted by (check, variable); position j of an edge = its rank in its check's row; the column table of a
                variable lists its edges in ascending check order and is padded to a multiple of four with a slot that holds 0.0.
    start       x = the float64 LLR clipped to [-500, 500] (a NaN stays); Q = (float)x; R = 0.
    iteration   check pass, then -- unless the parity flag is clear, which ends the block -- the variable pass; at most max_iter times.
    parity      flag = some check whose XOR of the SIGN BITS of its Q is 1.
    min-sum     per check, positions ascending: m = Q - R; av = |m|; c1 = av < m1; m2 = fmin(m2, c1 ? m1 : av); m1 = fmin(m1, av);
                imin = c1 ? j : imin (first minimum); neg_j = (m < 0) -- a COMPARISON, so -0.0 counts as positive; if the number of
                negatives is odd every neg_j is inverted; R_j = the bit pattern of m1 (m2 for j = imin) with neg_j as the sign bit.
    sum-product per check: e = exp(-|m|), t = copysign((1 - e) / (1 + e), m) -- below |m| < 2^-12, where 1 - e loses its bits,
                t = copysign(max(|m| / 2, FLT_MIN), m), and a zero message keeps t = 0 --; prod = ((1 t_0) t_1) ...;
                x_j = (1 / t_j) prod clipped to [-1, 1]; R_j = log((1 + x_j) / (1 - x_j)) clipped to [-500, 500]; NaN passes the clips.
                exp, log and the reciprocals are the hardware's approximate instructions in the kernel and NumPy's float32 functions
                here: this model is compared with a measured bound (tests/test_fp32_edges_gpu.py), not bit for bit.
    variable    Q_v = ((((0 + r_0) + r_1) + r_2) + r_3 ...) + (float)x_v over the padded column table.  (The running sum starts at
                +0.0 and can never become -0.0, so adding the padding slot's 0.0 changes no bit: the model adds it nevertheless.)
    result      k = the number of variable passes that ran; out_llrs = the float64 x itself when k == 0, else (double)Q;
                dec_word = the sign bit of out_llrs.
  Domain of the min-sum model: no NaN (a block with a NaN is flagged and decoded again by the float64 NaN-exact kernel) and checks
  of degree >= 2.  Min-sum is add, subtract, min and bit operations only: the model is bit-exact, ``out_llrs`` included.

DEMODULATOR -- ``demod_soft_sep_f32_kernel`` (square QAM) and ``demod_soft_f32_kernel`` (any table) (csrc/demod.hip): see
``demod_sep_f32`` and ``demod_gen_f32``, line-by-line transcriptions with ``np.exp2`` / ``np.log2`` for v_exp_f32 / v_log_f32, and
``demod_ref``, the long-double log-sum-exp of ``log sum_{bit=1} e^{-d^2/N0} - log sum_{bit=0} e^{-d^2/N0}``, finite at every finite input.

THE DEMODULATOR'S ERROR BOUND (``demod_bound``): |LLR_fast - LLR| <= A + K u T, u = 2^-24, T = max_a t_a, t_a = |y - c_a|^2 / N0 in nats,
for a constellation that contains -c with every c (then |y|^2 + max|c|^2 <= max_a |y - c_a|^2 =: D^2, so every component of y and of
every c is at most D in magnitude).  First order in u, roundings counted in the generic kernel (the separable one has fewer):

    dx = fl(fl(x) - fl(c_x))             |error| <= u (|x| + |c_x| + |dx|)            <= 3 u D       (two casts, one subtraction)
    dx^2, dy^2                           <= 2 |dx| 3 u D + u dx^2                                    (the square's own rounding)
    dx^2 + dy^2                          <= 6 u D (|dx| + |dy|) + u d^2 + u d^2       <= (6 sqrt 2 + 2) u D^2   (the sum's rounding)
    t = fl(that * fl(-log2 e / N0))      + 2 u t  (the cast of the factor, the product)              <= (6 sqrt 2 + 4) u T
    t - t_max                            + u T                                                       <= (6 sqrt 2 + 5) u T  = 13.49 u T

  A log-sum-exp moves by no more than its largest exponent error, and the LLR is a difference of two: 2 * 13.49 = 26.97 u T.  What
  follows is proportional to the result, and |log2 of a sum| <= T log2 e, |LLR| <= T: two v_log_f32 at one ulp each (2), the two
  additions m + log2 s of the re-summed form (2), the subtraction (1), the factor scale * ln 2 and its product (3): 8 u T.
  K = 35 >= 26.97 + 8 leaves room for the second-order terms.  A covers what does not grow with T -- v_exp_f32's ulp on every term
  of a sum and log2 of a sum near 1: it is MEASURED on the GPU against ``demod_ref`` on samples drawn next to the constellation with
  T <= 32 nats, times four (tests/test_fp32_edges_gpu.py prints it; DESIGN.md 4.4 records it).
"""
import numpy as np

F32 = np.float32
FLT_MIN = F32(1.17549435e-38)
SPA_SMALL = F32(2.0 ** -12)          # below: tanh(m / 2) = m / 2 to float32 precision (m^2 / 12 < 2^-27) and 1 - exp(-|m|) has < 12 bits
LN2_F = F32(0.6931471805599453)
F32_TINY = F32(1e-30)
DEMOD_K = 35.0
DEMOD_A = 3.4e-5                     # 4 x the 8.36e-6 measured on an MI355X (test_demod_measure_A in tests/test_fp32_edges_gpu.py)
U = 2.0 ** -24


# ---- Viterbi ------------------------------------------------------------------------------------------------------------------------
def _pred_tables(trellis):
    """Predecessors of every state in ascending order: [S, 2] previous state, input bit, output codeword."""
    nxt = np.asarray(trellis.next_state_table)
    out = np.asarray(trellis.output_table)
    S, I = nxt.shape
    assert I == 2 and int(trellis.k) == 1 and int(trellis.n) == 2, "the float32 kernel serves rate-1/2, k = 1 codes"
    ps, pi, pc = np.zeros((S, 2), np.int64), np.zeros((S, 2), np.int64), np.zeros((S, 2), np.int64)
    cnt = np.zeros(S, np.int64)
    for p in range(S):
        for i in range(I):
            s = nxt[p, i]
            ps[s, cnt[s]], pi[s, cnt[s]], pc[s, cnt[s]] = p, i, out[p, i]
            cnt[s] += 1
    assert np.all(cnt == 2)
    return ps, pi, pc


def _bit_metrics(r, decoding_type, dtype):
    """``(m0, m1)`` of one received value per row, in ``dtype`` (float32: bit_metrics_f32; float64: the same rule unrounded)."""
    if decoding_type == 'hard':
        ri = r.astype(np.int64)
        return (ri ^ 0).astype(dtype), (ri ^ 1).astype(dtype)
    if decoding_type == 'soft':
        x = np.clip(r, -500.0, 500.0).astype(dtype)
        return np.zeros(len(r), dtype), -x
    x = r.astype(dtype)
    d0, d1 = x + dtype(1.0), x - dtype(1.0)
    return d0 * d0, d1 * d1


def viterbi(coded, trellis, tb_depth=None, decoding_type='hard', dtype=F32, want_stats=False):
    """``coded [B, len]`` float64 -> int64 ``[B, L]``.  ``dtype=np.float64`` runs the SAME rule in float64 (the near-tie search of the tests).
    ``want_stats``: also ``{'select_ties', 'best_ties'}``, the exact ties met between the two candidates of a finite state and among
    the states that share the minimum."""
    x = np.ascontiguousarray(coded, dtype=np.float64)
    B, length = x.shape
    m, S = int(trellis.total_memory), int(trellis.number_states)
    L = length // 2
    tb = int(tb_depth) if tb_depth else min(5 * m, L)
    T = L + m - 1
    ps, pi, pc = _pred_tables(trellis)
    pad = -1.0 if decoding_type == 'unquantized' else 0.0
    pm = np.full((B, S), np.inf, dtype)
    pm[:, 0] = 0.0
    choice = np.zeros((T + 1, B, S), np.int8)
    best = np.zeros((T + 1, B), np.int64)
    stats = {'select_ties': 0, 'best_ties': 0}
    zero = dtype(0.0)
    with np.errstate(over='ignore', invalid='ignore'):
        for t in range(1, T + 1):
            r0 = x[:, 2 * t - 2] if t <= L else np.full(B, pad)
            r1 = x[:, 2 * t - 1] if t <= L else np.full(B, pad)
            m00, m01 = _bit_metrics(r0, decoding_type, dtype)
            m10, m11 = _bit_metrics(r1, decoding_type, dtype)
            bm = np.stack([(zero + m00) + m10, (zero + m00) + m11, (zero + m01) + m10, (zero + m01) + m11], axis=1)   # [B, 4]
            c0 = pm[:, ps[:, 0]] + bm[:, pc[:, 0]]
            c1 = pm[:, ps[:, 1]] + bm[:, pc[:, 1]]
            ch = c1 < c0                                             # v_cmp_lt_f32: false for a tie and for a NaN
            pm = np.fmin(c0, c1)                                     # v_min_f32
            mn = np.fmin.reduce(pm, axis=1)
            eq = pm == mn[:, None]
            choice[t] = ch
            best[t] = np.argmax(eq, axis=1)                          # first state equal to the minimum; none: 0
            if want_stats:
                stats['select_ties'] += int(np.sum((c0 == c1) & np.isfinite(c0)))
                stats['best_ties'] += int(np.sum(eq.sum(axis=1) > 1))
    out = np.zeros((B, max(T, L)), np.int64)
    rows = np.arange(B)
    H = tb - 2
    for s in range(1, T + 1):
        t0 = min(s + H, T)
        st = best[t0]
        for tt in range(t0, s, -1):
            st = ps[st, choice[tt, rows, st]]
        out[:, s - 1] = pi[st, choice[s, rows, st]]
    out = out[:, :L]
    return (out, stats) if want_stats else out


# ---- LDPC ---------------------------------------------------------------------------------------------------------------------------
class LdpcTables:
    """The tables of ``ldpc_resident_tables`` from an edge list sorted by (check, variable)."""

    def __init__(self, n_v, n_c, edge_check, edge_var):
        ec, ev = np.asarray(edge_check, np.int64), np.asarray(edge_var, np.int64)
        assert np.all(np.diff(ec * n_v + ev) > 0), "edges sorted by (check, variable), no duplicates"
        self.n_v, self.n_c = int(n_v), int(n_c)
        self.deg = np.bincount(ec, minlength=n_c)
        mcd = int(self.deg.max())
        assert self.deg.min() >= 2 and mcd <= 32
        self.cpad, self.rstride = (mcd + 3) & ~3, mcd | 1
        row_ptr = np.concatenate([[0], np.cumsum(self.deg)])
        pos = np.arange(len(ec)) - row_ptr[ec]
        self.row_q = np.full((n_c, self.cpad), n_v, np.int64)        # padding: the +inf slot behind Q
        self.row_q[ec, pos] = ev
        self.valid = self.row_q < n_v
        vdeg = np.bincount(ev, minlength=n_v)
        self.vpad = (int(vdeg.max()) + 3) & ~3
        self.n_r = n_c * self.rstride
        self.col_r = np.full((n_v, self.vpad), self.n_r, np.int64)   # padding: the zero slot behind R
        fill = np.zeros(n_v, np.int64)
        for e in range(len(ec)):                                     # edge order = ascending check per variable
            v = ev[e]
            self.col_r[v, fill[v]] = ec[e] * self.rstride + pos[e]
            fill[v] += 1

    @classmethod
    def from_params(cls, params):
        import oracle
        ec, ev = oracle.ldpc_edges(params)
        return cls(int(params['n_vnodes']), int(params['n_cnodes']), ec, ev)


def _clip_nan(x, lo, hi):
    return np.where(np.isnan(x), x, np.minimum(np.maximum(x, lo), hi))


def _check_msa(tab, Q, R):
    """One min-sum check pass over every check of every block: R [B, n_c, rstride] rewritten; returns the parity flag [B]."""
    B = Q.shape[0]
    inf = F32(np.inf)
    m1, m2 = np.full((B, tab.n_c), inf, F32), np.full((B, tab.n_c), inf, F32)
    imin = np.zeros((B, tab.n_c), np.int64)
    neg = np.zeros((B, tab.n_c, max(tab.cpad, tab.rstride)), bool)   # (a slot beyond cpad is written, with a clear bit, and never read)
    sx = np.zeros((B, tab.n_c), bool)
    for j in range(tab.cpad):
        q = Q[:, tab.row_q[:, j]]                                    # [B, n_c]; padding reads +inf
        r = R[:, :, j] if j < tab.rstride else np.zeros((B, tab.n_c), F32)   # (beyond the row: a finite neighbour, +inf - it = +inf)
        sx ^= np.signbit(q)
        with np.errstate(invalid='ignore'):
            m = q - r
        av = np.abs(m)
        c1 = av < m1
        m2 = np.fmin(m2, np.where(c1, m1, av))
        m1 = np.fmin(m1, av)
        imin = np.where(c1, j, imin)
        neg[:, :, j] = m < F32(0.0)
    odd = (neg.sum(axis=2) & 1).astype(bool)
    negp = neg ^ odd[:, :, None]
    b1, b2 = m1.view(np.uint32), m2.view(np.uint32)
    for j in range(tab.rstride):
        bits = np.where(imin == j, b2, b1) | (negp[:, :, j].astype(np.uint32) << np.uint32(31))
        R[:, :, j] = bits.astype(np.uint32).view(F32)
    return sx.any(axis=1)


def _tanh_half(m):
    """``t = tanh(m / 2)`` of check_spa_f32, float32."""
    av = np.abs(m)
    with np.errstate(under='ignore'):
        e = np.exp(-av)
        big = (F32(1.0) - e) / (F32(1.0) + e)
        small = np.where(av > F32(0.0), np.maximum(F32(0.5) * av, FLT_MIN), F32(0.0))
    return np.copysign(np.where(av < SPA_SMALL, small, big), m).astype(F32)


def _check_spa(tab, Q, R):
    B = Q.shape[0]
    prod = np.ones((B, tab.n_c), F32)
    sx = np.zeros((B, tab.n_c), bool)
    deg_max = int(tab.deg.max())
    T = np.ones((B, tab.n_c, deg_max), F32)
    with np.errstate(all='ignore'):
        for j in range(deg_max):
            live = tab.valid[:, j][None, :]
            q = Q[:, tab.row_q[:, j]]
            sx ^= np.signbit(q) & live
            m = np.where(live, q, F32(1.0)) - R[:, :, j]
            t = np.where(live, _tanh_half(m.astype(F32)), F32(1.0))
            prod = np.where(live, prod * t, prod).astype(F32)
            T[:, :, j] = t
        for j in range(deg_max):
            live = tab.valid[:, j][None, :]
            x = (F32(1.0) / T[:, :, j]) * prod
            x = _clip_nan(x, F32(-1.0), F32(1.0)).astype(F32)
            x = np.log((F32(1.0) + x) / (F32(1.0) - x))
            R[:, :, j] = np.where(live, _clip_nan(x, F32(-500.0), F32(500.0)), R[:, :, j]).astype(F32)
    return sx.any(axis=1)


def ldpc_decode(llr, tab, alg, max_iter):
    """``llr [B, n_v]`` float64 -> ``{'dec' int8 [B, n_v], 'out' float64 [B, n_v], 'iters' int32 [B], 'llr' the clipped input,
    'margin' [B] the smallest |Q| any check pass of the block read (how far its parity flags are from changing)}``."""
    x = _clip_nan(np.array(llr, dtype=np.float64, ndmin=2), -500.0, 500.0)
    B = x.shape[0]
    Q = np.concatenate([x.astype(F32), np.full((B, 1), np.inf, F32)], axis=1)
    R = np.zeros((B, tab.n_c, tab.rstride), F32)
    lf = x.astype(F32)
    iters = np.zeros(B, np.int32)
    margin = np.full(B, np.inf)                                      # the smallest |Q| a check pass of the block ever read
    live = np.ones(B, bool)                                          # blocks still iterating
    check = _check_msa if alg == 'MSA' else _check_spa
    for _ in range(int(max_iter)):
        idx = np.nonzero(live)[0]
        if not len(idx):
            break
        Qs, Rs = Q[idx], R[idx]
        margin[idx] = np.fmin(margin[idx], np.abs(Qs[:, :tab.n_v]).min(axis=1))
        flag = check(tab, Qs, Rs)
        go = idx[flag]
        live[idx[~flag]] = False
        if not len(go):
            break
        Rf = np.concatenate([Rs[flag].reshape(len(go), -1), np.zeros((len(go), 1), F32)], axis=1)
        msum = np.zeros((len(go), tab.n_v), F32)
        with np.errstate(invalid='ignore', over='ignore'):
            for q in range(tab.vpad):
                msum = msum + Rf[:, tab.col_r[:, q]]
            Q[go, :tab.n_v] = msum + lf[go]
        R[go] = Rs[flag]
        iters[go] += 1
    out = np.where((iters == 0)[:, None], x, Q[:, :tab.n_v].astype(np.float64))
    return {'dec': np.signbit(out).astype(np.int8), 'out': out, 'iters': iters, 'llr': x, 'margin': margin}


# ---- demodulator --------------------------------------------------------------------------------------------------------------------
def _lse2(t, sel):
    """lse2_subset: ``m + log2(sum 2^(t - m))`` over the columns ``sel`` of ``t [Ns, R]``, float32, ascending order."""
    m = np.full(t.shape[0], -np.inf, F32)
    for a in sel:
        m = np.fmax(m, t[:, a])
    s = np.zeros(t.shape[0], F32)
    for a in sel:
        s = s + np.exp2(t[:, a] - m)
    return m + np.log2(s)


def demod_sep_f32(constellation, y, noise_var, scale=1.0, want_stats=False):
    """demod_soft_sep_f32_kernel: label ``(a << NH) | b``, real part from ``a``, imaginary part from ``b``.  -> float64 ``[Ns * NB]``."""
    c = np.asarray(constellation, dtype=np.complex128)
    NB = int(np.log2(len(c)))
    NH, R = NB // 2, 1 << (NB // 2)
    axr = np.array([c[a << NH].real for a in range(R)]).astype(F32)
    axi = np.array([c[b].imag for b in range(R)]).astype(F32)
    y = np.atleast_1d(np.asarray(y, dtype=np.complex128))
    k = F32(-1.4426950408889634 / noise_var)
    sc = F32(scale) * LN2_F
    out = np.zeros((len(y), NB), F32)
    resummed = 0
    with np.errstate(all='ignore'):
        for ax, v, base in ((axr, y.real.astype(F32), NH), (axi, y.imag.astype(F32), 0)):
            d = v[:, None] - ax[None, :]
            t = d * d * k
            mx = t[:, 0]
            for a in range(1, R):
                mx = np.fmax(mx, t[:, a])
            e = np.exp2(t - mx[:, None])
            for b in range(NH):
                one = [a for a in range(R) if (a >> b) & 1]
                zero = [a for a in range(R) if not (a >> b) & 1]
                n, q = np.zeros(len(y), F32), np.zeros(len(y), F32)
                for a in range(R):
                    if (a >> b) & 1:
                        n = n + e[:, a]
                    else:
                        q = q + e[:, a]
                o = np.log2(n) - np.log2(q)
                again = ~(n >= F32_TINY) | ~(q >= F32_TINY)
                resummed += int(again.sum())
                out[:, base + b] = np.where(again, _lse2(t, one) - _lse2(t, zero), o)
        xr, xi = y.real.astype(F32), y.imag.astype(F32)
        poison = (xr - xr) + (xi - xi)
        out = (out + poison[:, None]) * sc
    res = out[:, ::-1].astype(np.float64).reshape(-1)                # out[b] -> llr[i * NB + NB - 1 - b]
    return (res, {'resummed': resummed}) if want_stats else res


def demod_gen_f32(constellation, y, noise_var, scale=1.0, want_stats=False):
    """demod_soft_f32_kernel: any table of M = 2^NB points, label bit b of point m = ``(m >> b) & 1``."""
    c = np.asarray(constellation, dtype=np.complex128)
    M, NB = len(c), int(np.log2(len(c)))
    cx, cy = c.real.astype(F32), c.imag.astype(F32)
    y = np.atleast_1d(np.asarray(y, dtype=np.complex128))
    x, yy = y.real.astype(F32), y.imag.astype(F32)
    k = F32(-1.4426950408889634 / noise_var)
    sc = F32(scale) * LN2_F
    Ns = len(y)
    resummed = 0
    with np.errstate(all='ignore'):
        t = np.zeros((Ns, M), F32)
        for m in range(M):
            dx, dy = x - cx[m], yy - cy[m]
            t[:, m] = (dx * dx + dy * dy) * k
        tmax = np.full(Ns, -np.inf, F32)
        for m in range(M):
            tmax = np.fmax(tmax, t[:, m])
        num, den = np.zeros((Ns, NB), F32), np.zeros((Ns, NB), F32)
        for m in range(M):
            e = np.exp2(t[:, m] - tmax)
            for b in range(NB):
                if (m >> b) & 1:
                    num[:, b] = num[:, b] + e
                else:
                    den[:, b] = den[:, b] + e
        out = np.log2(num) - np.log2(den)
        for b in range(NB):
            again = ~(num[:, b] >= F32_TINY) | ~(den[:, b] >= F32_TINY)
            resummed += int(again.sum())
            one = [m for m in range(M) if (m >> b) & 1]
            zero = [m for m in range(M) if not (m >> b) & 1]
            out[:, b] = np.where(again, _lse2(t, one) - _lse2(t, zero), out[:, b])
        out = out * sc
    res = out[:, ::-1].astype(np.float64).reshape(-1)
    return (res, {'resummed': resummed}) if want_stats else res


def demod_exponents(constellation, y, noise_var):
    """``t [Ns, M]`` = |y - c_a|^2 / N0 in nats, long double."""
    c = np.asarray(constellation, dtype=np.complex128)
    y = np.atleast_1d(np.asarray(y, dtype=np.complex128))
    dx = y.real.astype(np.longdouble)[:, None] - c.real.astype(np.longdouble)[None, :]
    dy = y.imag.astype(np.longdouble)[:, None] - c.imag.astype(np.longdouble)[None, :]
    return (dx * dx + dy * dy) / np.longdouble(noise_var)


def demod_ref(constellation, y, noise_var):
    """Long-double ``log sum_{bit=1} e^-t - log sum_{bit=0} e^-t``, each sum relative to its own smallest exponent: finite at every
    finite input.  -> long double ``[Ns * NB]``, most significant label bit first."""
    t = demod_exponents(constellation, y, noise_var)
    Ns, M = t.shape
    NB = int(np.log2(M))
    out = np.zeros((Ns, NB), np.longdouble)
    idx = np.arange(M)
    for b in range(NB):
        lse = []
        for want in (1, 0):
            ts = t[:, ((idx >> b) & 1) == want]
            mn = ts.min(axis=1)
            lse.append(-mn + np.log(np.exp(-(ts - mn[:, None])).sum(axis=1)))
        out[:, NB - 1 - b] = lse[0] - lse[1]
    return out.reshape(-1)


def demod_bound(constellation, y, noise_var, A=DEMOD_A):
    """``A + K 2^-24 max_a t_a`` per LLR (the module docstring derives it), float64 ``[Ns * NB]``."""
    t = demod_exponents(constellation, y, noise_var)
    NB = int(np.log2(t.shape[1]))
    return np.repeat(A + DEMOD_K * U * t.max(axis=1).astype(np.float64), NB)
