"""NumPy model of the tail-biting convolutional codec (csrc/tbcc.hip) -- TEST INFRASTRUCTURE ONLY.

The decoder rule, as the header, the kernel and ``tailbiting_decode`` state it (float64, sums in the order written):

    bm_t[c]  the sum over the n bits, MSB first and starting from 0.0, of viterbi_decode's per-bit metric for step t
    M[s] = 0 for every state before the first trip.  On trip w = 1 .. max_wraps:
    1. M_start = M
    2. steps t = 0 .. T - 1: every state takes its candidates in np.where order, cand_j = M[pred_j] + bm_t[code_j], and keeps the
       first minimum (a later candidate replaces the kept one only if it is strictly smaller); no rescaling across trips
    3. origin[s] = the state in which the survivor ending in s began this trip; net[s] = M[s] - M_start[origin[s]]
    4. s* = the first state of minimum M; origin[s*] == s*: that path, wraps = w, tailbiting = 1, metric = net[s*]
    5. otherwise c = the first state of minimum net among the states with origin[s] == s; c replaces the remembered candidate only
       if its net is strictly smaller; a remembered candidate keeps its bits
    6. after the last trip: the remembered candidate, wraps = max_wraps, tailbiting = 1; none: the path of the last s*,
       tailbiting = 0, metric = net[s*]
    A row with a NaN, or with +-inf under 'hard' / 'unquantized', is rejected: zero bits, wraps 0, tailbiting 0, metric NaN.

Loops over trips, steps, candidates and states are Python loops; every operation inside them is one NumPy call over the rows of the
batch.  Minima are taken by comparison loops (strictly smaller replaces), never by ``argmin``.  The origin is found here by walking
every survivor back over the trip's decisions -- the kernel carries it forward instead, so the two are independent.

The per-bit metric of 'soft' is ``log(exp(r) + 1)`` (bit 0) and that minus ``r`` (bit 1).  Its last bit depends on the routines that
evaluate exp and log, so ``soft_nll0`` restates the engine's (csrc/cpx_math.h: ``exp_pm500`` -- the device library's exp on
[-500, 500] -- and ``fast_log<false>``) operation for operation, the fused multiply-adds through an error-free product and sum;
tests/test_tbcc_host.py bounds it against ``np.log(np.exp(r) + 1)`` and checks ``fma`` against the C library's.
"""
import numpy as np

OUTCOME_REJECTED, OUTCOME_CLOSED, OUTCOME_CANDIDATE, OUTCOME_OPEN = 0, 1, 2, 3
_H = float.fromhex


# ---- the engine's exp and log -----------------------------------------------------------------------------------------------------------
def _two_prod(a, b):
    """a b = p + e exactly (Dekker / Veltkamp; no overflow or underflow at the magnitudes of the branch metrics)."""
    p = a * b
    t = 134217729.0 * a
    ah = t - (t - a)
    al = a - ah
    t = 134217729.0 * b
    bh = t - (t - b)
    bl = b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def fma(a, b, c):
    """a b + c rounded once: the exact product as p + e, the exact sum p + c as s + t, then s + (t + e)."""
    a, b, c = (np.asarray(v, dtype=np.float64) for v in (a, b, c))
    p, e = _two_prod(a, b)
    s = p + c
    bb = s - p
    t = (p - (s - bb)) + (c - bb)
    return s + (t + e)


def exp_pm500(x):
    """csrc/cpx_math.h exp_pm500, for |x| <= 500."""
    x = np.asarray(x, dtype=np.float64)
    dn = np.rint(x * _H('0x1.71547652b82fep+0'))
    f = fma(-dn, _H('0x1.62e42fefa39efp-1'), x)
    f = fma(-dn, _H('0x1.abc9e3b39803fp-56'), f)
    p = fma(f, _H('0x1.ade156a5dcb37p-26'), _H('0x1.28af3fca7ab0cp-22'))
    for c in ('0x1.71dee623fde64p-19', '0x1.a01997c89e6b0p-16', '0x1.a01a014761f6ep-13', '0x1.6c16c1852b7b0p-10', '0x1.1111111122322p-7',
              '0x1.55555555502a1p-5', '0x1.5555555555511p-3', '0x1.000000000000bp-1', '0x1p+0', '0x1p+0'):
        p = fma(f, p, _H(c))
    return np.ldexp(p, dn.astype(np.int64))


def log_ge1(x):
    """csrc/cpx_math.h fast_log<false>, for finite x >= 1."""
    ln2_hi, ln2_lo = 6.93147180369123816490e-01, 1.90821492927058770002e-10
    Lg1, Lg2, Lg3, Lg4 = 6.666666666666735130e-01, 3.999999999940941908e-01, 2.857142874366239149e-01, 2.222219843214978396e-01
    Lg5, Lg6, Lg7 = 1.818357216161805012e-01, 1.531383769920937332e-01, 1.479819860511658591e-01
    m, e = np.frexp(np.asarray(x, dtype=np.float64))
    lo = m < 7.07106781186547524401e-01
    m = np.where(lo, m + m, m)
    e = np.where(lo, e - 1, e)
    f = m - 1.0
    s = f / (2.0 + f)
    z = s * s
    w = z * z
    t1 = w * fma(w, fma(w, Lg6, Lg4), Lg2)
    t2 = z * fma(w, fma(w, fma(w, Lg7, Lg5), Lg3), Lg1)
    R = t2 + t1
    hfsq = 0.5 * f * f
    dk = e.astype(np.float64)
    return dk * ln2_hi - ((hfsq - (s * (hfsq + R) + dk * ln2_lo)) - f)


def soft_nll0(r):
    """log(exp(r) + 1) for r already clipped to +-500, as the engine evaluates it."""
    return log_ge1(exp_pm500(r) + 1.0)


# ---- trellis tables ---------------------------------------------------------------------------------------------------------------------
def pred_tables(trellis):
    """Predecessors of every state in np.where (row-major) order: [S, I] previous state, input, output code."""
    nxt, out = np.asarray(trellis.next_state_table), np.asarray(trellis.output_table)
    S, I = nxt.shape
    ps, pi, pc = (np.zeros((S, I), np.int64) for _ in range(3))
    cnt = np.zeros(S, np.int64)
    for p in range(S):
        for i in range(I):
            s = nxt[p, i]
            ps[s, cnt[s]], pi[s, cnt[s]], pc[s, cnt[s]] = p, i, out[p, i]
            cnt[s] += 1
    assert (cnt == I).all()
    return ps, pi, pc


def bit_metrics(coded, decoding_type):
    """viterbi_decode's per-bit metrics of every received value: (cost of code bit 0, cost of code bit 1)."""
    r = np.asarray(coded, dtype=np.float64)
    if decoding_type == 'hard':
        ri = r.astype(np.int64)
        return (ri ^ 0).astype(np.float64), (ri ^ 1).astype(np.float64)
    if decoding_type == 'soft':
        r = np.clip(r, -500.0, 500.0)
        nll0 = soft_nll0(r)
        return nll0, nll0 - r
    if decoding_type != 'unquantized':
        raise ValueError(decoding_type)
    d0, d1 = r - (-1.0), r - 1.0
    return d0 * d0, d1 * d1


def rejected_rows(coded, decoding_type):
    x = np.asarray(coded, dtype=np.float64)
    return np.isnan(x).any(axis=1) | (np.isinf(x).any(axis=1) if decoding_type != 'soft' else False)


def branch_metrics(coded, n, decoding_type):
    """[B, T, 2^n]: bm_t[c], the per-bit metrics summed MSB first from 0.0."""
    m0, m1 = bit_metrics(coded, decoding_type)
    B = m0.shape[0]
    m0, m1 = m0.reshape(B, -1, n), m1.reshape(B, -1, n)
    bm = np.zeros((B, m0.shape[1], 1 << n))
    for c in range(1 << n):
        for j in range(n):
            bm[:, :, c] = bm[:, :, c] + (m1[:, :, j] if (c >> (n - 1 - j)) & 1 else m0[:, :, j])
    return bm


# ---- encoder ----------------------------------------------------------------------------------------------------------------------------
def encode_batch(message_bits, trellis):
    """[B, T k] 0 / 1 -> (code words [B, T n] uint8, closed [B] bool): two table walks."""
    msg = np.asarray(message_bits).astype(np.int64)
    k, n = int(trellis.k), int(trellis.n)
    nxt, out = np.asarray(trellis.next_state_table), np.asarray(trellis.output_table)
    B, T = msg.shape[0], msg.shape[1] // k
    sym = np.zeros((B, T), np.int64)
    for b in range(k):
        sym = (sym << 1) | msg[:, b::k]
    st = np.zeros(B, np.int64)
    for t in range(T):
        st = nxt[st, sym[:, t]]
    start = st.copy()
    word = np.zeros((B, T * n), np.uint8)
    for t in range(T):
        code = out[st, sym[:, t]]
        for j in range(n):
            word[:, t * n + j] = (code >> (n - 1 - j)) & 1
        st = nxt[st, sym[:, t]]
    return word, st == start


def direct_metric(word_bits, coded, decoding_type):
    """The metric of a code word [B, T n] against the received rows: its per-bit metrics summed one after the other from 0.0."""
    m0, m1 = bit_metrics(coded, decoding_type)
    per = np.where(np.asarray(word_bits) != 0, m1, m0)
    acc = np.zeros(per.shape[0])
    for q in range(per.shape[1]):
        acc = acc + per[:, q]
    return acc


# ---- decoder ----------------------------------------------------------------------------------------------------------------------------
def decode_batch(coded, trellis, decoding_type='hard', max_wraps=4):
    """coded [B, T n] -> dict: 'bits' [B, T k] uint8, 'wraps' [B] int32, 'tailbiting' [B] uint8, 'metric' [B] float64, and for the
    tests 'outcome' [B] (OUTCOME_*) and 'mmax' [B], the largest state metric when the row finished."""
    x = np.array(coded, dtype=np.float64, ndmin=2)
    k, n, S = int(trellis.k), int(trellis.n), int(trellis.number_states)
    B, T = x.shape[0], x.shape[1] // n
    if B == 0:
        return {'bits': np.zeros((0, T * k), np.uint8), 'wraps': np.zeros(0, np.int32), 'tailbiting': np.zeros(0, np.uint8),
                'metric': np.zeros(0), 'outcome': np.zeros(0, np.int64), 'mmax': np.zeros(0)}
    ps, pi, pc = pred_tables(trellis)
    I = ps.shape[1]
    rejected = rejected_rows(x, decoding_type)
    x[rejected] = 0.0
    bm = branch_metrics(x, n, decoding_type)
    rows = np.arange(B)
    bits = np.zeros((B, T * k), np.uint8)
    wraps, tailbiting = np.zeros(B, np.int32), np.zeros(B, np.uint8)
    metric, mmax = np.full(B, np.nan), np.zeros(B)
    outcome = np.full(B, OUTCOME_REJECTED)
    done = rejected.copy()
    have_cand, cand_net = np.zeros(B, bool), np.zeros(B)
    M = np.zeros((B, S))

    def walk(start, choice):
        """The input symbols [B, T] of the survivors ending in ``start`` [B]."""
        st, sym = start.copy(), np.zeros((B, T), np.int64)
        for t in range(T - 1, -1, -1):
            j = choice[t, rows, st]
            sym[:, t] = pi[st, j]
            st = ps[st, j]
        return sym

    def keep(mask, start, choice):
        if mask.any():
            sym = walk(start, choice)
            for b in range(k):
                bits[mask, b::k] = ((sym[mask] >> (k - 1 - b)) & 1).astype(np.uint8)

    for w in range(1, max_wraps + 1):
        if done.all():
            break
        M_start = M.copy()
        choice = np.zeros((T, B, S), np.int64)
        for t in range(T):
            best = M[:, ps[:, 0]] + bm[:, t, :][:, pc[:, 0]]
            jb = np.zeros((B, S), np.int64)
            for j in range(1, I):
                cand = M[:, ps[:, j]] + bm[:, t, :][:, pc[:, j]]
                better = cand < best
                best = np.where(better, cand, best)
                jb = np.where(better, j, jb)
            M, choice[t] = best, jb
        origin = np.tile(np.arange(S), (B, 1))                   # walked back over the trip, every state of every row at once
        for t in range(T - 1, -1, -1):
            origin = ps[origin, choice[t][rows[:, None], origin]]
        net = M - np.take_along_axis(M_start, origin, axis=1)
        sstar, low = np.zeros(B, np.int64), M[:, 0].copy()
        for s in range(1, S):
            better = M[:, s] < low
            low = np.where(better, M[:, s], low)
            sstar = np.where(better, s, sstar)
        c, c_net, c_any = np.zeros(B, np.int64), np.zeros(B), np.zeros(B, bool)
        for s in range(S):
            take = (origin[:, s] == s) & (~c_any | (net[:, s] < c_net))
            c = np.where(take, s, c)
            c_net = np.where(take, net[:, s], c_net)
            c_any |= take
        live = ~done
        closed = live & (origin[rows, sstar] == sstar)
        keep(closed, sstar, choice)
        wraps[closed], tailbiting[closed], metric[closed], outcome[closed] = w, 1, net[rows, sstar][closed], OUTCOME_CLOSED
        live &= ~closed
        better = live & c_any & (~have_cand | (c_net < cand_net))
        keep(better, c, choice)
        have_cand |= better
        cand_net = np.where(better, c_net, cand_net)
        if w == max_wraps:
            cand, none = live & have_cand, live & ~have_cand
            wraps[live] = w
            tailbiting[cand], metric[cand], outcome[cand] = 1, cand_net[cand], OUTCOME_CANDIDATE
            keep(none, sstar, choice)
            metric[none], outcome[none] = net[rows, sstar][none], OUTCOME_OPEN
            closed = closed | live
        mmax[closed] = M.max(axis=1)[closed]
        done |= closed
    return {'bits': bits, 'wraps': wraps, 'tailbiting': tailbiting, 'metric': metric, 'outcome': outcome, 'mmax': mmax}


# ---- brute force ------------------------------------------------------------------------------------------------------------------------
def all_codewords(trellis, T):
    """Every tail-biting code word of T steps (k = 1): messages [2^T, T] and words [2^T, T n]; rows that do not close are dropped."""
    msgs = (np.arange(1 << T)[:, None] >> np.arange(T - 1, -1, -1)[None, :]) & 1
    words, closed = encode_batch(msgs, trellis)
    return msgs[closed], words[closed]


def brute_force_minimum(coded, words, decoding_type):
    """[B]: the smallest directly summed metric over ``words`` [W, T n] (the sum runs position by position from 0.0)."""
    m0, m1 = bit_metrics(coded, decoding_type)
    acc = np.zeros((m0.shape[0], words.shape[0]))
    for q in range(words.shape[1]):
        acc = acc + np.where(words[None, :, q] != 0, m1[:, q, None], m0[:, q, None])
    low = acc[:, 0].copy()
    for v in range(1, acc.shape[1]):
        low = np.where(acc[:, v] < low, acc[:, v], low)
    return low
