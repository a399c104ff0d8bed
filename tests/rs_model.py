"""A plain Python / NumPy model of Reed-Solomon codes with errors-and-erasures decoding, written from the definitions; no engine import.

Field: bch_model.Field.  A word is n symbols, symbol i the coefficient of x^(n-1-i) (its "degree" d = n-1-i): k message symbols, then
the r = n - k symbols of x^r m(x) mod g(x), g(x) = prod_{j<r} (x - alpha^(fcr+j)).

decode, with f flagged positions:
1. f > r: FAILURE.
2. S_j = R(alpha^(fcr+j)), j = 0 .. r-1, from the symbols as given.  All zero: accepted, 0 errors.
3. Gamma(x) = prod (1 - alpha^d x) over the flagged degrees d.
4. Berlekamp-Massey on rho = f .. r-1, started with C = B = Gamma, L = f, b = 1, shift 1; discrepancy sum_{q<=L} C_q S_(rho-q); the
   length changes when 2L <= rho + f, to rho + 1 - L + f.
5. FAILURE if 2(L - f) + f > r, if Lambda_L = 0, or if Lambda = C has not exactly L roots among alpha^(-d), d = 0 .. n-1.
6. Omega = S Lambda mod x^r; at every root Y = alpha^(d(1-fcr)) Omega(alpha^-d) / Lambda'(alpha^-d) is XORed into the symbol;
   errors = L - f.
7. After a failure the word is returned unchanged with errors = -1.
The outcome is a function of the syndromes and the flags, so decode_batch decodes every distinct (syndromes, flags) row once.
"""
import numpy as np

from bch_model import Field


def genpoly(f, r, fcr=1):
    """prod_{j<r} (x - alpha^(fcr+j)): a list of r + 1 field elements, lowest degree first."""
    g = [1]
    for j in range(r):
        root = f.exp[(fcr + j) % f.N]
        g = [a ^ b for a, b in zip([0] + g, [f.mul(c, root) for c in g] + [0])]
    return g


class Code:
    def __init__(self, n, k, m, prim_poly=None, fcr=1):
        self.field = Field(m, prim_poly)
        self.n, self.k, self.m, self.r, self.fcr = n, k, m, n - k, fcr
        assert 1 <= k < n <= self.field.N and 0 <= fcr < self.field.N
        self.g = genpoly(self.field, self.r, fcr)
        self.log_np = np.array([0] + self.field.log[1:], dtype=np.int64)


def encode_batch(msgs, code):
    """[B, k] -> [B, n] uint16: the division of x^r m(x) by g, one message symbol per step, all rows at once."""
    f, r = code.field, code.r
    msgs = np.asarray(msgs, dtype=np.int64).reshape(-1, code.k)
    assert msgs.size == 0 or (msgs.min() >= 0 and msgs.max() <= f.N)
    rem = np.zeros((len(msgs), r), dtype=np.int64)                # column i: the coefficient of x^i
    glog = [None if c == 0 else f.log[c] for c in code.g[:r]]
    for s in range(code.k):
        fb = rem[:, r - 1] ^ msgs[:, s]
        lf = code.log_np[fb]
        rem[:, 1:] = rem[:, :-1].copy()
        rem[:, 0] = 0
        for i in range(r):
            if glog[i] is not None:
                rem[:, i] ^= np.where(fb != 0, f.exp_np[(lf + glog[i]) % f.N], 0)
    return np.concatenate([msgs, rem[:, ::-1]], axis=1).astype(np.uint16)


def syndromes(words, code):
    """[B, n] -> [B, r] ints."""
    f, n = code.field, code.n
    words = np.atleast_2d(np.asarray(words)).astype(np.int64)
    deg = n - 1 - np.arange(n)
    lw = code.log_np[words]
    out = np.zeros((words.shape[0], code.r), dtype=np.int64)
    for j in range(code.r):
        terms = np.where(words != 0, f.exp_np[(lw + (code.fcr + j) * deg[None, :]) % f.N], 0)
        out[:, j] = np.bitwise_xor.reduce(terms, axis=1)
    return out


def poly_eval(f, poly, x):
    acc = 0
    for c in reversed(poly):
        acc = f.mul(acc, x) ^ c
    return acc


def corrections(S, flagged, code):
    """For the syndromes S and the list of flagged degrees: None after a failure, else (errors, [(degree, Y), ...])."""
    f, r, n = code.field, code.r, code.n
    nf = len(flagged)
    if nf > r:
        return None
    S = [int(s) for s in S]
    if not any(S):
        return 0, []
    C = [1]
    for d in flagged:                                             # times (1 - alpha^d x)
        C = [a ^ b for a, b in zip(C + [0], [0] + [f.mul(c, f.exp[d]) for c in C])]
    Bp, L, b, sh = list(C), nf, 1, 1
    for rho in range(nf, r):
        d = 0
        for q in range(min(L, len(C) - 1) + 1):
            d ^= f.mul(C[q], S[rho - q])
        if d == 0:
            sh += 1
            continue
        coef = f.div(d, b)
        T = list(C)
        C = C + [0] * (len(Bp) + sh - len(C))
        for i, v in enumerate(Bp):
            C[i + sh] ^= f.mul(coef, v)
        if 2 * L <= rho + nf:
            L, Bp, b, sh = rho + 1 - L + nf, T, d, 1
        else:
            sh += 1
    C = C + [0] * (L + 1 - len(C))
    assert not any(C[L + 1:])
    lam = C[:L + 1]
    if 2 * (L - nf) + nf > r or lam[L] == 0:
        return None
    degs = np.arange(n)
    v = np.zeros(n, dtype=np.int64)
    for q, c in enumerate(lam):                                   # Lambda(alpha^-d) at every degree d of the word
        if c:
            v ^= f.exp_np[(f.log[c] - degs * q) % f.N]
    roots = [int(x) for x in np.flatnonzero(v == 0)]
    if len(roots) != L:
        return None
    omega = [0] * r
    for i in range(r):
        for q in range(min(i, L) + 1):
            omega[i] ^= f.mul(lam[q], S[i - q])
    deriv = [lam[q] if q % 2 else 0 for q in range(1, L + 1)]     # Lambda'(x): the coefficient of x^(q-1) is q Lambda_q
    fixes = []
    for d in roots:
        x = f.exp[(-d) % f.N]
        y = f.div(poly_eval(f, omega, x), poly_eval(f, deriv, x))
        fixes.append((d, f.mul(y, f.exp[(d * (1 - code.fcr)) % f.N])))
    return L - nf, fixes


def decode_batch(words, code, erased=None, detail=False):
    """[B, n] symbols and [B, n] flags (non-zero = erased; None: no flags) -> {'symbols' [B, k], 'codeword' [B, n] uint16,
    'errors' [B] int32}; with ``detail`` also 'zero_at_unflagged' [B] bool: some unflagged root got Y = 0."""
    words = np.atleast_2d(np.asarray(words)).astype(np.int64)
    assert words.size == 0 or (words.min() >= 0 and words.max() <= code.field.N)
    flags = np.zeros(words.shape, dtype=bool) if erased is None else np.atleast_2d(np.asarray(erased)) != 0
    assert flags.shape == words.shape
    out = words.copy()
    errors = np.zeros(len(words), dtype=np.int32)
    odd = np.zeros(len(words), dtype=bool)
    if len(words):
        key = np.concatenate([syndromes(words, code), flags.astype(np.int64)], axis=1)
        uniq, inv = np.unique(key, axis=0, return_inverse=True)
        inv = inv.reshape(-1)
        for u, row in enumerate(uniq):
            flagged = [code.n - 1 - int(i) for i in np.flatnonzero(row[code.r:])]
            res = corrections(row[:code.r], flagged, code)
            rows = np.flatnonzero(inv == u)
            if res is None:
                errors[rows] = -1
                continue
            errors[rows] = res[0]
            for d, y in res[1]:
                out[rows, code.n - 1 - d] ^= y
                if y == 0 and d not in flagged:
                    odd[rows] = True
    out = out.astype(np.uint16)
    res = {"symbols": out[:, :code.k].copy(), "codeword": out, "errors": errors}
    if detail:
        res["zero_at_unflagged"] = odd
    return res


def brute_force(words, flags, cws, r):
    """Bounded-distance errors-and-erasures decoding by definition: per word the index of the unique code word c of ``cws`` with
    2 #{i unflagged: c_i != r_i} + f <= r, or -1; asserts that no two qualify.  Returns (index [B], unflagged differences [B])."""
    words, flags, cws = np.asarray(words, dtype=np.int64), np.asarray(flags) != 0, np.asarray(cws, dtype=np.int64)
    idx = np.full(len(words), -1, dtype=np.int64)
    diff = np.zeros(len(words), dtype=np.int64)
    for b in range(len(words)):
        e = ((cws != words[b][None, :]) & ~flags[b][None, :]).sum(axis=1)
        ok = np.flatnonzero(2 * e + flags[b].sum() <= r)
        assert len(ok) <= 1
        if len(ok):
            idx[b], diff[b] = ok[0], e[ok[0]]
    return idx, diff


def flag_sets(rs, B, n, counts):
    """[B, n] bool with exactly counts[b] flags in row b, uniform positions."""
    flags = np.zeros((B, n), dtype=bool)
    for b in range(B):
        flags[b, rs.choice(n, int(counts[b]), replace=False)] = True
    return flags


def with_errors(rs, words, flags, counts, q):
    """A copy of words [B, n] with counts[b] symbols of row b changed (to another value below q) at unflagged positions; returns the
    copy and the position lists.  Rows 0, 8, 16, ... take position 0 and rows 1, 9, 17, ... position n - 1 where they are free."""
    out = np.array(words, dtype=np.uint16, copy=True)
    sets = []
    for b in range(len(out)):
        free = np.flatnonzero(~np.asarray(flags[b], dtype=bool))
        e = int(counts[b])
        assert e <= len(free)
        pos = set(int(p) for p in rs.choice(free, e, replace=False))
        forced = 0 if b % 8 == 0 else out.shape[1] - 1 if b % 8 == 1 else None
        if e and forced is not None and forced in free and forced not in pos:
            pos.pop()
            pos.add(forced)
        pos = sorted(pos)
        for p in pos:
            out[b, p] ^= rs.randint(1, q)
        sets.append(pos)
    return out, sets
