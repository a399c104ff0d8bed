"""A plain Python / NumPy model of binary BCH codes, written from the definitions; no engine import.

Field: GF(2^m) with alpha = x under a primitive polynomial; elements are ints (bit j = coefficient of alpha^j).  A word is n bits,
bit i the coefficient of x^(n-1-i): k message bits, then the n - k bits of x^(n-k) m(x) mod g(x).

decode: S_j = r(alpha^j), j = 1 .. 2t.  All zero: accepted, 0 errors.  Otherwise Berlekamp-Massey over the 2t syndromes gives
sigma(x) = 1 + c_1 x + ... of length L (sum_i c_i S_(j-i) = 0); FAILURE if L > t, if c_L = 0, or if sigma has not exactly L roots
among alpha^(-d), d = 0 .. n - 1 (the inverse locators of the n positions; a root at a degree >= n of a shortened code therefore
fails).  Otherwise the positions of the roots are flipped and errors = L.  After a failure the word is returned unchanged with
errors = -1.  The outcome is a function of the syndromes, so decode_batch decodes every distinct syndrome vector once.
"""
import numpy as np

DEFAULT_PRIM_POLY = {1: 3, 2: 7, 3: 11, 4: 19, 5: 37, 6: 67, 7: 137, 8: 285, 9: 529, 10: 1033, 11: 2053, 12: 4179, 13: 8219, 14: 17475,
                     15: 32771, 16: 69643}


class Field:
    def __init__(self, m, prim_poly=None):
        self.m, self.N = m, (1 << m) - 1
        self.prim_poly = p = DEFAULT_PRIM_POLY[m] if prim_poly is None else prim_poly
        assert p >> m == 1
        self.exp, self.log = [0] * self.N, [None] * (self.N + 1)
        v = 1
        for e in range(self.N):
            assert self.log[v] is None, "x does not generate the multiplicative group"
            self.exp[e], self.log[v] = v, e
            v <<= 1
            if v >> m:
                v ^= p
        assert v == 1
        self.exp_np = np.array(self.exp, dtype=np.int64)

    def mul(self, a, b):
        return 0 if a == 0 or b == 0 else self.exp[(self.log[a] + self.log[b]) % self.N]

    def div(self, a, b):
        return 0 if a == 0 else self.exp[(self.log[a] - self.log[b]) % self.N]


def poly_mul2(a, b):
    """Product of two binary polynomials held in ints."""
    out, s = 0, 0
    while b >> s:
        if (b >> s) & 1:
            out ^= a << s
        s += 1
    return out


def minpoly(f, e):
    """prod (X + alpha^j) over the conjugates j = e, 2e, 4e, ... of alpha^e; an int."""
    conj, j = [], e % f.N
    while j not in conj:
        conj.append(j)
        j = 2 * j % f.N
    poly = [1]                                                    # lowest degree first, coefficients in the field
    for j in conj:
        shifted = [0] + poly
        scaled = [f.mul(c, f.exp[j]) for c in poly] + [0]
        poly = [x ^ y for x, y in zip(shifted, scaled)]
    assert all(c in (0, 1) for c in poly)
    return sum(c << i for i, c in enumerate(poly))


def genpoly(m, t, prim_poly=None):
    """lcm of the minimal polynomials of alpha^1 .. alpha^2t; an int."""
    f = Field(m, prim_poly)
    g, used = 1, set()
    for e in range(1, 2 * t + 1):
        mp = minpoly(f, e)
        if mp not in used:
            used.add(mp)
            g = poly_mul2(g, mp)
    return g


class Code:
    def __init__(self, n, t, m, prim_poly=None):
        self.field = Field(m, prim_poly)
        self.n, self.t, self.m = n, t, m
        self.g = genpoly(m, t, prim_poly)
        self.deg = self.g.bit_length() - 1
        self.k = n - self.deg
        assert 0 < self.k and n <= self.field.N


def encode(msg, code):
    """One message [k] -> the code word [n], by bitwise long division."""
    msg = [int(b) for b in msg]
    assert len(msg) == code.k and all(b in (0, 1) for b in msg)
    r = 0
    for b in msg:                                                 # r = (r x + b x^deg) mod g
        r <<= 1
        if ((r >> code.deg) & 1) ^ b:
            r ^= code.g
        r &= (1 << code.deg) - 1
    return np.array(msg + [(r >> (code.deg - 1 - p)) & 1 for p in range(code.deg)], dtype=np.uint8)


def encode_batch(msgs, code):
    return np.stack([encode(m, code) for m in msgs]) if len(msgs) else np.zeros((0, code.n), np.uint8)


def syndromes(words, code):
    """[B, n] -> [B, 2t] ints."""
    f, n = code.field, code.n
    words = np.atleast_2d(np.asarray(words)) != 0
    deg = n - 1 - np.arange(n)
    out = np.zeros((words.shape[0], 2 * code.t), dtype=np.int64)
    for j in range(1, 2 * code.t + 1):
        terms = f.exp_np[(j * deg) % f.N]
        out[:, j - 1] = np.bitwise_xor.reduce(np.where(words, terms[None, :], 0), axis=1)
    return out


def berlekamp_massey(S, f):
    """(sigma coefficients lowest first, length L) of the syndromes S[0 .. 2t)."""
    C, Bp, L, sh, b = [1], [1], 0, 1, 1
    for r in range(len(S)):
        d = S[r]
        for i in range(1, L + 1):
            if i < len(C):
                d ^= f.mul(C[i], S[r - i])
        if d == 0:
            sh += 1
            continue
        coef = f.div(d, b)
        T = list(C)
        C = C + [0] * (len(Bp) + sh - len(C))
        for i, v in enumerate(Bp):
            C[i + sh] ^= f.mul(coef, v)
        if 2 * L <= r:
            L, Bp, b, sh = r + 1 - L, T, d, 1
        else:
            sh += 1
    return C, L


def error_degrees(S, code):
    """The degrees to flip for the syndromes S, or None for a failure."""
    f = code.field
    if not any(S):
        return []
    C, L = berlekamp_massey([int(s) for s in S], f)
    C = C + [0] * (L + 1 - len(C))
    assert not any(C[L + 1:])
    if L > code.t or C[L] == 0:
        return None
    d = np.arange(code.n)
    v = np.zeros(code.n, dtype=np.int64)
    for q, c in enumerate(C[:L + 1]):                             # sigma(alpha^-d) at every degree d of the word
        if c:
            v ^= f.exp_np[(f.log[c] - d * q) % f.N]
    roots = [int(x) for x in np.flatnonzero(v == 0)]
    return roots if len(roots) == L else None


def decode_batch(words, code):
    """[B, n] hard decisions (non-zero = 1) -> {'bits' [B, k], 'codeword' [B, n] uint8, 'errors' [B] int32}."""
    words = (np.atleast_2d(np.asarray(words)) != 0).astype(np.uint8)
    out = words.copy()
    errors = np.zeros(len(words), dtype=np.int32)
    if len(words):
        S = syndromes(words, code)
        uniq, inv = np.unique(S, axis=0, return_inverse=True)
        inv = inv.reshape(-1)
        for u, row in enumerate(uniq):
            degs = error_degrees(row, code)
            rows = np.flatnonzero(inv == u)
            if degs is None:
                errors[rows] = -1
            else:
                errors[rows] = len(degs)
                for d in degs:
                    out[rows, code.n - 1 - d] ^= 1
    return {"bits": out[:, :code.k].copy(), "codeword": out, "errors": errors}


def decode(word, code):
    r = decode_batch(np.asarray(word)[None, :], code)
    return {k: v[0] for k, v in r.items()}


def with_errors(words, positions):
    """A copy of words [B, n] with row b flipped at positions[b] (a list per row)."""
    out = np.array(words, dtype=np.uint8, copy=True)
    for b, pos in enumerate(positions):
        out[b, list(pos)] ^= 1
    return out


def error_sets(rs, B, n, k, e):
    """B position lists of exactly e distinct errors each (e >= 1): row 0 holds position 0, row 1 position n - 1, row 2 only parity
    positions, row 3 only message positions (where e of them exist), the others uniform."""
    sets = []
    for b in range(B):
        lo, hi = 0, n
        if b % 8 == 2 and n - k >= e:
            lo = k
        elif b % 8 == 3 and k >= e:
            hi = k
        pos = set(int(p) for p in lo + rs.choice(hi - lo, e, replace=False))
        if b % 8 == 0:
            pos.pop()
            pos.add(0)
        elif b % 8 == 1:
            pos.pop()
            pos.add(n - 1)
        while len(pos) < e:                                       # the forced position was already drawn
            pos.add(int(rs.randint(n)))
        sets.append(sorted(pos))
    return sets
