"""NumPy model of the polar codec: the encoder, the CRC, successive cancellation (SC) and successive-cancellation list (SCL) decoding.

Plain and slow on purpose -- one path at a time, whole arrays copied at every fork -- so that it shares nothing with the kernels
but the definitions:

  x = u F^{(x)n} over GF(2), F = [[1,0],[1,1]], natural order; information bit k at the k-th smallest information position.
  f(a, b) = min(|a|, |b|), negated iff (a < 0) != (b < 0);  g(a, b, u) = b + a if u == 0 else b - a;  float64.
  Frozen bit: u = 0, the path metric grows by |lambda| iff lambda < 0.
  Information bit: every path r, in rank order, yields (r, 0) then (r, 1); candidate (r, u) costs PM_r + |lambda| if u != (lambda < 0)
  else PM_r; the candidates are sorted stably by metric and the first min(L, 2 live) survive, in that order.
  The chosen path is the lowest-ranked one whose information bits pass the CRC (rank 0 and crc_ok = 0 if none; rank 0 and
  crc_ok = 1 without a CRC).

The stable sort runs on ``metric_key``: the metric's bit pattern as an unsigned integer with the order of the values and every NaN
last.  For the metrics of finite LLRs (non-negative, never -0.0) this is the order of the metrics themselves.
"""
import numpy as np


def reliability_order(N):
    w = [sum(2.0 ** (j / 4.0) for j in range(N.bit_length()) if (i >> j) & 1) for i in range(N)]
    return np.array(sorted(range(N), key=lambda i: (w[i], i)), dtype=np.int64)


def frozen_mask(N, K, order=None):
    order = reliability_order(N) if order is None else np.asarray(order)
    fz = np.ones(N, dtype=np.uint8)
    fz[order[N - K:]] = 0
    return fz


def kron_matrix(N):
    G = np.array([[1]], dtype=np.int64)
    while G.shape[0] < N:
        G = np.kron(np.array([[1, 0], [1, 1]], dtype=np.int64), G)
    return G


def transform(u):
    """u F^{(x)n} for every row of ``u [..., N]`` by butterflies: x[i] ^= x[i + d] where bit d of i is clear."""
    x = np.array(u, dtype=np.uint8)
    N = x.shape[-1]
    d = 1
    while d < N:
        i = np.flatnonzero((np.arange(N) & d) == 0)
        x[..., i] ^= x[..., i + d]
        d *= 2
    return x


# ---- CRC ------------------------------------------------------------------------------------------------------------------------------
def crc_table(g, K):
    """[K] uint32: x^(K-1-k) mod g, g with its leading term."""
    c = g.bit_length() - 1
    tab, r = np.zeros(K, dtype=np.uint32), 1
    for k in range(K - 1, -1, -1):
        tab[k] = r
        r <<= 1
        if r >> c:
            r ^= g
    return tab


def crc_syndrome(bits, table):
    s = 0
    for k in np.flatnonzero(np.asarray(bits)):
        s ^= int(table[k])
    return s


def crc_long_division(message, g):
    """The c remainder bits of m(x) x^c mod g, most significant first, by bitwise long division."""
    c = g.bit_length() - 1
    reg = [int(b) for b in message] + [0] * c
    gb = [(g >> (c - j)) & 1 for j in range(c + 1)]
    for i in range(len(message)):
        if reg[i]:
            for j in range(c + 1):
                reg[i + j] ^= gb[j]
    return np.array(reg[len(message):], dtype=np.uint8)


def info_bits(message, K, g=None):
    """The K information bits of a message of A = K - deg g bits."""
    message = np.asarray(message, dtype=np.uint8)
    if g is None:
        assert message.size == K
        return message.copy()
    c = g.bit_length() - 1
    assert message.size == K - c
    s = crc_syndrome(message, crc_table(g, K)[:K - c])
    return np.concatenate([message, np.array([(s >> (c - 1 - j)) & 1 for j in range(c)], dtype=np.uint8)])


def encode(message, frozen, g=None):
    frozen = np.asarray(frozen)
    pos = np.flatnonzero(frozen == 0)
    u = np.zeros(frozen.size, dtype=np.uint8)
    u[pos] = info_bits(message, pos.size, g)
    return transform(u)


# ---- decoding -------------------------------------------------------------------------------------------------------------------------
def f(a, b):
    m = np.minimum(np.abs(a), np.abs(b))
    return np.where((a < 0) != (b < 0), -m, m)


def g_(a, b, u):
    return np.where(u == 0, b + a, b - a)


def metric_key(m):
    b = np.asarray(m, dtype=np.float64).view(np.uint64)
    key = np.where(b >> np.uint64(63), ~b, b | np.uint64(1 << 63))
    return np.where(np.isnan(m), np.uint64(2 ** 64 - 1), key)


class _Path:
    """One path: the LLR arrays of the levels (level s has 2^s values; level n is the channel), the re-encoded bits of the left
    children, the bits decided so far and the metric."""

    def __init__(self, llr):
        n = llr.size.bit_length() - 1
        self.n = n
        self.lv = [None] * n + [llr]
        self.xl = [None] * n
        self.u = []
        self.pm = np.float64(0.0)

    def fork(self):
        q = _Path.__new__(_Path)
        q.n, q.pm = self.n, self.pm
        q.lv = [None if v is None else v.copy() for v in self.lv]
        q.xl = [None if v is None else v.copy() for v in self.xl]
        q.u = list(self.u)
        return q

    def decision_llr(self, phi):
        top = self.n - 1 if phi == 0 else (phi & -phi).bit_length() - 1
        for s in range(top, -1, -1):
            src, h = self.lv[s + 1], 1 << s
            a, b = src[:h], src[h:]
            self.lv[s] = g_(a, b, self.xl[s]) if (phi >> s) & 1 else f(a, b)
        return self.lv[0][0]

    def decide(self, phi, bit):
        self.u.append(bit)
        x = np.array([bit], dtype=np.uint8)
        s = 0
        while (phi >> s) & 1:                       # a right child has returned: combine with its left sibling
            x = np.concatenate([self.xl[s] ^ x, x])
            s += 1
        if s < self.n:
            self.xl[s] = x


def decode(llr, frozen, L=1, g=None):
    """One word.  Returns a dict: bits [A], crc_ok, metric, u_llr [N] (L = 1 only, else None), list_bits [L, K], list_metric [L],
    live -- what the engine returns, rows past the live count zero / +inf."""
    llr = np.asarray(llr, dtype=np.float64)
    frozen = np.asarray(frozen)
    N = llr.size
    pos = np.flatnonzero(frozen == 0)
    K = pos.size
    c = 0 if g is None else g.bit_length() - 1
    paths = [_Path(llr)]
    u_llr = np.zeros(N) if L == 1 else None
    with np.errstate(invalid='ignore'):
        for phi in range(N):
            lam = [p.decision_llr(phi) for p in paths]
            if L == 1:
                u_llr[phi] = lam[0]
            if frozen[phi]:
                for p, l in zip(paths, lam):
                    if l < 0:
                        p.pm = p.pm + np.abs(l)
                    p.decide(phi, 0)
                continue
            cand = []
            for p, l in zip(paths, lam):
                for u in (0, 1):
                    cand.append((p, u, p.pm + np.abs(l) if u != int(l < 0) else p.pm))
            order = np.argsort(metric_key(np.array([m for _, _, m in cand])), kind='stable')[:min(L, len(cand))]
            new = []
            for i in order:
                p, u, m = cand[i]
                q = p.fork()
                q.pm = np.float64(m)
                q.decide(phi, u)
                new.append(q)
            paths = new
    live = len(paths)
    list_bits = np.zeros((L, K), dtype=np.uint8)
    list_metric = np.full(L, np.inf)
    for r, p in enumerate(paths):
        list_bits[r] = np.array(p.u, dtype=np.uint8)[pos]
        list_metric[r] = p.pm
    chosen, ok = 0, 1
    if g is not None:
        tab = crc_table(g, K)
        passing = [r for r in range(live) if crc_syndrome(list_bits[r], tab) == 0]
        chosen, ok = (passing[0], 1) if passing else (0, 0)
    return dict(bits=list_bits[chosen, :K - c].copy(), crc_ok=ok, metric=list_metric[chosen], u_llr=u_llr, list_bits=list_bits,
                list_metric=list_metric, live=live)


def decode_batch(llr, frozen, L=1, g=None):
    """Rows of ``llr [B, N]`` -> dict of stacked results."""
    rows = [decode(r, frozen, L, g) for r in np.atleast_2d(llr)]
    return {k: (None if rows[0][k] is None else np.stack([np.asarray(r[k]) for r in rows])) for k in rows[0]}


# ---- the seeded sets the host and GPU tests share -------------------------------------------------------------------------------------
def awgn_llrs(seed, frozen, g, n_words, ebn0_db):
    """(messages [n, A], llr [n, N]): BPSK over AWGN at Eb/N0 per message bit, LLR = 2 y / sigma^2."""
    frozen = np.asarray(frozen)
    N, K = frozen.size, int((frozen == 0).sum())
    A = K - (0 if g is None else g.bit_length() - 1)
    rs = np.random.RandomState(seed)
    msg = rs.randint(0, 2, (n_words, A)).astype(np.uint8)
    x = np.stack([encode(m, frozen, g) for m in msg])
    sigma2 = 1.0 / (2.0 * (A / N) * 10.0 ** (ebn0_db / 10.0))
    y = 1.0 - 2.0 * x + np.sqrt(sigma2) * rs.randn(n_words, N)
    return msg, 2.0 * y / sigma2


def sign_llrs(seed, n_words, N):
    """+-1-valued LLRs: path metrics are small integers, so final lists hold many exact ties."""
    return np.random.RandomState(seed).choice([-1.0, 1.0], size=(n_words, N))
