"""Generator polynomials of binary cyclic, BCH and Reed-Solomon codes (host only), from the field tables of ``gfields``."""
import numpy as np

from commpy_amd.channelcoding.gfields import MAX_M, clmul, field, whole

__all__ = ['cyclic_code_genpoly', 'bch_genpoly', 'rs_genpoly']


def cyclic_code_genpoly(n, k):
    """Every generator polynomial of a binary cyclic (n, k) code, as integers (bit i = coefficient of x^i).

    ``n`` is odd (ValueError otherwise) and divides ``2^m - 1`` for the smallest such m <= 16.  The n-th roots of unity of GF(2^m)
    are the ``alpha^e`` with ``e`` a multiple of ``(2^m - 1) / n``; they are visited in ascending tuple form, the first one that no
    earlier cyclotomic coset holds opens the next coset, and the cosets' minimal polynomials -- the irreducible factors of
    ``x^n - 1`` -- are taken in that order.  A generator is the product of a subset whose degrees sum to ``n - k``; subsets are
    listed as the integers ``1 .. 2^c - 1`` in rising order with the first coset at the most significant bit.  For ``n = 2^m - 1``
    this is the reference's list and order; for a proper divisor the reference multiplies factors of ``x^(2^m - 1) - 1`` that do
    not divide ``x^n - 1``, which this function does not (DESIGN: BCH codes).  Returns an int64 array, or an object array of
    Python ints where ``n - k`` exceeds 62."""
    n, k = whole(n, 'n', 1), whole(k, 'k', 1)
    if n % 2 == 0:
        raise ValueError('n cannot be an even number')
    if k >= n:
        raise ValueError('k = %d, need k < n = %d' % (k, n))
    m = next((m for m in range(1, MAX_M + 1) if ((1 << m) - 1) % n == 0), None)
    if m is None:
        raise ValueError('n = %d divides no 2^m - 1 with m <= %d' % (n, MAX_M))
    f = field(m)
    step = f.n // n
    seen = set()
    factors, degrees = [], []
    for v in range(1, f.n + 1):
        e = int(f.log[v])
        if e % step or e in seen:
            continue
        coset = f.coset(e)
        seen.update(coset)
        factors.append(f.minpoly(e))
        degrees.append(len(coset))
    tail = np.concatenate([np.cumsum(degrees[::-1])[::-1], [0]])      # degrees still available from factor i on
    found = []

    def choose(i, left, product):
        # leaving factor i out comes before taking it: rising order of the subset's integer, factor 0 at the top bit
        if left == 0:
            found.append(product)
            return
        if i == len(factors) or left > tail[i]:
            return
        choose(i + 1, left, product)
        if degrees[i] <= left:
            choose(i + 1, left - degrees[i], clmul(product, factors[i]))

    choose(0, n - k, 1)
    return np.array(found, dtype=np.int64 if n - k <= 62 else object)


def bch_genpoly(m, t, prim_poly=None):
    """The generator of the narrow-sense binary BCH code of length ``2^m - 1`` that corrects ``t`` errors: the least common multiple
    of the minimal polynomials of ``alpha^1 .. alpha^(2 t)`` in GF(2^m) under ``prim_poly`` (None: the default of that degree), as a
    Python int (degrees pass 63).  Needs ``2 t < 2^m - 1``."""
    f = field(m, prim_poly)
    t = whole(t, 't', 1)
    if 2 * t >= f.n:
        raise ValueError('t = %d, need 2 t < 2^m - 1 = %d' % (t, f.n))
    seen = set()
    g = 1
    for e in range(1, 2 * t + 1, 2):                      # alpha^(2 j) is a conjugate of alpha^j
        if e in seen:
            continue
        seen.update(f.coset(e))
        g = clmul(g, f.minpoly(e))
    return g


def rs_genpoly(m, nroots, fcr=1, prim_poly=None):
    """The generator of the Reed-Solomon codes over GF(2^m) with ``nroots`` parity symbols:
    ``g(x) = prod_{j < nroots} (x - alpha^(fcr + j))`` under ``prim_poly`` (None: the default of that degree), as an int64 array of
    ``nroots + 1`` field elements in tuple form, lowest degree first (the last one is 1).  Needs ``1 <= nroots < 2^m - 1`` and
    ``0 <= fcr < 2^m - 1``."""
    f = field(m, prim_poly)
    nroots, fcr = whole(nroots, 'nroots', 1, f.n - 1), whole(fcr, 'fcr', 0, f.n - 1)
    g = np.array([1], dtype=np.int64)
    for j in range(nroots):
        root = np.full(len(g), f.exp[(fcr + j) % f.n], dtype=np.int64)
        g = np.concatenate([[0], g]) ^ np.concatenate([f.mul(g, root), [0]])
    return g
