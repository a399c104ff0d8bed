"""Binary Galois fields GF(2^m), 1 <= m <= 16, on the host: the names and signatures of the reference's ``gfields`` module, computed
from one pair of antilog / log tables per (m, primitive polynomial) instead of a search per element.

An element is an integer whose bits are the coefficients of its polynomial ("tuple form"); its "power form" is the exponent ``e`` of
``alpha^e`` with ``alpha = x``.  The reference's conventions are kept: the power form of 0 is 0, the minimal polynomial of 0 is ``x``
(the integer 2), ``order`` returns floats and ``cosets`` groups the elements *given*, in the order given.
"""
import functools

import numpy as np

__all__ = ['GF', 'polydivide', 'polymultiply', 'poly_to_string']

# x^m + ... as integers, index m: the reference's table
DEFAULT_PRIM_POLY = (None, 3, 7, 11, 19, 37, 67, 137, 285, 529, 1033, 2053, 4179, 8219, 17475, 32771, 69643)
MAX_M = len(DEFAULT_PRIM_POLY) - 1


class Field:
    """The tables of GF(2^m) under ``prim_poly``: ``n = 2^m - 1``, ``exp [2 n]`` with ``exp[e] = alpha^(e mod n)`` (twice the period,
    so that the sum of two logarithms indexes it directly), ``log [2^m]`` with ``log[0] = 0`` by the reference's convention."""

    def __init__(self, m, prim_poly):
        self.m, self.prim_poly, self.n = m, prim_poly, (1 << m) - 1
        exp = np.zeros(2 * self.n, dtype=np.int64)
        log = np.zeros(self.n + 1, dtype=np.int64)
        v = 1
        for e in range(self.n):
            if e and v == 1:
                raise ValueError('prim_poly = %d is not primitive: x has order %d in GF(2^%d), not %d' % (prim_poly, e, m, self.n))
            exp[e] = exp[e + self.n] = v
            log[v] = e
            v <<= 1
            if v >> m:
                v ^= prim_poly
        if v != 1:
            raise ValueError('prim_poly = %d is not primitive: x does not return to 1 after %d steps' % (prim_poly, self.n))
        self.exp, self.log = exp, log

    def mul(self, a, b):
        """Element-wise product of two arrays of field elements."""
        return np.where((a == 0) | (b == 0), 0, self.exp[self.log[a] + self.log[b]])

    def coset(self, e):
        """The cyclotomic coset of the exponent ``e``: ``[e, 2 e, 4 e, ...] mod n`` until it closes."""
        out, v = [], e % self.n if self.n > 1 else 0
        while v not in out:
            out.append(v)
            v = 2 * v % self.n
        return out

    def minpoly(self, e):
        """The minimal polynomial of ``alpha^e`` as an integer: the product of ``X + alpha^j`` over the coset of ``e``."""
        poly = np.array([1], dtype=np.int64)                  # coefficients in the field, lowest degree first
        for j in self.coset(e):
            root = np.full(len(poly), self.exp[j], dtype=np.int64)
            poly = np.concatenate([[0], poly]) ^ np.concatenate([self.mul(poly, root), [0]])
        if poly.max() > 1:
            raise AssertionError('minimal polynomial with a coefficient outside GF(2)')
        return sum(int(c) << i for i, c in enumerate(poly))


def whole(v, name, lo, hi=None):
    """``v`` as an int; ValueError unless it is an integer (no bool) in lo .. hi."""
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or v < lo or (hi is not None and v > hi):
        raise ValueError('%s = %r, need an integer %s' % (name, v, '>= %d' % lo if hi is None else 'in %d .. %d' % (lo, hi)))
    return int(v)


@functools.lru_cache(maxsize=None)
def _field(m, prim_poly):
    return Field(m, prim_poly)


def field(m, prim_poly=None):
    """The cached ``Field`` of GF(2^m); ``prim_poly`` None: the default table.  ValueError for m outside 1 .. 16, a polynomial whose
    degree is not m, or one under which x does not generate the multiplicative group."""
    m = whole(m, 'm', 1, MAX_M)
    p = DEFAULT_PRIM_POLY[m] if prim_poly is None else whole(prim_poly, 'prim_poly', 2)
    if p.bit_length() - 1 != m:
        raise ValueError('prim_poly = %d has degree %d, need %d' % (p, p.bit_length() - 1, m))
    return _field(m, p)


class GF:
    """Elements of GF(2^m): ``x`` one int or an array of them, ``m`` the degree; ``prim_poly`` (a keyword the reference lacks)
    replaces the default primitive polynomial of that degree.  ``elements``, ``m`` and ``prim_poly`` are attributes."""

    def __init__(self, x, m, prim_poly=None):
        self._field = field(m, prim_poly)
        self.m, self.prim_poly = self._field.m, self._field.prim_poly
        if isinstance(x, (int, np.integer)) and not isinstance(x, (bool, np.bool_)):
            if not 0 <= x <= self._field.n:
                raise ValueError('x = %d is no element of GF(2^%d)' % (x, self.m))
            self.elements = np.array([int(x)])
        else:
            a = np.asarray(x)
            if a.ndim != 1 or a.size == 0 or a.dtype.kind not in 'iuf':
                raise ValueError('x must be an int or a non-empty 1-D array of numbers')
            self.elements = a.astype(int)

    def _like(self, elements):
        return GF(np.asarray(elements).astype(int), self.m, self.prim_poly)

    def _members(self):
        e = self.elements
        if e.min() < 0 or e.max() > self._field.n:
            raise ValueError('an element lies outside GF(2^%d)' % self.m)
        return e

    def _same_length(self, other):
        if not isinstance(other, GF) or (other.m, other.prim_poly) != (self.m, self.prim_poly):
            raise ValueError('the operands must be GF objects of one field')
        if len(other.elements) != len(self.elements):
            raise ValueError('the operands must have the same number of elements')
        return other

    def __add__(self, other):
        return self._like(self.elements ^ self._same_length(other).elements)

    def __mul__(self, other):
        return self._like(self._field.mul(self._members(), self._same_length(other)._members()))

    def power_to_tuple(self):
        """The elements read as exponents ``e``: ``alpha^e`` in tuple form."""
        return self._like(self._field.exp[self.elements % self._field.n] if self._field.n > 1 else np.ones_like(self.elements))

    def tuple_to_power(self):
        """The exponent of every element; 0 for the element 0, as for 1 (the reference's convention)."""
        return self._like(self._field.log[self._members()])

    def order(self):
        """The multiplicative order of every element, as floats (1.0 for 0)."""
        n = self._field.n
        return n / np.gcd(self._field.log[self._members()], n).astype(float)

    def cosets(self):
        """The given elements grouped by cyclotomic coset of their power form, as a list of ``GF`` objects.  Elements are visited in
        the order given; one that no earlier group took opens a group and takes every later, still free element whose exponent is
        another member of its coset -- so 0 and 1, both of exponent 0, form a group each, as in the reference."""
        f = self._field
        power = f.log[self._members()]
        group = np.zeros(len(power), dtype=np.int64)
        groups = 0
        for i in range(len(power)):
            if group[i]:
                continue
            groups += 1
            others = f.coset(int(power[i]))[1:]
            group[(group == 0) & np.isin(power, others)] = groups
            group[i] = groups
        return [self._like(self.elements[group == g]) for g in range(1, groups + 1)]

    def minpolys(self):
        """The minimal polynomial over GF(2) of every element, as integers (``x`` = 2 for the element 0)."""
        f = self._field
        known = {}
        out = np.zeros(len(self.elements), dtype=int)
        for i, v in enumerate(self._members()):
            if v == 0:
                out[i] = 2
                continue
            leader = min(f.coset(int(f.log[v])))
            if leader not in known:
                known[leader] = f.minpoly(leader)
            out[i] = known[leader]
        return out


def polydivide(x, y):
    """The remainder of the binary polynomial ``x`` divided by ``y`` (integers, bit i = coefficient of x^i)."""
    x, y = int(x), int(y)
    if x < 0 or y <= 0:
        raise ValueError('polydivide needs x >= 0 and y > 0')
    width = y.bit_length()
    while x.bit_length() >= width:
        x ^= y << (x.bit_length() - width)
    return x


def clmul(x, y):
    """The product of two binary polynomials (carry-less multiplication of Python ints)."""
    out = 0
    while y:
        low = y & -y
        out ^= x * low
        y ^= low
    return out


def polymultiply(x, y, m, prim_poly):
    """The product of the elements ``x`` and ``y`` of GF(2^m) under ``prim_poly``."""
    x, y = int(x), int(y)
    if x < 0 or y < 0:
        raise ValueError('polymultiply needs x, y >= 0')
    return polydivide(clmul(x, y), prim_poly)


def poly_to_string(x):
    """``'x^0 + x^1 + x^4 '`` for 19: the terms in rising degree, with the reference's trailing blank; ``''`` for 0."""
    x = int(x)
    terms = ['x^%d' % i for i in range(x.bit_length()) if (x >> i) & 1]
    return ' + '.join(terms) + ' ' if terms else ''
