"""Reed-Solomon codes on MI355X: systematic encoder and bounded-distance errors-and-erasures decoder (syndromes, erasure locator,
Berlekamp-Massey, Chien search, Forney's values).

A word is ``n`` symbols of GF(2^m) in the tuple form of ``gfields.GF``; symbol ``i`` is the coefficient of ``x^(n-1-i)``: the ``k``
message symbols first, then the ``n - k`` symbols of ``x^(n-k) m(x) mod g(x)``.  The generator (``algcode.rs_genpoly``) and the field
are host work; the kernels of csrc/rs.hip receive the generator and the field tables as data and equal the NumPy model
tests/rs_model.py symbol for symbol.
"""
import ctypes

import numpy as np

from commpy_amd import _lib
from commpy_amd._results import outputs, returned
from commpy_amd.channelcoding._algebraic import field_degree, rows
from commpy_amd.channelcoding.algcode import rs_genpoly
from commpy_amd.channelcoding.gfields import field, whole

__all__ = ['RSCode', 'rs_encode', 'rs_decode']

RS_MAX_NROOTS = 63                                # csrc/rs.hip
WANT = ('symbols', 'codeword', 'errors')


class RSCode:
    """The Reed-Solomon code of length ``n`` and dimension ``k`` over GF(2^m) with the generator
    ``g(x) = prod_{j < n-k} (x - alpha^(fcr+j))`` (``fcr = 1``: narrow sense): primitive for ``n = 2^m - 1``, shortened below (the
    highest degrees are dropped).  ``m`` defaults to the smallest degree with ``2^m - 1 >= n`` (at least 3), ``prim_poly`` to the
    default primitive polynomial of that degree.  Limits: 3 <= m <= 14, 1 <= k, 1 <= n - k <= 63, n <= 2^m - 1,
    0 <= fcr < 2^m - 1.  Attributes: ``n, k, m, nroots (= n - k), t (= nroots // 2), fcr, prim_poly, genpoly`` (int64
    ``[nroots + 1]``, lowest degree first, monic)."""

    def __init__(self, n, k, m=None, prim_poly=None, fcr=1):
        self.n = n = whole(n, 'n', 2)
        self.k = k = whole(k, 'k', 1)
        self.m = m = field_degree(n, m)
        self.nroots = whole(n - k, 'n - k', 1, RS_MAX_NROOTS)
        self.t = self.nroots // 2
        self.fcr = fcr = whole(fcr, 'fcr', 0, (1 << m) - 2)
        self.prim_poly = field(m, prim_poly).prim_poly
        self.genpoly = rs_genpoly(m, self.nroots, fcr, self.prim_poly)

        def create():
            h = ctypes.c_void_p()
            g = self.genpoly.astype(np.uint16)
            _lib.check(_lib.load().cpx_rs_create(m, self.prim_poly, n, k, fcr, _lib.ptr(g), ctypes.byref(h)))
            return h
        self._handles = _lib.DeviceHandles(create, 'cpx_rs_destroy')

    def _device_handle(self):
        return self._handles.get()


def _code(code):
    if not isinstance(code, RSCode):
        raise ValueError('code must be an RSCode')
    return code


def check_want(want):
    """``want`` as a tuple of names out of 'symbols', 'codeword', 'errors'."""
    return _lib.wanted(want, WANT)


def shapes(B, code):
    return {'symbols': ((B, code.k), np.uint16), 'codeword': ((B, code.n), np.uint16), 'errors': ((B,), np.int32)}


def _symbol_rows(symbols, name, width, m):
    top = (1 << m) - 1
    return rows(symbols, name, width, np.uint16, 'iu', 'integers', 'symbols', top, 'elements of GF(2^%d): 0 .. %d' % (m, top))


def _flag_rows(erasures, shape):
    a = np.asarray(erasures)
    if a.dtype.kind not in 'biu':
        raise ValueError('erasures must be boolean or integer, got dtype %s' % a.dtype)
    if a.shape != shape:
        raise ValueError('erasures has shape %s, need the symbols\' shape %s' % (a.shape, shape))
    return np.ascontiguousarray(np.atleast_2d(a != 0), dtype=np.uint8)


def rs_encode(message_symbols, code):
    """``message_symbols [B, k]`` (or 1-D ``[k]``), integers in ``0 .. 2^m - 1`` -> code words ``[B, n]`` (``[n]``) uint16,
    systematic: the message, then the parity symbols."""
    code = _code(code)
    msg, one = _symbol_rows(message_symbols, 'message_symbols', code.k, code.m)
    out = np.zeros((msg.shape[0], code.n), dtype=np.uint16)
    if msg.shape[0]:
        _lib.check(_lib.load().cpx_rs_encode(code._device_handle(), _lib.ptr(msg), msg.shape[0], _lib.ptr(out)))
    return out[0] if one else out


def rs_decode(symbols, code, erasures=None, want=('symbols',)):
    """Bounded-distance errors-and-erasures decoding of the received ``symbols [B, n]`` (or 1-D ``[n]``), integers in
    ``0 .. 2^m - 1``.  ``erasures``: a boolean or integer array of the same shape, non-zero = the position is flagged as unreliable
    (None: no flags).  ``want`` names the results; they are returned in the order listed here (a single result for one name):

    ``'symbols'`` message symbols ``[B, k]`` uint16; ``'codeword'`` ``[B, n]`` uint16; ``'errors'`` ``[B]`` int32, the number of
    corrected unflagged positions, -1 after a decoding failure.

    With ``r = n - k`` and ``f`` flagged positions in a word: ``f > r`` is a failure.  The syndromes ``S_j = R(alpha^(fcr+j))``,
    ``j < r``, are taken from the symbols as given (a flagged position keeps its value); all zero: accepted with 0 errors.  Otherwise
    Berlekamp-Massey, started from the erasure locator ``Gamma = prod (1 - alpha^d x)`` at ``rho = f`` with ``L = f`` (the length
    changes when ``2 L <= rho + f``, to ``rho + 1 - L + f``), gives ``Lambda`` of length ``L``; it is a failure if
    ``2 (L - f) + f > r``, if the coefficient of ``x^L`` is zero, or if ``Lambda`` has not exactly ``L`` roots among the inverse
    locators of the positions ``0 .. n - 1`` (for a shortened code a root in the shortened-away positions).  Otherwise
    ``Omega = S Lambda mod x^r`` and ``Y = alpha^(d (1 - fcr)) Omega(alpha^-d) / Lambda'(alpha^-d)`` is XORed into the symbol of
    degree ``d`` at every root (``Y`` may be zero at a flagged position); ``errors = L - f``.  After a failure ``'symbols'`` and
    ``'codeword'`` hold the received word unchanged."""
    code = _code(code)
    want = check_want(want)
    word, one = _symbol_rows(symbols, 'symbols', code.n, code.m)
    flags = None if erasures is None else _flag_rows(erasures, np.shape(symbols))
    B = word.shape[0]
    res, p = outputs(want, shapes(B, code))
    if B:
        _lib.check(_lib.load().cpx_rs_decode(code._device_handle(), _lib.ptr(word), None if flags is None else _lib.ptr(flags), B,
                                             p('symbols'), p('codeword'), p('errors')))
    return returned(res, one)
