"""Binary BCH codes on MI355X: systematic encoder, bounded-distance decoder (syndromes, Berlekamp-Massey, Chien search) and the
Chase-II soft-decision decoder with Pyndiah's soft output (csrc/bch_chase.hip, equal to tests/chase_model.py bit for bit).

A word is ``n`` bits; bit ``i`` is the coefficient of ``x^(n-1-i)``: the ``k`` message bits first, then the ``n - k`` bits of
``x^(n-k) m(x) mod g(x)``.  The generator (``algcode.bch_genpoly``) and the field are host work; the kernels of csrc/bch.hip receive
the generator and the field tables as data and equal the NumPy model tests/bch_model.py byte for byte.
"""
import ctypes

import numpy as np

from commpy_amd import _lib
from commpy_amd._results import outputs, returned
from commpy_amd.channelcoding._algebraic import field_degree, rows
from commpy_amd.channelcoding.algcode import bch_genpoly
from commpy_amd.channelcoding.gfields import field, whole

__all__ = ['BCHCode', 'bch_encode', 'bch_decode', 'chase_decode']

BCH_MAX_T = 32                                    # csrc/bch_dev.h
WANT = ('bits', 'codeword', 'errors')
CHASE_WANT = ('bits', 'codeword', 'extrinsic', 'metric', 'candidates')
CHASE_MAX_P = 8                                   # csrc/bch_chase.hip


class BCHCode:
    """The narrow-sense binary BCH code of length ``n`` that corrects ``t`` errors over GF(2^m): primitive for ``n = 2^m - 1``,
    shortened below.  ``m`` defaults to the smallest degree with ``2^m - 1 >= n`` (at least 3), ``prim_poly`` to the default
    primitive polynomial of that degree (DVB-S2's GF(2^14) uses 16427).  Limits: 3 <= m <= 14, 1 <= t <= 32,
    deg g < n <= 2^m - 1.  Attributes: ``n, k, t, m, prim_poly, genpoly`` (a Python int, bit i = coefficient of x^i)."""

    def __init__(self, n, t, m=None, prim_poly=None):
        self.n = n = whole(n, 'n', 2)
        self.t = t = whole(t, 't', 1, BCH_MAX_T)
        self.m = m = field_degree(n, m)
        self.prim_poly = field(m, prim_poly).prim_poly
        self.genpoly = bch_genpoly(m, t, self.prim_poly)
        deg = self.genpoly.bit_length() - 1
        if deg >= n:
            raise ValueError('the generator of t = %d over GF(2^%d) has degree %d, need less than n = %d' % (t, m, deg, n))
        self.k = n - deg

        def create():
            h = ctypes.c_void_p()
            bits = np.array([(self.genpoly >> i) & 1 for i in range(deg + 1)], dtype=np.uint8)
            _lib.check(_lib.load().cpx_bch_create(m, self.prim_poly, n, t, _lib.ptr(bits), deg, ctypes.byref(h)))
            return h
        self._handles = _lib.DeviceHandles(create, 'cpx_bch_destroy')

    def _device_handle(self):
        return self._handles.get()


def _code(code):
    if not isinstance(code, BCHCode):
        raise ValueError('code must be a BCHCode')
    return code


def check_want(want):
    """``want`` as a tuple of names out of 'bits', 'codeword', 'errors'."""
    return _lib.wanted(want, WANT)


def shapes(B, code):
    return {'bits': ((B, code.k), np.uint8), 'codeword': ((B, code.n), np.uint8), 'errors': ((B,), np.int32)}


def chase_shapes(rows, k, span):
    """The Chase decoder's results for words nested as ``rows`` (``(B,)``, on the device ``(B, J)``); 'codeword' and 'extrinsic' lie as
    the input does, ``span``: ``(B, n)``, on the device the extent that the strides cover."""
    return {'bits': (rows + (k,), np.uint8), 'codeword': (span, np.uint8), 'extrinsic': (span, np.float64), 'metric': (rows, np.float64),
            'candidates': (rows, np.int32)}


def _bit_rows(bits, name, width):
    return rows(bits, name, width, np.uint8, 'biu', 'integers 0 / 1', 'bits', 1, '0 / 1')


def bch_encode(message_bits, code):
    """``message_bits [B, k]`` (or 1-D ``[k]``) in 0 / 1 -> code words ``[B, n]`` (``[n]``) uint8, systematic: the message, then
    the parity bits."""
    code = _code(code)
    msg, one = _bit_rows(message_bits, 'message_bits', code.k)
    out = np.zeros((msg.shape[0], code.n), dtype=np.uint8)
    if msg.shape[0]:
        _lib.check(_lib.load().cpx_bch_encode(code._device_handle(), _lib.ptr(msg), msg.shape[0], _lib.ptr(out)))
    return out[0] if one else out


def bch_decode(bits, code, want=('bits',)):
    """Bounded-distance decoding of the hard decisions ``bits [B, n]`` (or 1-D ``[n]``) in 0 / 1.  ``want`` names the results; they
    are returned in the order listed here (a single result for one name):

    ``'bits'`` message bits ``[B, k]`` uint8; ``'codeword'`` ``[B, n]`` uint8; ``'errors'`` ``[B]`` int32, the number of corrected
    bits, -1 after a decoding failure.

    The syndromes ``S_1 .. S_2t`` all zero: accepted with 0 errors.  Otherwise Berlekamp-Massey gives the locator ``sigma`` of length
    ``L``; it is a failure if ``L > t``, if the coefficient of ``x^L`` is zero, or if ``sigma`` has not exactly ``L`` roots among the
    inverse locators of the positions ``0 .. n - 1`` (for a shortened code a root in the shortened-away positions).  After a failure
    ``'bits'`` and ``'codeword'`` hold the received word unchanged."""
    code = _code(code)
    want = check_want(want)
    hard, one = _bit_rows(bits, 'bits', code.n)
    B = hard.shape[0]
    res, p = outputs(want, shapes(B, code))
    if B:
        _lib.check(_lib.load().cpx_bch_decode(code._device_handle(), _lib.ptr(hard), B, p('bits'), p('codeword'), p('errors')))
    return returned(res, one)


def chase_args(code, p, beta, alpha, want):
    """The scalar arguments of the Chase decoder, checked: ``(code, p, beta, alpha, want)``."""
    code = _code(code)
    p = whole(p, 'p', 1, min(CHASE_MAX_P, code.n))
    for name, v in (('beta', beta), ('alpha', alpha)):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v):
            raise ValueError('%s = %r, need a finite number' % (name, v))
    if beta < 0:
        raise ValueError('beta = %r, need >= 0' % (beta,))
    return code, p, float(beta), float(alpha), _lib.wanted(want, CHASE_WANT)


def _llr_rows(llr, name, width):
    return rows(llr, name, width, np.float64, 'iuf', 'real numbers', 'values')


def chase_decode(llr, code, p, beta, prior=None, alpha=1.0, want=('bits',)):
    """Chase-II soft-decision decoding of ``llr [B, n]`` (or 1-D ``[n]``) float64, positive = bit 0, with Pyndiah's soft output.
    Per word: ``x = llr`` (``llr + alpha * prior`` with ``prior [B, n]``); the ``p`` least reliable positions by ``(|x_i|, i)``
    (``1 <= p <= min(8, n)``); each of the ``2^p`` test patterns over them is decoded by the rule of ``bch_decode``; the decision is
    the candidate code word of least metric (the sum of ``|x_i|`` where it differs from the hard decisions; ties go to the lowest
    pattern).  ``want`` names the results, returned in the order listed here (a single result for one name):

    ``'bits'`` ``[B, k]`` uint8; ``'codeword'`` ``[B, n]`` uint8, the decision; ``'extrinsic'`` ``[B, n]`` float64:
    ``s_i (M_C - M_D) - x_i`` with ``s_i = +-1`` the decision's sign and ``M_C`` the least metric of the candidates that differ from
    the decision at ``i``, ``s_i beta`` where no candidate does (``beta >= 0`` in LLR units) -- ``x + extrinsic`` is the max-log
    a-posteriori LLR over the candidate list; ``'metric'`` ``[B]`` float64; ``'candidates'`` ``[B]`` int32, the number of test
    patterns that decoded.

    Without a candidate the hard decisions are returned with metric ``+inf`` and extrinsic 0.  A word that holds a NaN or an
    infinity is rejected on its own: the same, with ``candidates = -1`` (a NaN counts as bit 0)."""
    code, p, beta, alpha, want = chase_args(code, p, beta, alpha, want)
    soft, one = _llr_rows(llr, 'llr', code.n)
    pri = None
    if prior is not None:
        pri, _ = _llr_rows(prior, 'prior', code.n)
        if pri.shape != soft.shape or (np.ndim(prior) == 1) != one:
            raise ValueError('prior has shape %s, need that of llr' % (np.shape(prior),))
    B = soft.shape[0]
    res, q = outputs(want, chase_shapes((B,), code.k, (B, code.n)))
    if B:
        _lib.check(_lib.load().cpx_chase_bch(code._device_handle(), _lib.ptr(soft), None if pri is None else _lib.ptr(pri), alpha, beta, p, B,
                                             q('bits'), q('codeword'), q('extrinsic'), q('metric'), q('candidates')))
    return returned(res, one)
