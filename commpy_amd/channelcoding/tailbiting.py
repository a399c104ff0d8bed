"""Tail-biting convolutional codes on MI355X: encoder and wrap-around Viterbi decoder (csrc/tbcc.hip).

A tail-biting block is ``T`` trellis steps without a tail: the encoder starts in the state in which it ends, so that the code word is
a closed path round the trellis (LTE's control and broadcast channels, 802.16).  The decoder does not know that state; it runs the
trellis round the block several times and looks for a survivor that closes.  The kernels equal the NumPy model tests/tbcc_model.py
bit for bit, the ``'metric'`` included.

Limits (csrc/tbcc.hip): the number of states is a power of two from 2 to 64; ``k <= 2`` and ``n <= 6``; ``T >= 1`` and
``T * k <= 8192`` (the block's decisions stay in LDS); ``1 <= max_wraps <= 32``.
"""
import numpy as np

from commpy_amd import _lib
from commpy_amd._results import outputs, returned
from commpy_amd.channelcoding.convcode import _VIT_TYPES, device_trellis

__all__ = ['tailbiting_encode', 'tailbiting_decode']

TBCC_MAX_STATES, TBCC_MAX_K, TBCC_MAX_N, TBCC_MAX_BITS, TBCC_MAX_WRAPS = 64, 2, 6, 8192, 32    # csrc/tbcc.hip
WANT = ('bits', 'wraps', 'tailbiting', 'metric')


def check_want(want):
    """``want`` as a tuple of names out of 'bits', 'wraps', 'tailbiting', 'metric'."""
    return _lib.wanted(want, WANT)


def shapes(B, T, k):
    return {'bits': ((B, T * k), np.uint8), 'wraps': ((B,), np.int32), 'tailbiting': ((B,), np.uint8), 'metric': ((B,), np.float64)}


def check_trellis(trellis):
    """``(k, n)`` of a trellis within the kernels' limits (ValueError naming the limit otherwise; host only)."""
    k, n, S = int(trellis.k), int(trellis.n), int(trellis.number_states)
    if S < 2 or S > TBCC_MAX_STATES or S & (S - 1):
        raise ValueError('the trellis has %d states, the limit is a power of two from 2 to %d' % (S, TBCC_MAX_STATES))
    if k < 1 or k > TBCC_MAX_K or n < 1 or n > TBCC_MAX_N:
        raise ValueError('k = %d, n = %d: the limits are k <= %d and n <= %d' % (k, n, TBCC_MAX_K, TBCC_MAX_N))
    return k, n


def check_steps(width, per_step, name):
    """The number of trellis steps ``T`` of rows of ``width`` values, ``per_step`` of them per step."""
    if width < per_step or width % per_step:
        raise ValueError('%s has %d values per row, need a positive multiple of %d (T >= 1)' % (name, width, per_step))
    return width // per_step


def check_block(T, k):
    if T < 1 or T * k > TBCC_MAX_BITS:
        raise ValueError('T = %d steps: the limits are T >= 1 and T * k <= %d' % (T, TBCC_MAX_BITS))
    return T


def check_max_wraps(max_wraps):
    if isinstance(max_wraps, (bool, np.bool_)) or not isinstance(max_wraps, (int, np.integer)) or not 1 <= max_wraps <= TBCC_MAX_WRAPS:
        raise ValueError('max_wraps = %r: the limit is an integer from 1 to %d' % (max_wraps, TBCC_MAX_WRAPS))
    return int(max_wraps)


def check_type(decoding_type):
    if decoding_type not in _VIT_TYPES:
        raise ValueError('The available decoding types are "hard", "soft" and "unquantized')
    return _VIT_TYPES[decoding_type]


def _rows(a, name):
    a = np.asarray(a)
    if a.ndim not in (1, 2):
        raise ValueError('%s must be 1-D or 2-D, got %d dimensions' % (name, a.ndim))
    return np.atleast_2d(a), a.ndim == 1


def tailbiting_encode(message_bits, trellis):
    """``message_bits [B, T*k]`` (or 1-D ``[T*k]``), integers 0 / 1 -> code words ``[B, T*n]`` (``[T*n]``) uint8.

    The encoder walks the message once from state 0, starts again in the state it ended in, and emits that second walk.
    ``ValueError`` if the second walk does not end where it began -- a recursive trellis, or a message shorter than the encoder
    memory -- and for any value other than 0 or 1.  ``trellis`` is a ``Trellis`` or any duck-typed trellis; limits: see the module."""
    k, n = check_trellis(trellis)
    msg, one = _rows(message_bits, 'message_bits')
    if msg.dtype.kind not in 'biu':
        raise ValueError('message_bits must hold integers, got dtype %s' % msg.dtype)
    T = check_block(check_steps(msg.shape[1], k, 'message_bits'), k)
    if msg.size and (msg.min() < 0 or msg.max() > 1):
        raise ValueError('message_bits must hold 0 / 1')
    msg = np.ascontiguousarray(msg, dtype=np.uint8)
    B = msg.shape[0]
    out = np.zeros((B, T * n), dtype=np.uint8)
    closed = np.ones(B, dtype=np.uint8)
    if B:
        _lib.check(_lib.load().cpx_tbcc_encode(device_trellis(trellis), _lib.ptr(msg), B, T, _lib.ptr(out), _lib.ptr(closed)))
    if not closed.all():
        raise ValueError('row %d does not tail-bite: started in the state the message leaves the encoder in, the encoder ends in '
                         'another one (a recursive trellis, or a message shorter than the encoder memory)' % int(np.argmin(closed)))
    return out[0] if one else out


def tailbiting_decode(coded, trellis, decoding_type='hard', max_wraps=4, want=('bits',)):
    """Wrap-around Viterbi decoding of tail-biting blocks ``coded [B, T*n]`` (or 1-D ``[T*n]``) float64, with the meaning
    ``viterbi_decode`` gives them per ``decoding_type`` ('hard' 0 / 1, 'soft' LLRs log P1/P0 clipped to +-500, 'unquantized' +-1
    levels).  ``want`` names the results; they are returned in the order listed here (a single result for one name):

    ``'bits'`` ``[B, T*k]`` uint8; ``'wraps'`` ``[B]`` int32, the number of trips round the trellis that were run, 0 = the row was
    rejected; ``'tailbiting'`` ``[B]`` uint8, 1 = the returned path starts and ends in the same state; ``'metric'`` ``[B]`` float64,
    the returned path's own metric.

    The rule (float64, sums in the order written): ``bm_t[c]`` is the sum over the ``n`` bits, MSB first and starting from 0.0, of
    ``viterbi_decode``'s per-bit metric for step ``t``; ``M[s] = 0`` for every state before the first trip.  On trip
    ``w = 1 .. max_wraps``: (1) ``M_start = M``.  (2) Steps ``t = 0 .. T-1``: every state takes its candidates in ``np.where`` order,
    ``cand_j = M[pred_j] + bm_t[code_j]``, and keeps the first minimum (a later candidate replaces it only if strictly smaller);
    metrics run on across trips without rescaling.  (3) ``origin[s]`` is the state in which the survivor ending in ``s`` began this
    trip, ``net[s] = M[s] - M_start[origin[s]]``.  (4) ``s*`` is the first state of minimum ``M``; if ``origin[s*] == s*`` that path is
    returned with ``wraps = w``, ``tailbiting = 1``, ``metric = net[s*]``.  (5) Otherwise ``c``, the first state of minimum ``net``
    among the states with ``origin[s] == s``, replaces the remembered candidate only if its ``net`` is strictly smaller; a remembered
    candidate keeps its bits.  (6) After the last trip the remembered candidate is returned with ``wraps = max_wraps``,
    ``tailbiting = 1``; if there is none, the path of the last ``s*`` with ``tailbiting = 0`` and ``metric = net[s*]``.

    A row that holds a NaN, or +-inf under 'hard' / 'unquantized', is rejected and not decoded: zero bits, ``wraps = 0``,
    ``tailbiting = 0``, ``metric = NaN``; no other row is affected.

    Limits, each refused with a ``ValueError`` before any device call: the number of states is a power of two from 2 to 64;
    ``k <= 2`` and ``n <= 6``; ``T >= 1`` and ``T * k <= 8192`` (the block's decisions stay in LDS); ``1 <= max_wraps <= 32``."""
    k, n = check_trellis(trellis)
    vtype = check_type(decoding_type)
    max_wraps = check_max_wraps(max_wraps)
    want = check_want(want)
    rows, one = _rows(coded, 'coded')
    T = check_block(check_steps(rows.shape[1], n, 'coded'), k)
    x = _lib.as_f64(rows)
    B = x.shape[0]
    res, p = outputs(want, shapes(B, T, k))
    if B:
        _lib.check(_lib.load().cpx_tbcc_decode(device_trellis(trellis), _lib.ptr(x), B, T, vtype, max_wraps, *map(p, WANT)))
    return returned(res, one)
