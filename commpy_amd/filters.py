"""Pulse-shaping filters (the reference's ``commpy/filters.py``) and the GPU filtering that uses them (csrc/fir.hip).

``rcosfilter``, ``rrcosfilter``, ``gaussianfilter`` and ``rectfilter`` keep the reference's signatures and return
``(time_idx, h)``; they are small host functions, evaluated array-wise.  The time axis is ``(arange(N) - N/2) / Fs``, so an
odd ``N`` never samples t = 0, and the removable singularities are recognised by exact floating-point equality
(``t == Ts/(2 alpha)`` for RC, ``t == Ts/(4 alpha)`` for RRC), every other sample taking the general formula -- both as in
the reference.

The reference leaves filtering to ``numpy.convolve`` over a zero-stuffed stream.  Here it runs on the GPU, complex128 with
float64 arithmetic (the precision switch does not apply):

* ``pulse_shape(symbols, taps, sps)`` = ``numpy.convolve(upsample(symbols, sps), taps)`` as a polyphase interpolator;
* ``matched_filter(y, taps, sps=1, offset=0)`` = ``numpy.convolve(y, taps)[offset::sps]``, computing only the kept samples;
* ``pulse_shape_batch`` / ``matched_filter_batch`` do the same for the B rows of a 2-D array.

Taps may be real or complex (at most ``FIR_MAX_TAPS``) and must be finite.  There is no CPU fallback: the filtering functions
raise when the library or the GPU is missing; their arguments are checked first, without a device.
"""
import ctypes
import numbers

import numpy as np

from commpy_amd import _lib

__all__ = ['rcosfilter', 'rrcosfilter', 'gaussianfilter', 'rectfilter', 'pulse_shape', 'pulse_shape_batch',
           'matched_filter', 'matched_filter_batch', 'FIR_MAX_TAPS']

FIR_MAX_TAPS = 8192


def _time_axis(N, Fs):
    return (np.arange(N) - N / 2) * (1 / float(Fs))


def rcosfilter(N, alpha, Ts, Fs):
    """Raised-cosine impulse response of N samples: ``(time_idx, h_rc)`` (filters.py:22)."""
    t = _time_axis(N, Fs)
    with np.errstate(divide='ignore', invalid='ignore'):
        arg = np.pi * t / Ts
        sinc = np.sin(arg) / arg
        twice = (2 * alpha * t) / Ts
        h = sinc * (np.cos(np.pi * alpha * t / Ts) / (1 - twice * twice))
        if alpha != 0:
            h = np.where(np.abs(t) == Ts / (2 * alpha), (np.pi / 4) * sinc, h)
    return t, np.where(t == 0.0, 1.0, h)


def rrcosfilter(N, alpha, Ts, Fs):
    """Root-raised-cosine impulse response of N samples: ``(time_idx, h_rrc)`` (filters.py:67)."""
    t = _time_axis(N, Fs)
    with np.errstate(divide='ignore', invalid='ignore'):
        four = 4 * alpha * t / Ts
        num = np.sin(np.pi * t * (1 - alpha) / Ts) + 4 * alpha * (t / Ts) * np.cos(np.pi * t * (1 + alpha) / Ts)
        h = num / (np.pi * t * (1 - four * four) / Ts)
        if alpha != 0:
            edge = (alpha / np.sqrt(2)) * (((1 + 2 / np.pi) * (np.sin(np.pi / (4 * alpha))))
                                          + ((1 - 2 / np.pi) * (np.cos(np.pi / (4 * alpha)))))
            h = np.where(np.abs(t) == Ts / (4 * alpha), edge, h)
    return t, np.where(t == 0.0, 1.0 - alpha + (4 * alpha / np.pi), h)


def gaussianfilter(N, alpha, Ts, Fs):
    """Gaussian impulse response of N samples: ``(time_idx, h_gaussian)`` (filters.py:115); ``Ts`` is unused, as there."""
    t = _time_axis(N, Fs)
    scaled = np.pi * t / alpha
    return t, (np.sqrt(np.pi) / alpha) * np.exp(-(scaled * scaled))


def rectfilter(N, Ts, Fs):
    """Rectangular impulse response of N samples: ``(time_idx, ones(N))`` (filters.py:149)."""
    return _time_axis(N, Fs), np.ones(N)


# ---- GPU filtering (csrc/fir.hip) ----------------------------------------------------------------------------------------------
def _whole(value, name, least):
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, numbers.Integral):
        raise ValueError('%s must be an integer, got %r' % (name, value))
    if value < least:
        raise ValueError('%s = %d, need at least %d' % (name, value, least))
    return int(value)


def _taps(taps):
    """(contiguous float64 or complex128 taps, is_complex), checked without a device."""
    h = np.asarray(taps)
    if h.ndim != 1:
        raise ValueError('taps must be 1-D, got %d dimensions' % h.ndim)
    if h.size == 0:
        raise ValueError('taps are empty')
    if h.size > FIR_MAX_TAPS:
        raise ValueError('%d taps are above the engine limit of %d' % (h.size, FIR_MAX_TAPS))
    cplx = np.iscomplexobj(h)
    return np.ascontiguousarray(h, dtype=np.complex128 if cplx else np.float64), cplx


def _rows(x, name, ndim):
    x = np.asarray(x)
    if x.ndim != ndim:
        raise ValueError('%s must be %d-D, got %d dimensions' % (name, ndim, x.ndim))
    if x.shape[-1] == 0:
        raise ValueError('%s is empty (numpy.convolve refuses an empty operand)' % name)
    return x


class _FirPlan:
    """The engine's copy of one tap vector, one handle per device."""

    def __init__(self, h, cplx):
        def create():
            p = ctypes.c_void_p()
            _lib.check(_lib.load().cpx_fir_create(_lib.ptr(h), h.size, int(cplx), ctypes.byref(p)))
            return p
        self._h = h                       # keeps the buffer alive for handles created later on other devices
        self._handles = _lib.DeviceHandles(create, 'cpx_fir_destroy')

    def handle(self):
        return self._handles.get()


_fir_plans = {}


def _fir_plan(h, cplx):
    key = (h.tobytes(), cplx)
    plan = _fir_plans.get(key)
    if plan is None:
        if len(_fir_plans) > 64:
            _fir_plans.clear()
        plan = _fir_plans[key] = _FirPlan(h.copy(), cplx)
    return plan


def pulse_shape_batch(symbols, taps, sps):
    """Row b of the result is ``numpy.convolve(upsample(symbols[b], sps), taps)``: ``symbols [B, n]`` -> complex128
    ``[B, n * sps + len(taps) - 1]``.  The zeros between symbols are never formed."""
    h, cplx = _taps(taps)
    sps = _whole(sps, 'sps', 1)
    x = _rows(symbols, 'symbols', 2)
    B, n = x.shape
    out = np.zeros((B, n * sps + h.size - 1), dtype=np.complex128)
    if B:
        x = np.ascontiguousarray(x, dtype=np.complex128)
        _lib.check(_lib.load().cpx_fir_interp(_fir_plan(h, cplx).handle(), _lib.ptr(x), B, n, sps, _lib.ptr(out)))
    return out


def pulse_shape(symbols, taps, sps):
    """``numpy.convolve(upsample(symbols, sps), taps)`` for a 1-D symbol stream."""
    return pulse_shape_batch(_rows(symbols, 'symbols', 1)[None], taps, sps)[0]


def matched_filter_batch(y, taps, sps=1, offset=0):
    """Row b of the result is ``numpy.convolve(y[b], taps)[offset::sps]``: ``y [B, n]`` -> complex128
    ``[B, ceil((n + len(taps) - 1 - offset) / sps)]``, with 0 <= offset < n + len(taps) - 1."""
    h, cplx = _taps(taps)
    sps = _whole(sps, 'sps', 1)
    y = _rows(y, 'y', 2)
    B, n = y.shape
    full = n + h.size - 1
    offset = _whole(offset, 'offset', 0)
    if offset >= full:
        raise ValueError('offset = %d is outside the %d samples of the full convolution' % (offset, full))
    out = np.zeros((B, -(-(full - offset) // sps)), dtype=np.complex128)
    if B:
        y = np.ascontiguousarray(y, dtype=np.complex128)
        _lib.check(_lib.load().cpx_fir_decim(_fir_plan(h, cplx).handle(), _lib.ptr(y), B, n, sps, offset, _lib.ptr(out)))
    return out


def matched_filter(y, taps, sps=1, offset=0):
    """``numpy.convolve(y, taps)[offset::sps]`` for a 1-D waveform."""
    return matched_filter_batch(_rows(y, 'y', 1)[None], taps, sps, offset)[0]
