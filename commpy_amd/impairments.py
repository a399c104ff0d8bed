"""Channel impairments (the reference's ``commpy/impairments.py``): a carrier frequency offset, applied on the GPU.

``add_frequency_offset(waveform, Fs, delta_f)`` multiplies sample k by ``exp(1j 2 pi (delta_f / Fs) k)``.  The host computes
the phase step ``(2 pi) (delta_f / Fs)`` in the reference's operation order; the kernel (csrc/fir.hip) forms ``step * k``
with one rounding and takes a full-range float64 sine and cosine of it.  Real waveforms give complex output, as in the
reference.  ``add_frequency_offset_batch`` takes ``[B, n]`` rows with one ``delta_f`` or one per row.  No CPU fallback.
"""
import numpy as np

from commpy_amd import _lib

__all__ = ['add_frequency_offset', 'add_frequency_offset_batch']


def _steps(Fs, delta_f, B):
    d = np.asarray(delta_f, dtype=np.float64)
    if d.ndim > 1 or (d.ndim == 1 and d.size != B):
        raise ValueError('delta_f must be a scalar or one value per row (%d), got shape %r' % (B, d.shape))
    fs = np.float64(Fs)
    if np.ndim(Fs) != 0:
        raise ValueError('Fs must be a scalar')
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.ascontiguousarray(np.atleast_1d((2 * np.pi) * (d / fs))), int(d.ndim == 1)


def add_frequency_offset_batch(waveforms, Fs, delta_f):
    """``waveforms [B, n]`` -> complex128 ``[B, n]``, row b shifted by ``delta_f`` (scalar) or ``delta_f[b]``."""
    x = np.asarray(waveforms)
    if x.ndim != 2:
        raise ValueError('waveforms must be [B, n], got %d dimensions' % x.ndim)
    B, n = x.shape
    step, batched = _steps(Fs, delta_f, B)
    out = np.zeros((B, n), dtype=np.complex128)
    if out.size:
        x = np.ascontiguousarray(x, dtype=np.complex128)
        _lib.check(_lib.load().cpx_freq_offset(_lib.ptr(x), B, n, _lib.ptr(step), batched, _lib.ptr(out)))
    return out


def add_frequency_offset(waveform, Fs, delta_f):
    """``waveform * exp(1j 2 pi (delta_f / Fs) arange(len(waveform)))`` (impairments.py:20) for a 1-D waveform."""
    x = np.asarray(waveform)
    if x.ndim != 1:
        raise ValueError('waveform must be 1-D, got %d dimensions' % x.ndim)
    if np.ndim(delta_f) != 0:
        raise ValueError('delta_f must be a scalar for a 1-D waveform')
    return add_frequency_offset_batch(x[None], Fs, delta_f)[0]
