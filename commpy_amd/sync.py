"""OFDM timing and carrier-frequency-offset synchronisation on the GPU (csrc/sync.hip): the stage between the channel and ``ofdm_rx``.

With ``y [B, nr, n]``, a lag ``D`` and a window ``W`` the engine forms, per row and for every position d < n - D - W + 1,

    P[d] = sum_{i=d}^{d+W-1} sum_r conj(y[r, i]) y[r, i + D]
    E[d] = sum_{i=d}^{d+W-1} 1/2 sum_r (|y[r, i]|^2 + |y[r, i + D]|^2)
    M[d] = |P[d]|^2 / E[d]^2        (0 where E is 0)

``D = W = nfft / 2`` is the Schmidl-Cox search on a preamble of two identical halves (``schmidl_cox_preamble``), ``D = nfft, W = cp_length``
the cyclic-prefix correlator.  ``sync_estimate_batch`` returns the first largest M of each row with the frequency offset read from the
phase of P there, ``sync_align_batch`` cuts the frame out of the row and removes the offset, ``frame_sync_batch`` does both.  ``y`` is
``[B, n]`` (one antenna) or ``[B, nr, n]`` everywhere.  Everything is validated here (ValueError) before a device is touched; there is
no CPU fallback.
"""
import numpy as np

from commpy_amd import _lib
from commpy_amd._results import outputs

__all__ = ['sync_metric_batch', 'sync_estimate_batch', 'sync_align_batch', 'schmidl_cox_preamble', 'frame_sync_batch',
           'SYNC_MAX_LAG', 'SYNC_MAX_ANTENNAS']

SYNC_MAX_LAG = 1 << 20          # lag and window
SYNC_MAX_ANTENNAS = 1024
_INT64_MAX = (1 << 63) - 1


def _whole(value, name):
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, np.integer)):
        raise ValueError('%s must be an integer, got %r' % (name, value))
    return int(value)


def _rows(y):
    """``y`` as complex128 ``[B, nr, n]`` and whether it was given without the antenna axis."""
    arr = np.asarray(y)
    if arr.dtype.kind not in 'biufc':
        raise ValueError('y must hold numbers, got dtype %s' % arr.dtype)
    if arr.ndim not in (2, 3):
        raise ValueError('y must be [B, n] or [B, nr, n], got shape %s' % (arr.shape,))
    flat = arr.ndim == 2
    if flat:
        arr = arr[:, None, :]
    if arr.shape[1] < 1:
        raise ValueError('y has no antenna (nr = 0)')
    if arr.shape[1] > SYNC_MAX_ANTENNAS:
        raise ValueError('nr = %d is above the engine limit of %d' % (arr.shape[1], SYNC_MAX_ANTENNAS))
    return np.ascontiguousarray(arr, dtype=np.complex128), flat


def _window_sizes(B, n, lag, window):
    """(D, W, nd), checked as the engine checks them."""
    D, W = _whole(lag, 'lag'), _whole(window, 'window')
    if D < 1 or W < 1:
        raise ValueError('lag = %d, window = %d, need at least 1 of each' % (D, W))
    if D > SYNC_MAX_LAG or W > SYNC_MAX_LAG:
        raise ValueError('lag = %d, window = %d: the engine limit is %d' % (D, W, SYNC_MAX_LAG))
    nd = n - D - W + 1
    if B and nd < 1:
        raise ValueError('n = %d samples hold no window of lag + window = %d' % (n, D + W))
    return D, W, max(nd, 0)


def sync_metric_batch(y, lag, window, want=('m',)):
    """The timing metric of every position: a tuple of the members of ``(M, E, P)`` that ``want`` names ('m', 'e', 'p'), in that
    order, each ``[B, n - lag - window + 1]`` (M and E float64, P complex128).  A diagnostic: the search itself
    (``sync_estimate_batch``) writes no such array."""
    want = _lib.wanted(want, ('m', 'e', 'p'))
    ya, _ = _rows(y)
    B, nr, n = ya.shape
    D, W, nd = _window_sizes(B, n, lag, window)
    out, p = outputs(want, {'m': ((B, nd), np.float64), 'e': ((B, nd), np.float64), 'p': ((B, nd), np.complex128)})
    if B:
        _lib.check(_lib.load().cpx_sync_metric(_lib.ptr(ya), B, nr, n, D, W, p('p'), p('e'), p('m')))
    return tuple(out.values())


def _search_range(search, B, nd):
    if search is None:
        return 0, _INT64_MAX
    try:
        lo, hi = search
    except (TypeError, ValueError):
        raise ValueError('search must be None or (d_lo, d_hi), got %r' % (search,))
    lo, hi = _whole(lo, 'search[0]'), _whole(hi, 'search[1]')
    if lo >= hi or not (-_INT64_MAX <= lo and hi <= _INT64_MAX):
        raise ValueError('the search range [%d, %d) is empty' % (lo, hi))
    if B and max(lo, 0) >= min(hi, nd):
        raise ValueError("the search range [%d, %d) holds none of the row's %d positions" % (lo, hi, nd))
    return lo, hi


def sync_estimate_batch(y, lag, window, search=None):
    """The fused search: ``(d_hat [B] int64, peak [B], step [B])``.  ``d_hat[b]`` is the smallest position of ``search = (d_lo, d_hi)``
    (None: the whole row) whose M is the largest among the non-NaN values, ``peak`` that M, ``step = -angle(P[d_hat]) / lag`` in
    radians per sample -- the value ``sync_align_batch`` (or ``cpx_freq_offset``) takes to remove the offset; the offset itself is
    ``-step / (2 pi)`` cycles per sample, unambiguous while ``|offset * lag| < 1/2``.  A row without a non-NaN M gives (-1, NaN, NaN)."""
    ya, _ = _rows(y)
    B, nr, n = ya.shape
    D, W, nd = _window_sizes(B, n, lag, window)
    lo, hi = _search_range(search, B, nd)
    d_hat, peak, step = np.zeros(B, dtype=np.int64), np.zeros(B), np.zeros(B)
    if B:
        _lib.check(_lib.load().cpx_sync_estimate(_lib.ptr(ya), B, nr, n, D, W, lo, hi, _lib.ptr(d_hat), _lib.ptr(peak), _lib.ptr(step)))
    return d_hat, peak, step


def sync_align_batch(y, start, step, nout):
    """``out[b, r, k] = y[b, r, start[b] + k] * exp(1j * step[b] * k)`` for k < nout, zeros where the index leaves the row; ``start``
    (int, one per row or a scalar) may be negative, ``step`` (one per row, a scalar or None) rotates exactly as
    ``add_frequency_offset`` does; None is a pure copy.  Returns complex128 ``[B, nr, nout]`` (``[B, nout]`` for ``y [B, n]``)."""
    ya, flat = _rows(y)
    B, nr, n = ya.shape
    nout = _whole(nout, 'nout')
    if nout < 1:
        raise ValueError('nout = %d, need at least 1' % nout)
    st = np.asarray(start)
    if st.dtype.kind not in 'iu' or st.ndim > 1 or (st.ndim == 1 and st.shape[0] != B):
        raise ValueError('start must hold integers, a scalar or one per row (%d), got dtype %s, shape %s' % (B, st.dtype, st.shape))
    st = np.ascontiguousarray(np.broadcast_to(st.astype(np.int64), (B,)))
    sp = None
    if step is not None:
        sp = np.asarray(step)
        if sp.dtype.kind not in 'biuf' or sp.ndim > 1 or (sp.ndim == 1 and sp.shape[0] != B):
            raise ValueError('step must hold real numbers, a scalar or one per row (%d), got dtype %s, shape %s' % (B, sp.dtype, sp.shape))
        sp = np.ascontiguousarray(np.broadcast_to(sp.astype(np.float64), (B,)))
    out = np.zeros((B, nr, nout), dtype=np.complex128)
    if B:
        _lib.check(_lib.load().cpx_sync_align(_lib.ptr(ya), B, nr, n, _lib.ptr(st), None if sp is None else _lib.ptr(sp), 0, nout,
                                              _lib.ptr(out)))
    return out[:, 0, :] if flat else out


def schmidl_cox_preamble(nfft, nsc, values=None):
    """One OFDM symbol whose body is two identical halves: a ``[nsc]`` row for ``ofdm_tx`` (host NumPy) that carries ``values`` --
    default: unit-modulus QPSK points from a seeded generator -- on the used subcarriers whose FFT bin under ``ofdm_tx``'s bin map
    (subcarrier k < nsc/2 on bin nfft - nsc/2 + k, the others on bin k - nsc/2 + 1) is even, and zeros on the others, scaled by
    sqrt(2) so that the symbol keeps the power of a fully loaded one.  ``values`` is one value per used subcarrier (``[nsc]``; those
    on odd bins are ignored)."""
    from commpy_amd.modulation import _ofdm_sizes
    nfft, nsc, _ = _ofdm_sizes(nfft, nsc, 0)
    if nfft % 2:
        raise ValueError('nfft = %d is odd: the symbol has no two halves' % nfft)
    h = nsc // 2
    k = np.arange(nsc)
    bins = np.where(k < h, nfft - h + k, k - h + 1)
    if values is None:
        pts = np.random.RandomState(0x5C0C).randint(0, 4, nsc)
        vals = np.exp(0.5j * np.pi * pts + 0.25j * np.pi)
    else:
        vals = np.asarray(values)
        if vals.dtype.kind not in 'biufc' or vals.shape != (nsc,):
            raise ValueError('values must be %d numbers, got dtype %s, shape %s' % (nsc, vals.dtype, vals.shape))
        vals = vals.astype(np.complex128)
    return np.where(bins % 2 == 0, vals * np.sqrt(2.0), 0.0).astype(np.complex128)


def frame_sync_batch(y, nfft, cp_length, nout):
    """Find a Schmidl-Cox preamble in every row, cut the frame out and remove its frequency offset:
    ``sync_estimate_batch(y, nfft / 2, nfft / 2)``, then ``sync_align_batch`` from ``d_hat - cp_length`` (the first sample of the
    preamble's cyclic prefix when d_hat is the first sample of its body) over ``nout`` samples.  Returns ``(aligned, d_hat, peak,
    step)``; the aligned rows start with the preamble symbol, so ``ofdm_rx_batch`` of them yields it as symbol 0."""
    nfft, cp_length = _whole(nfft, 'nfft'), _whole(cp_length, 'cp_length')
    if nfft < 2 or nfft % 2:
        raise ValueError('nfft = %d, need an even number >= 2' % nfft)
    if cp_length < 0:
        raise ValueError('cp_length = %d is negative' % cp_length)
    if _whole(nout, 'nout') < 1:
        raise ValueError('nout = %d, need at least 1' % nout)
    d_hat, peak, step = sync_estimate_batch(y, nfft // 2, nfft // 2)
    return sync_align_batch(y, d_hat - cp_length, step, nout), d_hat, peak, step
