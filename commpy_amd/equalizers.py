"""Time-domain equalisation of a known multipath channel on MI355X: maximum-likelihood sequence estimation and its max-log-MAP
soft output with a-priori LLRs (csrc/mlse.hip).

A block of ``n`` symbols with labels ``a_0 .. a_{n-1}`` and values ``c[a]`` is sent in silence through ``L`` taps:
``y_t = sum_l h_l c[a_{t-l}] + w_t``, the terms with ``t - l < 0`` or ``t - l >= n`` absent -- what
``modem.modulate -> channels.multipath_batch -> awgn`` produces.  The equaliser is a Viterbi decoder over the ``M^(L-1)`` states
``(a_t, .., a_{t-L+2})`` whose branch metrics come from the row's own taps; with ``'llr'`` it is the detector half of turbo
equalisation (the decoder half: ``ldpc_bp_decode``, ``map_decode``).  The kernels equal the NumPy model tests/mlse_model.py bit for
bit.

Limits (csrc/mlse.hip): ``L >= 2``; ``M <= 16``; ``M^(L-1) <= 256`` states; ``1 <= n <= 4096``.
"""
import numpy as np

from commpy_amd import _lib

__all__ = ['mlse_equalize_batch']

MLSE_MAX_M, MLSE_MAX_STATES, MLSE_MAX_N = 16, 256, 4096      # csrc/mlse.hip
WANT = ('indices', 'bits', 'metric', 'llr')


def check_want(want):
    """``want`` as a tuple of names out of 'indices', 'bits', 'metric', 'llr'."""
    return _lib.wanted(want, WANT)


def check_sizes(modem, L, n):
    """``(M, m)`` of a modem whose trellis over ``L`` taps and ``n`` symbols is within the kernels' limits (ValueError naming the
    limit otherwise; host only)."""
    M, m = int(modem.m), int(modem.num_bits_symbol)
    if M < 2 or M > MLSE_MAX_M or M != 1 << m:
        raise ValueError('the constellation has %d points, the limit is 2 <= M <= %d, a power of two' % (M, MLSE_MAX_M))
    if L < 2:
        raise ValueError('h has %d taps, the limit is L >= 2' % L)
    if m * (L - 1) > 8:
        raise ValueError('M = %d, L = %d: M^(L-1) states, the limit is M^(L-1) <= %d' % (M, L, MLSE_MAX_STATES))
    if n < 1 or n > MLSE_MAX_N:
        raise ValueError('n = %d symbols per row, the limit is 1 <= n <= %d' % (n, MLSE_MAX_N))
    return M, m


def check_noise_var(noise_var, B, needed):
    """``noise_var`` as ``(float64 array [1] or [B], batched)`` or ``(None, False)``; ValueError for a value <= 0, for a shape other than
    scalar or ``[B]``, and for None where it is needed.  NaN and infinities pass: they reject their rows."""
    if noise_var is None:
        if needed:
            raise ValueError("noise_var is required when 'llr' is wanted or a_priori is given")
        return None, False
    nv = np.asarray(noise_var, dtype=np.float64)
    if nv.ndim > 1 or (nv.ndim == 1 and nv.shape[0] != B):
        raise ValueError('noise_var must be a scalar or [B] = [%d], got shape %s' % (B, nv.shape))
    if (nv <= 0).any():
        raise ValueError('noise_var must be positive')
    return np.ascontiguousarray(nv.reshape(-1)), nv.ndim == 1


def mlse_equalize_batch(y, h, modem, noise_var=None, a_priori=None, tail=True, want=('indices',)):
    """Equalise rows ``y [B, n_y]`` complex (or 1-D for one row) received through the taps ``h [L]`` (shared) or ``[B, L]``;
    ``modem`` is any ``Modem``, labels and bits as ``Modem.modulate`` defines them (MSB first).  With ``tail=True`` a row holds
    ``n + L - 1`` samples -- exactly what ``multipath_batch`` returns -- with ``tail=False`` the first ``n``.  ``noise_var``: a scalar
    or ``[B]``, positive; required when ``'llr'`` is wanted or ``a_priori`` is given.  ``a_priori``: ``[B, n*m]`` float64 LLRs, positive
    = bit 0 (the convention of ``list_apriori_batch`` and the LDPC decoders); None = zeros.

    ``want`` names the results; they are returned in the order listed here (a single result for one name): ``'indices'`` ``[B, n]``
    int32; ``'bits'`` ``[B, n*m]`` uint8; ``'metric'`` ``[B]`` float64, the cost of the returned sequence (the prior's included);
    ``'llr'`` ``[B, n*m]`` float64, posterior, positive = bit 0, scaled by ``1 / noise_var`` with ``noise_var`` used as-is, like
    ``Modem.demodulate``; the extrinsic part is ``llr - a_priori``.

    The rule (float64; real and imaginary parts are separate doubles; every product is rounded before it is added; sums run in the
    order written).  The state after step ``t`` is ``s' = a_t M^(L-2) + .. + a_{t-L+2}``; its candidates, in the order
    ``old = 0 .. M-1``, come from ``pred = (s' mod M^(L-2)) M + old``.  Branch metric: ``xh = sum_l h_l c[a_{t-l}]``, ``l`` ascending
    from 0.0, each product ``(hr cr - hi ci, hr ci + hi cr)``, the terms with ``t - l < 0`` skipped; ``e = y_t - xh``;
    ``d = er er + ei ei``.  Prior cost: ``P_t[a] = noise_var * (sum of La over the bits 1 of a, MSB first, from 0.0)``.  Forward:
    ``alpha_0 = 0``; ``alpha_{t+1}[s'] = (first minimum over old of alpha_t[pred] + d) + P_t[a_t]``, a later candidate winning only if
    strictly smaller.  Tail: ``beta_n[s] = sum_j |y_{n+j} - xh_j(s)|^2``, ``j = 0 .. L-2`` ascending from 0.0, ``xh_j(s)`` over
    ``l = j+1 .. L-1``; zero with ``tail=False``.  Hard output: ``s*`` is the first minimum of ``alpha_n + beta_n`` -- the ``'metric'`` --
    and the indices follow from ``s*`` and the decisions.  Soft output: ``beta_t[s] = min_a (d_t(s, a) + (P_t[a] + beta_{t+1}[s']))``,
    ``Lambda_t[s'] = alpha_{t+1}[s'] + beta_{t+1}[s']``, ``llr[t m + i] = (min of Lambda_t over the s' whose a_t has bit i = 1 - the
    same with bit i = 0) / noise_var``.

    A row whose ``y``, ``h``, prior or ``noise_var`` holds a NaN or +-inf is rejected: zero indices and bits, NaN metric and NaN LLRs;
    no other row is affected.

    Limits, each refused with a ``ValueError`` before any device call: ``L >= 2``; ``M <= 16``; ``M^(L-1) <= 256`` states;
    ``1 <= n <= 4096``."""
    want = check_want(want)
    ya, ha = np.asarray(y), np.asarray(h)
    for name, a in (('y', ya), ('h', ha)):
        if a.dtype.kind not in 'biufc':
            raise ValueError('%s must hold numbers, got dtype %s' % (name, a.dtype))
    if ya.ndim not in (1, 2):
        raise ValueError('y must be [B, n_y] or 1-D, got %d dimensions' % ya.ndim)
    one = ya.ndim == 1
    ya = np.atleast_2d(ya)
    B, n_y = ya.shape
    if ha.ndim not in (1, 2) or (ha.ndim == 2 and ha.shape[0] != B):
        raise ValueError('y is [%d, n_y]: h must be [L] or [%d, L], got shape %s' % (B, B, ha.shape))
    L = ha.shape[-1]
    n = n_y - (L - 1) if tail else n_y
    M, m = check_sizes(modem, L, n)
    nv, nv_batched = check_noise_var(noise_var, B, 'llr' in want or a_priori is not None)
    prior = None
    if a_priori is not None:
        prior = np.asarray(a_priori, dtype=np.float64)
        prior = prior[None, :] if one and prior.ndim == 1 else prior
        if prior.shape != (B, n * m):
            raise ValueError('a_priori must be [B, n*m] = [%d, %d], got shape %s' % (B, n * m, prior.shape))
        prior = np.ascontiguousarray(prior)
    ya = np.ascontiguousarray(ya, dtype=np.complex128)
    ha = np.ascontiguousarray(ha, dtype=np.complex128)
    shapes = {'indices': ((B, n), np.int32), 'bits': ((B, n * m), np.uint8), 'metric': ((B,), np.float64), 'llr': ((B, n * m), np.float64)}
    res = {name: np.zeros(*shapes[name]) for name in WANT if name in want}
    if B:
        p = lambda v: None if v is None else _lib.ptr(v)
        _lib.check(_lib.load().cpx_mlse(modem._device_handle(), _lib.ptr(ya), _lib.ptr(ha), int(ha.ndim == 2), B, n, L, int(bool(tail)),
                                        p(nv), int(nv_batched), p(prior), p(res.get('indices')), p(res.get('bits')),
                                        p(res.get('metric')), p(res.get('llr'))))
    out = [res[name][0] if one else res[name] for name in WANT if name in want]
    return out[0] if len(out) == 1 else tuple(out)
