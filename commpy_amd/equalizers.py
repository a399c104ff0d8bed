"""Time-domain equalisation of a known multipath channel on MI355X: maximum-likelihood sequence estimation and its max-log-MAP
soft output with a-priori LLRs (csrc/mlse.hip).

A block of ``n`` symbols with labels ``a_0 .. a_{n-1}`` and values ``c[a]`` is sent in silence through ``L`` taps:
``y_t = sum_l h_l c[a_{t-l}] + w_t``, the terms with ``t - l < 0`` or ``t - l >= n`` absent -- what
``modem.modulate -> channels.multipath_batch -> awgn`` produces.  The equaliser is a Viterbi decoder over the ``M^(L-1)`` states
``(a_t, .., a_{t-L+2})`` whose branch metrics come from the row's own taps; with ``'llr'`` it is the detector half of turbo
equalisation (the decoder half: ``ldpc_bp_decode``, ``map_decode``).  The kernels equal the NumPy model tests/mlse_model.py bit for
bit.

Limits (csrc/mlse.hip): ``L >= 2``; ``M <= 16``; ``M^(L-1) <= 256`` states; ``1 <= n <= 4096``.

Beyond those limits -- 64-QAM, or more than a handful of taps -- ``mmse_equalize_batch`` is the finite-length MMSE equaliser
(csrc/equalize.hip): ``nf`` feed-forward taps designed per row from ``h`` and ``noise_var`` by an ``L D L^H`` solve, and, with
``nb >= 1``, ``nb`` feedback taps that cancel the post-cursor of past decisions (decision feedback).  Cost grows with
``nf^3 + n nf``, not with ``M^L``: up to 64 taps each way and any constellation up to 256 points.  Bit for bit equal to
tests/equalize_model.py.

Where the channel is not known, ``adaptive_equalize_batch`` (csrc/adaptive.hip) learns the taps of a linear or decision-feedback
equaliser from a training prefix and then tracks on its own decisions, with the LMS, the normalised LMS or the RLS update; its
feed-forward taps are one sample apart, so with ``sps = 2`` it is T/2-spaced.  Bit for bit equal to tests/adaptive_model.py.
"""
import numpy as np

from commpy_amd import _lib
from commpy_amd._results import outputs, returned

__all__ = ['mlse_equalize_batch', 'mmse_equalize_batch', 'adaptive_equalize_batch']

MLSE_MAX_M, MLSE_MAX_STATES, MLSE_MAX_N = 16, 256, 4096      # csrc/mlse.hip
WANT = ('indices', 'bits', 'metric', 'llr')
MMSE_MAX_TAPS, MMSE_MAX_M, MMSE_MAX_N = 64, 256, 1 << 30            # csrc/equalize.hip
MMSE_WANT = ('indices', 'bits', 'estimate', 'llr', 'noise', 'ff', 'fb', 'gain')
ADAPT_MAX_TAPS, ADAPT_RLS_MAX_TAPS, ADAPT_MAX_M, ADAPT_MAX_N, ADAPT_MAX_SPS = 64, 32, 256, 1 << 30, 8     # csrc/adaptive.hip
ADAPT_WANT = ('indices', 'bits', 'estimate', 'error', 'ff', 'fb')
ADAPT_ALGORITHMS = ('lms', 'nlms', 'rls')                   # the C-ABI's algorithm is the position


def check_want(want):
    """``want`` as a tuple of names out of 'indices', 'bits', 'metric', 'llr'."""
    return _lib.wanted(want, WANT)


def mlse_shapes(B, n, m):
    return {'indices': ((B, n), np.int32), 'bits': ((B, n * m), np.uint8), 'metric': ((B,), np.float64), 'llr': ((B, n * m), np.float64)}


def mmse_shapes(B, n, m, nf, nb):
    return {'indices': ((B, n), np.int32), 'bits': ((B, n * m), np.uint8), 'estimate': ((B, n), np.complex128),
            'llr': ((B, n * m), np.float64), 'noise': ((B,), np.float64), 'ff': ((B, nf), np.complex128), 'fb': ((B, nb), np.complex128),
            'gain': ((B,), np.float64)}


def _rows_and_taps(y, h, tail):
    """``(y [B, n_y], h, one, B, n, L)``: the rows and the taps as contiguous complex128 arrays, whether ``y`` was 1-D, and the sizes."""
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
    return (np.ascontiguousarray(ya, dtype=np.complex128), np.ascontiguousarray(ha, dtype=np.complex128), one, B,
            n_y - (L - 1) if tail else n_y, L)


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


def check_per_row(value, B, name, upper=None):
    """A positive parameter given once or per row, as ``(float64 array [1] or [B], batched)``; ValueError for a value <= 0 (or above
    ``upper``) and for a shape other than scalar or ``[B]``.  A NaN, and an infinity within the limits, pass: they reject their rows."""
    v = np.asarray(value, dtype=np.float64)
    if v.ndim > 1 or (v.ndim == 1 and v.shape[0] != B):
        raise ValueError('%s must be a scalar or [B] = [%d], got shape %s' % (name, B, v.shape))
    if (v <= 0).any():
        raise ValueError('%s must be positive' % name)
    if upper is not None and (v > upper).any():
        raise ValueError('%s must be at most %g' % (name, upper))
    return np.ascontiguousarray(v.reshape(-1)), v.ndim == 1


def check_noise_var(noise_var, B, needed):
    """``noise_var`` through ``check_per_row``, or ``(None, False)``; ValueError for None where it is needed."""
    if noise_var is None:
        if needed:
            raise ValueError("noise_var is required when 'llr' is wanted or a_priori is given")
        return None, False
    return check_per_row(noise_var, B, 'noise_var')


def adaptive_shapes(B, n, m, nf, nb):
    return {'indices': ((B, n), np.int32), 'bits': ((B, n * m), np.uint8), 'estimate': ((B, n), np.complex128),
            'error': ((B, n), np.complex128), 'ff': ((B, nf), np.complex128), 'fb': ((B, nb), np.complex128)}


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
    ya, ha, one, B, n, L = _rows_and_taps(y, h, tail)
    M, m = check_sizes(modem, L, n)
    nv, nv_batched = check_noise_var(noise_var, B, 'llr' in want or a_priori is not None)
    prior = None
    if a_priori is not None:
        prior = np.asarray(a_priori, dtype=np.float64)
        prior = prior[None, :] if one and prior.ndim == 1 else prior
        if prior.shape != (B, n * m):
            raise ValueError('a_priori must be [B, n*m] = [%d, %d], got shape %s' % (B, n * m, prior.shape))
        prior = np.ascontiguousarray(prior)
    res, p = outputs(want, mlse_shapes(B, n, m))
    if B:
        _lib.check(_lib.load().cpx_mlse(modem._device_handle(), _lib.ptr(ya), _lib.ptr(ha), int(ha.ndim == 2), B, n, L, int(bool(tail)),
                                        None if nv is None else _lib.ptr(nv), int(nv_batched), None if prior is None else _lib.ptr(prior),
                                        *map(p, WANT)))
    return returned(res, one)


def check_mmse_sizes(modem, L, n, nf, nb, delay, want):
    """``(M, m, delay)`` of an MMSE equaliser within the kernels' limits, the default delay filled in (ValueError naming the limit
    otherwise; host only).  ``m`` is 0 for a constellation that is no power of two."""
    M = int(modem.m)
    if L < 1 or L > MMSE_MAX_TAPS:
        raise ValueError('h has %d taps, the limit is 1 <= L <= %d' % (L, MMSE_MAX_TAPS))
    if nf < 1 or nf > MMSE_MAX_TAPS:
        raise ValueError('nf = %d feed-forward taps, the limit is 1 <= nf <= %d' % (nf, MMSE_MAX_TAPS))
    if nb < 0 or nb > MMSE_MAX_TAPS:
        raise ValueError('nb = %d feedback taps, the limit is 0 <= nb <= %d' % (nb, MMSE_MAX_TAPS))
    if delay is None:
        delay = (nf + L - 2) // 2 if nb == 0 else nf - 1
    if delay < 0:
        raise ValueError('delay = %d, the limit is 0 <= delay' % delay)
    if delay + nb > nf + L - 2:
        raise ValueError('delay = %d, nb = %d: the limit is delay + nb <= nf + L - 2 = %d' % (delay, nb, nf + L - 2))
    if M < 2 or M > MMSE_MAX_M:
        raise ValueError('the constellation has %d points, the limit is 2 <= M <= %d' % (M, MMSE_MAX_M))
    pow2 = M & (M - 1) == 0
    if not pow2 and ('bits' in want or 'llr' in want):
        raise ValueError("the constellation has %d points, the limit for 'bits' and 'llr' is M a power of two" % M)
    if n < 1 or n > MMSE_MAX_N:
        raise ValueError('n = %d symbols per row, the limit is 1 <= n <= 2^30' % n)
    return M, (M.bit_length() - 1 if pow2 else 0), delay


def mmse_equalize_batch(y, h, modem, noise_var, nf, nb=0, delay=None, tail=True, want=('indices',)):
    """Equalise rows ``y [B, n_y]`` complex (or 1-D for one row) received through the taps ``h [L]`` (shared) or ``[B, L]`` with the
    finite-length MMSE equaliser of ``nf`` feed-forward taps: the linear equaliser for ``nb = 0``, the decision-feedback equaliser
    with ``nb`` feedback taps for ``nb >= 1``.  ``modem`` is any ``Modem`` (labels and bits as ``Modem.modulate`` defines them, MSB
    first; its ``Es`` is the symbol energy); ``noise_var``: a scalar or ``[B]``, positive, required.  With ``tail=True`` a row holds
    ``n + L - 1`` samples -- exactly what ``multipath_batch`` returns -- with ``tail=False`` the first ``n``.  ``delay=None`` means
    ``(nf + L - 2) // 2`` for ``nb = 0``, else ``nf - 1``.

    ``want`` names the results; they are returned in the order listed here (a single result for one name): ``'indices'`` ``[B, n]``
    int32; ``'bits'`` ``[B, n*m]`` uint8; ``'estimate'`` ``[B, n]`` complex128, the unbiased symbol estimates; ``'llr'`` ``[B, n*m]``
    float64, positive = bit 0, max-log, scaled by ``1 / nu`` like ``mlse_equalize_batch`` and ``Modem.demodulate`` scale by
    ``1 / noise_var`` -- with feedback they take the past decisions for correct, so they are optimistic after a decision error;
    ``'noise'`` ``[B]`` float64, the effective noise variance ``nu``; ``'ff'`` ``[B, nf]`` and ``'fb'`` ``[B, nb]`` complex128, the
    taps; ``'gain'`` ``[B]`` float64, the bias of the MMSE estimate.

    The rule (float64; real and imaginary parts are separate doubles; every product is rounded before it is added; every sum starts
    at 0.0 and runs in ascending index order; ``a b = (ar br - ai bi, ar bi + ai br)``, ``a conj(b) = (ar br + ai bi, ai br - ar bi)``),
    with ``d = delay``, ``Es = modem.Es``, ``N0 = noise_var``.  Design: ``H[i][k] = h_{k-i}`` for ``0 <= k-i < L``, ``i < nf``; ``K`` is
    all columns but ``d+1 .. d+nb``; for ``j <= i``, ``S[i][j]`` is the sum over ``k`` in ``K``, ``i <= k < j+L``, of
    ``h_{k-i} conj(h_{k-j})``, ``R[i][j] = Es S[i][j]``, plus ``N0`` on the diagonal, whose imaginary part is never computed;
    ``p_i = Es h_{d-i}`` (0 outside the taps).  ``L D L^H`` without a square root, column ``j``: ``g_k = (D_k Lr[j][k], -(D_k Li[j][k]))``
    for ``k < j``; ``v_i = R[i][j] - sum_{k<j} L[i][k] g_k`` for ``i >= j``; ``D_j = Re v_j``; ``L[i][j] = (vr / D_j, vi / D_j)``.
    Solve: ``a_i = p_i - sum_{k<i} L[i][k] a_k``; ``b_i = (ar / D_i, ai / D_i)``; ``u_i = b_i - sum_{k>i} u_k conj(L[k][i])``, ``i``
    descending, every sum over ``k`` ascending.  Taps: ``ff_i = conj(u_i)``; ``fb_j = sum_i ff_i h_{d+j-i}`` over the ``i`` with
    ``0 <= d+j-i < L``; ``gain = sum_i (ffr hr - ffi hi)`` of ``h_{d-i}`` over the ``i`` with ``0 <= d-i < L``;
    ``nu = (Es (1 - gain)) / gain``.  Equalise: ``z_t = sum_{i<nf} ff_i y_{t+d-i} - sum_{j=1..nb, t-j>=0} fb_j c[a^_{t-j}]``, the two
    sums formed separately, a sample outside the row read as 0.0 and multiplied like any other; ``x^_t = (zr / gain, zi / gain)``;
    ``a^_t`` is the first minimum over ``a`` ascending of ``e = x^_t - c[a]``, ``er er + ei ei``, a later point winning only if
    strictly smaller.  Soft output: ``llr[t m + i] = (min over the a with bit i = 1 - min over the a with bit i = 0 of that
    distance) / nu``, each minimum from +inf over ``a`` ascending, replaced only by a strictly smaller value.

    A row whose ``y``, ``h`` or ``noise_var`` holds a NaN or +-inf, one of whose pivots ``D_j`` is not positive and finite, or whose
    ``gain`` is not a finite number in (0, 1) -- an all-zero ``h`` gives ``gain = 0`` -- is rejected: zero indices and bits, NaN
    everywhere else; no other row is affected.

    Limits, each refused with a ``ValueError`` before any device call: ``1 <= L <= 64``; ``1 <= nf <= 64``; ``0 <= nb <= 64``;
    ``0 <= delay``; ``delay + nb <= nf + L - 2``; ``2 <= M <= 256``; ``M`` a power of two when ``'bits'`` or ``'llr'`` is wanted;
    ``1 <= n <= 2^30``; ``noise_var > 0``."""
    want = _lib.wanted(want, MMSE_WANT)
    ya, ha, one, B, n, L = _rows_and_taps(y, h, tail)
    nf, nb = int(nf), int(nb)
    M, m, delay = check_mmse_sizes(modem, L, n, nf, nb, None if delay is None else int(delay), want)
    if noise_var is None:
        raise ValueError('noise_var is required')
    nv, nv_batched = check_noise_var(noise_var, B, False)
    res, p = outputs(want, mmse_shapes(B, n, m, nf, nb))
    if B:
        _lib.check(_lib.load().cpx_mmse_equalize(modem._device_handle(), float(modem.Es), _lib.ptr(ya), _lib.ptr(ha), int(ha.ndim == 2), B,
                                                 n, L, int(bool(tail)), _lib.ptr(nv), int(nv_batched), nf, nb, delay, *map(p, MMSE_WANT)))
    return returned(res, one)


def check_adaptive_sizes(modem, n_y, n, nt, nf, nb, delay, sps, algorithm, step_given, eps, want):
    """``(M, m, delay, algorithm code)`` of an adaptive equaliser within the kernels' limits, the default delay filled in (ValueError
    naming the limit otherwise; host only).  ``m`` is 0 for a constellation that is no power of two."""
    M = int(modem.m)
    if algorithm not in ADAPT_ALGORITHMS:
        raise ValueError("algorithm = %r, the limit is one of 'lms', 'nlms', 'rls'" % (algorithm,))
    if nf < 1 or nf > ADAPT_MAX_TAPS:
        raise ValueError('nf = %d feed-forward taps, the limit is 1 <= nf <= %d' % (nf, ADAPT_MAX_TAPS))
    if nb < 0 or nb > ADAPT_MAX_TAPS:
        raise ValueError('nb = %d feedback taps, the limit is 0 <= nb <= %d' % (nb, ADAPT_MAX_TAPS))
    if algorithm == 'rls' and nf + nb > ADAPT_RLS_MAX_TAPS:
        raise ValueError("nf + nb = %d with 'rls', the limit is nf + nb <= %d" % (nf + nb, ADAPT_RLS_MAX_TAPS))
    if delay is None:
        delay = (nf - 1) // 2 if nb == 0 else nf - 1
    if delay < 0 or delay > 2 ** 31 - 1:
        raise ValueError('delay = %d, the limit is 0 <= delay' % delay)
    if sps < 1 or sps > ADAPT_MAX_SPS:
        raise ValueError('sps = %d samples per symbol, the limit is 1 <= sps <= %d' % (sps, ADAPT_MAX_SPS))
    if M < 2 or M > ADAPT_MAX_M:
        raise ValueError('the constellation has %d points, the limit is 2 <= M <= %d' % (M, ADAPT_MAX_M))
    pow2 = M & (M - 1) == 0
    if not pow2 and 'bits' in want:
        raise ValueError("the constellation has %d points, the limit for 'bits' is M a power of two" % M)
    if n < 1 or n > ADAPT_MAX_N:
        raise ValueError('n = %d symbols per row, the limit is 1 <= n <= 2^30' % n)
    if n_y > ADAPT_MAX_N * ADAPT_MAX_SPS:
        raise ValueError('n_y = %d samples per row, the limit is n_y <= 2^33' % n_y)
    if nt < 0 or nt > n:
        raise ValueError('nt = %d training symbols, the limit is 0 <= nt <= n = %d' % (nt, n))
    if algorithm == 'rls' and step_given:
        raise ValueError("step is given with 'rls', which takes forgetting and delta")
    if algorithm != 'rls' and not step_given:
        raise ValueError("step is required with 'lms' and 'nlms'")
    if eps < 0:
        raise ValueError('eps = %g, the limit is eps >= 0' % eps)
    return M, (M.bit_length() - 1 if pow2 else 0), delay, ADAPT_ALGORITHMS.index(algorithm)


def _initial_taps(taps, B, count, name):
    """``(complex128 array or None, batched)`` of initial taps ``[count]`` or ``[B, count]``."""
    if taps is None:
        return None, False
    t = np.asarray(taps)
    if t.dtype.kind not in 'biufc' or t.ndim not in (1, 2) or t.shape[-1] != count or (t.ndim == 2 and t.shape[0] != B):
        raise ValueError('%s must be numbers of shape [%d] or [%d, %d], got dtype %s, shape %s' % (name, count, B, count, t.dtype, t.shape))
    return np.ascontiguousarray(t, dtype=np.complex128), t.ndim == 2


def adaptive_equalize_batch(y, modem, training, nf, nb=0, algorithm='lms', step=None, forgetting=1.0, delta=0.01, eps=1e-6,
                            delay=None, sps=1, n=None, ff0=None, fb0=None, want=('indices',)):
    """Equalise rows ``y [B, n_y]`` complex (or 1-D for one row) of an unknown channel with an adaptive equaliser: ``nf`` feed-forward
    taps one *sample* apart (``y`` holds ``sps`` samples per symbol, so with ``sps = 2`` the equaliser is T/2-spaced) and ``nb``
    feedback taps one symbol apart (0: the linear equaliser).  ``training``: integer labels ``[nt]`` (shared) or ``[B, nt]``, the
    known first ``nt`` symbols (``0 <= nt <= n``); after them the equaliser is decision-directed.  ``modem`` is any ``Modem`` (labels
    and bits as ``Modem.modulate`` defines them, MSB first; a ``Modem`` and its device handle hold a power-of-two constellation only,
    so the checks for other sizes -- no ``'bits'`` for them -- guard a case that no modem can bring today).  ``algorithm``: ``'lms'`` or ``'nlms'`` with ``step`` (mu, required;
    ``'nlms'`` also takes ``eps >= 0``), or ``'rls'`` with ``forgetting`` (lambda in (0, 1]) and ``delta > 0`` (``step`` is refused);
    ``step``, ``forgetting`` and ``delta`` are each a scalar or ``[B]``, so one call can sweep a learning curve.  ``delay`` is in
    samples; None means ``(nf - 1) // 2`` for ``nb = 0``, else ``nf - 1``.  ``n``: symbols per row, None means ``n_y // sps``.
    ``ff0 [nf]`` or ``[B, nf]`` and ``fb0 [nb]`` or ``[B, nb]``: the initial taps, None = zeros; with the ``'ff'`` and ``'fb'`` results
    of one call they continue the equaliser over the next block.  The next call knows no sample from before its first, so a linear
    LMS / NLMS equaliser equals one call over both blocks bit for bit only with ``delay >= nf - 1``, where no step reaches back past
    its block's first sample (with a smaller delay, the default for ``nb = 0`` included, the first steps read 0.0 there); with
    feedback the past references start empty again as well.  RLS restarts its ``P`` at ``I / delta`` in every call.

    ``want`` names the results; they are returned in the order listed here (a single result for one name): ``'indices'`` ``[B, n]``
    int32, the decisions ``a^_t`` (at every ``t``, training included); ``'bits'`` ``[B, n*m]`` uint8; ``'estimate'`` ``[B, n]``
    complex128, the ``z_t``; ``'error'`` ``[B, n]`` complex128, the a-priori ``e_t`` -- the learning curve; ``mean |e|^2`` over a
    stretch is the ``noise_var`` to hand to ``Modem.demodulate(estimate, 'soft', ...)``; ``'ff'`` ``[B, nf]`` and ``'fb'``
    ``[B, nb]`` complex128, the taps after the last symbol, in the convention of ``mmse_equalize_batch``.

    The rule (float64; real and imaginary parts are separate doubles; every product is rounded before it is added; every sum starts
    at 0.0 and runs in ascending index order; ``a b = (ar br - ai bi, ar bi + ai br)``, ``a conj(b) = (ar br + ai bi, ai br - ar bi)``),
    with ``d = delay``, ``N = nf + nb``, ``c`` the constellation, ``theta = (ff, fb)``, for ``t = 0 .. n-1``.  Regressor:
    ``x[i] = y[t sps + d - i]`` for ``i < nf``, a sample outside the row read as 0.0 and multiplied like any other;
    ``x[nf + j - 1] = -r_{t-j}`` (each part negated) for ``j = 1 .. nb``, and 0.0 where ``t - j < 0``, multiplied like any other.
    Output: ``z_t = (sum_{k<nf} theta_k x_k) + (sum_{nf<=k<N} theta_k x_k)``, no conjugate, the two sums formed separately.
    Decision: ``a^_t`` is the first minimum over ``a`` ascending of ``e = z_t - c[a]``, ``er er + ei ei``, a later point winning only
    if strictly smaller.  Reference: ``r_t = c[training[t]]`` for ``t < nt``, else ``c[a^_t]``; ``e_t = r_t - z_t``.  LMS:
    ``w = (mu er, mu ei)``; ``theta_k <- theta_k + w conj(x_k)``.  NLMS: the same with ``mu_t = mu / (eps + sum_{k<N} (xr xr + xi xi))``
    in place of ``mu``.  RLS: ``P = I / delta`` (``1.0 / delta`` on the diagonal); ``g_i = sum_{j<N} P[i][j] conj(x_j)``;
    ``den = lambda + sum_{k<N} (xr gr - xi gi)``; ``kappa_i = (gr_i / den, gi_i / den)``; ``theta_i <- theta_i + kappa_i e_t``;
    ``P[i][j] <- ((Pr - qr) / lambda, (Pi - qi) / lambda)`` with ``q = kappa_i conj(g_j)``.

    A row whose ``y``, ``ff0``, ``fb0``, ``step``, ``forgetting``, ``delta`` or ``eps`` holds a NaN or +-inf, one of whose training
    labels is negative or ``>= M``, one of whose ``z_t`` is not finite (a diverged LMS), or one of whose ``den`` is not positive and
    finite is rejected: zero indices and bits, NaN everywhere else; no other row is affected.

    Limits, each refused with a ``ValueError`` before any device call: ``algorithm`` one of the three; ``1 <= nf <= 64``;
    ``0 <= nb <= 64``; ``nf + nb <= 32`` with ``'rls'`` (``P`` is then 16 KiB per row); ``0 <= delay``; ``1 <= sps <= 8``;
    ``2 <= M <= 256``; ``M`` a power of two when ``'bits'`` is wanted; ``1 <= n <= 2^30``; ``0 <= nt <= n``; ``step > 0``, required
    with ``'lms'`` and ``'nlms'`` and refused with ``'rls'``; ``0 < forgetting <= 1``; ``delta > 0``; ``eps >= 0``."""
    want = _lib.wanted(want, ADAPT_WANT)
    ya = np.asarray(y)
    if ya.dtype.kind not in 'biufc':
        raise ValueError('y must hold numbers, got dtype %s' % ya.dtype)
    if ya.ndim not in (1, 2):
        raise ValueError('y must be [B, n_y] or 1-D, got %d dimensions' % ya.ndim)
    one = ya.ndim == 1
    ya = np.ascontiguousarray(np.atleast_2d(ya), dtype=np.complex128)
    B, n_y = ya.shape
    tr = np.asarray(training)
    if tr.size and tr.dtype.kind not in 'biu':
        raise ValueError('training must hold integer labels, got dtype %s' % tr.dtype)
    if tr.ndim not in (1, 2) or (tr.ndim == 2 and tr.shape[0] != B):
        raise ValueError('y is [%d, n_y]: training must be [nt] or [%d, nt], got shape %s' % (B, B, tr.shape))
    nf, nb, sps, nt = int(nf), int(nb), int(sps), tr.shape[-1]
    n = n_y // max(sps, 1) if n is None else int(n)
    M, m, delay, code = check_adaptive_sizes(modem, n_y, n, nt, nf, nb, None if delay is None else int(delay), sps, algorithm,
                                             step is not None, float(eps), want)
    tr = np.ascontiguousarray(np.clip(tr, -1, M), dtype=np.int32)          # out of range stays out of range: it rejects the row
    rls = algorithm == 'rls'
    st, st_b = (None, False) if rls else check_per_row(step, B, 'step')
    fg, fg_b = check_per_row(forgetting, B, 'forgetting', 1.0) if rls else (None, False)
    dl, dl_b = check_per_row(delta, B, 'delta') if rls else (None, False)
    f0, f0_b = _initial_taps(ff0, B, nf, 'ff0')
    b0, b0_b = _initial_taps(fb0, B, nb, 'fb0')
    opt = lambda a: None if a is None else _lib.ptr(a)
    res, p = outputs(want, adaptive_shapes(B, n, m, nf, nb))
    if B:
        _lib.check(_lib.load().cpx_adaptive_equalize(modem._device_handle(), _lib.ptr(ya), B, n_y, n, sps, _lib.ptr(tr), int(tr.ndim == 2),
                                                     nt, nf, nb, delay, code, opt(st), int(st_b), opt(fg), int(fg_b), opt(dl), int(dl_b),
                                                     float(eps), opt(f0), int(f0_b), opt(b0), int(b0_b), *map(p, ADAPT_WANT)))
    return returned(res, one)
