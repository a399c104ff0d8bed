"""Symbol-timing and carrier recovery of a single-carrier burst on MI355X (csrc/recovery.hip): the synchroniser between
``filters.matched_filter`` and the equalisers / ``Modem.demodulate``.

``timing_recover_batch`` runs the classical interpolator / timing-error detector / loop filter / controller loop on rows of
matched-filter output at nominally ``sps`` samples per symbol, each row with its own unknown fractional delay, sample-clock offset and
-- with ``carrier`` -- residual phase and frequency offset, which a decision-directed PLL on the strobes removes in the same kernel.
One row of the batch is one independent loop; gains are per call or per row, so one call can sweep a loop bandwidth.  ``loop_gains``
turns a noise bandwidth and a damping factor into the two gains of either loop.  The kernel equals the NumPy model
tests/recovery_model.py bit for bit.
"""
import numbers

import numpy as np

from commpy_amd import _lib
from commpy_amd._results import outputs, returned

__all__ = ['timing_recover_batch', 'loop_gains']

RECOVERY_MIN_SPS, RECOVERY_MAX_SPS, RECOVERY_MAX_M, RECOVERY_MAX_N = 2, 8, 256, 1 << 30           # csrc/recovery.hip
RECOVERY_WANT = ('symbols', 'indices', 'bits', 'position', 'error', 'phase', 'count')
RECOVERY_TEDS = ('gardner', 'mm')                            # the C-ABI's ted and interp are the positions
RECOVERY_INTERPS = ('linear', 'cubic')


def recovery_shapes(B, n, m):
    return {'symbols': ((B, n), np.complex128), 'indices': ((B, n), np.int32), 'bits': ((B, n * m), np.uint8),
            'position': ((B, n), np.float64), 'error': ((B, n), np.float64), 'phase': ((B, n), np.float64), 'count': ((B,), np.int32)}


def loop_gains(bandwidth, damping=0.7071067811865476, detector_gain=1.0):
    """``(k1, k2)``, the proportional and the integral gain of a second-order loop with a proportional-plus-integral filter, from
    ``bandwidth = Bn T`` (noise bandwidth times symbol time), the damping factor and the detector's gain (output per unit of the
    quantity tracked): with ``theta = bandwidth / (damping + 1 / (4 damping))`` and ``d = 1 + 2 damping theta + theta^2``,
    ``k1 = 4 damping theta / d / detector_gain`` and ``k2 = 4 theta^2 / d / detector_gain``.  Host only.  The result is in units of the
    tracked quantity per symbol: for the timing loop of ``timing_recover_batch`` (samples) multiply by ``sps``; for its carrier loop
    (turns) use it as it is."""
    bandwidth, damping, detector_gain = float(bandwidth), float(damping), float(detector_gain)
    if not (bandwidth > 0 and np.isfinite(bandwidth)):
        raise ValueError('bandwidth = %g, the limit is bandwidth > 0' % bandwidth)
    if not (damping > 0 and np.isfinite(damping)):
        raise ValueError('damping = %g, the limit is damping > 0' % damping)
    if not (detector_gain > 0 and np.isfinite(detector_gain)):
        raise ValueError('detector_gain = %g, the limit is detector_gain > 0' % detector_gain)
    theta = bandwidth / (damping + 1.0 / (4.0 * damping))
    d = 1.0 + 2.0 * damping * theta + theta * theta
    return 4.0 * damping * theta / d / detector_gain, 4.0 * theta * theta / d / detector_gain


def whole_sps(sps):
    """``sps`` as an int; ValueError for anything but an integer (a non-integer nominal rate is not rounded)."""
    if isinstance(sps, (bool, np.bool_)) or not isinstance(sps, numbers.Integral):
        raise ValueError('sps must be an integer, got %r' % (sps,))
    return int(sps)


def check_recovery_sizes(modem, n_y, n, nt, sps, ted, interp, carrier, training, want):
    """``(M, m, ted code, interp code)`` of a recovery loop within the kernel's limits (ValueError naming the limit otherwise; host
    only).  ``M = 0`` without a modem; ``m`` is 0 without one and for a constellation that is no power of two."""
    if ted not in RECOVERY_TEDS:
        raise ValueError("ted = %r, the limit is one of 'gardner', 'mm'" % (ted,))
    if interp not in RECOVERY_INTERPS:
        raise ValueError("interp = %r, the limit is one of 'linear', 'cubic'" % (interp,))
    if sps < RECOVERY_MIN_SPS or sps > RECOVERY_MAX_SPS:
        raise ValueError('sps = %d samples per symbol, the limit is %d <= sps <= %d' % (sps, RECOVERY_MIN_SPS, RECOVERY_MAX_SPS))
    if n < 1 or n > RECOVERY_MAX_N:
        raise ValueError('n = %d strobes per row, the limit is 1 <= n <= 2^30' % n)
    if n_y < 1 or n_y > RECOVERY_MAX_N * RECOVERY_MAX_SPS:
        raise ValueError('n_y = %d samples per row, the limit is 1 <= n_y <= 2^33' % n_y)
    M = m = 0
    if modem is None:
        for needs, what in ((ted == 'mm', "ted = 'mm'"), (carrier, 'carrier'), (training, 'training'), ('indices' in want, "'indices'"),
                            ('bits' in want, "'bits'")):
            if needs:
                raise ValueError('%s needs a modem' % what)
    else:
        M = int(modem.m)
        if M < 2 or M > RECOVERY_MAX_M:
            raise ValueError('the constellation has %d points, the limit is 2 <= M <= %d' % (M, RECOVERY_MAX_M))
        pow2 = M & (M - 1) == 0
        if not pow2 and 'bits' in want:
            raise ValueError("the constellation has %d points, the limit for 'bits' is M a power of two" % M)
        m = M.bit_length() - 1 if pow2 else 0
    if 'phase' in want and not carrier:
        raise ValueError("'phase' is wanted without carrier")
    if nt < 0 or nt > n:
        raise ValueError('nt = %d training symbols, the limit is 0 <= nt <= n = %d' % (nt, n))
    return M, m, RECOVERY_TEDS.index(ted), RECOVERY_INTERPS.index(interp)


def _per_row(value, B, name, lo, hi, open_hi, limit):
    """A parameter given once or per row, as ``(float64 array [1] or [B], batched)``; ValueError for a value below ``lo`` or above
    ``hi`` (at ``hi`` too with ``open_hi``) and for a shape other than scalar or ``[B]``.  A NaN passes: it rejects its row."""
    v = np.asarray(value, dtype=np.float64)
    if v.ndim > 1 or (v.ndim == 1 and v.shape[0] != B):
        raise ValueError('%s must be a scalar or [B] = [%d], got shape %s' % (name, B, v.shape))
    if (v < lo).any() or (v > hi).any() or (open_hi and (v == hi).any()):
        raise ValueError('%s, the limit is %s' % (name, limit))
    return np.ascontiguousarray(v.reshape(-1)), v.ndim == 1


def timing_recover_batch(y, sps, modem=None, ted='gardner', interp='cubic', k1=None, k2=None, carrier=None, training=None, n=None, m0=0,
                         mu0=0.0, phase0=0.0, want=('symbols',)):
    """Recover the symbol timing -- and, with ``carrier``, the carrier phase -- of rows ``y [B, n_y]`` complex (or 1-D for one row) of
    matched-filter output at nominally ``sps`` samples per symbol (an integer, ``2 <= sps <= 8``), and return the ``n`` strobes of
    every row (None: ``n_y // sps``).  ``ted``: ``'gardner'`` (non-data-aided, no modem needed) or ``'mm'`` (Mueller-Mueller,
    decision-directed, needs ``modem``).  ``interp``: ``'linear'`` (2 samples) or ``'cubic'`` (4-sample Lagrange in Farrow form).
    ``k1``, ``k2``: proportional and integral gain of the timing loop in samples per unit of detector output, each a scalar or ``[B]``,
    finite and ``>= 0`` (None: ``loop_gains(0.01)`` times ``sps``; the detector's gain grows with the signal's power, so scale them
    to it).  ``carrier``: None or ``(kc1, kc2)``, each a scalar or ``[B]``, in turns per unit of detector output: a decision-directed
    PLL on the strobes; needs ``modem``.  ``training``: None, ``[nt]`` or ``[B, nt]`` integer labels, the known first strobes
    (``0 <= nt <= n``): the reference of ``'mm'`` and of the carrier detector while they last, which resolves the constellation's
    rotational ambiguity; needs ``modem``.  ``m0`` (integer, ``0 <= m0 < n_y``), ``mu0`` (``0 <= mu0 < 1``) and ``phase0`` (turns,
    ``|phase0| <= 0.5``), each a scalar or ``[B]``: where the loop starts.  The loop's state is not carried across calls.

    ``want`` names the results; they are returned in the order listed here (a single result for one name): ``'symbols'`` ``[B, n]``
    complex128, the strobes, derotated when ``carrier`` is given; ``'indices'`` ``[B, n]`` int32 and ``'bits'`` ``[B, n*m]`` uint8, the
    decisions (need ``modem``; labels and bits as ``Modem.modulate`` defines them, MSB first); ``'position'`` ``[B, n]`` float64,
    ``(double)m + mu`` at each strobe; ``'error'`` ``[B, n]`` float64, the timing detector's output; ``'phase'`` ``[B, n]`` float64,
    turns, after the update of that strobe (refused without ``carrier``); ``'count'`` ``[B]`` int32, the strobes all of whose
    interpolator reads lay inside the row.

    The rule (float64; real and imaginary parts are separate doubles; every product is rounded before it is added; no fused
    multiply-add; a sample index outside ``[0, n_y)`` reads 0.0 and is used like any other sample).  Per-row state: the position ``m``
    (int64) and ``mu``; the timing integrator ``v = 0.0``; the period ``w = (double)sps``; ``phi = phase0`` and its integrator
    ``f = 0.0``; the previous strobe and the previous reference.  For ``k = 0 .. n-1``.  Interpolate: ``z_k = I(m, mu)``, each part on
    its own; ``'linear'``: ``x0 + mu (x1 - x0)`` with ``x0 = y[m]``, ``x1 = y[m+1]``; ``'cubic'``, with ``xm = y[m-1]``, ``x0 = y[m]``,
    ``x1 = y[m+1]``, ``x2 = y[m+2]`` and ``S = 0.16666666666666666`` (the double nearest 1/6: the divisions are multiplications by
    ``S`` and by 0.5): ``v3 = ((x2 - xm) + 3.0 (x0 - x1)) S``, ``v2 = ((x1 + xm) 0.5) - x0``,
    ``v1 = ((6.0 x1 - x2) - (3.0 x0 + 2.0 xm)) S``, ``I = ((v3 mu + v2) mu + v1) mu + x0``.  Derotate: with ``carrier``,
    ``(c, s) = unit_phasor(phi)`` and ``z'_k = (zr c + zi s, zi c - zr s)``; without, ``z' = z``.  Decide: with a modem, ``a^_k`` is the
    first minimum over ``a`` ascending of ``e = z'_k - c[a]``, ``er er + ei ei``, a later point winning only if strictly smaller;
    ``r_k = c[training[k]]`` for ``k < nt``, else ``c[a^_k]``.  Timing error: ``e_0 = 0.0``, and no midpoint is read at ``k = 0``;
    ``'gardner'``: ``t = mu - 0.5 w``, ``fl = floor(t)``, ``zm = I(m + fl, t - fl)``,
    ``e_k = (zr_{k-1} - zr_k) zmr + (zi_{k-1} - zi_k) zmi`` on the unrotated strobes (the detector is blind to phase); ``'mm'``:
    ``e_k = (rr_{k-1} z'r_k + ri_{k-1} z'i_k) - (rr_k z'r_{k-1} + ri_k z'i_{k-1})``.  Carrier: ``ep = z'i_k rr_k - z'r_k ri_k``;
    ``f <- f + kc2 ep``; ``phi <- phi + (f + kc1 ep)``; ``phi <- phi - rint(phi)``; the row is rejected unless ``|phi| <= 0.5``.  Loop
    filter: ``v <- v + k2 e_k``; ``w = sps + (v + k1 e_k)``; the row is rejected unless ``0.5 sps < w < 1.5 sps``.  Controller:
    ``t = mu + w``, ``fl = floor(t)``, ``m <- m + fl``, ``mu <- t - fl``.  ``unit_phasor(u)`` for ``|u| <= 0.5`` is a fixed polynomial,
    not the library's sincos: ``q = rint(4 u)``, ``r = u - 0.25 q``, ``x = r 6.283185307179586``, ``x2 = x x``, ``sin = x P(x2)``,
    ``cos = Q(x2)``, the Taylor polynomials through ``x^17`` and ``x^16`` by Horner's rule, the quadrant by swaps and negations; each
    part is within ``2^-51`` of the true value.

    A row whose ``y``, ``k1``, ``k2``, ``kc1``, ``kc2``, ``mu0`` or ``phase0`` holds a NaN or +-inf, one of whose training labels is
    negative or ``>= M``, one of whose ``w`` fails ``0.5 sps < w < 1.5 sps`` or one of whose ``phi`` fails ``|phi| <= 0.5`` (a NaN fails) is rejected:
    zero integers, NaN floats; no other row is affected.

    Limits, each refused with a ``ValueError`` before any device call: ``ted`` and ``interp`` one of their two names;
    ``sps`` an integer, ``2 <= sps <= 8``; ``1 <= n <= 2^30``; ``1 <= n_y <= 2^33``; a modem for ``'mm'``, ``carrier``, ``training``, ``'indices'`` and
    ``'bits'``; ``2 <= M <= 256``; ``M`` a power of two when ``'bits'`` is wanted; ``'phase'`` only with ``carrier``;
    ``0 <= nt <= n``; ``k1, k2, kc1, kc2 >= 0``; ``0 <= m0 < n_y``; ``0 <= mu0 < 1``; ``|phase0| <= 0.5``.  ``B = 0`` returns empty
    arrays without a device call."""
    want = _lib.wanted(want, RECOVERY_WANT)
    ya = np.asarray(y)
    if ya.dtype.kind not in 'biufc':
        raise ValueError('y must hold numbers, got dtype %s' % ya.dtype)
    if ya.ndim not in (1, 2):
        raise ValueError('y must be [B, n_y] or 1-D, got %d dimensions' % ya.ndim)
    one = ya.ndim == 1
    ya = np.ascontiguousarray(np.atleast_2d(ya), dtype=np.complex128)
    B, n_y = ya.shape
    sps = whole_sps(sps)
    tr = np.zeros(0, dtype=np.int32) if training is None else np.asarray(training)
    if tr.size and tr.dtype.kind not in 'biu':
        raise ValueError('training must hold integer labels, got dtype %s' % tr.dtype)
    if tr.ndim not in (1, 2) or (tr.ndim == 2 and tr.shape[0] != B):
        raise ValueError('y is [%d, n_y]: training must be [nt] or [%d, nt], got shape %s' % (B, B, tr.shape))
    nt = tr.shape[-1]
    n = n_y // max(sps, 1) if n is None else int(n)
    if carrier is not None and (not isinstance(carrier, (tuple, list)) or len(carrier) != 2):
        raise ValueError('carrier must be None or (kc1, kc2)')
    M, m, ted_code, interp_code = check_recovery_sizes(modem, n_y, n, nt, sps, ted, interp, carrier is not None, training is not None, want)
    tr = np.ascontiguousarray(np.clip(tr, -1, max(M, 1)), dtype=np.int32)   # out of range stays out of range: it rejects the row
    if k1 is None or k2 is None:
        d1, d2 = loop_gains(0.01)
        k1, k2 = (d1 * sps if k1 is None else k1), (d2 * sps if k2 is None else k2)
    inf = float('inf')
    g1, g1_b = _per_row(k1, B, 'k1', 0.0, inf, False, 'k1 >= 0')
    g2, g2_b = _per_row(k2, B, 'k2', 0.0, inf, False, 'k2 >= 0')
    c1 = c2 = None
    c1_b = c2_b = False
    if carrier is not None:
        c1, c1_b = _per_row(carrier[0], B, 'kc1', 0.0, inf, False, 'kc1 >= 0')
        c2, c2_b = _per_row(carrier[1], B, 'kc2', 0.0, inf, False, 'kc2 >= 0')
    mu, mu_b = _per_row(mu0, B, 'mu0', 0.0, 1.0, True, '0 <= mu0 < 1')
    ph, ph_b = _per_row(phase0, B, 'phase0', -0.5, 0.5, False, '|phase0| <= 0.5')
    ms = np.asarray(m0)
    if ms.dtype.kind not in 'biu':
        raise ValueError('m0 must hold integers, got dtype %s' % ms.dtype)
    if ms.ndim > 1 or (ms.ndim == 1 and ms.shape[0] != B):
        raise ValueError('m0 must be a scalar or [B] = [%d], got shape %s' % (B, ms.shape))
    if (ms < 0).any() or (ms >= n_y).any():
        raise ValueError('m0, the limit is 0 <= m0 < n_y = %d' % n_y)
    ms_b, ms = ms.ndim == 1, np.ascontiguousarray(ms.reshape(-1), dtype=np.int64)
    opt = lambda a: None if a is None else _lib.ptr(a)
    res, p = outputs(want, recovery_shapes(B, n, m))
    if B:
        _lib.check(_lib.load().cpx_timing_recover(None if modem is None else modem._device_handle(), _lib.ptr(ya), B, n_y, n, sps, ted_code,
                                                  interp_code, _lib.ptr(g1), int(g1_b), _lib.ptr(g2), int(g2_b), opt(c1), int(c1_b), opt(c2),
                                                  int(c2_b), _lib.ptr(tr) if nt else None, int(tr.ndim == 2), nt, _lib.ptr(ms), int(ms_b),
                                                  _lib.ptr(mu), int(mu_b), _lib.ptr(ph), int(ph_b), *map(p, RECOVERY_WANT)))
    return returned(res, one)
