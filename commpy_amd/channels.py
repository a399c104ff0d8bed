"""Flat SISO channel models used to drive the decoders (host side, NumPy RNG).

Mirrors the part of /root/reference/commpy/channels.py the decoding path uses:
``SISOFlatChannel`` (channels.py:99-240, with ``_FlatChannel.set_SNR_dB`` :57-74 and
``generate_noises`` :37-55) and the ``bec`` / ``bsc`` / ``awgn`` helpers (:630-708).
``SISOFlatChannel.propagate`` also accepts a 2-D ``[batch, nsym]`` message so that a whole Monte-Carlo batch is
generated at once.  ``MIMOFlatChannel`` (channels.py:242-627, the Kronecker model) produces the per-vector channel
matrices the MIMO detectors of commpy_amd.modulation consume; it draws from NumPy's global generator in the reference's
order (noises, then gains) so that a seeded run reproduces the reference's outputs.

Kept quirk B7: for a complex channel the generated noise is
``(randn + 1j*randn) * noise_std * 0.5`` (channels.py:53) while receivers are told
``noise_std**2`` (links.py:242-243).
"""
import numpy as np
from numpy import abs, absolute, asarray, isrealobj, sqrt, where, zeros
from scipy.linalg import sqrtm
from numpy.random import randn, random, standard_normal

__all__ = ['SISOFlatChannel', 'MIMOFlatChannel', 'bec', 'bsc', 'awgn', 'multipath_batch', 'fading_params_batch', 'fading_gains_batch',
           'fading_convolve_batch', 'fading_multipath_batch', 'tap_frequency_response', 'FADING_SCRATCH_BYTES', 'FADING_MAX_SINUSOIDS']


class SISOFlatChannel:
    """AWGN / Rice / Rayleigh flat SISO channel -- same constructor and attributes as channels.py:99."""

    def __init__(self, noise_std=None, fading_param=(1, 0)):
        self.noises = None
        self.channel_gains = None
        self.unnoisy_output = None
        self.noise_std = noise_std
        self.fading_param = fading_param

    nb_tx = nb_rx = property(lambda self: 1, doc='one antenna on each side (channels.py:223-231)')

    @property
    def isComplex(self):
        return self._isComplex

    @property
    def fading_param(self):
        return self._fading_param

    @fading_param.setter
    def fading_param(self, value):
        mean, variance = value[0], value[1]
        if variance + absolute(mean) ** 2 != 1:                      # energy conservation test of channels.py:205-206
            raise ValueError('fading_param = (mean, variance) must satisfy variance + |mean|^2 == 1: this channel would '
                             'add or remove energy')
        self._isComplex = isinstance(mean, complex)
        self._fading_param = value

    @property
    def k_factor(self):
        return absolute(self.fading_param[0]) ** 2 / absolute(self.fading_param[1])

    def set_SNR_dB(self, SNR_dB, code_rate=1., Es=1):
        """noise_std = sqrt((isComplex + 1) * nb_tx * Es / (code_rate * 10^(SNR/10)))  (channels.py:74)."""
        self.noise_std = sqrt((self.isComplex + 1) * self.nb_tx * Es / (code_rate * 10 ** (SNR_dB / 10)))

    def set_SNR_lin(self, SNR_lin, code_rate=1, Es=1):
        self.noise_std = sqrt((self.isComplex + 1) * self.nb_tx * Es / (code_rate * SNR_lin))

    def generate_noises(self, dims):
        """Noise samples for one propagation (channels.py:37-55).  Draw order and scaling are the reference's: real part
        first, and HALF of noise_std per component on the complex branch (:53) -- the receiver is told noise_std**2."""
        if self.noise_std is None:
            raise AssertionError('Noise standard deviation must be set before propagation.')
        noises = standard_normal(dims)
        if self.isComplex:
            noises = (noises + 1j * standard_normal(dims)) * self.noise_std * 0.5
        else:
            noises = noises * self.noise_std
        self.noises = noises

    def propagate(self, msg):
        """Fading + noise (channels.py:181-221); ``msg`` may be 1-D or ``[batch, nsym]``."""
        msg = asarray(msg)
        cplx = self.isComplex
        if not (cplx or isrealobj(msg)):
            raise TypeError('a complex message cannot be propagated in a real channel.')
        dims = msg.shape
        self.generate_noises(dims)                             # draw order of the reference: noise first, then the fading
        mean, variance = self.fading_param
        if cplx:
            scatter = (standard_normal(dims) + 1j * standard_normal(dims)) * sqrt(0.5 * variance)
        else:
            scatter = standard_normal(dims) * sqrt(variance)
        gains = self.channel_gains = mean + scatter
        clean = self.unnoisy_output = gains * msg
        return clean + self.noises



def _exponent_matrix(n):
    """[[j - i]] for i, j < n: the exponents of the exponential correlation model."""
    k = np.arange(n)
    return k[None, :] - k[:, None]


class MIMOFlatChannel:
    """nb_tx x nb_rx flat-fading channel of the Kronecker model -- same constructor, attributes and setters as
    channels.py:242.  ``fading_param = (mean [nb_rx, nb_tx], Rt [nb_tx, nb_tx], Rr [nb_rx, nb_rx])``; the default is
    uncorrelated Rayleigh fading.  ``channel_gains[i]`` is the [nb_rx, nb_tx] matrix of the i-th vector."""

    def __init__(self, nb_tx, nb_rx, noise_std=None, fading_param=None):
        self.noises = None
        self.channel_gains = None
        self.unnoisy_output = None
        self.nb_tx, self.nb_rx = nb_tx, nb_rx
        self.noise_std = noise_std
        if fading_param is None:
            fading_param = (zeros((nb_rx, nb_tx)), np.identity(nb_tx), np.identity(nb_rx))
        self.fading_param = fading_param

    # the SISO channel's noise and SNR rules are the reference's shared base-class ones (channels.py:37-90)
    generate_noises = SISOFlatChannel.generate_noises
    set_SNR_dB = SISOFlatChannel.set_SNR_dB
    set_SNR_lin = SISOFlatChannel.set_SNR_lin
    isComplex = SISOFlatChannel.isComplex

    @staticmethod
    def _gains(param):
        """(NLOS power tr(Rt^T kron Rr), LOS power sum |mean|^2)."""
        mean, rt, rr = param
        return np.trace(rt) * np.trace(rr), np.sum(absolute(mean) ** 2)

    @property
    def fading_param(self):
        return self._fading_param

    @fading_param.setter
    def fading_param(self, value):
        nlos, los = self._gains(value)
        if absolute(nlos + los - self.nb_tx * self.nb_rx) > 1e-3:
            raise ValueError('With this parameters, the channel would add or remove energy.')
        self._fading_param = value
        self._isComplex = isinstance(value[0][0, 0], complex)

    @property
    def k_factor(self):
        """LOS / NLOS power ratio."""
        nlos, los = self._gains(self.fading_param)
        return los / nlos

    def propagate(self, msg):
        """Send ``msg`` (padded with zeros to a multiple of nb_tx) as vectors of nb_tx symbols; returns [nb_vect, nb_rx]."""
        cplx = self.isComplex
        if not cplx and isinstance(msg[0], complex):
            raise TypeError('a complex message cannot be propagated in a real channel.')
        nb_vect = -(-len(msg) // self.nb_tx)
        short = nb_vect * self.nb_tx - len(msg)
        x = np.hstack((msg, zeros(short))) if short else np.asarray(msg)
        x = x.reshape(nb_vect, self.nb_tx)
        shape = (nb_vect, self.nb_rx, self.nb_tx)
        self.generate_noises(shape[:2])                             # noises first, then the gains (channels.py:359-366)
        g = standard_normal(shape)
        g = (g + 1j * standard_normal(shape)) * sqrt(0.5) if cplx else g
        mean, rt, rr = self.fading_param
        g = np.matmul(np.matmul(sqrtm(rr), g), sqrtm(rt).T) + mean
        self.channel_gains = g
        self.unnoisy_output = np.matmul(g, x[:, :, None])[:, :, 0]
        return self.unnoisy_output + self.noises

    def specular_compo(self, thetat, dt, thetar, dr):
        """Line-of-sight component exp(2j pi (n dr cos thetar + m dt cos thetat)) [nb_rx, nb_tx] (channels.py:437)."""
        if dr < 0 or dt < 0:
            raise ValueError("the distance must be positive ")
        rx = np.arange(self.nb_rx)[:, None] * dr * np.cos(thetar)
        tx = np.arange(self.nb_tx)[None, :] * dt * np.cos(thetat)
        return np.exp(1j * 2 * np.pi * (rx + tx))

    def _kbsm(self, betat, betar):
        """KBSM-BD-AA weighting of the correlation matrices (channels.py:404-430)."""
        if betar < 0 or betat < 0:
            raise ValueError("beta must be positif")
        et = np.exp(-betat * abs(_exponent_matrix(self.nb_tx)))
        er = np.exp(-betar * abs(_exponent_matrix(self.nb_rx)))
        mean, rt, rr = self.fading_param
        self.fading_param = mean, rt * et, rr * er

    @staticmethod
    def _check_unit(t, r):
        for name, v in (('t', t), ('r', r)):
            if abs(v) - 1 > 1e-4:
                raise ValueError('abs(%s) must be one.' % name)

    def _scaled_mean(self, mean, k_factor):
        nlos = mean.size / (k_factor + 1)
        return mean * sqrt(k_factor * nlos / np.sum(absolute(mean) ** 2)), nlos

    def uncorr_rayleigh_fading(self, dtype):
        """Uncorrelated Rayleigh fading of type ``dtype`` (complex or float)."""
        self.fading_param = zeros((self.nb_rx, self.nb_tx), dtype), np.identity(self.nb_tx), np.identity(self.nb_rx)

    def expo_corr_rayleigh_fading(self, t, r, betat=0, betar=0):
        """Rayleigh fading with exponential correlation t^(j-i) / r^(j-i), |t| = |r| = 1, optional KBSM betas."""
        self._check_unit(t, r)
        self.fading_param = (zeros((self.nb_rx, self.nb_tx), complex), t ** _exponent_matrix(self.nb_tx),
                             r ** _exponent_matrix(self.nb_rx))
        self._kbsm(betat, betar)

    def uncorr_rician_fading(self, mean, k_factor):
        """Uncorrelated Rician fading: ``mean`` rescaled to the requested k-factor."""
        mean, nlos = self._scaled_mean(mean, k_factor)
        self.fading_param = mean, np.identity(self.nb_tx) * nlos / mean.size, np.identity(self.nb_rx)

    def expo_corr_rician_fading(self, mean, k_factor, t, r, betat=0, betar=0):
        """Rician fading with exponential correlation; ``mean`` rescaled to the requested k-factor."""
        self._check_unit(t, r)
        mean, nlos = self._scaled_mean(mean, k_factor)
        self.fading_param = mean, t ** _exponent_matrix(self.nb_tx) * nlos / mean.size, r ** _exponent_matrix(self.nb_rx)
        self._kbsm(betat, betar)

def bec(input_bits, p_e):
    """Binary erasure channel: erased bits become -1 (channels.py:630-649)."""
    output_bits = asarray(input_bits).copy()
    output_bits[random(len(output_bits)) <= p_e] = -1
    return output_bits


def bsc(input_bits, p_t):
    """Binary symmetric channel (channels.py:652-673)."""
    bits = asarray(input_bits)
    return where(random(len(bits)) <= p_t, 1 ^ bits, bits)          # one uniform draw per bit, flipped where it is <= p_t


def awgn(input_signal, snr_dB, rate=1.0):
    """White Gaussian noise at ``snr_dB`` relative to the signal's own mean energy (channels.py:676-708).

    The noise power per real dimension is ``mean(|x|^2) / (2 * rate * 10^(snr_dB / 10))``; a complex signal gets that on each axis,
    a real one twice that on its single axis.  The draws come from NumPy's global generator in the reference's order (all real
    parts, then all imaginary parts) and the mean energy is NumPy's pairwise ``sum`` (the reference module imports ``sum`` from
    numpy), so a seeded call returns the reference's samples bit for bit (tests/test_links_host.py)."""
    x = asarray(input_signal)
    n = len(x)
    energy = abs(x) * abs(x)
    per_axis = (energy.sum() / n) / (2 * rate * 10 ** (snr_dB / 10.0))
    if isinstance(x[0], complex):                                  # (the reference's own type test: element 0 decides)
        sigma = sqrt(per_axis)
        re, im = randn(n), randn(n)
        return x + (sigma * re + sigma * im * 1j)
    return x + sqrt(2 * per_axis) * randn(n)


MULTIPATH_MAX_L = 1024
MULTIPATH_MAX_TAPS = 2048


def multipath_batch(x, g):
    """Frequency-selective channel on the GPU (csrc/ofdm_chan.hip): ``y[b][r] = sum_t convolve(x[b][t], g[b][r][t])``, full length.
    ``x [B, nt, n]`` with ``g [B, nr, nt, L]`` or ``[nr, nt, L]`` (shared by all rows) -> complex128 ``[B, nr, n + L - 1]``; the SISO
    short forms ``x [B, n]`` with ``g [B, L]`` or ``[L]`` -> ``[B, n + L - 1]``.  No noise: add it with ``awgn`` or, on the device,
    ``cpx_awgn_dev``.  ``L <= 1024`` and ``nr nt L <= 2048``."""
    from commpy_amd import _lib
    xa, ga = np.asarray(x), np.asarray(g)
    for name, a in (('x', xa), ('g', ga)):
        if a.dtype.kind not in 'biufc':
            raise ValueError('%s must hold numbers, got dtype %s' % (name, a.dtype))
    siso = xa.ndim == 2
    if siso:
        if ga.ndim not in (1, 2):
            raise ValueError('x is [B, n]: g must be [L] or [B, L], got shape %s' % (ga.shape,))
        xa = xa[:, None, :]
        ga = ga[None, None, :] if ga.ndim == 1 else ga[:, None, None, :]
    elif xa.ndim != 3:
        raise ValueError('x must be [B, nt, n] or [B, n], got shape %s' % (xa.shape,))
    if ga.ndim not in (3, 4):
        raise ValueError('x is [B, nt, n]: g must be [nr, nt, L] or [B, nr, nt, L], got shape %s' % (ga.shape,))
    B, nt, n = xa.shape
    nr, L = ga.shape[-3], ga.shape[-1]
    if ga.shape[-2] != nt or (ga.ndim == 4 and ga.shape[0] != B):
        raise ValueError('shape mismatch: x %s, g %s' % (xa.shape, ga.shape))
    if nt < 1 or nr < 1 or L < 1:
        raise ValueError('nt = %d, nr = %d, L = %d, need at least 1 of each' % (nt, nr, L))
    if B and n < 1:
        raise ValueError('n = 0 (an empty row cannot be convolved)')
    if L > MULTIPATH_MAX_L or nr * nt * L > MULTIPATH_MAX_TAPS:
        raise ValueError('L = %d, nr nt L = %d: above the engine limits of %d and %d' % (L, nr * nt * L, MULTIPATH_MAX_L, MULTIPATH_MAX_TAPS))
    xa = np.ascontiguousarray(xa, dtype=np.complex128)
    ga = np.ascontiguousarray(ga, dtype=np.complex128)
    out = np.zeros((B, nr, n + L - 1), dtype=np.complex128)
    if B:
        _lib.check(_lib.load().cpx_multipath(_lib.ptr(xa), _lib.ptr(ga), int(ga.ndim == 4), B, nt, nr, n, L, _lib.ptr(out)))
    return out[:, 0, :] if siso else out


# ---- Doppler-fading multipath channel: time-varying taps (csrc/fading.hip; include/commpy_amd.h has the definitions) ---------------

FADING_SCRATCH_BYTES = 64 << 20     # the most scratch cpx_fading_channel holds gains in (CPX_FADING_SCRATCH_BYTES)
FADING_MAX_SINUSOIDS = 256
_TWO52 = 1 << 52
_UINT64_MAX = (1 << 64) - 1


def _whole(value, name, lo=None, hi=None):
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, np.integer)):
        raise ValueError('%s must be an integer, got %r' % (name, value))
    value = int(value)
    if (lo is not None and value < lo) or (hi is not None and value > hi):
        raise ValueError('%s = %d is outside [%s, %s]' % (name, value, lo, '...' if hi is None else hi))
    return value


def _real(value, name, lo, hi):
    try:
        v = float(value)
    except (TypeError, ValueError):
        raise ValueError('%s must be a real number, got %r' % (name, value)) from None
    if isinstance(value, (bool, np.bool_)) or not lo <= v <= hi:            # NaN fails the comparison
        raise ValueError('%s = %r is outside [%g, %g]' % (name, value, lo, hi))
    return v


class _FadingModel:
    """The validated parameters of the fading model, as the C entry points take them."""

    def __init__(self, B, nr, nt, pdp, fd, hold, t0, n_sin, k_factor, fd_los, seed, stream_id, first_row):
        self.B = _whole(B, 'B', 0)
        self.nr, self.nt = _whole(nr, 'nr', 1), _whole(nt, 'nt', 1)
        pa = np.asarray(pdp)
        if pa.dtype.kind not in 'biuf' or pa.ndim != 1 or pa.size < 1:
            raise ValueError('pdp must be a 1-D array of at least one real tap power')
        self.pdp = np.ascontiguousarray(pa, dtype=np.float64)
        self.L = L = self.pdp.size
        if not np.all(np.isfinite(self.pdp) & (self.pdp >= 0)):
            raise ValueError('pdp must hold finite powers >= 0')
        if L > MULTIPATH_MAX_L or self.nr * self.nt * L > MULTIPATH_MAX_TAPS:
            raise ValueError('L = %d, nr nt L = %d: above the engine limits of %d and %d'
                             % (L, self.nr * self.nt * L, MULTIPATH_MAX_L, MULTIPATH_MAX_TAPS))
        self.kf = None
        if k_factor is not None:
            ka = np.asarray(k_factor)
            if ka.dtype.kind not in 'biuf' or ka.ndim > 1:
                raise ValueError('k_factor must be a real number or one per tap')
            ka = np.ascontiguousarray(np.broadcast_to(ka, (L,)) if ka.ndim == 0 else ka, dtype=np.float64)
            if ka.shape != (L,) or not np.all(np.isfinite(ka) & (ka >= 0)):
                raise ValueError('k_factor must hold %d finite values >= 0' % L)
            with np.errstate(over='ignore'):
                if not np.all(np.isfinite(self.pdp * ka)):
                    raise ValueError('pdp * k_factor overflows')
            self.kf = ka
        self.fd, self.fd_los = _real(fd, 'fd', 0.0, 0.5), _real(fd_los, 'fd_los', -0.5, 0.5)
        self.n_sin = _whole(n_sin, 'n_sin', 1, FADING_MAX_SINUSOIDS)
        self.hold, self.t0 = _whole(hold, 'hold', 1), _whole(t0, 't0', 0)
        self.seed, self.stream_id = _whole(seed, 'seed', 0, _UINT64_MAX), _whole(stream_id, 'stream_id', 0, _UINT64_MAX)
        self.first_row = _whole(first_row, 'first_row', 0, _UINT64_MAX)

    def blocks(self, nblk):
        nblk = _whole(nblk, 'nblk', 1)
        if self.t0 + nblk * self.hold >= _TWO52:
            raise ValueError('t0 + nblk * hold = %d reaches 2^52' % (self.t0 + nblk * self.hold))
        return nblk

    def shapes(self, lout, nblk):
        """The channel's results for rows of ``lout`` output samples and ``nblk`` blocks of gains."""
        return {'y': ((self.B, self.nr, lout), np.complex128), 'g': ((self.B, nblk, self.nr, self.nt, self.L), np.complex128)}

    def draw_args(self):
        return (self.n_sin, self.fd, self.fd_los)

    def tap_args(self):
        from commpy_amd import _lib
        return (_lib.ptr(self.pdp), None if self.kf is None else _lib.ptr(self.kf))

    def key_args(self):
        return (self.seed, self.stream_id, self.first_row)


def fading_params_batch(B, nr, nt, L, fd, n_sin=16, fd_los=0.0, seed=0, stream_id=0, first_row=0):
    """``(nu, phi)`` of every sinusoid of the fading model, float64 ``[B, nr, nt, L, n_sin + 1, 2]``: Doppler ``nu`` in cycles per
    sample and phase ``phi`` in cycles of sinusoid s < n_sin of each path, then of the path's line of sight (``nu = fd_los``).  With
    these the channel is known analytically: ``G(tau) = a_l sum_s exp(2j pi (nu_s tau + phi_s))`` (+ the line of sight), see
    ``fading_gains_batch``."""
    from commpy_amd import _lib
    md = _FadingModel(B, nr, nt, np.ones(_whole(L, 'L', 1)), fd, 1, 0, n_sin, None, fd_los, seed, stream_id, first_row)
    out = np.zeros((md.B, md.nr, md.nt, md.L, md.n_sin + 1, 2), dtype=np.float64)
    if md.B:
        _lib.check(_lib.load().cpx_fading_params(md.B, md.nr, md.nt, md.L, *md.draw_args(), *md.key_args(), _lib.ptr(out)))
    return out


def fading_gains_batch(B, nr, nt, pdp, fd, nblk, hold=1, t0=0, n_sin=16, k_factor=None, fd_los=0.0, seed=0, stream_id=0, first_row=0):
    """Tap gains of the Doppler-fading channel on the GPU (csrc/fading.hip), complex128 ``[B, nblk, nr, nt, L]``: block j holds the
    gains at time ``t0 + j * hold`` (in samples).  Clarke's model: every path (row, antenna pair, tap) is a sum of ``n_sin`` sinusoids
    with Dopplers ``fd cos(2 pi u)`` (``fd`` = maximum Doppler in cycles per sample, at most 0.5) and uniform phases, scaled to the
    tap's power ``pdp[l]``; ``k_factor`` (a number or one per tap) adds a line of sight of Doppler ``fd_los`` with that Rician K.  The
    draws come from the Philox stream ``(seed, stream_id)``: a gain is a pure function of (seed, stream id, first_row + b, r, t, l,
    time), so rows and time spans may be generated in any number of calls."""
    from commpy_amd import _lib
    md = _FadingModel(B, nr, nt, pdp, fd, hold, t0, n_sin, k_factor, fd_los, seed, stream_id, first_row)
    nblk = md.blocks(nblk)
    out = np.zeros((md.B, nblk, md.nr, md.nt, md.L), dtype=np.complex128)
    if md.B:
        _lib.check(_lib.load().cpx_fading_gains(md.B, md.nr, md.nt, md.L, *md.tap_args(), *md.draw_args(), md.hold, md.t0, nblk,
                                                *md.key_args(), _lib.ptr(out)))
    return out


def _fading_rows(x):
    xa = np.asarray(x)
    if xa.dtype.kind not in 'biufc':
        raise ValueError('x must hold numbers, got dtype %s' % xa.dtype)
    siso = xa.ndim == 2
    if siso:
        xa = xa[:, None, :]
    elif xa.ndim != 3:
        raise ValueError('x must be [B, nt, n] or [B, n], got shape %s' % (xa.shape,))
    if xa.shape[1] < 1:
        raise ValueError('x has no antenna (nt = 0)')
    if xa.shape[0] and xa.shape[2] < 1:
        raise ValueError('n = 0 (an empty row cannot be convolved)')
    return np.ascontiguousarray(xa, dtype=np.complex128), siso


def fading_convolve_batch(x, G, hold):
    """Time-varying convolution on the GPU: ``y[b][r][m] = sum_t sum_l G[b][m // hold][r][t][l] x[b][t][m - l]``, full length.
    ``x [B, nt, n]`` with ``G [B, nblk, nr, nt, L]`` or ``[nblk, nr, nt, L]`` (shared by all rows), ``nblk = ceil((n + L - 1) / hold)``
    -> complex128 ``[B, nr, n + L - 1]``; the SISO short form ``x [B, n]`` with ``G [B, nblk, L]`` or ``[nblk, L]`` -> ``[B, n + L - 1]``.
    With gains that do not change from block to block this is ``multipath_batch`` bit for bit."""
    from commpy_amd import _lib
    xa, siso = _fading_rows(x)
    ga = np.asarray(G)
    if ga.dtype.kind not in 'biufc':
        raise ValueError('G must hold numbers, got dtype %s' % ga.dtype)
    hold = _whole(hold, 'hold', 1)
    if siso:
        if ga.ndim not in (2, 3):
            raise ValueError('x is [B, n]: G must be [nblk, L] or [B, nblk, L], got shape %s' % (ga.shape,))
        ga = ga[..., None, None, :]
    if ga.ndim not in (4, 5):
        raise ValueError('x is [B, nt, n]: G must be [nblk, nr, nt, L] or [B, nblk, nr, nt, L], got shape %s' % (ga.shape,))
    B, nt, n = xa.shape
    nr, L = ga.shape[-3], ga.shape[-1]
    if nr < 1 or L < 1:
        raise ValueError('nr = %d, L = %d, need at least 1 of each' % (nr, L))
    if L > MULTIPATH_MAX_L or nr * nt * L > MULTIPATH_MAX_TAPS:
        raise ValueError('L = %d, nr nt L = %d: above the engine limits of %d and %d' % (L, nr * nt * L, MULTIPATH_MAX_L, MULTIPATH_MAX_TAPS))
    nblk = -(-(n + L - 1) // hold)
    if ga.shape[-2] != nt or (ga.ndim == 5 and ga.shape[0] != B) or (B and ga.shape[-4] != nblk):
        raise ValueError('shape mismatch: x %s, G %s, hold %d (%d blocks)' % (xa.shape, ga.shape, hold, nblk))
    ga = np.ascontiguousarray(ga, dtype=np.complex128)
    out = np.zeros((B, nr, n + L - 1), dtype=np.complex128)
    if B:
        _lib.check(_lib.load().cpx_fading_convolve(_lib.ptr(xa), _lib.ptr(ga), int(ga.ndim == 5), B, nt, nr, n, L, hold, _lib.ptr(out)))
    return out[:, 0, :] if siso else out


def fading_multipath_batch(x, nr, pdp, fd, hold=1, t0=0, n_sin=16, k_factor=None, fd_los=0.0, seed=0, stream_id=0, first_row=0,
                           want=('y',)):
    """``x`` through the Doppler-fading multipath channel on the GPU: the gains of ``fading_gains_batch`` for ``ceil((n + L - 1) /
    hold)`` blocks from ``t0``, then ``fading_convolve_batch``.  ``x [B, nt, n]`` -> ``y [B, nr, n + L - 1]``; the SISO short form
    ``x [B, n]`` (with ``nr = 1``) -> ``[B, n + L - 1]``.  Returns ``y``, or ``(y, G)`` with 'g' in ``want`` (``G [B, nblk, nr, nt, L]``
    always: with ``tap_frequency_response`` it is the perfect channel state per block).  Without 'g' the gains never leave the
    device, where they take at most ``FADING_SCRATCH_BYTES``.  No noise: add it with ``awgn`` or ``cpx_awgn_dev``."""
    from commpy_amd import _lib
    from commpy_amd._results import outputs
    want = _lib.wanted(want, ('y', 'g'))
    xa, siso = _fading_rows(x)
    B, nt, n = xa.shape
    md = _FadingModel(B, nr, nt, pdp, fd, hold, t0, n_sin, k_factor, fd_los, seed, stream_id, first_row)
    if siso and md.nr != 1:
        raise ValueError('x is [B, n]: nr must be 1, got %d' % md.nr)
    lout = n + md.L - 1
    nblk = md.blocks(-(-lout // md.hold)) if B else 1
    out, p = outputs(want, md.shapes(lout, nblk))
    if B:
        _lib.check(_lib.load().cpx_fading_channel(_lib.ptr(xa) if 'y' in want else None, B, nt, md.nr, n, md.L, *md.tap_args(),
                                                  *md.draw_args(), md.hold, md.t0, *md.key_args(), p('y'), p('g')))
    if 'y' in want and siso:
        out['y'] = out['y'][:, 0, :]
    return out['y'] if want == ('y',) else tuple(out.values())


def tap_frequency_response(G, nfft, nsc):
    """Host-side helper (plain NumPy, no device): the frequency response of tap sets ``G [..., L]`` on the ``nsc`` used subcarriers of
    an ``nfft``-point OFDM symbol, ``H[..., k] = sum_l G[..., l] exp(-2j pi f(k) l / nfft)`` with ``f = ofdm_subcarrier_frequencies(nsc)``
    -> complex128 ``[..., nsc]``.  For ``G [B, nblk, nr, nt, L]`` of ``fading_multipath_batch`` with ``hold`` = one OFDM symbol it is
    the perfect-CSI ``H`` per symbol (``L <= cp_length + 1``)."""
    from commpy_amd.modulation import ofdm_subcarrier_frequencies
    ga = np.asarray(G)
    if ga.dtype.kind not in 'biufc' or ga.ndim < 1 or ga.shape[-1] < 1:
        raise ValueError('G must be a numeric array [..., L] with L >= 1')
    nfft, nsc = _whole(nfft, 'nfft', 1), _whole(nsc, 'nsc', 1)
    if nsc < 2 or nsc % 2 or nsc // 2 > nfft - 1:
        raise ValueError('nsc = %d must be even, at least 2, with nsc / 2 <= nfft - 1 = %d' % (nsc, nfft - 1))
    f = ofdm_subcarrier_frequencies(nsc)
    l = np.arange(ga.shape[-1])
    E = np.exp(-2j * np.pi * ((f[None, :] * l[:, None]) % nfft) / nfft)       # [L, nsc]; the phase index is reduced exactly
    return np.asarray(ga, dtype=np.complex128) @ E
