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

__all__ = ['SISOFlatChannel', 'MIMOFlatChannel', 'bec', 'bsc', 'awgn', 'multipath_batch']


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
