"""Host side of the Doppler-fading multipath channel: the NumPy model against exact rational arithmetic, brute-force loops and the
statistics of Clarke's model; the C-ABI's names; every refusal (ValueError / CPX_EINVAL / CPX_ELIMIT before any device is touched) and
the loud failure without a device."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest
from scipy.special import j0

import fading_model as M
import rng_model as R
from commpy_amd import _lib, channels, deviceops
from commpy_amd.channels import (FADING_SCRATCH_BYTES, fading_convolve_batch, fading_gains_batch, fading_multipath_batch,
                                 fading_params_batch, tap_frequency_response)
from commpy_amd.modulation import ofdm_subcarrier_frequencies

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["cpx_fading_params", "cpx_fading_params_dev", "cpx_fading_gains", "cpx_fading_gains_dev", "cpx_fading_convolve",
         "cpx_fading_convolve_dev", "cpx_fading_channel", "cpx_fading_channel_dev"]


def cplx(rs, *shape):
    return rs.randn(*shape) + 1j * rs.randn(*shape)


# ---- the model ----------------------------------------------------------------------------------------------------------------------
def test_model_counters_and_draws():
    B, nr, nt, L, Ns = 2, 2, 3, 4, 5
    m_a, m_b = M.draws(B, nr, nt, L, Ns, 7, 1, first_row=3)
    for b, r, t, l, s in ((0, 0, 0, 0, 0), (1, 1, 2, 3, 5), (0, 1, 0, 2, 4), (1, 0, 1, 0, 5)):
        p = (((3 + b) * nr + r) * nt + t) * L + l
        w = R.philox(np.uint64(p * (Ns + 1) + s), 1, 7)
        assert int(m_a[b, r, t, l, s]) == int(R.u01(w[0], w[1])[0]) and int(m_b[b, r, t, l, s]) == int(R.u01(w[2], w[3])[0])
    # rows are a pure function of first_row + b, also across the wrap of the 64-bit path number
    assert np.array_equal(M.draws(3, nr, nt, L, Ns, 7, 1, first_row=1)[0][2], m_a[0])
    big = 2 ** 64 - 1
    assert np.array_equal(M.draws(2, 1, 1, 3, 2, 0, 0, first_row=big)[1][1], M.draws(1, 1, 1, 3, 2, 0, 0, first_row=0)[1][0])
    prm = M.params(B, nr, nt, L, Ns, 0.25, -0.125, 7, 1, first_row=3)
    assert prm.shape == (B, nr, nt, L, Ns + 1, 2) and np.all(prm[..., Ns, 0] == -0.125)
    assert np.all(np.abs(prm[..., :Ns, 0]) <= 0.25) and np.all((prm[..., 1] > 0) & (prm[..., 1] <= 1))
    assert np.array_equal(prm[..., 1], m_b * 2.0 ** -53)
    assert np.all(M.params(1, 1, 1, 2, 3, 0.0, 0.0, 0, 0)[..., 0] == 0)


def test_model_phase_reduction_is_exact():
    rs = np.random.RandomState(0)
    n = 400
    nu = 0.5 * np.cos(2 * np.pi * rs.rand(n))
    nu[:8] = [0.5, -0.5, 0.0, 2.0 ** -60, 1 / 3, -0.49999999999999994, 0.25, 1e-300]
    phi = (rs.randint(1, 2 ** 53, n).astype(np.float64) + 1) * 2.0 ** -53
    tau = np.concatenate([[0, 1, 2 ** 52 - 1, 2 ** 40], rs.randint(0, 2 ** 51, n - 4)]).astype(np.int64)
    rho = M.reduced_phase(nu, phi, tau)
    for i in range(n):
        exact = M.reduced_phase_exact(nu[i], phi[i], int(tau[i]))
        d = abs(Fraction(*rho[i].as_integer_ratio()) - exact)
        assert min(d, abs(d - 1)) <= Fraction(1, 2 ** 62), (i, nu[i], phi[i], tau[i])
        assert abs(exact) <= Fraction(1, 2)
    # the phasor: exact values at the quadrants, unit modulus elsewhere
    cs, sn = M.phasor(np.array([0, 0.25, 0.5, -0.25, -0.5, 0.125], np.longdouble))
    assert list(cs[:5]) == [1, 0, -1, 0, -1] and list(sn[:5]) == [0, 1, 0, -1, 0]
    assert abs(cs[5] - np.sqrt(0.5)) <= 2.0 ** -53 and abs(sn[5] - np.sqrt(0.5)) <= 2.0 ** -53


def test_model_gains_against_loops():
    B, nr, nt, Ns = 2, 1, 2, 3
    pdp, kf = np.array([0.5, 0.0, 0.25, 2.0]), np.array([0.0, 3.0, 0.0, 1e6])
    prm = M.params(B, nr, nt, 4, Ns, 0.05, 0.01, 5, 9)
    taus = [0, 7, 123456789]
    G = M.gains_from_params(prm, pdp, kf, taus)
    assert G.shape == (B, 3, nr, nt, 4)
    for b in range(B):
        for j, tau in enumerate(taus):
            for t in range(nt):
                for l in range(4):
                    z = sum(np.exp(2j * np.pi * float(M.reduced_phase_exact(prm[b, 0, t, l, s, 0], prm[b, 0, t, l, s, 1], tau))) for s in range(Ns))
                    want = np.sqrt(pdp[l] / ((1 + kf[l]) * Ns)) * z
                    if kf[l] > 0:
                        want += np.sqrt(pdp[l] * kf[l] / (1 + kf[l])) * np.exp(
                            2j * np.pi * float(M.reduced_phase_exact(prm[b, 0, t, l, Ns, 0], prm[b, 0, t, l, Ns, 1], tau)))
                    assert abs(G[b, j, 0, t, l] - want) <= 1e-14 * (1 + abs(want))
    zero = G[..., 1]
    assert np.all(zero == 0) and not np.any(np.signbit(zero.real) | np.signbit(zero.imag))
    assert np.array_equal(M.gains(B, nr, nt, pdp, 0.05, 3, hold=7, t0=0, Ns=Ns, kf=kf, fd_los=0.01, seed=5, stream=9)[:, :2], G[:, :2])
    bound = M.gain_bound(pdp, kf, Ns, 0.05, 0.01, taus, 2.0)
    assert bound.shape == (3, 4) and np.all(bound[:, [0, 2, 3]] > 0) and np.all(bound < 1e-6)


def test_model_convolution_against_loops():
    rs = np.random.RandomState(2)
    B, nt, nr, n, L, hold = 2, 2, 3, 23, 4, 5
    nblk = -(-(n + L - 1) // hold)
    x, G = cplx(rs, B, nt, n), cplx(rs, B, nblk, nr, nt, L)
    y = M.convolve(x, G, hold)
    want = np.zeros_like(y)
    for b in range(B):
        for r in range(nr):
            for m in range(n + L - 1):
                for t in range(nt):
                    for l in range(L):
                        if 0 <= m - l < n:
                            want[b, r, m] += G[b, m // hold, r, t, l] * x[b, t, m - l]
    assert np.max(np.abs(y - want)) < 1e-13
    assert np.array_equal(M.convolve(x, G[0], hold), M.convolve(x, np.stack([G[0], G[0]]), hold))
    assert M.convolve_bound(x, G, hold).shape == y.shape
    # static taps: the convolution of the static channel, for every hold
    import ofdm_chan_model as OC
    for h in (1, 3, 26, 1000):
        nb = -(-(n + L - 1) // h)
        assert np.max(np.abs(M.convolve(x, np.repeat(G[:, :1], nb, axis=1), h) - OC.multipath(x, G[:, 0]))) < 1e-13
    assert M.conv_kernel(1, 1, 1, 1, 1, 1) == "fading_direct_kernel" and M.conv_kernel(2, 2, 3, 1000, 17, 1024) == "fading_tiled_kernel<4>"
    assert M.conv_kernel(2, 2, 3, 1000, 17, 1) == "fading_direct_kernel" and M.conv_kernel(1, 1, 1, 2100, 600, 2700) == "fading_tiled_kernel<1>"


@pytest.mark.parametrize("seed, stream", [(0, 0), (7, 1)])
def test_model_statistics(seed, stream):
    """Clarke's model: E[G(tau0 + d) conj(G(tau0))] / pdp = J0(2 pi fd d).  Over P = 16384 independent paths each product has mean J0 and
    variance <= 1: 6 standard errors = 6 / sqrt(P) = 0.047 (a NumPy-RNG run of the same estimator gave 0.011 to 0.012)."""
    B, L, Ns, fd, t0 = 1024, 16, 16, 0.01, 1000
    pdp = np.full(L, 1.0 / L)
    P = B * L
    tol = 6 / np.sqrt(P)
    prm = M.params(B, 1, 1, L, Ns, fd, 0.0, seed, stream)
    G = M.gains_from_params(prm, pdp, None, [t0 + d for d in M.STAT_DELTAS])
    for i, d in enumerate(M.STAT_DELTAS):
        ac = M.autocorrelation(G[:, 0], G[:, i], pdp)
        assert abs(ac - j0(2 * np.pi * fd * d)) <= tol, (d, ac)
    assert abs(np.mean(np.abs(G[:, 0]) ** 2 / pdp) - 1) <= tol


def test_tap_frequency_response():
    rs = np.random.RandomState(3)
    nfft, nsc, L = 64, 52, 5
    G = cplx(rs, 2, 3, 2, 2, L)
    H = tap_frequency_response(G, nfft, nsc)
    assert H.shape == (2, 3, 2, 2, nsc) and H.dtype == np.complex128
    f = ofdm_subcarrier_frequencies(nsc)
    want = sum(G[..., l, None] * np.exp(-2j * np.pi * f * l / nfft) for l in range(L))
    assert np.max(np.abs(H - want)) < 1e-13
    # against the DFT of the zero-padded taps
    full = np.fft.fft(np.concatenate([G[0, 0, 0, 0], np.zeros(nfft - L)]))
    assert np.max(np.abs(H[0, 0, 0, 0] - full[f % nfft])) < 1e-13
    for bad in (lambda: tap_frequency_response(G, 64, 51), lambda: tap_frequency_response(G, 16, 52), lambda: tap_frequency_response(np.zeros(0), 64, 52),
                lambda: tap_frequency_response(np.array(['a']), 64, 52), lambda: tap_frequency_response(G, 64.0, 52)):
        with pytest.raises(ValueError):
            bad()


# ---- names --------------------------------------------------------------------------------------------------------------------------
def test_abi_names():
    text = open(os.path.join(ROOT, "include", "commpy_amd.h")).read()
    assert "#define CPX_FADING_SCRATCH_BYTES %d " % FADING_SCRATCH_BYTES in text
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(cpx_fading_[a-z0-9_]+)\s*\(", text))
    assert declared == set(NAMES) == {s for s in _lib.SYMBOLS if s.startswith("cpx_fading_")}
    lib = _lib.load()
    assert all(hasattr(lib, s) for s in NAMES)
    assert set(channels.__all__) >= {"fading_params_batch", "fading_gains_batch", "fading_convolve_batch", "fading_multipath_batch",
                                     "tap_frequency_response", "FADING_SCRATCH_BYTES"}
    assert {"fading_params_dev", "fading_gains_dev", "fading_convolve_dev", "fading_channel_dev"} <= set(deviceops.__all__)


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def no_device(monkeypatch):
    """Any attempt to load the engine fails the test: the refusals below must come from the host-side checks."""
    def boom(*a, **k):
        raise AssertionError("the engine was touched")
    monkeypatch.setattr(_lib, "load", boom)


def test_python_refusals(no_device):
    pdp = np.ones(4) / 4
    x, x2 = np.zeros((2, 2, 50), complex), np.zeros((2, 50), complex)
    g = lambda **k: fading_gains_batch(**{**dict(B=1, nr=1, nt=1, pdp=pdp, fd=0.01, nblk=3), **k})
    mp = lambda xx=x, **k: fading_multipath_batch(xx, **{**dict(nr=2, pdp=pdp, fd=0.01), **k})
    G = np.zeros((2, 53, 3, 2, 4), complex)
    for bad in (lambda: g(fd=-0.01), lambda: g(fd=0.51), lambda: g(fd=np.nan), lambda: g(fd='a'), lambda: g(fd_los=0.6), lambda: g(fd_los=-0.6),
                lambda: g(n_sin=0), lambda: g(n_sin=257), lambda: g(n_sin=4.0), lambda: g(hold=0), lambda: g(hold=True), lambda: g(t0=-1),
                lambda: g(nblk=0), lambda: g(nblk=2.0), lambda: g(t0=2 ** 52 - 3), lambda: g(hold=2 ** 51, nblk=2), lambda: g(B=-1),
                lambda: g(nr=0), lambda: g(nt=0), lambda: g(pdp=[]), lambda: g(pdp=[[1.0]]), lambda: g(pdp=[-1.0]), lambda: g(pdp=[np.inf]),
                lambda: g(pdp=[np.nan]), lambda: g(pdp=['a']), lambda: g(pdp=[1j]), lambda: g(pdp=np.ones(1025)), lambda: g(nr=2, nt=2, pdp=np.ones(513)),
                lambda: g(k_factor=-1.0), lambda: g(k_factor=[1.0, 2.0]), lambda: g(k_factor=np.inf), lambda: g(k_factor=[0, 1, np.nan, 0]),
                lambda: g(pdp=[1e300], k_factor=1e300), lambda: g(seed=-1), lambda: g(seed=2 ** 64), lambda: g(stream_id=1.5), lambda: g(first_row=-1),
                lambda: fading_params_batch(1, 1, 1, 0, 0.1), lambda: fading_params_batch(1, 1, 1, 4, 0.7), lambda: fading_params_batch(1, 1, 1, 4, 0.1, n_sin=300),
                lambda: fading_params_batch(1, 1, 1, 2000, 0.1),
                lambda: mp(fd=1.0), lambda: mp(want=()), lambda: mp(want=('y', 'h')), lambda: mp(x2), lambda: mp(np.zeros(5)), lambda: mp(np.zeros((1, 2, 0))),
                lambda: mp(np.zeros((1, 0, 5))), lambda: mp(np.zeros((1, 2, 5), dtype='U1')), lambda: mp(hold=0), lambda: mp(t0=2 ** 52 - 10),
                lambda: mp(nr=300), lambda: mp(n_sin=0),
                lambda: fading_convolve_batch(x, G, 0), lambda: fading_convolve_batch(x, G, 2), lambda: fading_convolve_batch(x, G[:1], 1),
                lambda: fading_convolve_batch(x, G[..., :1, :], 1), lambda: fading_convolve_batch(x, G[0, :, 0], 1), lambda: fading_convolve_batch(x2, G, 1),
                lambda: fading_convolve_batch(x, np.zeros((53, 3, 2, 0)), 1), lambda: fading_convolve_batch(x, np.zeros((2, 1, 2, 2, 513)), 10 ** 6),
                lambda: fading_convolve_batch(x, np.zeros((53, 3, 2, 4), dtype='U1'), 1), lambda: fading_convolve_batch(x, G, 1.0),
                lambda: deviceops.fading_gains_dev(1, 1, 1, pdp, 0.9, 3), lambda: deviceops.fading_params_dev(1, 1, 1, 0, 0.1),
                lambda: deviceops.fading_channel_dev(None, 1, 1, 1, 0, pdp, 0.1), lambda: deviceops.fading_channel_dev(None, 1, 1, 1, 8, pdp, 0.1, want='x')):
        with pytest.raises(ValueError):
            bad()
    # empty batches need no device
    assert fading_gains_batch(0, 2, 3, pdp, 0.1, 5).shape == (0, 5, 2, 3, 4)
    assert fading_params_batch(0, 2, 3, 4, 0.1, n_sin=8).shape == (0, 2, 3, 4, 9, 2)
    assert fading_convolve_batch(np.zeros((0, 2, 50)), G[:0], 1).shape == (0, 3, 53)
    y, Ge = fading_multipath_batch(np.zeros((0, 2, 50)), 3, pdp, 0.1, hold=10, want=('y', 'g'))
    assert y.shape == (0, 3, 53) and Ge.shape[0] == 0 and Ge.shape[2:] == (3, 2, 4)
    assert fading_multipath_batch(np.zeros((0, 50)), 1, pdp, 0.1).shape == (0, 53)


def test_engine_checks_without_device():
    """The C entry points: argument errors are reported before the device is looked for; a valid call fails loudly without one."""
    lib = _lib.load()
    buf = np.zeros(1 << 16)
    pdp, kf = np.ones(4) / 4, np.array([0.0, 1.0, 0.0, 2.0])
    P = _lib.ptr
    E, Lm = _lib.CPX_EINVAL, _lib.CPX_ELIMIT

    def params(B=1, nr=1, nt=1, L=4, ns=4, fd=0.1, fl=0.0, out=P(buf)):
        return lib.cpx_fading_params(B, nr, nt, L, ns, fd, fl, 0, 0, 0, out)

    def gains(B=1, nr=1, nt=1, L=4, p=P(pdp), k=P(kf), ns=4, fd=0.1, fl=0.0, hold=1, t0=0, nblk=3, out=P(buf)):
        return lib.cpx_fading_gains(B, nr, nt, L, p, k, ns, fd, fl, hold, t0, nblk, 0, 0, 0, out)

    def conv(x=P(buf), g=P(buf), gb=0, B=1, nt=1, nr=1, n=8, L=4, hold=1, y=P(buf[4096:])):
        return lib.cpx_fading_convolve(x, g, gb, B, nt, nr, n, L, hold, y)

    def chan(x=P(buf), B=1, nt=1, nr=1, n=8, L=4, p=P(pdp), k=P(kf), ns=4, fd=0.1, fl=0.0, hold=1, t0=0, y=P(buf[4096:]), g=None):
        return lib.cpx_fading_channel(x, B, nt, nr, n, L, p, k, ns, fd, fl, hold, t0, 0, 0, 0, y, g)

    for call in (params, gains, chan):
        for kw in (dict(B=-1), dict(nr=0), dict(nt=0), dict(L=0), dict(ns=0), dict(fd=-0.1), dict(fd=0.6), dict(fd=np.nan), dict(fl=0.6), dict(fl=-0.6)):
            assert call(**kw) == E and _lib.last_error().startswith("fading_"), kw
        for kw in (dict(L=1025), dict(nr=2, nt=2, L=513), dict(ns=257)):
            assert call(**kw) == Lm, kw
    assert params(out=None) == E and _lib.last_error() == "fading_params: null pointer"
    for call in (gains, chan):
        for kw in (dict(hold=0), dict(t0=-1), dict(t0=2 ** 52), dict(hold=2 ** 52), dict(p=None)):
            assert call(**kw) == E, kw
        for bad in ([1, -1, 1, 1], [1, np.inf, 1, 1], [np.nan, 1, 1, 1]):
            arr = np.array(bad, float)
            assert call(p=P(arr)) == E and "pdp[" in _lib.last_error()
            assert call(k=P(arr)) == E and "kf[" in _lib.last_error()
    assert gains(nblk=0) == E and gains(t0=2 ** 52 - 3, nblk=3) == E and gains(hold=2 ** 50, nblk=4) == E and "2^52" in _lib.last_error()
    assert gains(out=None) == E and _lib.last_error() == "fading_gains: null pointer"
    assert chan(n=0) == E and chan(t0=2 ** 52 - 5) == E
    assert chan(y=None, g=None) == E and _lib.last_error() == "fading_channel: no output requested"
    assert chan(B=0, y=None, g=None) == E
    assert chan(x=None) == E and _lib.last_error() == "fading_channel: null pointer"
    for kw in (dict(B=-1), dict(nt=0), dict(nr=0), dict(L=0), dict(n=0), dict(hold=0), dict(gb=2), dict(x=None), dict(g=None), dict(y=None),
               dict(B=2 ** 40, n=2 ** 40)):
        assert conv(**kw) == E and _lib.last_error().startswith("fading_convolve:"), kw
    assert conv(L=1025) == Lm and conv(nt=2, nr=2, L=513) == Lm
    # empty batches succeed without a device, in both forms
    assert params(B=0, out=None) == _lib.CPX_OK and gains(B=0, p=None, out=None) == _lib.CPX_OK
    assert conv(B=0, x=None, g=None, y=None) == _lib.CPX_OK and chan(B=0, x=None, p=None) == _lib.CPX_OK
    assert lib.cpx_fading_params_dev(0, 1, 1, 4, 4, 0.1, 0.0, 0, 0, 0, None, None) == _lib.CPX_OK
    assert lib.cpx_fading_gains_dev(0, 1, 1, 4, None, None, 4, 0.1, 0.0, 1, 0, 3, 0, 0, 0, None, None) == _lib.CPX_OK
    assert lib.cpx_fading_convolve_dev(None, None, 0, 0, 1, 1, 8, 4, 1, None, None) == _lib.CPX_OK
    assert lib.cpx_fading_channel_dev(None, 0, 1, 1, 8, 4, None, None, 4, 0.1, 0.0, 1, 0, 0, 0, 0, P(buf), None, None) == _lib.CPX_OK
    # the _dev forms refuse as the host forms do
    assert lib.cpx_fading_gains_dev(1, 1, 1, 4, P(pdp), None, 300, 0.1, 0.0, 1, 0, 3, 0, 0, 0, P(buf), None) == Lm
    assert lib.cpx_fading_convolve_dev(P(buf), P(buf), 0, 1, 1, 1, 8, 4, 0, P(buf), None) == E
    assert lib.cpx_fading_channel_dev(P(buf), 1, 1, 1, 8, 4, P(pdp), None, 4, 0.7, 0.0, 1, 0, 0, 0, 0, P(buf), None, None) == E
    if _lib.device_count() > 0:
        return
    for rc in (params(), gains(), conv(), chan(), chan(g=P(buf[8192:]))):
        assert rc == _lib.CPX_ENODEV and _lib.last_error().startswith("no HIP device available")


def test_entry_points_fail_loudly_without_device():
    if _lib.device_count() > 0:
        pytest.skip("a HIP device is present")
    pdp = np.ones(4) / 4
    x = np.zeros((2, 2, 300), complex)
    for call in (lambda: fading_params_batch(2, 1, 1, 4, 0.1), lambda: fading_gains_batch(2, 2, 2, pdp, 0.01, 5, hold=80),
                 lambda: fading_convolve_batch(x, np.zeros((4, 3, 2, 4)), 100), lambda: fading_multipath_batch(x, 3, pdp, 0.01, hold=80),
                 lambda: fading_multipath_batch(x[:, 0], 1, pdp, 0.01, want=('y', 'g'))):
        with pytest.raises(_lib.EngineError):
            call()
