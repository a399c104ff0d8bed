"""The MMSE equalisers' NumPy model (tests/equalize_model.py) against a direct solve of its own normal equations, the Wiener property,
noise-free chains, the LE / DFE / MLSE ordering on Proakis' channel B, the refusals of the Python layer and of the C-ABI.  CPU only.

Bound.  The model solves R u = p by an L D L^H factorisation in float64.  A backward-stable solve of an nf x nf Hermitian positive
definite system has a relative error of the order nf^2 u kappa_2(R), so the comparison is ||ff - ff_np|| / ||ff_np|| <=
K nf^2 2^-52 kappa_2(R).  K is derived, not fitted to this test: against an exact ``fractions.Fraction`` solve of the same float R and p
on the 36 seeded cases of SHAPES (three seeds each, the draw of ``case``) the model's worst ratio was 0.2473 (at nf = 1; 0.1165 at
nf = 2, below 0.01 from nf = 4 on); four times that, rounded up to a power of two, is K = 1."""
import numpy as np
import pytest

import equalize_model as E
import mlse_model
from commpy_amd import _lib, deviceops
from commpy_amd.equalizers import mlse_equalize_batch, mmse_equalize_batch
from commpy_amd.modulation import PSKModem, QAMModem

K = 1.0
SHAPES = [(1, 1, 0), (2, 2, 0), (4, 2, 1), (8, 3, 0), (8, 3, 2), (16, 3, 0), (16, 3, 2), (24, 3, 0), (24, 3, 2), (12, 8, 7), (32, 8, 0),
          (32, 8, 7)]
CHANNEL_B = np.array([0.407, 0.815, 0.407])


def case(nf, L, nb, seed):
    """``(h [1, L], Es, N0)``: random taps with a clear first one, 5 to 20 dB."""
    rs = np.random.RandomState(1000 * nf + 10 * L + nb + 100 * seed)
    h = (rs.randn(1, L) + 1j * rs.randn(1, L)) / np.sqrt(2 * L)
    h[0, 0] += 1
    N0 = 10 ** (-rs.uniform(0.5, 2.0))
    return h, (1.0 if seed else 2.0), N0


def full(des):
    """``(R, p)`` of a one-row design as complex arrays, the upper triangle filled in."""
    Rr, Ri = des['R']
    R = (Rr + 1j * Ri)[:, :, 0]
    return R + np.tril(R, -1).conj().T, (des['p'][0] + 1j * des['p'][1])[:, 0]


@pytest.fixture(scope="module")
def designs():
    out = []
    for nf, L, nb in SHAPES:
        for seed in range(3):
            h, Es, N0 = case(nf, L, nb, seed)
            des = E.design(h, Es, N0, nf, nb)
            R, p = full(des)
            out.append((nf, L, nb, seed, h, des, R, p, np.linalg.cond(R)))
    return out


def test_model_equals_a_direct_solve(designs):
    worst = 0.0
    for nf, L, nb, seed, h, des, R, p, kappa in designs:
        assert kappa <= 1e4, (nf, L, nb, seed, kappa)
        assert not des['bad'][0]
        ff_np = np.linalg.solve(R, p).conj()
        err = np.linalg.norm(des['ff'][0] - ff_np) / np.linalg.norm(ff_np)
        bound = K * nf * nf * 2.0 ** -52 * kappa
        print("nf=%d L=%d nb=%d seed=%d: kappa %.3g, error %.3g, bound %.3g" % (nf, L, nb, seed, kappa, err, bound))
        assert err <= bound, (nf, L, nb, seed, err, bound)
        worst = max(worst, err / bound)
    print("worst error over bound: %.3g" % worst)


def test_wiener_property(designs):
    """The taps solve the normal equations: ||R u - p|| within the same bound (relative to ||p||); the feedback taps are the
    post-cursor of the combined response, the gain its cursor, and 0 < gain < 1."""
    for nf, L, nb, seed, h, des, R, p, kappa in designs:
        u = des['ff'][0].conj()
        assert np.linalg.norm(R @ u - p) <= K * nf * nf * 2.0 ** -52 * kappa * np.linalg.norm(p), (nf, L, nb, seed)
        d = E.default_delay(nf, nb, L)
        combined = np.convolve(des['ff'][0], h[0])
        assert np.allclose(des['fb'][0], combined[d + 1:d + 1 + nb], rtol=1e-12, atol=1e-15)
        assert abs(des['gain'][0] - combined[d].real) < 1e-12 and abs(combined[d].imag) < 1e-9
        assert 0 < des['gain'][0] < 1 and des['noise'][0] > 0


@pytest.mark.parametrize("M", [4, 16, 64])
@pytest.mark.parametrize("nb", [0, 2])
def test_noise_free_chain_recovers_every_index(M, nb):
    modem = QAMModem(M)
    m = modem.num_bits_symbol
    taps = np.array([1, 0.5, 0.2 + 0.1j])
    for seed in (1, 2, 3):
        bits = np.random.RandomState(seed).randint(0, 2, 500 * m)
        y = np.convolve(modem.modulate(bits), taps)
        got = E.equalize(y, taps, modem.constellation, modem.Es, 1e-6, 24, nb)
        assert np.array_equal(got['bits'][0], bits), (M, nb, seed)
        assert np.array_equal(got['indices'][0], bits.reshape(-1, m).dot(1 << np.arange(m - 1, -1, -1)))
        assert np.array_equal(got['llr'][0] < 0, bits == 1)


def test_ordering_on_channel_b():
    """QPSK at 14 dB through (0.407, 0.815, 0.407), 4000 symbols: the DFE makes fewer symbol errors than the LE, and the trellis
    equaliser no more than the DFE."""
    modem = QAMModem(4)
    rs = np.random.RandomState(14)
    n = 4000
    idx = rs.randint(0, 4, n)
    N0 = modem.Es / 10 ** 1.4
    y = np.convolve(modem.constellation[idx], CHANNEL_B) + np.sqrt(N0 / 2) * (rs.randn(n + 2) + 1j * rs.randn(n + 2))
    le = (E.equalize(y, CHANNEL_B, modem.constellation, modem.Es, N0, 16)['indices'][0] != idx).sum()
    dfe = (E.equalize(y, CHANNEL_B, modem.constellation, modem.Es, N0, 16, 2)['indices'][0] != idx).sum()
    mlse = (mlse_model.equalize(y, CHANNEL_B, modem.constellation)['indices'][0] != idx).sum()
    print("channel B, QPSK, 14 dB, %d symbols: LE %d, DFE %d, MLSE %d symbol errors" % (n, le, dfe, mlse))
    assert dfe < le and mlse <= dfe


def test_64qam_through_eight_taps():
    """Out of the trellis equaliser's reach, within this one's."""
    modem = QAMModem(64)
    rs = np.random.RandomState(8)
    taps = np.array([1.0, 0.4, -0.25j, 0.15, 0.1j, -0.08, 0.05, 0.03])
    idx = rs.randint(0, 64, 200)
    y = np.convolve(modem.constellation[idx], taps)
    with pytest.raises(ValueError):
        mlse_equalize_batch(y, taps, modem)
    for nb in (0, 7):
        got = E.equalize(y, taps, modem.constellation, modem.Es, 1e-5, 32, nb)
        assert np.array_equal(got['indices'][0], idx), nb


def test_model_options_agree():
    """Shared and per-row taps and noise_var give the same rows; a rejected row stays in its row; no bits for six points."""
    modem = QAMModem(16)
    rs = np.random.RandomState(5)
    h = (rs.randn(4, 3) + 1j * rs.randn(4, 3)) / 2
    h[:, 0] += 1
    y = np.stack([np.convolve(modem.constellation[rs.randint(0, 16, 30)], h[b]) for b in range(4)]) + 0.05 * rs.randn(4, 32)
    whole = E.equalize(y, h, modem.constellation, modem.Es, np.full(4, 0.01), 9, 2)
    for b in range(4):
        one = E.equalize(y[b], h[b], modem.constellation, modem.Es, 0.01, 9, 2)
        for key in whole:
            assert np.array_equal(one[key][0], whole[key][b]), key
    y2, h2, nv2 = y.copy(), h.copy(), np.full(4, 0.01)
    y2[0, 31], h2[1, 2], nv2[2] = np.inf, np.nan, np.nan
    h2[3] = 0
    rej = E.equalize(y2[:, :], h2, modem.constellation, modem.Es, nv2, 9, 2)
    assert not rej['indices'].any() and not rej['bits'].any()
    for key in ('estimate', 'llr', 'noise', 'ff', 'fb', 'gain'):
        assert np.isnan(rej[key].real).all() and (rej[key].dtype.kind != 'c' or np.isnan(rej[key].imag).all()), key
    six = E.equalize(y, h, np.exp(2j * np.pi * np.arange(6) / 6), 1.0, 0.01, 9)
    assert 'bits' not in six and 'llr' not in six and six['indices'].max() <= 5


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def no_device(monkeypatch):
    """Any attempt to load the engine fails the test: the refusals below must come from the host-side checks."""
    def boom(*a, **k):
        raise AssertionError("the engine was touched")
    monkeypatch.setattr(_lib, "load", boom)


def test_python_refusals(no_device):
    qpsk = QAMModem(4)
    y, buf = np.zeros((2, 20), complex), object()
    h = lambda L: np.ones(L, complex)

    class Duck:
        num_bits_symbol, Es = 2, 1.0

        def __init__(self, M):
            self.m, self.constellation = M, np.ones(M, complex)
    for bad, limit in (
            (lambda: mmse_equalize_batch(np.zeros((2, 70), complex), h(65), qpsk, 1.0, 4), '1 <= L <= 64'),
            (lambda: mmse_equalize_batch(y, np.ones((2, 0), complex), qpsk, 1.0, 4, tail=False), '1 <= L <= 64'),
            (lambda: mmse_equalize_batch(y, h(3), qpsk, 1.0, 0), '1 <= nf <= 64'),
            (lambda: mmse_equalize_batch(y, h(3), qpsk, 1.0, 65), '1 <= nf <= 64'),
            (lambda: mmse_equalize_batch(y, h(3), qpsk, 1.0, 4, -1), '0 <= nb <= 64'),
            (lambda: mmse_equalize_batch(y, h(3), qpsk, 1.0, 64, 65), '0 <= nb <= 64'),
            (lambda: mmse_equalize_batch(y, h(3), qpsk, 1.0, 4, 0, -1), '0 <= delay'),
            (lambda: mmse_equalize_batch(y, h(3), qpsk, 1.0, 4, 0, 6), 'delay + nb <= nf + L - 2'),
            (lambda: mmse_equalize_batch(y, h(3), qpsk, 1.0, 4, 3), 'delay + nb <= nf + L - 2'),
            (lambda: mmse_equalize_batch(y, h(3), qpsk, 1.0, 4, 2, 4), 'delay + nb <= nf + L - 2'),
            (lambda: mmse_equalize_batch(y, h(3), Duck(1), 1.0, 4), '2 <= M <= 256'),
            (lambda: mmse_equalize_batch(y, h(3), Duck(257), 1.0, 4), '2 <= M <= 256'),
            (lambda: mmse_equalize_batch(y, h(3), Duck(6), 1.0, 4, want='bits'), 'power of two'),
            (lambda: mmse_equalize_batch(y, h(3), Duck(6), 1.0, 4, want=('indices', 'llr')), 'power of two'),
            (lambda: mmse_equalize_batch(np.zeros((2, 2), complex), h(3), qpsk, 1.0, 4), '1 <= n'),
            (lambda: mmse_equalize_batch(np.zeros((2, 0), complex), h(1), qpsk, 1.0, 4), '1 <= n'),
            (lambda: mmse_equalize_batch(y, h(3), qpsk, None, 4), 'noise_var is required'),
            (lambda: mmse_equalize_batch(y, h(3), qpsk, 0.0, 4), 'positive'),
            (lambda: mmse_equalize_batch(y, h(3), qpsk, np.array([1.0, -1.0]), 4), 'positive'),
            (lambda: mmse_equalize_batch(y, h(3), qpsk, np.ones(3), 4), 'scalar or [B]'),
            (lambda: mmse_equalize_batch(np.zeros((2, 3, 4), complex), h(3), qpsk, 1.0, 4), '1-D'),
            (lambda: mmse_equalize_batch(y, np.ones((3, 2), complex), qpsk, 1.0, 4), 'h must be'),
            (lambda: mmse_equalize_batch(y.astype(str), h(3), qpsk, 1.0, 4), 'numbers'),
            (lambda: mmse_equalize_batch(y, h(3), qpsk, 1.0, 4, want=()), 'want'),
            (lambda: mmse_equalize_batch(y, h(3), qpsk, 1.0, 4, want=('indices', 'metric')), 'want'),
            (lambda: deviceops.mmse_equalize_dev(qpsk, buf, buf, False, 2, 18, 65, buf, False, 4), '1 <= L <= 64'),
            (lambda: deviceops.mmse_equalize_dev(qpsk, buf, buf, False, 2, 18, 3, buf, False, 65), '1 <= nf <= 64'),
            (lambda: deviceops.mmse_equalize_dev(qpsk, buf, buf, False, 2, 18, 3, buf, False, 4, 65), '0 <= nb <= 64'),
            (lambda: deviceops.mmse_equalize_dev(qpsk, buf, buf, False, 2, 18, 3, buf, False, 4, 2, 4), 'delay + nb <= nf + L - 2'),
            (lambda: deviceops.mmse_equalize_dev(qpsk, buf, buf, False, -1, 18, 3, buf, False, 4), 'B'),
            (lambda: deviceops.mmse_equalize_dev(qpsk, buf, buf, False, 2, 0, 3, buf, False, 4), 'n'),
            (lambda: deviceops.mmse_equalize_dev(qpsk, buf, buf, False, 2, 18, 3, None, False, 4), 'noise_var is required'),
            (lambda: deviceops.mmse_equalize_dev(Duck(6), buf, buf, False, 2, 18, 3, buf, False, 4, want='llr'), 'power of two'),
            (lambda: deviceops.mmse_equalize_dev(qpsk, buf, buf, False, 2, 18, 3, buf, False, 4, want='metric'), 'want')):
        with pytest.raises(ValueError) as err:
            bad()
        assert limit in str(err.value), (limit, str(err.value))


def test_c_abi_refuses_before_a_device_is_looked_for():
    lib = _lib.load()
    none = (None,) * 8
    assert lib.cpx_mmse_equalize(None, 1.0, None, None, 0, 2, 10, 2, 1, None, 0, 4, 0, 2, *none) == _lib.CPX_EINVAL
    assert _lib.last_error() == "mmse_equalize: null pointer"
    assert lib.cpx_mmse_equalize_dev(None, 1.0, None, None, 0, 2, 10, 2, 1, None, 0, 4, 0, 2, *none, None) == _lib.CPX_EINVAL
    assert _lib.last_error() == "mmse_equalize: null pointer"


def test_fails_loudly_without_a_device():
    if _lib.device_count() == 0:
        with pytest.raises(_lib.EngineError):
            mmse_equalize_batch(np.zeros((2, 11), complex), np.ones(2, complex), PSKModem(2), 0.1, 4)
