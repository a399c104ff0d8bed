"""The equaliser's NumPy model (tests/mlse_model.py) against enumeration of all M^n sequences, the refusals of the Python layer and of
the C-ABI, and the loud failure without a device.  CPU only.

Bounds.  A row's cost is a sum of n_y terms |y_t - xh_t|^2 with |y_t - xh_t| <= |y_t| + max|c| sum|h_l| =: r_t.  xh_t is a sum of at most L
complex products (relative error below (L + 2) u each way), the square and the running sum add (n_y + 3) u, the prior's cost and the
forward / backward split a few more; with u = 2^-53 the two evaluations -- the model's and the enumeration's -- differ by less than
(n_y + 4 L + 8) 2^-52 sum_t r_t^2.  An LLR is the difference of
two such minima over noise_var: twice that bound over noise_var."""
import numpy as np
import pytest

import mlse_model as M
from commpy_amd import _lib, deviceops
from commpy_amd.equalizers import mlse_equalize_batch
from commpy_amd.modulation import Modem, PSKModem, QAMModem
from mlse_model import draw

MODEMS = {2: lambda: PSKModem(2), 4: lambda: QAMModem(4), 8: lambda: PSKModem(8)}
GRID = [(m, L) for m in (2, 4, 8) for L in (2, 3, 4, 5) if m ** (L - 1) <= 256]
VARIANTS = (('tail', True, False), ('head', False, False), ('prior', True, True))


def metric_bound(y, h, const):
    L = h.shape[-1]
    r = np.abs(y) + np.abs(const).max() * np.abs(h).sum()
    return (y.size + 4 * L + 8) * 2.0 ** -52 * float((r * r).sum())


def test_model_equals_enumeration():
    left_out, worst_metric, worst_llr, cases = 0, 0.0, 0.0, 0
    for m, L in GRID:
        modem = MODEMS[m]()
        const = modem.constellation
        for n in range(1, 9):
            for name, tail, with_prior in VARIANTS:
                seed = 1000 * m + 100 * L + 10 * n + len(name)
                idx, y, h = draw(modem, L, n, 1, seed, tail)
                rs = np.random.RandomState(seed + 7)
                nv = 0.3 + rs.rand()
                prior = 2.0 * rs.randn(1, n * modem.num_bits_symbol) if with_prior else None
                got = M.equalize(y, h, const, nv, prior, tail, soft=True)
                cost, llr = M.brute_force(y[0], h[0], const, nv, None if prior is None else prior[0], tail)
                bound = metric_bound(y[0], h[0], const)
                flat = np.sort(cost.reshape(-1))
                cases += 1
                if flat.size > 1 and flat[1] - flat[0] <= bound:
                    left_out += 1
                    continue
                best = np.unravel_index(int(np.argmin(cost)), cost.shape)
                assert got['indices'][0].tolist() == list(best), (m, L, n, name)
                assert got['bits'][0].tolist() == [(a >> (modem.num_bits_symbol - 1 - i)) & 1 for a in best
                                                   for i in range(modem.num_bits_symbol)]
                err = abs(got['metric'][0] - flat[0])
                assert err <= bound, (m, L, n, name, err, bound)
                worst_metric = max(worst_metric, err / bound)
                lerr = np.abs(got['llr'][0] - llr).max()
                assert lerr <= 2 * bound / nv, (m, L, n, name, lerr, 2 * bound / nv)
                worst_llr = max(worst_llr, lerr / (2 * bound / nv))
                # the metric is not above the metric of the transmitted sequence
                assert got['metric'][0] <= cost[tuple(idx[0])] + bound
    print("mlse model against enumeration: %d cases, %d left out, worst metric error %.3g of the bound, worst LLR error %.3g of its bound"
          % (cases, left_out, worst_metric, worst_llr))
    assert cases == 240 and left_out == 0


def test_model_options_agree():
    """Shared and per-row taps, scalar and per-row noise_var, hard and soft calls give the same rows; a rejected row stays in its row."""
    modem = QAMModem(4)
    idx, y, h = draw(modem, 3, 12, 5, 3)
    prior = np.random.RandomState(4).randn(5, 24)
    full = M.equalize(y, h, modem.constellation, np.full(5, 0.7), prior, soft=True)
    for b in range(5):
        one = M.equalize(y[b], h[b], modem.constellation, 0.7, prior[b], soft=True)
        for key in ('indices', 'bits', 'metric', 'llr'):
            assert np.array_equal(one[key][0], full[key][b])
    hard = M.equalize(y, h, modem.constellation, np.full(5, 0.7), prior)
    assert 'llr' not in hard and all(np.array_equal(hard[k], full[k]) for k in hard)
    y2, h2, nv2, prior2 = y.copy(), h.copy(), np.full(5, 0.7), prior.copy()
    y2[0, 3], h2[1, 0], nv2[2], prior2[3, 5] = np.nan, np.inf, np.inf, -np.inf
    rej = M.equalize(y2, h2, modem.constellation, nv2, prior2, soft=True)
    assert not rej['indices'][:4].any() and not rej['bits'][:4].any()
    assert np.isnan(rej['metric'][:4]).all() and np.isnan(rej['llr'][:4]).all()
    for key in ('indices', 'bits', 'metric', 'llr'):
        assert np.array_equal(rej[key][4], full[key][4])
    # without a prior the sign of an LLR agrees with the bit: positive = bit 0
    free = M.equalize(y, h, modem.constellation, 0.7, None, soft=True)
    assert np.array_equal(free['llr'] < 0, free['bits'] == 1) and (free['llr'] != 0).all()


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def no_device(monkeypatch):
    """Any attempt to load the engine fails the test: the refusals below must come from the host-side checks."""
    def boom(*a, **k):
        raise AssertionError("the engine was touched")
    monkeypatch.setattr(_lib, "load", boom)


def test_python_refusals(no_device):
    bpsk, qpsk, psk8, qam16, qam64 = PSKModem(2), QAMModem(4), PSKModem(8), QAMModem(16), QAMModem(64)
    y, buf = np.zeros((2, 20), complex), object()
    h = lambda L: np.ones(L, complex)
    for bad, limit in (
            (lambda: mlse_equalize_batch(y, h(1), bpsk), 'L >= 2'),
            (lambda: mlse_equalize_batch(y, h(2), qam64), 'M <= 16'),
            (lambda: mlse_equalize_batch(y, h(10), bpsk), 'M^(L-1) <= 256'),
            (lambda: mlse_equalize_batch(y, h(6), qpsk), 'M^(L-1) <= 256'),
            (lambda: mlse_equalize_batch(y, h(4), psk8), 'M^(L-1) <= 256'),
            (lambda: mlse_equalize_batch(y, h(4), qam16), 'M^(L-1) <= 256'),
            (lambda: mlse_equalize_batch(np.zeros((2, 2), complex), h(3), bpsk), '1 <= n <= 4096'),
            (lambda: mlse_equalize_batch(np.zeros((1, 4098), complex), h(2), bpsk), '1 <= n <= 4096'),
            (lambda: mlse_equalize_batch(np.zeros((1, 4097), complex), h(2), bpsk, tail=False), '1 <= n <= 4096'),
            (lambda: mlse_equalize_batch(np.zeros((2, 3, 4), complex), h(2), bpsk), '1-D'),
            (lambda: mlse_equalize_batch(y, np.ones((3, 2), complex), bpsk), 'h must be'),
            (lambda: mlse_equalize_batch(y, np.ones((1, 2, 2), complex), bpsk), 'h must be'),
            (lambda: mlse_equalize_batch(y.astype(str), h(2), bpsk), 'numbers'),
            (lambda: mlse_equalize_batch(y, h(2), bpsk, want='llr'), 'noise_var is required'),
            (lambda: mlse_equalize_batch(y, h(2), bpsk, a_priori=np.zeros((2, 19))), 'noise_var is required'),
            (lambda: mlse_equalize_batch(y, h(2), bpsk, 0.0, want='llr'), 'positive'),
            (lambda: mlse_equalize_batch(y, h(2), bpsk, np.array([1.0, -1.0]), want='llr'), 'positive'),
            (lambda: mlse_equalize_batch(y, h(2), bpsk, np.ones(3), want='llr'), 'scalar or [B]'),
            (lambda: mlse_equalize_batch(y, h(2), bpsk, 1.0, a_priori=np.zeros((2, 20))), 'a_priori must be'),
            (lambda: mlse_equalize_batch(y, h(2), qpsk, 1.0, a_priori=np.zeros((2, 19))), 'a_priori must be'),
            (lambda: mlse_equalize_batch(y, h(2), bpsk, want=()), 'want'),
            (lambda: mlse_equalize_batch(y, h(2), bpsk, want=('indices', 'symbols')), 'want'),
            (lambda: deviceops.mlse_equalize_dev(bpsk, buf, buf, False, 2, 19, 1), 'L'),
            (lambda: deviceops.mlse_equalize_dev(bpsk, buf, buf, False, -1, 19, 2), 'B'),
            (lambda: deviceops.mlse_equalize_dev(bpsk, buf, buf, False, 2, 0, 2), 'n'),
            (lambda: deviceops.mlse_equalize_dev(bpsk, buf, buf, False, 2, 4097, 2), '1 <= n <= 4096'),
            (lambda: deviceops.mlse_equalize_dev(qam64, buf, buf, False, 2, 19, 2), 'M <= 16'),
            (lambda: deviceops.mlse_equalize_dev(qam16, buf, buf, False, 2, 19, 4), 'M^(L-1) <= 256'),
            (lambda: deviceops.mlse_equalize_dev(bpsk, buf, buf, False, 2, 19, 2, want='llr'), 'noise_var is required'),
            (lambda: deviceops.mlse_equalize_dev(bpsk, buf, buf, False, 2, 19, 2, d_prior=buf), 'noise_var is required'),
            (lambda: deviceops.mlse_equalize_dev(bpsk, buf, buf, False, 2, 19, 2, want='soft'), 'want')):
        with pytest.raises(ValueError) as err:
            bad()
        assert limit in str(err.value), (limit, str(err.value))
    # a duck-typed modem whose point count is no power of two is refused on the host as well
    class Six:
        m, num_bits_symbol, constellation = 6, 2, np.ones(6, complex)
    with pytest.raises(ValueError) as err:
        mlse_equalize_batch(y, h(2), Six())
    assert 'power of two' in str(err.value)
    # a one-point constellation has no trellis
    with pytest.raises(ValueError) as err:
        mlse_equalize_batch(y, h(2), Modem(np.array([1.0]), reorder_as_gray=False))
    assert '2 <= M' in str(err.value)


def test_c_abi_refuses_before_a_device_is_looked_for():
    lib = _lib.load()
    assert lib.cpx_mlse(None, None, None, 0, 2, 10, 2, 1, None, 0, None, None, None, None, None) == _lib.CPX_EINVAL
    assert _lib.last_error() == "mlse: null pointer"
    assert lib.cpx_mlse_dev(None, None, None, 0, 2, 10, 2, 1, None, 0, None, None, None, None, None, None) == _lib.CPX_EINVAL


def test_fails_loudly_without_a_device():
    if _lib.device_count() > 0:
        pytest.skip("a HIP device is present")
    with pytest.raises(_lib.EngineError):
        mlse_equalize_batch(np.zeros((2, 11), complex), np.ones(2, complex), PSKModem(2))
