"""The linear MIMO detectors without a GPU: the NumPy model of tests/mimo_linear_model.py against an exact rational solve and the
textbook identities, the refusals of the Python layer and of the C-ABI (which come before any device is touched), and the plans
DeviceMimoLink accepts and refuses for the new detector strings."""
import numpy as np
import pytest

import mimo_linear_model as L
from commpy_amd import _lib, devicelink
from commpy_amd.channels import MIMOFlatChannel
from commpy_amd.devicelink import DeviceMimoLink
from commpy_amd.links import mimo_receiver
from commpy_amd.modulation import (Modem, QAMModem, linear_batch, linear_equalize_batch, mmse_detector, zf_detector)
from helpers import ldpc_params

Q16 = QAMModem(16)


def _chan(nr=4, nt=4, kind=complex):
    ch = MIMOFlatChannel(nt, nr)
    ch.uncorr_rayleigh_fading(kind)
    return ch


@pytest.fixture
def no_engine(monkeypatch):
    """Any use of the engine fails the test: refusals must come first."""
    def refuse():
        raise AssertionError('the engine was loaded before the arguments were checked')
    monkeypatch.setattr(_lib, 'load', refuse)
    monkeypatch.setattr(_lib, 'require_device', refuse)


# ---- the model ---------------------------------------------------------------------------------------------------------------------

def test_model_against_the_exact_solve():
    """The float64 model against exact rational arithmetic on 64 seeded vectors: the measured worst ratio is the one the model
    file records, and the kernels' bound is four times it, rounded up to a power of two."""
    rx, rn, count = L.measure_model_ratio()
    print("model / exact: xhat %.4g, nu %.4g of nt nr 2^-52 kappa(A), %d vectors" % (rx, rn, count))
    assert count == 64
    worst = max(rx, rn)
    assert worst <= L.MODEL_RATIO and worst > L.MODEL_RATIO / 2        # the recorded figure is the measured one
    assert L.K_BOUND == 2.0 ** np.ceil(np.log2(4 * L.MODEL_RATIO))


def test_const_of_is_the_modems_constellation():
    for m in (4, 16, 64):
        assert np.array_equal(L.const_of(m), QAMModem(m).constellation)
    assert np.array_equal(L.const_of(2), L.BPSK)


@pytest.mark.parametrize("nr,nt", [(4, 4), (6, 3), (8, 8)])
def test_zf_on_noise_free_input_returns_x(nr, nt):
    const = L.const_of(16)
    y, h = L.conditioned_inputs(5, 40, nr, nt, const, False, 8.0, noise=0.0)
    rs = np.random.RandomState(5)
    x = const[rs.randint(0, 16, (40, nt))]
    y = np.matmul(h, x[:, :, None])[:, :, 0]
    out = L.linear_model(y, h, const, 0.0, 0.1)
    assert not out["bad"].any()
    assert np.all(L.rel_err(out["xhat"], x) <= L.K_BOUND * nt * nr * L.EPS * L.kappa(h, 0.0) + 8 * L.EPS)
    assert np.array_equal(const[out["idx"]], x)
    # nu = noise_var * diag((H^H H)^-1)
    want = 0.1 * np.array([np.linalg.inv(hb.conj().T.dot(hb)).diagonal().real for hb in h])
    assert np.allclose(out["nu"], want, rtol=1e-9, atol=0)


def test_mmse_tends_to_zf_as_reg_vanishes():
    const = L.const_of(16)
    y, h = L.conditioned_inputs(6, 30, 5, 4, const, False, 8.0)
    zf = L.linear_model(y, h, const, 0.0, 0.2)
    gaps = []
    for reg in (1e-3, 1e-6, 1e-9):
        mm = L.linear_model(y, h, const, reg, 0.2)
        gaps.append(max(L.rel_err(mm["xhat"], zf["xhat"]).max(), L.rel_err(mm["nu"], zf["nu"]).max()))
    assert gaps[0] > gaps[1] > gaps[2] and gaps[2] < 1e-6              # first order in reg (kappa <= 64)


def test_unbiased_gain_is_one():
    """(W H)_ii / (1 - reg a_i) = 1 with W = A^-1 H^H: the estimate's gain on its own stream."""
    const = L.const_of(4)
    for nr, nt, reg in ((4, 4, 0.3), (3, 5, 1.0), (7, 2, 0.05)):
        _, h = L.conditioned_inputs(7, 20, nr, nt, const, False, 6.0)
        for hb in h:
            A = hb.conj().T.dot(hb) + reg * np.eye(nt)
            W = np.linalg.solve(A, hb.conj().T)
            a = np.linalg.inv(A).diagonal().real
            gain = W.dot(hb).diagonal() / (1 - reg * a)
            assert np.allclose(gain, 1.0, rtol=0, atol=1e-9)
            # and the model's xhat of a noise-free one-stream input is that stream's symbol
            x = np.zeros(nt, complex)
            x[0] = const[1]
            out = L.linear_model(hb.dot(x)[None], hb, const, reg, 0.1)
            assert abs(out["xhat"][0, 0] - const[1]) <= 1e-9


def test_model_failures_and_ties():
    const = L.const_of(4)
    y, h = L.conditioned_inputs(8, 6, 3, 3, const, False, 4.0)
    y, h = y.copy(), h.copy()
    y[1, 0] = np.nan
    h[2, 1, 1] = np.inf
    h[3, :, 2] = h[3, :, 0]                                              # exactly singular
    out = L.linear_model(y, h, const, 0.0, 0.1)
    assert list(out["bad"]) == [False, True, True, True, False, False]
    assert np.isnan(out["xhat"][1:4]).all() and np.isnan(out["nu"][1:4]).all() and np.isnan(out["llr"][1:4]).all()
    assert not out["idx"][1:4].any()
    # nt > nr: zero forcing fails, MMSE does not
    y, h = L.conditioned_inputs(9, 4, 2, 3, const, True, 4.0)
    assert L.linear_model(y, h, const, 0.0, 0.1)["bad"].all() and not L.linear_model(y, h, const, 0.5, 0.1)["bad"].any()
    # a tie goes to the lowest index: xhat = 0 is equally far from every QPSK point
    out = L.linear_model(np.zeros((1, 2)), np.eye(2), const, 0.0, 0.1)
    assert not out["idx"].any() and not out["llr"].any() and out["margin"][0] == 0


# ---- refusals of the Python layer ----------------------------------------------------------------------------------------------------

def test_python_refusals_come_before_the_engine(no_engine):
    y, h = np.zeros((3, 4), complex), np.ones((4, 4), complex)
    with pytest.raises(ValueError, match="method"):
        linear_batch(y, h, Q16, 0.1, method='ml')
    with pytest.raises(ValueError, match="output_type"):
        linear_batch(y, h, Q16, 0.1, output_type='list')
    with pytest.raises(ValueError, match="reg"):
        linear_batch(y, h, Q16, 0.1, reg=-1.0)
    with pytest.raises(ValueError, match="reg"):
        linear_batch(y, h, Q16, 0.1, reg=float('nan'))
    with pytest.raises(ValueError, match="NaN"):
        linear_batch(y, h, Q16, float('nan'))
    with pytest.raises(ValueError, match="shape mismatch"):
        linear_batch(y, np.ones((3, 4), complex), Q16, 0.1)
    with pytest.raises(ValueError, match="method"):
        linear_equalize_batch(y, h, 0.1, 'mmse2')
    with pytest.raises(ValueError, match="reg"):
        linear_equalize_batch(y, h, 0.1, 'zf', reg=-0.5)
    with pytest.raises(ValueError, match="output_type"):
        zf_detector(y[0], h, Q16.constellation, 0.1, 'both')
    with pytest.raises(ValueError, match="nr, nt"):
        mmse_detector(y[0], np.ones((2, 4, 4)), Q16.constellation, 0.1)
    with pytest.raises(ValueError, match="output_type"):
        mimo_receiver(Q16, 'mmse', output_type='list')
    with pytest.raises(ValueError, match="2\\^num_bits_symbol"):
        md = Modem(np.arange(4.0), reorder_as_gray=False)
        md.m = 3
        linear_batch(y, h, md, 0.1)
    # an empty batch needs no device
    assert linear_batch(np.zeros((0, 4)), h, Q16, 0.1).shape == (0, 4)
    assert linear_batch(np.zeros((0, 4)), h, Q16, 0.1, 'zf', 'soft').shape == (0, 16)
    xh, nu = linear_equalize_batch(np.zeros((0, 4)), h, 0.1, 'zf')
    assert xh.shape == nu.shape == (0, 4) and xh.dtype == np.complex128


def test_existing_receiver_refusals_are_unchanged(no_engine):
    for kw in (dict(detector='viterbi'), dict(detector='ml', output_type='soft'), dict(detector='kbest', output_type='list')):
        with pytest.raises(ValueError, match="detector must be 'kbest'"):
            mimo_receiver(Q16, **kw)
    assert mimo_receiver(Q16, 'zf').batched and mimo_receiver(Q16, 'mmse', output_type='soft').batched


# ---- refusals of the C-ABI, and no result without a device ---------------------------------------------------------------------------

def test_c_abi_refusals_without_device():
    lib = _lib.load()
    y, h = np.zeros((2, 2), complex), np.ones((2, 2), complex)
    idx, llr = np.zeros((2, 2), np.int32), np.zeros((2, 4))
    py, ph, pi, pl = _lib.ptr(y), _lib.ptr(h), _lib.ptr(idx), _lib.ptr(llr)
    for fn, tail in ((lib.cpx_mimo_linear, ()), (lib.cpx_mimo_linear_dev, (None,))):
        for reg, nv, outs, word in ((-1.0, 0.1, (pi, None, None, None), "reg"), (float('nan'), 0.1, (pi, None, None, None), "reg"),
                                    (0.0, float('nan'), (None, pl, None, None), "noise_var"),
                                    (0.0, 0.1, (None, None, None, None), "no output")):
            assert fn(None, py, ph, 0, 2, 2, 2, reg, nv, *outs, *tail) == _lib.CPX_EINVAL
            assert word in _lib.last_error(), _lib.last_error()
    # the device form refuses a null modem, an empty batch included (the handle is checked first)
    for B in (2, 0):
        assert lib.cpx_mimo_linear_dev(None, py, ph, 0, B, 2, 2, 0.0, 0.1, pi, None, None, None, None) == _lib.CPX_EINVAL
        assert _lib.last_error() == "mimo_linear: null modem"
    if _lib.device_count() > 0:
        return
    # the host form reaches ensure_device() next, as cpx_mimo_ml and the K-best forms do
    for B in (2, 0):
        assert lib.cpx_mimo_linear(None, None, None, 0, B, 2, 2, 0.0, 0.1, pi, None, None, None) == _lib.CPX_ENODEV
        assert _lib.last_error().startswith("no HIP device available (")


def test_no_result_without_device():
    if _lib.device_count() > 0:
        pytest.skip("a HIP device is present")
    y, h = np.zeros((3, 4), complex), np.ones((4, 4), complex)
    for call in (lambda: linear_batch(y, h, Q16, 0.1), lambda: linear_batch(y, h, Q16, 0.1, 'zf', 'soft'),
                 lambda: linear_equalize_batch(y, h, 0.1, 'mmse'), lambda: zf_detector(y[0], h, Q16.constellation, 0.1),
                 lambda: mmse_detector(y[0], h, Q16.constellation, 0.1, 'soft'),
                 lambda: mimo_receiver(Q16, 'mmse')(y, h, Q16.constellation, 0.1),
                 lambda: DeviceMimoLink(Q16, _chan(), detector='mmse')):
        with pytest.raises(_lib.EngineError):
            call()


# ---- DeviceMimoLink._plan ------------------------------------------------------------------------------------------------------------

def _plan(modem, channel, detector, output_type, ldpc=None, send_chunk=720, **idd):
    link = DeviceMimoLink.__new__(DeviceMimoLink)
    link.modem, link.channel, link.K = modem, channel, 16
    link._plan(detector, output_type, (1, 3, 5), ldpc, 'MSA', send_chunk, *idd.get('idd', ()))
    return link


@pytest.mark.parametrize("detector", ['zf', 'mmse'])
def test_plan_accepts_the_linear_detectors(detector):
    link = _plan(Q16, _chan(), detector, 'hard')
    assert not link.coded and link.vectors_per_tx == 45 and link.stacks is None
    link = _plan(Q16, _chan(), detector, 'soft', ldpc_params("wimax1440"))
    assert link.coded and (link.k, link.n) == (720, 1440) and link.vectors_per_tx == 90
    # shapes the tree searches refuse: more columns than rows, one receive antenna
    assert _plan(QAMModem(4), _chan(3, 4), detector, 'hard', send_chunk=16).vectors_per_tx == 2
    assert _plan(QAMModem(4), _chan(1, 1), detector, 'hard', send_chunk=16).vectors_per_tx == 8
    assert _plan(QAMModem(4), _chan(12, 12), detector, 'hard', send_chunk=48).vectors_per_tx == 2


LINEAR_REFUSED = [
    dict(detector='zf', output_type='soft'),                             # soft output without a code
    dict(detector='mmse', output_type='soft'),
    dict(detector='zf', output_type='hard', ldpc=True),                  # hard output into a decoder
    dict(detector='mmse', ldpc=True),
    dict(detector='mmse', output_type='list'),
    dict(detector='mmse', output_type='soft', ldpc=True, idd_iters=1),   # IDD stays the list detector's
    dict(detector='zf', output_type='soft', ldpc=True, idd_iters=2),
    dict(detector='mmse', kind=float),                                   # real channel
    dict(detector='zf', nr=48, nt=48),                                   # one vector's state above the wave kernel's LDS
    dict(detector='mmse', output_type='soft', ldpc=True, send_chunk=1000),
]


@pytest.mark.parametrize("case", LINEAR_REFUSED, ids=[str(i) for i in range(len(LINEAR_REFUSED))])
def test_link_refusals_come_before_the_engine(monkeypatch, case):
    def refuse():
        raise AssertionError('the engine was loaded before the arguments were checked')
    monkeypatch.setattr(devicelink._lib, 'load', refuse)
    monkeypatch.setattr(devicelink._lib, 'require_device', refuse)
    case = dict(case)
    ch = _chan(case.pop('nr', 4), case.pop('nt', 4), case.pop('kind', complex))
    if case.pop('ldpc', False):
        case['ldpc_params'] = ldpc_params("wimax1440")
    with pytest.raises(ValueError):
        DeviceMimoLink(Q16, ch, **case)
