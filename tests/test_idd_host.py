"""Host side of iterative detection and decoding: every refusal of list_apriori_batch / apriori_detector /
DeviceMimoLink(idd_iters=...) comes before the engine is touched, the new entry points fail loudly without a device, and the
NumPy model of the list detector with priors reproduces the committed fixture (tests/golden/idd.npz,
tests/golden/make_golden_idd.py)."""
import os
from inspect import getfullargspec

import numpy as np
import pytest

from commpy_amd import _lib, devicelink
from commpy_amd.channels import MIMOFlatChannel
from commpy_amd.devicelink import DeviceMimoLink
from commpy_amd.modulation import QAMModem, apriori_detector, list_apriori_batch
from helpers import ldpc_params

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "idd.npz"))
DET_CASES = sorted({k[4:-2] for k in G.files if k.startswith("det_") and k.endswith("_y")})
Q16 = QAMModem(16)


def list_model(y, h, const, labels, cand, prior, noise_var, clip):
    """The list detector with priors, as tests/golden/make_golden_idd.py states it: cost_c = |y - h x_c|^2 / (2 noise_var) +
    sum_k b_k(c) La_k with La the prior clipped to +-clip; L_k = min_{b_k = 1} cost - min_{b_k = 0} cost (an empty side +inf),
    clipped to +-clip; a NaN in y, h or the prior makes every LLR NaN."""
    la = np.clip(np.asarray(prior, dtype=float), -clip, clip)
    bits = labels[cand].reshape(len(cand), -1).astype(bool)
    if np.isnan(y).any() or np.isnan(h).any() or np.isnan(la).any():
        return np.full(bits.shape[1], np.nan)
    dist = np.linalg.norm(y[:, None] - h.dot(const[cand].T), axis=0) ** 2
    cost = dist / (2 * noise_var) + np.where(bits, la[None, :], 0.0).sum(axis=1)
    out = np.empty(bits.shape[1])
    with np.errstate(invalid="ignore"):
        for k in range(bits.shape[1]):
            one = np.min(np.append(cost[bits[:, k]], np.inf))
            zero = np.min(np.append(cost[~bits[:, k]], np.inf))
            out[k] = one - zero
    return np.clip(out, -clip, clip)


@pytest.fixture
def no_engine(monkeypatch):
    """Any use of the native library fails the test: the checks must come first."""
    def refuse():
        raise AssertionError("the engine was touched")
    monkeypatch.setattr(_lib, "load", refuse)
    monkeypatch.setattr(_lib, "require_device", refuse)


def _chan(nr=4, nt=4):
    ch = MIMOFlatChannel(nt, nr)
    ch.uncorr_rayleigh_fading(complex)
    return ch


def _vec(nr, nt, n=3, seed=0):
    rs = np.random.RandomState(seed)
    h = rs.randn(n, nr, nt) + 1j * rs.randn(n, nr, nt)
    return rs.randn(n, nr) + 1j * rs.randn(n, nr), h


# ---- the model is the committed fixture's -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", DET_CASES)
def test_model_reproduces_the_golden_file(case):
    g = lambda k: G["det_%s_%s" % (case, k)]  # noqa: E731
    const, labels, nv, clip = g("const"), g("labels"), float(g("noise_var")), float(g("clip"))
    for i in range(len(g("y"))):
        cand = g("cand")[i, :g("count")[i]].astype(int)
        post = list_model(g("y")[i], g("h")[i], const, labels, cand, g("prior")[i], nv, clip)
        np.testing.assert_allclose(post, g("post")[i], rtol=1e-12, atol=1e-12)
        zero = list_model(g("y")[i], g("h")[i], const, labels, cand, np.zeros(labels.shape[1] * cand.shape[1]), nv, np.inf)
        np.testing.assert_allclose(zero, g("ref")[i], rtol=1e-9, atol=1e-9)          # La = 0, clip = inf: max_log_approx
    assert (np.abs(g("prior")) > clip).any() and (np.abs(g("post")) == clip).any()


def test_golden_loop_has_no_decision_on_a_knife_edge():
    """The loop anchor's acceptance rule, as its generator asserts it: every stored final LLR exceeds 100 times the chain's
    sensitivity to a 1e-9 relative change of the detector's outputs."""
    sens, smallest = float(G["idd_llr_sensitivity"]), min(np.min(np.abs(G["loop_final_it%d" % n])) for n in (1, 2, 3))
    assert 0 < 100 * sens < smallest
    assert (np.abs(G["loop_final_it3"]) == float(G["loop_clip"])).mean() > 0.05       # bits without a counter-hypothesis stay in


def test_model_edge_semantics():
    g = lambda k: G["det_qam16_4x4_%s" % k]  # noqa: E731
    y, h, const, labels = g("y")[0], g("h")[0], g("const"), g("labels")
    cand = g("cand")[0, :g("count")[0]].astype(int)
    big = np.where(np.arange(16) % 2, 1e6, -1e6)
    assert np.array_equal(list_model(y, h, const, labels, cand, big, 0.25, 500.0),
                          list_model(y, h, const, labels, cand, np.clip(big, -500, 500), 0.25, 500.0))
    bad = np.zeros(16)
    bad[5] = np.nan
    assert np.isnan(list_model(y, h, const, labels, cand, bad, 0.25, 500.0)).all()
    one = list_model(y, h, const, labels, cand[:1], np.zeros(16), 0.25, 7.0)          # one candidate: every bit is +-clip
    assert np.array_equal(one, np.where(labels[cand[0]].reshape(-1), -7.0, 7.0))


# ---- refusals before the engine --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kw", [dict(K=0), dict(K=-3), dict(llr_clip=0.0), dict(llr_clip=-1.0), dict(llr_clip=float("nan")),
                                dict(K=2.5)])
def test_list_apriori_argument_checks(no_engine, kw):
    y, h = _vec(4, 4)
    args = dict(K=16, llr_clip=500.0)
    args.update(kw)
    with pytest.raises((ValueError, TypeError)):
        list_apriori_batch(y, h, Q16, args["K"], 0.1, None, args["llr_clip"])
    with pytest.raises((ValueError, TypeError)):
        apriori_detector(Q16, args["K"], args["llr_clip"])


def test_list_apriori_shape_checks(no_engine):
    y, h = _vec(4, 4)
    with pytest.raises(ValueError):
        list_apriori_batch(y, h, Q16, 16, 0.1, np.zeros((3, 15)))                     # prior of the wrong width
    with pytest.raises(ValueError):
        list_apriori_batch(y, h, Q16, 16, 0.1, np.zeros((2, 16)))                     # ... of the wrong batch
    y, h = _vec(3, 4)
    with pytest.raises(ValueError):
        list_apriori_batch(y, h, Q16, 16, 0.1)                                        # more columns than rows
    y, h = _vec(17, 17)
    with pytest.raises(ValueError):
        list_apriori_batch(y, h, Q16, 16, 0.1)                                        # 68 bits per vector
    y, h = _vec(4, 4)
    with pytest.raises(ValueError):
        list_apriori_batch(y, h, Q16, 5000, 0.1)                                      # a list the kernel cannot hold
    with pytest.raises(ValueError):
        list_apriori_batch(y, h[:2], Q16, 16, 0.1)
    for bad in (0.0, -0.1, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            list_apriori_batch(y, h, Q16, 16, bad)                                    # noise_var
    assert list_apriori_batch(np.zeros((0, 4)), np.zeros((4, 4)), Q16, 16, 0.1).shape == (0, 16)   # empty: no device needed


def test_apriori_detector_prototype(no_engine):
    det = apriori_detector(Q16, 16)
    assert getfullargspec(det).args == ['y', 'h', 'constellation', 'noise_var', 'a_priori']


IDD_REFUSED = [
    dict(idd_iters=1),                                                                 # no code
    dict(idd_iters=1, detector='kbest', output_type='hard'),
    dict(idd_iters=2, detector='best_first', ldpc=True),
    dict(idd_iters=1, detector='ml'),
    dict(idd_iters=-1, detector='kbest', output_type='soft', ldpc=True),
    dict(idd_iters=1.5, detector='kbest', output_type='soft', ldpc=True),
    dict(idd_iters=1, detector='kbest', output_type='soft', ldpc=True, idd_clip=0.0),
    dict(idd_iters=1, detector='kbest', output_type='soft', ldpc=True, idd_clip=float("nan")),
    dict(idd_iters=1, detector='kbest', output_type='soft', ldpc=True, idd_decision='soft'),
    dict(idd_iters=1, detector='kbest', output_type='soft', ldpc=True, K=5000),        # a list the kernel cannot hold
    dict(idd_iters=1, detector='kbest', output_type='soft', ldpc=True, K=0),
]


@pytest.mark.parametrize("case", IDD_REFUSED, ids=[str(i) for i in range(len(IDD_REFUSED))])
def test_idd_link_refusals_come_before_the_engine(no_engine, case):
    case = dict(case)
    if case.pop('ldpc', False):
        case['ldpc_params'] = ldpc_params("wimax1440")
    with pytest.raises(ValueError):
        DeviceMimoLink(Q16, _chan(), **case)


def test_idd_plan_is_accepted_without_a_device():
    link = DeviceMimoLink.__new__(DeviceMimoLink)
    link.modem, link.channel, link.K = Q16, _chan(), 16
    link._plan('kbest', 'soft', (1, 3, 5), ldpc_params("wimax1440"), 'MSA', 720, 3, 500.0, 'hard')
    assert (link.idd_iters, link.idd_clip, link.idd_decision, link.Ke) == (3, 500.0, 'hard', 16)
    assert link.vectors_per_tx == 90 and link.codewords_per_tx == 1
    link._plan('kbest', 'soft', (1, 3, 5), ldpc_params("wimax1440"), 'MSA', 720)      # the arguments before this feature
    assert link.idd_iters == 0
    assert getfullargspec(DeviceMimoLink.__init__).args[-3:] == ['idd_iters', 'idd_clip', 'idd_decision']


# ---- no device: no result ------------------------------------------------------------------------------------------------------

def test_new_entry_points_fail_loudly_without_device():
    if _lib.device_count() > 0:
        pytest.skip("a HIP device is present")
    y, h = _vec(4, 4)
    with pytest.raises(_lib.EngineError):
        list_apriori_batch(y, h, Q16, 16, 0.1)
    with pytest.raises(_lib.EngineError):
        apriori_detector(Q16, 16)(y[0], h[0], Q16.constellation, 0.1, np.zeros(16))
    with pytest.raises(_lib.EngineError):
        DeviceMimoLink(Q16, _chan(), detector='kbest', output_type='soft', ldpc_params=ldpc_params("wimax1440"), idd_iters=2)
    lib = _lib.load()
    cand, count, dist, llr = np.zeros((2, 4, 2), np.int32), np.ones(2, np.int32), np.zeros((2, 4)), np.zeros((2, 8))
    rc = lib.cpx_mimo_list_llr(None, _lib.ptr(cand), _lib.ptr(count), _lib.ptr(dist), 2, 2, 4, None, 0.1, 500.0, _lib.ptr(llr))
    assert rc == _lib.CPX_EINVAL and "null modem" in _lib.last_error()
    rc = lib.cpx_mimo_list_dist(None, None, None, 1, 2, 2, 2, _lib.ptr(cand), _lib.ptr(count), 4, _lib.ptr(dist))
    assert rc == _lib.CPX_EINVAL
    assert devicelink.DeviceMimoLink is DeviceMimoLink
