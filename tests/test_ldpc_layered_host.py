"""The layered min-sum rule without a GPU: tests/ldpc_layered_model.py against a scalar transcription of the rule, the first-fit schedule,
the properties a decoder has to have, the iteration advantage over the flooding schedule, and every refusal of the Python layer."""
import ctypes
import math

import numpy as np
import pytest

import ldpc_layered_model as M
import oracle
from commpy_amd import _lib, deviceops
from commpy_amd.channelcoding import ldpc_layered_decode, ldpc_layers
from commpy_amd.channelcoding import ldpc_layered as LL
from helpers import ldpc_params

SCALINGS = ((1.0, 0.0), (0.75, 0.0), (0.8, 0.3))
FIXTURES = ("gallager96", "gallager96b", "wimax960", "wimax1440", "n1944")


def random_code(rs, n_v, degrees):
    """A check of every degree listed, each over random distinct variables; every variable is used (the first rows sweep them)."""
    rows, nxt = [], 0
    for d in degrees:
        if nxt < n_v:
            vs = np.arange(nxt, min(nxt + d, n_v))
            vs = np.concatenate([vs, rs.choice(np.setdiff1d(np.arange(n_v), vs), d - len(vs), replace=False)])
            nxt += d
        else:
            vs = rs.choice(n_v, d, replace=False)
        rows.append(vs)
    return M.code_from_rows(n_v, rows)


def bpsk_llr(words, ebn0_db, rate, rs):
    """LLRs (positive = bit 0) of BPSK over AWGN."""
    sigma2 = 1.0 / (2.0 * rate * 10.0 ** (ebn0_db / 10.0))
    y = 1.0 - 2.0 * np.asarray(words, dtype=float) + math.sqrt(sigma2) * rs.randn(*np.shape(words))
    return 2.0 * y / sigma2


def naive(llr, code, schedule, n_iters, alpha, beta, early_stop=True, llr_clip=500.0):
    """The rule once more, read off its text: one block, Python floats, a loop over the edges of each check."""
    ev, rp = code.edge_var.tolist(), code.row_ptr.tolist()
    if any(math.isnan(x) for x in llr):
        return [0] * code.n_v, [math.nan] * code.n_v, 0, 0
    Q = [min(max(float(x), -llr_clip), llr_clip) for x in llr]
    R = [0.0] * len(ev)
    neg = lambda x: math.copysign(1.0, x) < 0

    def parity_ok():
        return all(sum(neg(Q[ev[e]]) for e in range(rp[c], rp[c + 1])) % 2 == 0 for c in range(code.n_c))
    for it in range(1, n_iters + 1):
        for layer in schedule:
            for c in layer:
                es = range(rp[c], rp[c + 1])
                m = {e: Q[ev[e]] - R[e] for e in es}
                for e in es:
                    a = min(abs(m[i]) for i in es if i != e)
                    g = max(alpha * a - beta, 0.0)
                    s = False
                    for i in es:
                        if i != e:
                            s ^= neg(m[i])
                    R[e] = -g if s else g
                    Q[ev[e]] = m[e] + R[e]
        if early_stop and parity_ok():
            return [int(neg(q)) for q in Q], Q, it, 1
    return [int(neg(q)) for q in Q], Q, n_iters, int(parity_ok())


def same_as_naive(llr, code, schedule, n_iters, alpha, beta, early_stop=True, llr_clip=500.0):
    got = M.decode(llr, code, schedule, n_iters, alpha, beta, early_stop, llr_clip)
    for b, row in enumerate(np.atleast_2d(llr)):
        bits, q, it, conv = naive(row.tolist(), code, [l.tolist() for l in schedule], n_iters, alpha, beta, early_stop, llr_clip)
        assert got['bits'][b].tolist() == bits and got['iters'][b] == it and got['converged'][b] == conv
        assert np.array_equal(got['llr'][b].view(np.int64), np.array(q, dtype=np.float64).view(np.int64))
    return got


# ---- the model against the scalar transcription ----------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha,beta", SCALINGS)
def test_model_equals_the_naive_transcription_on_gallager96(alpha, beta):
    code = M.code_from_params(ldpc_params("gallager96"))
    sched = M.first_fit(code)
    rs = np.random.RandomState(3)
    llr = bpsk_llr(np.zeros((5, 96)), 2.0, 0.5, rs)
    llr[3] = rs.randn(96)                                        # pure noise: runs to the cap
    llr[4, ::7] = -0.0
    got = same_as_naive(llr, code, sched, 6, alpha, beta)
    assert got['converged'][3] == 0 and got['iters'][3] == 6
    same_as_naive(llr, code, sched, 3, alpha, beta, early_stop=False, llr_clip=2.5)


@pytest.mark.parametrize("alpha,beta", SCALINGS)
@pytest.mark.parametrize("seed,n_v,degrees", [(0, 40, [2, 32, 3, 5, 7, 4]), (1, 77, [6] * 20 + [2, 9]), (2, 200, [11] * 30 + [32, 2, 17])])
def test_model_equals_the_naive_transcription_on_random_structures(seed, n_v, degrees, alpha, beta):
    rs = np.random.RandomState(seed)
    code = random_code(rs, n_v, degrees)
    sched = M.first_fit(code)
    assert M.is_schedule(code, sched)
    llr = 3.0 * rs.randn(4, n_v) + 2.0
    llr[1, rs.choice(n_v, 5)] = 0.0
    llr[2, 0], llr[2, 1] = np.inf, -np.inf
    llr[3, 5] = np.nan
    got = same_as_naive(llr, code, sched, 4, alpha, beta)
    assert got['iters'][3] == 0 and np.isnan(got['llr'][3]).all() and not got['bits'][3].any()


def test_alpha_one_beta_zero_is_the_plain_minimum():
    """g = max(1.0 * a - 0.0, 0.0) is a itself for every a >= 0."""
    a = np.abs(np.random.RandomState(0).randn(1000)) * 10.0 ** np.random.RandomState(1).randint(-300, 300, 1000)
    a[:3] = 0.0, np.finfo(float).tiny / 4, np.finfo(float).max
    g = np.maximum(np.float64(1.0) * a - np.float64(0.0), 0.0)
    assert np.array_equal(g.view(np.int64), a.view(np.int64))


def test_the_order_of_checks_inside_a_layer_does_not_matter():
    rs = np.random.RandomState(5)
    for name in ("gallager96", "wimax960"):
        code = M.code_from_params(ldpc_params(name))
        sched = M.first_fit(code)
        llr = bpsk_llr(np.zeros((3, code.n_v)), 2.5, 1.0 - code.n_c / code.n_v, rs)
        ref = M.decode(llr, code, sched, 5, 0.8, 0.3, early_stop=False)
        shuffled = M.decode(llr, code, [rs.permutation(l) for l in sched], 5, 0.8, 0.3, early_stop=False)
        assert all(np.array_equal(ref[k], shuffled[k]) for k in ref) and np.array_equal(ref['llr'].view(np.int64), shuffled['llr'].view(np.int64))


# ---- the default schedule --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,sizes", [("n1944", [81] * 8), ("wimax1440", [120, 120, 120, 120, 120, 60, 60]), ("wimax960", [40] * 6)])
def test_first_fit_recovers_the_block_rows(name, sizes):
    p = ldpc_params(name)
    layers = ldpc_layers(p)
    assert [len(l) for l in layers] == sizes and all(l.dtype == np.int32 for l in layers)
    assert all(np.array_equal(a, b) for a, b in zip(layers, M.first_fit(M.code_from_params(p))))


def test_first_fit_is_a_valid_partition_elsewhere():
    rs = np.random.RandomState(9)
    cases = [ldpc_params("gallager96"), ldpc_params("gallager96b")]
    cases += [M.params_from_code(random_code(rs, n_v, list(rs.randint(2, 12, n_c)))) for n_v, n_c in ((40, 9), (120, 60), (200, 33))]
    for p in cases:
        code = M.code_from_params(p)
        layers = ldpc_layers(p)
        assert M.is_schedule(code, layers)
        assert all(np.array_equal(a, b) for a, b in zip(layers, M.first_fit(code)))
        # first fit: a check conflicts with every layer before its own
        where = {int(c): i for i, l in enumerate(layers) for c in l}
        for c in range(code.n_c):
            vs = set(code.edge_var[code.row_ptr[c]:code.row_ptr[c + 1]].tolist())
            for i in range(where[c]):
                earlier = [d for d in layers[i] if d < c]
                assert any(vs & set(code.edge_var[code.row_ptr[d]:code.row_ptr[d + 1]].tolist()) for d in earlier)


# ---- what a decoder owes ----------------------------------------------------------------------------------------------------------
def test_converged_means_a_zero_syndrome():
    rs = np.random.RandomState(11)
    code = M.code_from_params(ldpc_params("wimax960"))
    llr = bpsk_llr(np.zeros((24, 960)), 2.0, 0.75, rs)
    llr[::5] = rs.randn(*llr[::5].shape)
    got = M.decode(llr, code, M.first_fit(code), 12, 0.75, 0.0)
    syn = M.syndrome(code, got['bits'].astype(bool)).any(axis=1)
    assert np.array_equal(got['converged'] == 1, ~syn)           # and a block that did not converge has a non-zero one
    assert 0 < got['converged'].sum() < 24
    assert (got['iters'][got['converged'] == 0] == 12).all()


@pytest.mark.parametrize("name", ["wimax1440", "wimax960"])
def test_noise_free_code_words_decode_to_themselves_in_one_iteration(name):
    p = ldpc_params(name)
    code = M.code_from_params(p)
    P = deviceops.gf2_generator(dict(p))                         # [m, k] over GF(2), on the host
    rs = np.random.RandomState(2)
    msg = rs.randint(0, 2, (6, code.n_v - code.n_c))
    msg[0] = 0                                                   # the all-zero word
    words = np.concatenate([msg, msg.dot(P.T) % 2], axis=1)
    assert not M.syndrome(code, words.astype(bool)).any()
    for alpha, beta in SCALINGS:
        got = M.decode(4.0 * (1.0 - 2.0 * words), code, M.first_fit(code), 5, alpha, beta)
        assert np.array_equal(got['bits'], words) and (got['iters'] == 1).all() and (got['converged'] == 1).all()


# measured here (sum of layered iterations / sum of flooding iterations, 12 blocks, cap 30, alpha = 1):
#   WiMAX (1440,720) at 2 dB: 110 / 152 = 0.724;  (1944,1296) at 3 dB: 45 / 77 = 0.584
@pytest.mark.parametrize("name,ebn0_db,seed", [("wimax1440", 2.0, 21), ("n1944", 3.0, 22)])
def test_layered_needs_fewer_iterations_than_flooding(name, ebn0_db, seed):
    p = ldpc_params(name)
    code = M.code_from_params(p)
    rs = np.random.RandomState(seed)
    llr = bpsk_llr(np.zeros((12, code.n_v)), ebn0_db, 1.0 - code.n_c / code.n_v, rs)
    _, _, flood = oracle.ldpc_bp_decode(llr.reshape(-1).copy(), dict(p), "MSA", 30, True)
    got = M.decode(llr, code, M.first_fit(code), 30)
    layered, flooding = int(got['iters'].sum()), int(np.sum(flood))
    print("%s at %.1f dB: layered %d, flooding %d iterations, ratio %.3f" % (name, ebn0_db, layered, flooding, layered / flooding))
    assert layered <= 0.8 * flooding


# ---- refusals: all on the host ---------------------------------------------------------------------------------------------------------
@pytest.fixture
def no_device(monkeypatch):
    """Any attempt to load the engine fails the test: the refusals below must come from the host-side checks."""
    def boom(*a, **k):
        raise AssertionError("the engine was touched")
    monkeypatch.setattr(_lib, "load", boom)


def small():
    return M.params_from_code(M.code_from_rows(8, [[0, 1, 2], [2, 3, 4], [4, 5, 6], [6, 7]]))


@pytest.mark.parametrize("call", ["host", "dev"])
def test_python_refusals(no_device, call):
    if call == "host":
        dec = lambda p, n_iters=3, llr=None, **kw: ldpc_layered_decode(np.zeros((2, p['n_vnodes'])) if llr is None else llr, p, n_iters, **kw)
    else:
        dec = lambda p, n_iters=3, llr=None, **kw: deviceops.ldpc_layered_decode_dev(p, None, 2, n_iters, **kw)

    def refused(words, *a, **kw):
        with pytest.raises(ValueError) as e:
            dec(*a, **kw)
        assert all(w in str(e.value) for w in words), str(e.value)

    refused(("degree 1", "2 .. 32"), M.params_from_code(M.code_from_rows(8, [[0, 1, 2], [3]])))
    refused(("degree 33", "2 .. 32"), M.params_from_code(M.code_from_rows(40, [range(33), [33, 34]])))
    refused(("8 n_v + 24 n_c", "164800", "163840"), M.params_from_code(M.code_from_rows(20000, [[2 * c, 2 * c + 1] for c in range(200)])))
    for bad in ([[0, 2], [1]], [[0, 2], [1, 3], [3]], [[0, 2], [1, 3], [4]], [[0, 2], [1, 3], []], [], [[0.5, 2], [1, 3]]):
        refused(("partition",), small(), schedule=bad)
    refused(("conflict-free", "layer 0"), small(), schedule=[[0, 1], [2, 3]])
    for bad in (0, -1, True, 1.5, None):
        refused(("n_iters >= 1",), small(), n_iters=bad)
    for bad in (0.0, -0.5, math.inf, math.nan):
        refused(("alpha > 0",), small(), alpha=bad)
        refused(("llr_clip > 0",), small(), llr_clip=bad)
    for bad in (-0.1, math.inf, math.nan):
        refused(("beta >= 0",), small(), beta=bad)
    for bad in ((), ("bits", "metric"), "all"):
        refused(("want must name",), small(), want=bad)
    if call == "host":
        refused(("n_v = 8",), small(), llr=np.zeros((2, 9)))
        refused(("1-D or 2-D",), small(), llr=np.zeros((2, 2, 8)))


def test_every_fixture_code_fits(no_device):
    for name in FIXTURES:
        p = ldpc_params(name)
        plan = LL.plan(p)
        assert 8 * plan.n_v + 24 * plan.n_c <= LL.LL_LDS_MAX
        assert LL.plan(p) is plan and LL.plan(p, ldpc_layers(p)[::-1]) is not plan            # cached per code and schedule
    assert 8 * 1944 + 24 * 648 == 31104


def test_c_abi_refuses_before_a_device_is_looked_for():
    lib = _lib.load()
    h = ctypes.c_void_p()
    i32 = lambda *v: np.array(v, dtype=np.int32)
    create = lambda n_v, n_c, ec, ev, start, order: lib.cpx_ldpc_layered_create(n_v, n_c, len(ec), _lib.ptr(ec), _lib.ptr(ev), len(start) - 1,
                                                                                 _lib.ptr(start), _lib.ptr(order), ctypes.byref(h))
    assert lib.cpx_ldpc_layered_create(4, 2, 4, None, None, 1, None, None, ctypes.byref(h)) == _lib.CPX_EINVAL
    assert _lib.last_error() == "ldpc_layered: null pointer"
    ec, ev = i32(0, 0, 1, 1), i32(0, 1, 1, 2)
    assert create(3, 2, i32(0, 0, 0, 1), i32(0, 1, 2, 2), i32(0, 1, 2), i32(0, 1)) == _lib.CPX_ELIMIT and "degree 1" in _lib.last_error()
    assert create(3, 2, ec, i32(1, 0, 1, 2), i32(0, 1, 2), i32(0, 1)) == _lib.CPX_EINVAL and "not sorted" in _lib.last_error()
    assert create(3, 2, ec, ev, i32(0, 2), i32(0, 1)) == _lib.CPX_ELIMIT and "conflict-free" in _lib.last_error()
    assert create(3, 2, ec, ev, i32(0, 1, 2), i32(0, 0)) == _lib.CPX_ELIMIT and "partition" in _lib.last_error()
    assert create(4, 2, ec, i32(0, 1, 2, 3), i32(0, 2, 2), i32(0, 1)) == _lib.CPX_ELIMIT and "partition" in _lib.last_error()
    big = np.repeat(np.arange(200, dtype=np.int32), 2)
    assert create(20000, 200, big, np.arange(400, dtype=np.int32), i32(0, 200), np.arange(200, dtype=np.int32)) == _lib.CPX_ELIMIT
    assert "LDS budget" in _lib.last_error()
    assert h.value is None
    assert lib.cpx_ldpc_layered_decode(None, None, 1, 5, 1.0, 0.0, 1, 500.0, None, None, None, None) == _lib.CPX_EINVAL
    assert lib.cpx_ldpc_layered_decode_dev(None, None, 1, 5, 1.0, 0.0, 1, 500.0, None, None, None, None, None) == _lib.CPX_EINVAL
    assert lib.cpx_ldpc_layered_destroy(None) == _lib.CPX_OK


def test_fails_loudly_without_a_device():
    if _lib.device_count() > 0:
        pytest.skip("a HIP device is present")
    with pytest.raises(_lib.EngineError):
        ldpc_layered_decode(np.zeros(8), small(), 3)
