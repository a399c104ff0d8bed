"""The layered min-sum decoder on the GPU against tests/ldpc_layered_model.py: every output is compared exactly (``array_equal``; ``'llr'``
by its bit pattern), on the fixture codes (layers of 40, 60, 120 and 81 = 64 + 17 checks), random structures with checks of degree 2 and
32, single-check layers and a code whose checks all conflict, batches on both sides of what is resident, iteration limits 1 .. 50 with
and without early stop, dyadic and non-dyadic scalings, special values and other schedules."""
import ctypes
import itertools
import re

import numpy as np
import pytest

import ldpc_layered_model as M
from commpy_amd import _lib, deviceops
from commpy_amd.channelcoding import ldpc_layered_decode, ldpc_layers
from commpy_amd.deviceops import DeviceBuf
from helpers import ldpc_params
from test_ldpc_layered_host import bpsk_llr, random_code

pytestmark = pytest.mark.gpu
EVERYTHING = ("bits", "llr", "iters", "converged")
DTYPES = {"bits": np.int8, "llr": np.float64, "iters": np.int32, "converged": np.uint8}
SCALINGS = ((1.0, 0.0), (0.75, 0.0), (0.8125, 0.5), (0.8, 0.3))     # the last pair is not dyadic: a contracted multiply-add fails it
_codes = {}


def fixture_code(name):
    """(parameter dictionary, model code, default schedule), made once per name."""
    if name not in _codes:
        p = ldpc_params(name)
        code = M.code_from_params(p)
        _codes[name] = (p, code, M.first_fit(code))
    return _codes[name]


def mixed(code, B, seed, ebn0_db=3.0):
    """Rows in turn: a noise-free all-zero word, the word at ``ebn0_db``, pure noise -- neighbours retire at different iterations."""
    rs = np.random.RandomState(seed)
    llr = bpsk_llr(np.zeros((B, code.n_v)), ebn0_db, 1.0 - code.n_c / code.n_v, rs)
    llr[0::3] = 6.0
    llr[2::3] = 2.0 * rs.randn(*llr[2::3].shape)
    return llr


def equal(a, b):
    view = lambda x: x.view(np.int64) if x.dtype == np.float64 else x
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(view(a), view(b))


def same(got, ref, what=None):
    """Every output against the model's, the LLRs by their bit pattern (a rejected row: NaN in both)."""
    for key, g in zip(EVERYTHING, got):
        assert g.dtype == DTYPES[key], (what, key)
        if key == "llr":
            assert np.array_equal(np.isnan(g), np.isnan(ref[key])), (what, key)
            ok = ~np.isnan(g)
            assert np.array_equal(g[ok].view(np.int64), ref[key][ok].view(np.int64)), (what, key)
        else:
            assert np.array_equal(g, ref[key]), (what, key)
    return ref


def check(llr, p, code, sched, n_iters, what=None, schedule=None, **kw):
    before = llr.copy()
    got = ldpc_layered_decode(llr, p, n_iters, schedule=schedule, want=EVERYTHING, **kw)
    assert np.array_equal(llr.view(np.int64), before.view(np.int64)), what        # the caller's input is unchanged
    return same(got, M.decode(llr, code, sched if schedule is None else schedule, n_iters, **kw), what)


def resident_blocks():
    """Blocks that the decoder's grid holds at once, from what the launcher reports."""
    waves, lds, per_cu, resident = (int(v) for v in re.search(r"waves=(\d+) lds=(\d+) per_cu=(\d+) resident=(\d+)",
                                                              _lib.last_kernel()).groups())
    assert resident % (per_cu * waves) == 0 and lds * per_cu <= 160 * 1024 and waves <= 8
    return resident


# ---- codes -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,cap", [("gallager96", 8), ("wimax960", 16), ("wimax1440", 8), ("n1944", 12)])
def test_fixture_codes(gpu, name, cap):
    p, code, sched = fixture_code(name)
    ref = check(mixed(code, 13, 1), p, code, sched, 7, name, alpha=0.75)
    assert _lib.last_kernel().startswith("ldpc_layered_kernel<%d> " % cap)
    assert (ref['iters'] == 1).any() and (ref['converged'] == 0).any() and len(set(ref['iters'].tolist())) >= 3
    one = ldpc_layered_decode(mixed(code, 13, 1)[4], p, 7, alpha=0.75, want=EVERYTHING)           # the 1-D form
    assert all(equal(np.asarray(o), r[4]) for o, r in zip(one, (ref[k] for k in EVERYTHING)))


def all_conflict(rs, n_v, n_c):
    """Every check holds variable 0: every check conflicts with every other, n_layers = n_c."""
    return M.code_from_rows(n_v, [np.concatenate([[0], 1 + rs.choice(n_v - 1, rs.randint(1, 9), replace=False)]) for _ in range(n_c)])


RANDOM = {
    "deg2_deg32": lambda rs: random_code(rs, 40, [2, 32, 3, 5, 7, 4, 2, 9]),
    "deg32_many": lambda rs: random_code(rs, 200, [32] * 7 + [2] * 70 + [17, 24, 25, 13]),
    "deg12": lambda rs: random_code(rs, 131, list(rs.randint(2, 13, 90))),
    "all_conflict": lambda rs: all_conflict(rs, 57, 23),
}


@pytest.mark.parametrize("name", sorted(RANDOM))
def test_random_structures(gpu, name):
    rs = np.random.RandomState(sorted(RANDOM).index(name))
    code = RANDOM[name](rs)
    p = M.params_from_code(code)
    sched = ldpc_layers(p)
    assert M.is_schedule(code, sched) and all(np.array_equal(a, b) for a, b in zip(sched, M.first_fit(code)))
    if name == "all_conflict":
        assert len(sched) == code.n_c
    llr = 2.0 * rs.randn(70, code.n_v) + 1.5
    for (alpha, beta), n_iters in zip(SCALINGS, (1, 2, 7, 50)):
        check(llr, p, code, sched, n_iters, (name, alpha, beta), alpha=alpha, beta=beta)
    serial = [np.array([c], dtype=np.int32) for c in rs.permutation(code.n_c)]          # single-check layers, in a random order
    check(llr[:9], p, code, sched, 3, (name, "serial"), schedule=serial, alpha=0.8, beta=0.3)


# ---- batch sizes ---------------------------------------------------------------------------------------------------------------------
def test_batches_round_the_resident_grid(gpu):
    p, code, sched = fixture_code("gallager96")
    ldpc_layered_decode(np.zeros((1, 96)), p, 1)
    R = resident_blocks()
    llr = np.resize(mixed(code, 999, 2), (2 * R + 1, 96))
    ref = M.decode(llr[:999], code, sched, 4, 0.75, 0.0)
    ref = {k: np.resize(v, (2 * R + 1,) + v.shape[1:]) for k, v in ref.items()}
    for B in (1, 2, R - 1, R, R + 1, 2 * R + 1):                # R + 1: one more than a pass of the grid
        got = ldpc_layered_decode(llr[:B], p, 4, alpha=0.75, want=EVERYTHING)
        same(got, {k: v[:B] for k, v in ref.items()}, B)
    empty = ldpc_layered_decode(np.zeros((0, 96)), p, 4, want=EVERYTHING)
    assert [e.shape for e in empty] == [(0, 96), (0, 96), (0,), (0,)]


def test_more_blocks_than_are_resident_on_the_largest_code(gpu):
    p, code, sched = fixture_code("n1944")
    ldpc_layered_decode(np.zeros((1, 1944)), p, 1)
    R = resident_blocks()
    assert "lds=%d " % (31104 * (160 * 1024 // 31104)) in _lib.last_kernel()
    base = mixed(code, 24, 3)
    ref = M.decode(base, code, sched, 3, 1.0, 0.0)
    B = R + 1
    got = ldpc_layered_decode(np.resize(base, (B, 1944)), p, 3, want=EVERYTHING)
    same(got, {k: np.resize(v, (B,) + v.shape[1:]) for k, v in ref.items()})


# ---- iterations ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("early_stop", [True, False])
@pytest.mark.parametrize("n_iters", [1, 2, 7, 50])
def test_iteration_limits(gpu, n_iters, early_stop):
    p, code, sched = fixture_code("wimax960")
    ref = check(mixed(code, 21, 4, ebn0_db=3.0), p, code, sched, n_iters, (n_iters, early_stop), early_stop=early_stop)
    if not early_stop:
        assert (ref['iters'] == n_iters).all() and ref['converged'].any() and not ref['converged'].all()
    elif n_iters >= 7:
        assert len(set(ref['iters'].tolist())) >= 3 and ref['iters'].max() == n_iters


# ---- scaling -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha,beta", SCALINGS)
def test_scalings(gpu, alpha, beta):
    p, code, sched = fixture_code("wimax1440")
    ref = check(mixed(code, 12, 5, ebn0_db=2.0), p, code, sched, 9, (alpha, beta), alpha=alpha, beta=beta)
    plain = M.decode(mixed(code, 12, 5, ebn0_db=2.0), code, sched, 9)
    if (alpha, beta) != (1.0, 0.0):
        assert not np.array_equal(ref['llr'], plain['llr'])


# ---- special values ---------------------------------------------------------------------------------------------------------------------
def test_special_values(gpu):
    p, code, sched = fixture_code("wimax960")
    rs = np.random.RandomState(6)
    llr = mixed(code, 16, 6)
    llr[1] = 0.0                                                 # all-zero LLRs
    llr[2, rs.choice(960, 300, replace=False)] = 0.0             # +-0.0 mixed in
    llr[2, rs.choice(960, 300, replace=False)] = -0.0
    llr[3] = np.where(rs.rand(960) < 0.5, 0.0, -0.0)
    llr[4, ::9], llr[4, 1::9] = np.inf, -np.inf                  # +-inf and |LLR| above the clip
    llr[5] *= 1e4
    llr[6, 17] = np.nan                                          # NaN rows between good rows
    llr[8] = np.nan
    llr[9, -1], llr[9, 0] = np.nan, np.inf
    llr[15, 0] = -np.nan
    for clip, (alpha, beta) in ((500.0, (1.0, 0.0)), (20.0, (0.8, 0.3)), (20.0, (0.8125, 0.5))):
        ref = check(llr, p, code, sched, 6, (clip, alpha), alpha=alpha, beta=beta, llr_clip=clip)
        assert (ref['iters'][[6, 8, 9, 15]] == 0).all() and (ref['iters'][[5, 7, 10, 14]] > 0).all()
        assert np.isfinite(ref['llr'][4]).all()                  # the clip has been applied to +-inf


# ---- schedules ---------------------------------------------------------------------------------------------------------------------
def test_other_schedules(gpu):
    p, code, sched = fixture_code("wimax1440")
    llr = mixed(code, 9, 7, ebn0_db=2.0)
    default = check(llr, p, code, sched, 4, "default", alpha=0.75, early_stop=False)
    for name, other in (("reversed", sched[::-1]), ("serial", [np.array([c], dtype=np.int32) for c in range(code.n_c)])):
        ref = check(llr, p, code, sched, 4, name, schedule=other, alpha=0.75, early_stop=False)
        assert not np.array_equal(ref['llr'], default['llr']), name
    assert equal(ldpc_layered_decode(llr, p, 4, alpha=0.75, early_stop=False, want='llr'), default['llr'])      # the cached default is intact


# ---- layout independence ------------------------------------------------------------------------------------------------------------
def test_batch_size_position_and_requested_outputs_do_not_matter(gpu):
    p, code, sched = fixture_code("gallager96")
    llr = mixed(code, 259, 8, ebn0_db=2.0)
    llr[100, 3] = np.nan
    full = ldpc_layered_decode(llr, p, 8, 0.8, 0.3, want=EVERYTHING)
    same(full, M.decode(llr, code, sched, 8, 0.8, 0.3))
    for B in (1, 5, 64, 65):
        part = ldpc_layered_decode(llr[:B], p, 8, 0.8, 0.3, want=EVERYTHING)
        assert all(equal(a, f[:B]) for a, f in zip(part, full))
    moved = ldpc_layered_decode(llr[::-1], p, 8, 0.8, 0.3, want=EVERYTHING)
    assert all(equal(mv[::-1], f) or key == "llr" for key, mv, f in zip(EVERYTHING, moved, full))
    ok = ~np.isnan(full[1])
    assert np.array_equal(moved[1][::-1][ok].view(np.int64), full[1][ok].view(np.int64)) and np.isnan(moved[1][::-1][~ok]).all()
    rows = [0, 1, 2, 99, 101, 258]
    part = ldpc_layered_decode(llr[rows], p, 8, 0.8, 0.3, want=EVERYTHING)
    assert all(equal(a, f[rows]) for a, f in zip(part, full))
    for r in (1, 2, 3, 4):
        for names in itertools.combinations(EVERYTHING, r):
            for order in itertools.permutations(names):
                got = ldpc_layered_decode(llr[:99], p, 8, 0.8, 0.3, want=order)
                got = (got,) if r == 1 else got
                assert len(got) == r
                for key, g in zip(names, got):                   # results come in the order of the documentation
                    assert equal(g, full[EVERYTHING.index(key)][:99]), order
    assert equal(ldpc_layered_decode(llr[:99], p, 8, 0.8, 0.3), full[0][:99])


def test_streams_and_device_buffers(gpu):
    p, code, sched = fixture_code("wimax960")
    lib = _lib.load()
    B = 37
    llr = mixed(code, B, 9)
    host = ldpc_layered_decode(llr, p, 10, 0.75, want=EVERYTHING)
    shapes = {"bits": (B, 960), "llr": (B, 960), "iters": (B,), "converged": (B,)}
    streams = [ctypes.c_void_p() for _ in range(2)]
    for s in streams:
        _lib.check(lib.cpx_stream_create(ctypes.byref(s)))
    try:
        d_llr = DeviceBuf.from_array(llr)
        outs = [deviceops.ldpc_layered_decode_dev(p, d_llr, B, 10, 0.75, want=EVERYTHING, stream=s) for s in streams + [None]]
        assert _lib.last_kernel().startswith("ldpc_layered_kernel<16> ")
        for s in streams + [None]:
            _lib.check(lib.cpx_stream_sync(s))
        for decoded in outs:
            for key, d, want in zip(EVERYTHING, decoded, host):
                assert equal(d.to_array(shapes[key], DTYPES[key]), want), key
        assert equal(d_llr.to_array((B, 960), np.float64), llr)                      # the device input is unchanged too
        d_q = deviceops.ldpc_layered_decode_dev(p, d_llr, B, 10, 0.75, want="llr")
        d_c, d_i = deviceops.ldpc_layered_decode_dev(p, d_llr, B, 10, 0.75, want=("converged", "iters"))[::-1]
        _lib.check(lib.cpx_stream_sync(None))
        assert equal(d_q.to_array((B, 960), np.float64), host[1]) and equal(d_i.to_array((B,), np.int32), host[2])
        assert equal(d_c.to_array((B,), np.uint8), host[3])
    finally:
        for s in streams:
            lib.cpx_stream_destroy(s)


def test_the_kernel_is_named(gpu):
    p, code, sched = fixture_code("wimax1440")
    ldpc_layered_decode(np.ones((3, 1440)), p, 2)
    assert re.match(r"ldpc_layered_kernel<8> waves=\d+ lds=\d+ per_cu=\d+ resident=\d+ passes=12$", _lib.last_kernel())
