"""Chase-II BCH decoding on the GPU against tests/chase_model.py: every output equals the model, floats by bit pattern, at the sizes
where the kernel changes its path -- fewer positions than lanes, one 64-position chunk and one position more, remainders of the grouped
syndrome and Chien loops, every table size class, p from 1 to 8, ties, rejected words, batches above the resident grid -- and in every
call form: host and device buffers, streams, strided rows and columns, the soft output written over the prior."""
import ctypes
import itertools

import numpy as np
import pytest

import bch_model as M
import chase_model as CM
from commpy_amd import _lib, deviceops
from commpy_amd.channelcoding import BCHCode, bch_decode, chase_decode
from commpy_amd.deviceops import DeviceBuf
from test_bch_host import DVB_PRIM_POLY

pytestmark = pytest.mark.gpu
EVERYTHING = ("bits", "codeword", "extrinsic", "metric", "candidates")
COMPUTE_UNITS = 256                                               # of an MI355X: the grid below is sized from it


def both(n, t, m, prim_poly=None):
    return BCHCode(n, t, m=m, prim_poly=prim_poly), M.Code(n, t, m, prim_poly)


def same(got, ref):
    got, ref = np.asarray(got), np.asarray(ref)
    if got.dtype != ref.dtype or got.shape != ref.shape:
        return False
    return np.array_equal(got.view(np.int64), ref.view(np.int64)) if got.dtype == np.float64 else np.array_equal(got, ref)


def noisy_llr(model, B, sigma, seed):
    """B code words over BPSK and AWGN as LLRs 2 y / sigma^2; some of the words beyond the code's reach."""
    rs = np.random.RandomState(seed)
    sent = M.encode_batch(rs.randint(0, 2, (B, model.k)), model)
    return 2.0 * (1.0 - 2.0 * sent + sigma * rs.randn(B, model.n)) / sigma ** 2


def check(code, model, x, p, beta=0.5, prior=None, alpha=1.0):
    """Every output of the engine against the model; returns the model's results."""
    got = chase_decode(x, code, p, beta, prior=prior, alpha=alpha, want=EVERYTHING)
    assert _lib.last_kernel() == "bch_chase_kernel"
    ref = CM.decode_batch(x, model, p, beta, prior, alpha)
    ref["metric"], ref["candidates"] = ref["metric"].astype(np.float64), ref["candidates"].astype(np.int32)
    for name, g in zip(EVERYTHING, got):
        assert same(g, ref[name]), (name, code.n, code.k, p)
    return ref


# ---- the shapes ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", range(1, 8))
def test_hamming_7_4_at_every_p(gpu, p):
    code, model = both(7, 1, 3)
    rs = np.random.RandomState(p)
    ref = check(code, model, np.concatenate([2.0 * rs.randn(40, 7), rs.randint(-3, 4, (40, 7)).astype(np.float64)]), p)
    assert (ref["candidates"] == 1 << p).all()                    # a perfect code


@pytest.mark.parametrize("n, t, m, p", [(15, 2, 4, 4), (15, 3, 4, 4), (15, 3, 4, 6), (63, 2, 6, 4), (65, 2, 7, 4), (100, 2, 7, 5), (127, 2, 7, 4),
                                        (255, 2, 8, 4), (255, 2, 8, 6), (63, 2, 6, 8), (31, 2, 5, 3), (511, 4, 9, 3)])
def test_shapes(gpu, n, t, m, p):
    """(63, 51), the shortened lengths 65 and 100 over m = 7, (127, 113) and (255, 239) with four chunks: the chunk boundaries of the
    ballots and of the grouped syndrome and Chien loops; p = 8 on (63, 51)."""
    code, model = both(n, t, m)
    rs = np.random.RandomState(n + p)
    x = np.concatenate([noisy_llr(model, 6, 0.55, n + p), 2.0 * rs.randn(3, n)])
    ref = check(code, model, x, p)
    assert (ref["candidates"] > 0).any() and (ref["candidates"] < (1 << p)).any()
    assert (ref["extrinsic"][ref["candidates"] > 0] != 0).any()


@pytest.mark.parametrize("p, B", [(4, 3), (6, 1)])
def test_dvb_s2_short_frame_code(gpu, p, B):
    code, model = both(3240, 12, 14, DVB_PRIM_POLY)
    x = noisy_llr(model, B, 0.37, 14 + p)
    hard_errors = M.decode_batch(x < 0, model)["errors"]
    ref = check(code, model, x, p, beta=2.0)
    assert (hard_errors != 0).any() and (ref["candidates"] > 0).all()


@pytest.mark.parametrize("n, t, m, sigma", [(1023, 10, 10, 0.4), (1023, 32, 10, 0.5)])
def test_p_8_at_the_longest_accepted_words_of_m_10(gpu, n, t, m, sigma):
    code, model = both(n, t, m)
    x = noisy_llr(model, 2, sigma, t)
    ref = check(code, model, x, 8)
    assert (x < 0).sum() > t and (ref["candidates"] > 0).any()


# ---- values -------------------------------------------------------------------------------------------------------------------------
def test_ties_zeros_and_negative_zeros(gpu):
    code, model = both(15, 2, 4)
    rs = np.random.RandomState(154)
    x = rs.randint(-3, 4, (60, 15)).astype(np.float64)
    x[50] = 0.0
    x[51] = -0.0
    x[52, ::2] = -0.0
    x[53] = 1.0
    x[54] = -1.0
    for p in (1, 4, 7):
        ref = check(code, model, x, p)
    assert len(set(ref["metric"][:50])) < 40                      # equal metrics abound
    check(code, model, x, 4, beta=0.0)                            # s_i * 0: a signed zero
    code, model = both(65, 2, 7)
    check(code, model, rs.randint(-2, 3, (20, 65)).astype(np.float64), 5)


def test_rejected_words_between_good_ones(gpu):
    code, model = both(100, 2, 7)
    x = noisy_llr(model, 9, 0.5, 8)
    x[1, 0], x[3, 99], x[4, 64], x[6, 63], x[6, 5] = np.nan, np.inf, -np.inf, np.nan, -np.inf
    clean = np.delete(np.arange(9), [1, 3, 4, 6])
    ref = check(code, model, x, 4)
    assert ref["candidates"].tolist()[1:7:1] == [-1, ref["candidates"][2], -1, -1, ref["candidates"][5], -1]
    alone = chase_decode(x[clean], code, 4, 0.5, want=EVERYTHING)
    assert all(same(a, ref[name][clean]) for name, a in zip(EVERYTHING, alone))
    prior = np.zeros_like(x)
    prior[0, 7], x[1, 0] = np.inf, 1.0                            # a prior can reject a word too; alpha = 0 does not save it (0 inf = NaN)
    ref = check(code, model, x, 4, prior=prior, alpha=0.0)
    assert ref["candidates"][0] == -1 and ref["candidates"][1] >= 0


# ---- batch edges --------------------------------------------------------------------------------------------------------------------
def test_empty_single_and_larger_than_the_resident_grid(gpu):
    code, model = both(7, 1, 3)
    got = chase_decode(np.zeros((0, 7)), code, 2, 0.5, want=EVERYTHING)
    assert [g.shape for g in got] == [(0, 4), (0, 7), (0, 7), (0,), (0,)]
    rs = np.random.RandomState(5)
    x = 2.0 * rs.randn(64, 7)
    check(code, model, x[:1], 3)
    one = chase_decode(x[0], code, 3, 0.5, want=EVERYTHING)
    ref = CM.decode_batch(x, model, 3, 0.5)
    assert all(same(o, ref[name][0]) for name, o in zip(EVERYTHING, one)) and one[0].shape == (4,) and one[3].shape == ()
    # 4 words per workgroup, at most 8 workgroups per compute unit: one word more than the grid decodes in one pass
    B = 4 * 8 * COMPUTE_UNITS + 1
    got = chase_decode(np.resize(x, (B, 7)), code, 3, 0.5, want=EVERYTHING)
    for name, g in zip(EVERYTHING, got):
        r = ref[name].astype(g.dtype)
        assert same(g, np.resize(r, (B,) + r.shape[1:])), name


# ---- layout and call forms ----------------------------------------------------------------------------------------------------------
def test_batch_size_position_and_requested_outputs_do_not_matter(gpu):
    code, model = both(127, 2, 7)
    x = noisy_llr(model, 67, 0.55, 3)
    full = chase_decode(x, code, 4, 0.5, want=EVERYTHING)
    assert (full[4] == 0).any() or (full[4] < 16).any()
    for B in (1, 5):
        assert all(same(p, f[:B]) for p, f in zip(chase_decode(x[:B], code, 4, 0.5, want=EVERYTHING), full))
    for i in (0, 33, 66):
        assert all(same(a, f[i]) for a, f in zip(chase_decode(x[i], code, 4, 0.5, want=EVERYTHING), full))
    moved = chase_decode(x[::-1], code, 4, 0.5, want=EVERYTHING)
    assert all(same(mv[::-1], f) for mv, f in zip(moved, full))
    for r in range(1, 6):
        for want in itertools.combinations(EVERYTHING, r):
            got = chase_decode(x, code, 4, 0.5, want=want[::-1])
            got = (got,) if r == 1 else got
            assert len(got) == r and all(same(g, full[EVERYTHING.index(name)]) for name, g in zip(want, got)), want
    assert same(chase_decode(x, code, 4, 0.5, want="metric"), full[3])


def test_prior_and_alpha(gpu):
    code, model = both(63, 2, 6)
    x = noisy_llr(model, 12, 0.6, 1)
    prior = np.random.RandomState(2).randn(12, 63)
    refs = [check(code, model, x, 4, prior=prior, alpha=alpha) for alpha in (0.0, 0.5, 1.0)]
    assert not same(refs[0]["extrinsic"], refs[1]["extrinsic"]) and not same(refs[1]["extrinsic"], refs[2]["extrinsic"])
    assert same(chase_decode(x, code, 4, 0.5, prior=prior[0] * 0 + prior, alpha=0.0, want="extrinsic"), chase_decode(x, code, 4, 0.5, want="extrinsic"))


def device_results(bufs, names, shapes):
    return {name: buf.to_array(*shapes[name]) for name, buf in zip(names, bufs)}


def test_streams_and_device_buffers(gpu):
    code, model = both(255, 2, 8)
    lib = _lib.load()
    x = noisy_llr(model, 37, 0.55, 4)
    prior = 0.5 * np.random.RandomState(5).randn(37, 255)
    host = chase_decode(x, code, 5, 0.7, prior=prior, alpha=0.5, want=EVERYTHING)
    shapes = {"bits": ((37, code.k), np.uint8), "codeword": ((37, 255), np.uint8), "extrinsic": ((37, 255), np.float64),
              "metric": ((37,), np.float64), "candidates": ((37,), np.int32)}
    streams = [ctypes.c_void_p() for _ in range(2)]
    for s in streams:
        _lib.check(lib.cpx_stream_create(ctypes.byref(s)))
    try:
        d_x, d_prior = DeviceBuf.from_array(x), DeviceBuf.from_array(prior)
        outs = [deviceops.bch_chase_dev(code, d_x, 37, 5, 0.7, d_prior=d_prior, alpha=0.5, want=EVERYTHING, stream=s) for s in streams + [None]]
        assert _lib.last_kernel() == "bch_chase_kernel"
        for s in streams + [None]:
            _lib.check(lib.cpx_stream_sync(s))
        for bufs in outs:
            got = device_results(bufs, EVERYTHING, shapes)
            assert all(same(got[name], h) for name, h in zip(EVERYTHING, host))
        d_m = deviceops.bch_chase_dev(code, d_x, 37, 5, 0.7, d_prior=d_prior, alpha=0.5, want="metric")
        # the soft output over the prior
        d_same = deviceops.bch_chase_dev(code, d_x, 37, 5, 0.7, d_prior=d_prior, alpha=0.5, want="extrinsic", d_extrinsic=d_prior)
        _lib.check(lib.cpx_stream_sync(None))
        assert d_same is d_prior and same(d_prior.to_array(*shapes["extrinsic"]), host[2]) and same(d_m.to_array(*shapes["metric"]), host[3])
    finally:
        for s in streams:
            lib.cpx_stream_destroy(s)


def test_rows_and_columns_of_a_block_in_place(gpu):
    """[B, n_c, n_r] = [3, 15, 7]: the rows are words of (7, 4), the columns words of (15, 7); the strided forms equal the flat form on
    the words gathered by the host."""
    row, row_model = both(7, 1, 3)
    col, col_model = both(15, 2, 4)
    rs = np.random.RandomState(9)
    B, nc, nr = 3, 15, 7
    x, prior = 2.0 * rs.randn(B, nc, nr), rs.randn(B, nc, nr)
    lib = _lib.load()
    for axis, code, model, J, strides, k in ((2, row, row_model, nc, (nc * nr, nr, 1), 4), (1, col, col_model, nr, (nc * nr, 1, nr), 7)):
        ref = CM.decode_batch(CM.words_of(x, axis), model, 3, 0.5, CM.words_of(prior, axis), 0.5)
        flat = chase_decode(CM.words_of(x, axis), code, 3, 0.5, prior=CM.words_of(prior, axis), alpha=0.5, want=EVERYTHING)
        assert all(same(f, ref[name].astype(f.dtype)) for name, f in zip(EVERYTHING, flat))
        d_x, d_prior = DeviceBuf.from_array(x), DeviceBuf.from_array(prior)
        bufs = deviceops.bch_chase_dev(code, d_x, B, 3, 0.5, d_prior=d_prior, alpha=0.5, want=EVERYTHING, J=J, strides=strides, d_extrinsic=d_prior)
        _lib.check(lib.cpx_stream_sync(None))
        assert bufs[2] is d_prior
        assert same(bufs[1].to_array((B, nc, nr), np.uint8), CM.block_of(ref["codeword"], (B, nc, nr), axis))
        assert same(d_prior.to_array((B, nc, nr), np.float64), CM.block_of(ref["extrinsic"], (B, nc, nr), axis))
        assert same(bufs[3].to_array((B * J,), np.float64), ref["metric"]) and same(bufs[4].to_array((B * J,), np.int32), ref["candidates"].astype(np.int32))
        bits = bufs[0].to_array((B, J, k) if axis == 2 else (B, k, J), np.uint8)
        want_bits = ref["bits"].reshape(B, J, k)
        assert same(bits, want_bits if axis == 2 else np.ascontiguousarray(want_bits.transpose(0, 2, 1)))
        assert same(d_x.to_array((B, nc, nr), np.float64), x)      # the input is only read


def test_bch_decode_still_equals_its_model_on_the_same_hard_decisions(gpu):
    """Both kernels call the same syndrome, Berlekamp-Massey and Chien code (bch_dev.h, cpx_gf.h)."""
    for n, t, m, pp in ((100, 2, 7, None), (255, 2, 8, None), (1023, 10, 10, None), (3240, 12, 14, DVB_PRIM_POLY)):
        code, model = both(n, t, m, pp)
        hard = (noisy_llr(model, 8, 0.5 if n < 2000 else 0.37, n) < 0).astype(np.uint8)
        ref = M.decode_batch(hard, model)
        bits, word, errors = bch_decode(hard, code, want=("bits", "codeword", "errors"))
        assert _lib.last_kernel() == "bch_decode_kernel"
        assert same(bits, ref["bits"]) and same(word, ref["codeword"]) and same(errors, ref["errors"])


# ---- limits ---------------------------------------------------------------------------------------------------------------------------
def test_limits_are_refused_on_the_host(gpu):
    lib = _lib.load()
    big = BCHCode(16383, 12, m=14)
    with pytest.raises(ValueError, match=r"needs \d+ bytes of LDS"):
        chase_decode(np.ones((1, 16383)), big, 1, 0.5)
    code = BCHCode(15, 2)
    h, buf = code._device_handle(), DeviceBuf(8 * 4 * 60)
    E = _lib.CPX_EINVAL
    args = lambda p=2, B=2, J=4, sb=60, sj=15, si=1, beta=0.5, alpha=1.0, out=buf.ptr: (h, buf.ptr, None, alpha, beta, p, B, J, sb, sj, si, None, None, out,
                                                                                       None, None, None)
    assert lib.cpx_chase_bch_dev(*args(B=0)) == _lib.CPX_OK
    for bad, text in ((args(p=0), "p = 0"), (args(p=9), "p = 9"), (args(B=-1), "B = -1"), (args(J=0), "J = 0"), (args(si=0), "strides"),
                      (args(sj=-1), "strides"), (args(sj=14), "overlap"), (args(sj=1, si=3), "overlap"), (args(sb=59), "blocks overlap"),
                      (args(beta=-1.0), "beta"), (args(beta=float("nan")), "beta"), (args(alpha=float("inf")), "alpha"),
                      (args(out=None), "no output")):
        assert lib.cpx_chase_bch_dev(*bad) == E and text in _lib.last_error(), (text, _lib.last_error())
