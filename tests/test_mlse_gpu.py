"""The equaliser on the GPU against tests/mlse_model.py: every output equals the model's bit for bit (floats by their bit pattern), for
every (M, S) class of the kernel, block lengths round the first L-1 steps, a traceback segment of S steps, the traceback's unrolling
and the length at which the decisions leave LDS, batches on both sides of a workgroup's rows and above the grid's cap, with and without
tail, priors, per-row taps and per-row noise_var."""
import ctypes
import itertools
import re

import numpy as np
import pytest

import mlse_model as M
from commpy_amd import _lib, deviceops
from commpy_amd.channels import multipath_batch
from commpy_amd.deviceops import DeviceBuf
from commpy_amd.equalizers import mlse_equalize_batch
from commpy_amd.modulation import Modem, PSKModem, QAMModem
from mlse_model import draw

pytestmark = pytest.mark.gpu
EVERYTHING = ("indices", "bits", "metric", "llr")
CUSTOM = np.array([1.0 + 0.2j, -0.7 + 1.0j, 0.1 - 1.1j, -1.2 - 0.3j])          # four points, labels in no Gray order
MODEMS = {2: lambda: PSKModem(2), 4: lambda: QAMModem(4), 8: lambda: PSKModem(8), 16: lambda: QAMModem(16),
          'custom': lambda: Modem(CUSTOM, reorder_as_gray=False)}
CASES = [(2, 2), (2, 3), (2, 7), (2, 8), (2, 9), (4, 2), (4, 4), (4, 5), (8, 2), (8, 3), (16, 2), (16, 3), ('custom', 3)]
DEC_LDS_MAX = 49152                                                # csrc/mlse.hip MLSE_DEC_LDS_MAX
# (tail, per-row h, prior, per-row noise_var)
OPTIONS = list(itertools.product((True, False), repeat=4))


def shape(modem, L):
    """``(S, rows per workgroup, waves per row, traceback unrolling)`` of the kernel class."""
    S = modem.m ** (L - 1)
    return S, max(1, 64 // S), max(1, S // 64), (8 if modem.num_bits_symbol <= 2 else 4)


def lengths(modem, L):
    S, _, waves, U = shape(modem, L)
    ns = {1, L - 2, L - 1, L, L + 1, U - 1, U, U + 1, S - 1, S, S + 1}
    edge = DEC_LDS_MAX // (8 * modem.num_bits_symbol * waves)      # the longest block whose decisions stay in LDS
    if edge < 4096:                                                # (BPSK below 128 states never leaves LDS)
        ns |= {edge, edge + 1}
    return sorted(v for v in ns if v >= 1)


def same(got, ref, what=None):
    idx, bits, metric, llr = got
    assert idx.dtype == np.int32 and bits.dtype == np.uint8 and metric.dtype == np.float64 and llr.dtype == np.float64
    assert np.array_equal(idx, ref['indices']), what
    assert np.array_equal(bits, ref['bits']), what
    for g, r in ((metric, ref['metric']), (llr, ref['llr'])):
        assert g.shape == r.shape, what
        assert np.array_equal(np.isnan(g), np.isnan(r)), what
        ok = ~np.isnan(g)
        assert np.array_equal(g[ok].view(np.int64), r[ok].view(np.int64)), what


def inputs(modem, L, n, B, seed, opt):
    tail, per_row_h, with_prior, per_row_nv = opt
    _, y, h = draw(modem, L, n, B, seed, tail, per_row_h=per_row_h)
    rs = np.random.RandomState(seed + 1)
    nv = 0.2 + rs.rand(B) if per_row_nv else 0.2 + rs.rand()
    prior = 2.0 * rs.randn(B, n * modem.num_bits_symbol) if with_prior else None
    return y, h, nv, prior, tail


@pytest.mark.parametrize("M_, L", CASES)
def test_equals_the_model(gpu, M_, L):
    modem = MODEMS[M_]()
    S, R, waves, _ = shape(modem, L)
    const = modem.constellation
    seen = set()
    for k, n in enumerate(lengths(modem, L)):
        opt = OPTIONS[(5 * k + L) % 16]
        B = R + 3
        y, h, nv, prior, tail = inputs(modem, L, n, B, 100 * n + L, opt)
        ref = M.equalize(y, h, const, nv, prior, tail, soft=True)
        got = mlse_equalize_batch(y, h, modem, nv, prior, tail, want=EVERYTHING)
        same(got, ref, (M_, L, n, opt))
        name = _lib.last_kernel()
        assert name.startswith("mlse_kernel<%d,%d> rows=%d " % (modem.num_bits_symbol, modem.num_bits_symbol * (L - 1), R)), name
        assert ("dec=lds" in name) == (8 * modem.num_bits_symbol * waves * n <= DEC_LDS_MAX), name
        for b in sorted({1, max(R - 1, 1), R + 1}):                # one row, a workgroup short of one row, a workgroup and one row
            sub = mlse_equalize_batch(y[:b], h[:b] if opt[1] else h, modem, nv[:b] if opt[3] else nv, None if prior is None else prior[:b],
                                      tail, want=EVERYTHING)
            same(sub, {key: v[:b] for key, v in ref.items()}, (M_, L, n, opt, b))
        # the hard call alone: no noise_var needed without a prior
        if prior is None:
            idx, metric = mlse_equalize_batch(y, h, modem, tail=tail, want=("indices", "metric"))
            assert np.array_equal(idx, ref['indices']) and np.array_equal(metric.view(np.int64), ref['metric'].view(np.int64))
        seen.add(opt)
    for pos in range(4):
        assert {o[pos] for o in seen} == {True, False}


@pytest.mark.parametrize("M_, L, n", [(2, 2, 2), (4, 4, 2), (16, 3, 2), (16, 3, 385)])
def test_batch_above_the_grid(gpu, M_, L, n):
    """Workgroups take a second group of rows; at n = 385 the decisions and alpha of the 256-state class are in arena slabs, which the
    second group writes over."""
    modem = MODEMS[M_]()
    S, R, _, _ = shape(modem, L)
    y, h, nv, prior, tail = inputs(modem, L, n, 37, 5, (True, True, True, True))
    ref = M.equalize(y, h, modem.constellation, nv, prior, tail, soft=True)
    same(mlse_equalize_batch(y, h, modem, nv, prior, tail, want=EVERYTHING), ref)
    cap = int(re.search(r"cap=(\d+)", _lib.last_kernel()).group(1))
    B = cap * R + 1
    assert B > 256 and ("dec=arena" in _lib.last_kernel()) == (n > 2)
    tile = lambda v: np.resize(v, (B,) + v.shape[1:])
    got = mlse_equalize_batch(tile(y), tile(h), modem, tile(nv), tile(prior), tail, want=EVERYTHING)
    same(got, {key: tile(v) for key, v in ref.items()})


def test_exact_ties(gpu):
    """Gaussian-integer y and h with BPSK: every metric is an integer, ties are exact and the first minimum decides."""
    modem = PSKModem(2)
    rs = np.random.RandomState(11)
    for L in (2, 3, 5):
        B, n = 40, 33
        h = rs.randint(-1, 2, (B, L)) + 1j * rs.randint(-1, 2, (B, L))
        y = rs.randint(-2, 3, (B, n + L - 1)) + 1j * rs.randint(-2, 3, (B, n + L - 1))
        h[0], y[1] = 0, 0                                          # every sequence ties | every step ties
        ref = M.equalize(y, h, np.round(modem.constellation), 2.0, None, True, soft=True)
        assert (ref['metric'] == np.round(ref['metric'])).all() and (ref['llr'] == 0).any()
        tied = Modem(np.round(modem.constellation), reorder_as_gray=False)
        same(mlse_equalize_batch(y, h, tied, 2.0, want=EVERYTHING), ref, L)
        assert not ref['indices'][0].any()


def test_rejected_rows_stay_in_their_row(gpu):
    modem = QAMModem(4)
    y, h, nv, prior, tail = inputs(modem, 3, 20, 9, 21, (True, True, True, True))
    clean = M.equalize(y, h, modem.constellation, nv, prior, tail, soft=True)
    y, h, nv, prior = y.copy(), h.copy(), nv.copy(), prior.copy()
    y[0, 0] = np.nan
    y[1, 21] = complex(0.0, np.inf)                                # in the tail
    h[2, 2] = -np.inf
    h[3, 0] = complex(np.nan, 1.0)
    prior[4, 39], prior[5, 0] = np.nan, np.inf
    nv[6], nv[7] = np.inf, np.nan
    ref = M.equalize(y, h, modem.constellation, nv, prior, tail, soft=True)
    assert np.isnan(ref['metric'][:8]).all() and not np.isnan(ref['metric'][8])
    got = mlse_equalize_batch(y, h, modem, nv, prior, tail, want=EVERYTHING)
    same(got, ref)
    assert not got[0][:8].any() and not got[1][:8].any() and np.isnan(got[3][:8]).all()
    assert np.array_equal(got[3][8].view(np.int64), clean['llr'][8].view(np.int64))
    # a shared h or a scalar noise_var that is not finite rejects every row
    for bad_h, bad_nv in ((np.array([1.0, np.nan, 0.5]), 1.0), (np.array([1.0, 0.2, 0.5]), np.inf)):
        idx, metric, llr = mlse_equalize_batch(y[8:], bad_h, modem, bad_nv, want=("indices", "metric", "llr"))
        assert not idx.any() and np.isnan(metric).all() and np.isnan(llr).all()


def test_same_bits_whatever_the_call(gpu):
    """Batch size, row position, stream, host or device form and the subset of ``want`` change no bit."""
    modem = PSKModem(8)
    L, n, B = 3, 70, 11
    y, h, nv, prior, tail = inputs(modem, L, n, B, 31, (True, True, True, True))
    ref = M.equalize(y, h, modem.constellation, nv, prior, tail, soft=True)
    same(mlse_equalize_batch(y, h, modem, nv, prior, tail, want=EVERYTHING), ref)
    # row positions: reversed
    rev = mlse_equalize_batch(y[::-1], h[::-1], modem, nv[::-1], prior[::-1], tail, want=EVERYTHING)
    same(rev, {key: v[::-1] for key, v in ref.items()})
    # subsets of want, and one row as a 1-D call
    for r in range(1, 4):
        for names in itertools.combinations(EVERYTHING, r):
            got = mlse_equalize_batch(y, h, modem, nv, prior, tail, want=names)
            got = (got,) if len(names) == 1 else got
            for g, key in zip(got, names):
                assert np.array_equal(g.view(np.int64) if g.dtype == np.float64 else g,
                                      ref[key].view(np.int64) if g.dtype == np.float64 else ref[key]), names
    one = mlse_equalize_batch(y[4], h[4], modem, nv[4], prior[4], tail, want=EVERYTHING)
    same(tuple(v[None] for v in one[:2]) + (np.array([one[2]]), one[3][None]), {key: v[4:5] for key, v in ref.items()})
    # the device form on a stream of its own, twice on two streams
    lib = _lib.load()
    streams = []
    for _ in range(2):
        st = ctypes.c_void_p()
        _lib.check(lib.cpx_stream_create(ctypes.byref(st)))
        streams.append(st)
    try:
        as_pairs = lambda v: np.ascontiguousarray(v, dtype=np.complex128).view(np.float64)
        d_y, d_h, d_nv, d_pr = (DeviceBuf.from_array(v) for v in (as_pairs(y), as_pairs(h), nv, prior))
        outs = [deviceops.mlse_equalize_dev(modem, d_y, d_h, True, B, n, L, d_nv, True, d_pr, tail, want=EVERYTHING, stream=st)
                for st in streams]
        for st, out in zip(streams, outs):
            _lib.check(lib.cpx_stream_sync(st))
            m = modem.num_bits_symbol
            got = (out[0].to_array((B, n), np.int32), out[1].to_array((B, n * m), np.uint8), out[2].to_array((B,), np.float64),
                   out[3].to_array((B, n * m), np.float64))
            same(got, ref)
        d_idx = deviceops.mlse_equalize_dev(modem, d_y, d_h, True, B, n, L, d_nv, True, d_pr, tail, stream=streams[0])
        _lib.check(lib.cpx_stream_sync(streams[0]))
        assert np.array_equal(d_idx.to_array((B, n), np.int32), ref['indices'])
    finally:
        for st in streams:
            lib.cpx_stream_destroy(st)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_noise_free_chain_recovers_every_index(gpu, seed):
    rs = np.random.RandomState(seed)
    for M_, L in ((2, 5), (4, 4), (8, 3), (16, 2), ('custom', 3)):
        modem = MODEMS[M_]()
        m, B, n = modem.num_bits_symbol, 7, 50
        bits = rs.randint(0, 2, (B, n * m))
        x = modem.modulate(bits.reshape(-1)).reshape(B, n)
        h = (rs.randn(B, L) + 1j * rs.randn(B, L)) / np.sqrt(2 * L)
        h[:, 0] += 1.0                                             # a clear first tap: distinct sequences give distinct waveforms
        y = multipath_batch(x, h)
        idx, out, llr = mlse_equalize_batch(y, h, modem, 0.1, want=("indices", "bits", "llr"))
        assert np.array_equal(out, bits)
        assert np.array_equal(idx, bits.reshape(B, n, m).dot(1 << np.arange(m - 1, -1, -1)))
        assert np.array_equal(llr < 0, bits == 1) and (llr != 0).all()


def test_engine_refuses_the_limits(gpu):
    lib = _lib.load()
    h16, h2 = QAMModem(16)._device_handle(), PSKModem(2)._device_handle()
    h64 = QAMModem(64)._device_handle()
    buf = DeviceBuf(1 << 16)
    call = lambda md, n, L, nvp=None, llr=None: lib.cpx_mlse_dev(md, buf.ptr, buf.ptr, 0, 1, n, L, 1, nvp, 0, None, buf.ptr, None, None, llr,
                                                                None)
    assert call(h2, 10, 1) == _lib.CPX_EINVAL and "L >= 2" in _lib.last_error()
    assert call(h64, 10, 2) == _lib.CPX_EINVAL and "2 to 16" in _lib.last_error()
    assert call(h16, 10, 4) == _lib.CPX_EINVAL and "M^(L-1) <= 256" in _lib.last_error()
    assert call(h2, 10, 10) == _lib.CPX_EINVAL and "M^(L-1) <= 256" in _lib.last_error()
    assert call(h2, 0, 2) == _lib.CPX_EINVAL and call(h2, 4097, 2) == _lib.CPX_EINVAL and "1 <= n <= 4096" in _lib.last_error()
    assert call(h2, 10, 2, None, buf.ptr) == _lib.CPX_EINVAL and "noise_var is required" in _lib.last_error()
