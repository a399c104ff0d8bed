"""The MMSE linear and decision-feedback equalisers on the GPU against tests/equalize_model.py: every output equals the model's bit for
bit (floats by their bit pattern, NaNs by position), at the smallest and largest tap counts, delays at both ends, block lengths round
the filter kernel's tile of 256 steps, batches on both sides of a wave of 64 rows and above every grid cap, shared and per-row taps and
noise_var, with and without tail, every constellation size and one in no Gray order."""
import ctypes
import re

import numpy as np
import pytest

import equalize_model as E
from commpy_amd import _lib, deviceops
from commpy_amd.channels import multipath_batch
from commpy_amd.deviceops import DeviceBuf
from commpy_amd.equalizers import MMSE_WANT, mmse_equalize_batch
from commpy_amd.modulation import Modem, PSKModem, QAMModem
from mlse_model import draw

pytestmark = pytest.mark.gpu
EVERYTHING = MMSE_WANT
TILE = 256                                                                       # csrc/equalize.hip EQ_TILE
CUSTOM = np.array([1.0 + 0.2j, -0.7 + 1.0j, 0.1 - 1.1j, -1.2 - 0.3j])          # four points, labels in no Gray order
MODEMS = {2: lambda: PSKModem(2), 4: lambda: QAMModem(4), 16: lambda: QAMModem(16), 64: lambda: QAMModem(64), 256: lambda: QAMModem(256),
          'custom': lambda: Modem(CUSTOM, reorder_as_gray=False)}
# (nf, L, nb, delay ('first' = 0, None = the default, 'last' = nf + L - 2 - nb), n, M)
CASES = [(1, 1, 0, None, 1, 2), (2, 2, 1, None, 2, 4), (2, 2, 0, 'last', 2, 'custom'), (63, 2, 0, 'first', TILE - 1, 16),
         (64, 64, 63, None, TILE, 4), (64, 2, 64, 'last', TILE + 1, 4), (63, 64, 0, None, TILE + 1, 2), (2, 1, 1, 'first', 2, 64),
         (3, 2, 1, None, 2, 256), (64, 2, 1, 'last', TILE, 16), (5, 3, 2, None, TILE + 44, 64), (1, 2, 0, 'last', 1, 'custom')]


def the_delay(kind, nf, L, nb):
    return {'first': 0, None: None, 'last': nf + L - 2 - nb}[kind]


def same(got, ref, names=EVERYTHING, what=None):
    got = (got,) if len(names) == 1 else got
    assert len(got) == len(names)
    for g, key in zip(got, names):
        r = ref[key]
        assert g.shape == r.shape and g.dtype == r.dtype, (what, key, g.shape, r.shape, g.dtype)
        if g.dtype.kind in 'iu':
            assert np.array_equal(g, r), (what, key)
            continue
        g, r = np.ascontiguousarray(g).view(np.float64), np.ascontiguousarray(r).view(np.float64)
        assert np.array_equal(np.isnan(g), np.isnan(r)), (what, key)
        ok = ~np.isnan(g)
        assert np.array_equal(g[ok].view(np.int64), r[ok].view(np.int64)), (what, key)


def inputs(modem, L, n, B, seed, tail=True, per_row_h=True, per_row_nv=True, snr_db=12.0):
    _, y, h = draw(modem, L, n, B, seed, tail, snr_db, per_row_h)
    rs = np.random.RandomState(seed + 1)
    nv = modem.Es * (0.05 + 0.1 * (rs.rand(B) if per_row_nv else rs.rand()))
    return y, h, nv


def model(y, h, modem, nv, nf, nb, delay, tail=True):
    return E.equalize(y, h, modem.constellation, modem.Es, nv, nf, nb, delay, tail)


@pytest.mark.parametrize("k", range(len(CASES)))
def test_equals_the_model(gpu, k):
    nf, L, nb, kind, n, M_ = CASES[k]
    modem, delay = MODEMS[M_](), the_delay(kind, nf, L, nb)
    tail, per_row_h, per_row_nv = ((k >> 0) & 1) == 0, ((k >> 1) & 1) == 0, ((k >> 2) & 1) == 0
    y, h, nv = inputs(modem, L, n, 3, 100 + k, tail, per_row_h, per_row_nv)
    ref = model(y, h, modem, nv, nf, nb, delay, tail)
    assert not np.isnan(ref['gain']).any()
    got = mmse_equalize_batch(y, h, modem, nv, nf, nb, delay, tail, want=EVERYTHING)
    name = _lib.last_kernel()
    assert name.startswith("%s<%d> nf=%d nb=%d designs=3 " % ("eq_dfe_kernel" if nb else "eq_filter_kernel", modem.num_bits_symbol, nf, nb)), name
    same(got, ref, what=CASES[k])
    # the hard call alone: the kernels without the per-bit minima, and one design for all rows where nothing differs between them
    idx = mmse_equalize_batch(y, h, modem, nv, nf, nb, delay, tail)
    assert np.array_equal(idx, ref['indices'])
    assert ("<0> nf=%d nb=%d designs=%d " % (nf, nb, 3 if per_row_h or per_row_nv else 1)) in _lib.last_kernel(), _lib.last_kernel()


@pytest.mark.parametrize("nb", [0, 2])
def test_batch_sizes_round_a_wave(gpu, nb):
    """One row, one row short of a wave of 64 rows, one over; shared taps and noise_var solve one design for all of them."""
    modem = QAMModem(16)
    nf, L, n = 6, 3, 9
    y, h, nv = inputs(modem, L, n, 65, 7, per_row_h=False, per_row_nv=False)
    ref = model(y, h, modem, nv, nf, nb, None)
    replicated = np.broadcast_to(h, (65, L)).copy()
    for B in (1, 63, 65):
        sub = {key: v[:B] for key, v in ref.items()}
        same(mmse_equalize_batch(y[:B], h, modem, nv, nf, nb, want=EVERYTHING), sub, what=B)
        assert "designs=%d " % B in _lib.last_kernel()
        names = ("indices", "bits", "estimate", "llr")
        same(mmse_equalize_batch(y[:B], h, modem, nv, nf, nb, want=names), sub, names, B)
        assert "designs=1 " in _lib.last_kernel()
        same(mmse_equalize_batch(y[:B], replicated[:B], modem, np.full(B, nv), nf, nb, want=names), sub, names, B)
        assert "designs=%d " % B in _lib.last_kernel()


def test_batch_above_every_grid_cap(gpu):
    """Every workgroup of the design, filter and feedback kernels takes a second item."""
    modem = PSKModem(2)
    y, h, nv = inputs(modem, 2, 2, 70, 9)
    ref = model(y, h, modem, nv, 1, 1, 0)
    same(mmse_equalize_batch(y, h, modem, nv, 1, 1, 0, want=EVERYTHING), ref)
    caps = {key: int(v) for key, v in re.findall(r"(\w+)_cap=(\d+)", _lib.last_kernel())}
    B = max(caps['design'], caps['filter'], 64 * caps['dfe']) + 1
    tile = lambda v: np.resize(v, (B,) + v.shape[1:])
    got = mmse_equalize_batch(tile(y), tile(h), modem, tile(nv), 1, 1, 0, want=EVERYTHING)
    same(got, {key: tile(v) for key, v in ref.items()})
    got = mmse_equalize_batch(tile(y)[:caps['filter'] + 1], tile(h)[:caps['filter'] + 1], modem, tile(nv)[:caps['filter'] + 1], 1, 0, 0,
                              want=EVERYTHING)
    lin = model(y, h, modem, nv, 1, 0, 0)
    same(got, {key: np.resize(v, (caps['filter'] + 1,) + v.shape[1:]) for key, v in lin.items()})


def test_exact_ties(gpu):
    """L = nf = 1, h = 1, Es = 1, noise_var = 1: R = 2, p = 1, u = 1/2 and gain = 1/2, so x^ = y exactly and nu = 1.  With the
    Gaussian-integer points (1, i, -1, -i) and y at midpoints the first minimum wins and the LLRs of the tied bits are exactly 0."""
    tied = Modem(np.array([1.0, 1.0j, -1.0, -1.0j]), reorder_as_gray=False)
    assert tied.Es == 1.0
    y = np.array([[0.0, 0.5 + 0.5j, -0.5 + 0.5j, 0.5 - 0.5j, 1.0, 2.0j, -0.5 - 0.5j, 0.25]])
    ref = E.equalize(y, np.ones(1), tied.constellation, tied.Es, 1.0, 1, 0, None)
    assert ref['gain'][0] == 0.5 and ref['noise'][0] == 1.0 and np.array_equal(ref['estimate'], y)
    assert ref['indices'][0].tolist() == [0, 0, 1, 0, 0, 1, 2, 0]
    assert (ref['llr'][0].reshape(-1, 2)[:4] == [[0, 0], [2, 0], [0, 0], [0, 0]]).all()
    same(mmse_equalize_batch(y, np.ones(1), tied, 1.0, 1, want=EVERYTHING), ref)
    # the same with a feedback tap: h = (1, 1), nf = 1, nb = 1, delay 0, so x^_t = y_t - c[a^_{t-1}]: 1, 0, 1/2 + i/2, i
    y2 = np.array([[1.0, 1.0, 1.5 + 0.5j, 1.0 + 1.0j, 1.0j]])
    ref = E.equalize(y2, np.ones(2), tied.constellation, tied.Es, 1.0, 1, 1, 0)
    assert ref['indices'][0].tolist() == [0, 0, 0, 1] and (ref['llr'][0, 2:4] == 0).all() and ref['fb'][0, 0] == 0.5
    same(mmse_equalize_batch(y2, np.ones(2), tied, 1.0, 1, 1, 0, want=EVERYTHING), ref)


@pytest.mark.parametrize("nb", [0, 2])
def test_rejected_rows_stay_in_their_row(gpu, nb):
    modem = QAMModem(4)
    nf, L, n = 5, 3, 20
    y, h, nv = inputs(modem, L, n, 9, 21)
    clean = model(y, h, modem, nv, nf, nb, None)
    y, h, nv = y.copy(), h.copy(), nv.copy()
    y[0, 0] = np.nan
    y[1, 21] = complex(0.0, np.inf)                                # in the tail
    h[2, 2] = -np.inf
    h[3, 0] = complex(np.nan, 1.0)
    nv[4], nv[5] = np.inf, np.nan
    h[6] = 0.0                                                     # gain = 0
    ref = model(y, h, modem, nv, nf, nb, None)
    assert np.isnan(ref['gain'][:7]).all() and not np.isnan(ref['gain'][7:]).any()
    got = mmse_equalize_batch(y, h, modem, nv, nf, nb, want=EVERYTHING)
    same(got, ref)
    assert not got[0][:7].any() and not got[1][:7].any() and all(np.isnan(g[:7].view(np.float64)).all() for g in got[2:])
    same(tuple(g[7:] for g in got), {key: v[7:] for key, v in clean.items()})
    # a shared h or a scalar noise_var that is not finite rejects every row; a y that is not finite only its own
    for bad_h, bad_nv in ((np.array([1.0, np.nan, 0.5]), 1.0), (np.array([1.0, 0.2, 0.5]), np.inf), (np.zeros(3), 1.0)):
        idx, est, llr = mmse_equalize_batch(y[7:], bad_h, modem, bad_nv, nf, nb, want=("indices", "estimate", "llr"))
        assert not idx.any() and np.isnan(est.view(np.float64)).all() and np.isnan(llr).all()
    shared = model(y, h[8], modem, nv[8], nf, nb, None)
    names = ("indices", "estimate", "llr")
    same(mmse_equalize_batch(y, h[8], modem, nv[8], nf, nb, want=names), shared, names)
    assert "designs=1 " in _lib.last_kernel() and np.isnan(shared['llr'][:2]).all() and not np.isnan(shared['llr'][2:]).any()


@pytest.mark.parametrize("nb", [0, 3])
def test_same_bits_whatever_the_call(gpu, nb):
    """Batch size, row position, stream, host or device form and the subset of ``want`` change no bit."""
    modem = QAMModem(16)
    nf, L, n, B = 7, 4, 70, 11
    y, h, nv = inputs(modem, L, n, B, 31)
    ref = model(y, h, modem, nv, nf, nb, None)
    same(mmse_equalize_batch(y, h, modem, nv, nf, nb, want=EVERYTHING), ref)
    same(mmse_equalize_batch(y[::-1], h[::-1], modem, nv[::-1], nf, nb, want=EVERYTHING), {key: v[::-1] for key, v in ref.items()})
    # a subset of every size, each name in some subset; one row as a 1-D call
    for r in range(1, len(EVERYTHING)):
        for start in range(0, len(EVERYTHING), 3):
            names = tuple(sorted((EVERYTHING[(start + i) % len(EVERYTHING)] for i in range(r)), key=EVERYTHING.index))
            same(mmse_equalize_batch(y, h, modem, nv, nf, nb, want=names), ref, names, names)
    one = mmse_equalize_batch(y[4], h[4], modem, nv[4], nf, nb, want=EVERYTHING)
    same(tuple(np.asarray(v)[None] for v in one), {key: v[4:5] for key, v in ref.items()})
    lib = _lib.load()
    streams = []
    for _ in range(2):
        st = ctypes.c_void_p()
        _lib.check(lib.cpx_stream_create(ctypes.byref(st)))
        streams.append(st)
    try:
        as_pairs = lambda v: np.ascontiguousarray(v, dtype=np.complex128).view(np.float64)
        d_y, d_h, d_nv = (DeviceBuf.from_array(v) for v in (as_pairs(y), as_pairs(h), nv))
        outs = [deviceops.mmse_equalize_dev(modem, d_y, d_h, True, B, n, L, d_nv, True, nf, nb, want=EVERYTHING, stream=st) for st in streams]
        shapes = {key: (v.shape, v.dtype) for key, v in ref.items()}
        for st, out in zip(streams, outs):
            _lib.check(lib.cpx_stream_sync(st))
            same(tuple(o.to_array(*shapes[key]) for o, key in zip(out, EVERYTHING)), ref)
        d_idx = deviceops.mmse_equalize_dev(modem, d_y, d_h, True, B, n, L, d_nv, True, nf, nb, stream=streams[0])
        _lib.check(lib.cpx_stream_sync(streams[0]))
        assert np.array_equal(d_idx.to_array((B, n), np.int32), ref['indices'])
    finally:
        for st in streams:
            lib.cpx_stream_destroy(st)


def test_channel_b_end_to_end(gpu):
    """modulate -> multipath_batch -> noise -> mmse_equalize_batch on Proakis' channel B, QPSK at 14 dB: the error counts of the
    linear and the feedback equaliser equal the model's, so their order, asserted on the model, holds here too."""
    modem = QAMModem(4)
    rs = np.random.RandomState(3)
    B, n = 8, 250
    bits = rs.randint(0, 2, (B, 2 * n))
    x = modem.modulate(bits.reshape(-1)).reshape(B, n)
    taps = np.array([0.407, 0.815, 0.407])
    N0 = modem.Es / 10 ** 1.4
    y = multipath_batch(x, taps) + np.sqrt(N0 / 2) * (rs.randn(B, n + 2) + 1j * rs.randn(B, n + 2))
    counts = []
    for nb in (0, 2):
        ref = model(y, taps, modem, N0, 16, nb, None)
        out = mmse_equalize_batch(y, taps, modem, N0, 16, nb, want='bits')
        assert np.array_equal(out, ref['bits'])
        counts.append(int((out != bits).sum()))
        assert counts[-1] == int((ref['bits'] != bits).sum())
    print("channel B on the device: LE %d, DFE %d bit errors of %d" % (counts[0], counts[1], bits.size))
    assert counts[1] < counts[0]


def test_engine_refuses_the_limits(gpu):
    lib = _lib.load()
    h4, h64 = QAMModem(4)._device_handle(), QAMModem(64)._device_handle()
    buf, out = DeviceBuf.from_array(np.ones(1 << 10)), DeviceBuf(1 << 10)
    call = lambda md, n, L, nf, nb, d, nvp=buf.ptr, es=1.0: lib.cpx_mmse_equalize_dev(md, es, buf.ptr, buf.ptr, 0, 1, n, L, 1, nvp, 0, nf, nb,
                                                                                     d, out.ptr, *((None,) * 7), None)
    for args, limit in (((h4, 10, 65, 4, 0, 0), "1 <= L <= 64"), ((h4, 10, 0, 4, 0, 0), "1 <= L <= 64"), ((h4, 10, 3, 0, 0, 0), "1 <= nf <= 64"),
                        ((h4, 10, 3, 65, 0, 0), "1 <= nf <= 64"), ((h4, 10, 3, 4, 65, 0), "0 <= nb <= 64"), ((h4, 10, 3, 4, -1, 0), "0 <= nb <= 64"),
                        ((h4, 10, 3, 4, 0, -1), "0 <= delay"), ((h4, 10, 3, 4, 2, 4), "delay + nb <= nf + L - 2"),
                        ((h4, 0, 3, 4, 0, 0), "1 <= n"), ((h4, 10, 3, 4, 0, 0, None), "noise_var is required"),
                        ((h4, 10, 3, 4, 0, 0, buf.ptr, 0.0), "Es must be positive")):
        assert call(*args) == _lib.CPX_EINVAL and limit in _lib.last_error(), (limit, _lib.last_error())
    assert call(h64, 10, 3, 4, 0, 0) == _lib.CPX_OK                # 64-QAM is within the limits
    assert out.to_array((10,), np.int32).max() < 64
