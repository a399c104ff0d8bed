"""The adaptive equalisers on the GPU against tests/adaptive_model.py: every output equals the model's bit for bit (floats by their bit
pattern, NaNs by position), at the smallest and largest tap counts, both row layouts of the LMS kernel (64 and 32 rows per wave) and
the sizes on either side of the switch, RLS at 1, 8 and 32 taps, every constellation size, T, T/2 and T/3 spacing, block lengths that
wrap the history rings, batches on both sides of a wave and above every grid cap."""
import ctypes
import itertools
import re

import numpy as np
import pytest

import adaptive_model as A
from commpy_amd import _lib, deviceops
from commpy_amd.channels import awgn, multipath_batch
from commpy_amd.deviceops import DeviceBuf
from commpy_amd.equalizers import ADAPT_WANT, adaptive_equalize_batch
from commpy_amd.modulation import Modem, PSKModem, QAMModem

pytestmark = pytest.mark.gpu
EVERYTHING = ADAPT_WANT
CUSTOM = np.array([1.0 + 0.2j, -0.7 + 1.0j, 0.1 - 1.1j, -1.2 - 0.3j])          # four points, labels in no Gray order
# a modem handle holds a power-of-two constellation only (cpx_modem_create), so three points reach no kernel: the model runs them in
# test_adaptive_host.py, and the refusal of 'bits' for them is tested there on both layers
MODEMS = {2: lambda: PSKModem(2), 4: lambda: QAMModem(4), 16: lambda: QAMModem(16), 64: lambda: QAMModem(64), 256: lambda: QAMModem(256),
          'custom': lambda: Modem(CUSTOM, reorder_as_gray=False)}
TAPS = np.array([1.0, 0.3 + 0.2j, -0.1j])
PARAMS = {'lms': dict(step=0.01), 'nlms': dict(step=0.3), 'rls': dict(forgetting=0.98, delta=0.05)}
# (algorithm, nf, nb, M, sps, nt ('zero' = none, with non-zero ff0; 'one'; 'all' = n), n)
CASES = [('lms', 1, 0, 2, 1, 'one', 1), ('lms', 7, 1, 16, 2, 'all', 65), ('lms', 64, 64, 4, 1, 'all', 130), ('nlms', 64, 7, 64, 3, 'one', 65),
         ('nlms', 7, 64, 256, 1, 'zero', 130), ('lms', 1, 7, 'custom', 1, 'all', 65), ('nlms', 7, 0, 16, 2, 'zero', 130),
         ('lms', 64, 24, 16, 1, 'all', 65), ('lms', 64, 25, 4, 1, 'one', 65),       # 64 and 32 rows per wave, either side of the switch
         ('rls', 1, 0, 2, 1, 'all', 65), ('rls', 7, 1, 16, 2, 'one', 130), ('rls', 32, 0, 64, 3, 'all', 65), ('rls', 1, 31, 4, 1, 'all', 130),
         ('rls', 7, 1, 'custom', 1, 'zero', 1)]


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


def draw(modem, n, B, seed, sps=1):
    """``(idx [B, n], y [B, n sps + 2])``: the symbols, zero-stuffed by ``sps``, through TAPS, with a little noise."""
    rs = np.random.RandomState(seed)
    idx = rs.randint(0, modem.m, (B, n))
    up = np.zeros((B, n * sps), dtype=np.complex128)
    up[:, ::sps] = modem.constellation[idx]
    y = np.stack([np.convolve(up[b], TAPS) for b in range(B)])
    return idx, y + 0.03 * np.sqrt(modem.Es) * (rs.randn(*y.shape) + 1j * rs.randn(*y.shape))


def start_taps(rs, B, nf, nb, d, per_row):
    """Initial taps near a pass-through: 1 at the delay (where a tap is there), small elsewhere."""
    shape = (B,) if per_row else ()
    ff0 = 0.05 * (rs.randn(*shape, nf) + 1j * rs.randn(*shape, nf))
    ff0[..., min(d, nf - 1)] += 1.0
    return ff0, 0.05 * (rs.randn(*shape, nb) + 1j * rs.randn(*shape, nb))


def model(y, modem, tr, nf, nb, algorithm, **kw):
    return A.equalize(y, modem.constellation, tr, nf, nb, algorithm, **kw)


@pytest.mark.parametrize("k", range(len(CASES)))
def test_equals_the_model(gpu, k):
    algorithm, nf, nb, M_, sps, kind, n = CASES[k]
    modem, B = MODEMS[M_](), 3
    per_row_tr, per_row_par, per_row_taps = ((k >> 0) & 1) == 0, ((k >> 1) & 1) == 0, ((k >> 2) & 1) == 0
    idx, y = draw(modem, n, B, 200 + k, sps)
    nt = {'zero': 0, 'one': 1, 'all': n}[kind]
    tr = idx[:, :nt] if per_row_tr else idx[0, :nt]
    rs = np.random.RandomState(300 + k)
    kw = {key: (v * (1 + 0.2 * rs.rand(B)) if per_row_par and key != 'forgetting' else v) for key, v in PARAMS[algorithm].items()}
    kw.update(sps=sps, n=n)
    if kind == 'zero' or k % 2:
        kw['ff0'], kw['fb0'] = start_taps(rs, B, nf, nb, A.default_delay(nf, nb), per_row_taps)
    ref = model(y, modem, tr, nf, nb, algorithm, **kw)
    assert not ref['bad'].any()
    names = EVERYTHING
    got = adaptive_equalize_batch(y, modem, tr, nf, nb, algorithm, want=names, **kw)
    name = _lib.last_kernel()
    if algorithm == 'rls':
        assert name.startswith("ad_rls_kernel nf=%d nb=%d rows_per_wave=2 " % (nf, nb)), name
    else:
        width = 1 << (nf - 1).bit_length()
        assert name.startswith("ad_lms_kernel %s nf=%d nb=%d rows_per_wave=%d " % (algorithm, nf, nb, 64 if nf + nb + width <= 152 else 32)), name
    same(got, ref, names, CASES[k])
    assert np.array_equal(adaptive_equalize_batch(y, modem, tr, nf, nb, algorithm, **kw), ref['indices'])


@pytest.mark.parametrize("algorithm,nf,nb", [('lms', 5, 2), ('nlms', 4, 0), ('rls', 5, 2)])
def test_batch_sizes_round_a_wave(gpu, algorithm, nf, nb):
    """One row, one short of a wave of 64 rows, a wave, one over, two waves and two rows: every row equals the same row computed alone
    (the model computes every row on its own)."""
    modem, n, nt = QAMModem(16), 9, 4
    idx, y = draw(modem, n, 130, 17)
    kw = dict(PARAMS[algorithm], n=n)
    ref = model(y, modem, idx[:, :nt], nf, nb, algorithm, **kw)
    for B in (1, 63, 64, 65, 130):
        sub = {key: v[:B] for key, v in ref.items()}
        same(adaptive_equalize_batch(y[:B], modem, idx[:B, :nt], nf, nb, algorithm, want=EVERYTHING, **kw), sub, what=B)
    alone = adaptive_equalize_batch(y[77], modem, idx[77, :nt], nf, nb, algorithm, want=EVERYTHING, **kw)
    same(tuple(np.asarray(v)[None] for v in alone), {key: v[77:78] for key, v in ref.items()})


@pytest.mark.parametrize("algorithm", ['lms', 'rls'])
def test_batch_above_the_grid_cap(gpu, algorithm):
    """Every workgroup takes a second group of rows."""
    modem, n, nf, nb = PSKModem(2), 2, 1, 1
    idx, y = draw(modem, n, 70, 19)
    kw = dict(PARAMS[algorithm], n=n)
    ref = model(y, modem, idx[:, :1], nf, nb, algorithm, **kw)
    same(adaptive_equalize_batch(y, modem, idx[:, :1], nf, nb, algorithm, want=EVERYTHING, **kw), ref)
    name = _lib.last_kernel()
    cap, rows = int(re.search(r"(?:lms|rls)_cap=(\d+)", name).group(1)), int(re.search(r"rows_per_wave=(\d+)", name).group(1))
    B = cap * rows + 1
    tile = lambda v: np.resize(v, (B,) + v.shape[1:])
    got = adaptive_equalize_batch(tile(y), modem, tile(idx[:, :1]), nf, nb, algorithm, want=EVERYTHING, **kw)
    same(got, {key: tile(v) for key, v in ref.items()})


@pytest.mark.parametrize("algorithm", ['lms', 'rls'])
def test_exact_ties(gpu, algorithm):
    """Gaussian-integer points (1, i, -1, -i); ff0 = 1, so z_0 = y_0 exactly: on a decision boundary the first minimum wins.  With a
    feedback tap fb0 = 1 and a first symbol received exactly (e_0 = 0: no tap moves), z_1 = y_1 - c[a_0] exactly."""
    tied = Modem(np.array([1.0, 1.0j, -1.0, -1.0j]), reorder_as_gray=False)
    kw = PARAMS[algorithm]
    y = np.array([0.0, 0.5 + 0.5j, -0.5 + 0.5j, 0.5 - 0.5j, 1.0, 2.0j, -0.5 - 0.5j, 0.25]).reshape(-1, 1)
    none = np.zeros(0, dtype=int)
    ref = model(y, tied, none, 1, 0, algorithm, ff0=np.ones(1), **kw)
    assert np.array_equal(ref['estimate'], y) and ref['indices'][:, 0].tolist() == [0, 0, 1, 0, 0, 1, 2, 0]
    same(adaptive_equalize_batch(y, tied, none, 1, 0, algorithm, ff0=np.ones(1), want=EVERYTHING, **kw), ref)
    y2 = np.array([[1.0, 1.5 + 0.5j], [1.0j, 0.5 + 0.5j], [-1.0, -0.5 - 0.5j]])
    first = np.array([[0], [1], [2]])
    ref = model(y2, tied, first, 1, 1, algorithm, ff0=np.ones(1), fb0=np.ones(1), delay=0, **kw)
    assert ref['estimate'][:, 1].tolist() == [0.5 + 0.5j, 0.5 - 0.5j, 0.5 - 0.5j] and ref['indices'][:, 1].tolist() == [0, 0, 0]
    same(adaptive_equalize_batch(y2, tied, first, 1, 1, algorithm, ff0=np.ones(1), fb0=np.ones(1), delay=0, want=EVERYTHING, **kw), ref)


def as_pairs(v):
    return np.ascontiguousarray(v, dtype=np.complex128).view(np.float64)


@pytest.mark.parametrize("algorithm", ['lms', 'nlms', 'rls'])
def test_rejected_rows_stay_in_their_row(gpu, algorithm):
    modem, nf, nb, n, nt, B = QAMModem(4), 5, 2, 20, 6, 11
    idx, y = draw(modem, n, B, 23)
    rs = np.random.RandomState(24)
    ff0, fb0 = start_taps(rs, B, nf, nb, 0, True)
    par = {key: np.full(B, v) for key, v in PARAMS[algorithm].items()}
    fixed = dict(delay=0, n=n)                                     # delay 0: no step reads the last two samples of a row
    clean = model(y, modem, idx[:, :nt], nf, nb, algorithm, ff0=ff0, fb0=fb0, **fixed, **par)
    assert not clean['bad'].any()
    y, ff0, fb0, tr = y.copy(), ff0.copy(), fb0.copy(), idx[:, :nt].copy()
    y[0, 3] = np.nan
    y[1, n + 1] = complex(0.0, np.inf)                             # behind the last sample any step reads: the scan finds it
    ff0[2, 1] = complex(np.nan, 1.0)
    fb0[3, 0] = -np.inf
    tr[4, 2] = 4                                                   # a label out of range
    if algorithm == 'rls':
        par['delta'][5], par['forgetting'][6], par['delta'][7] = np.nan, np.nan, np.inf
    else:
        par['step'][5], par['step'][6], par['step'][7] = 1e200, np.nan, np.inf      # row 5 diverges: the model's own z stops being finite
    ref = model(y, modem, tr, nf, nb, algorithm, ff0=ff0, fb0=fb0, **fixed, **par)
    assert ref['bad'].tolist() == [True] * 8 + [False] * 3
    got = adaptive_equalize_batch(y, modem, tr, nf, nb, algorithm, ff0=ff0, fb0=fb0, want=EVERYTHING, **fixed, **par)
    same(got, ref)
    assert not got[0][:8].any() and not got[1][:8].any() and all(np.isnan(g[:8].view(np.float64)).all() for g in got[2:])
    same(tuple(g[8:] for g in got), {key: v[8:] for key, v in clean.items()})
    # the device form, which hands the labels on as they are: a negative one too
    tr[8, 0] = -1
    ref = model(y, modem, tr, nf, nb, algorithm, ff0=ff0, fb0=fb0, **fixed, **par)
    assert ref['bad'].tolist() == [True] * 9 + [False] * 2
    bufs = {key: DeviceBuf.from_array(v) for key, v in par.items()}
    out = deviceops.adaptive_equalize_dev(modem, DeviceBuf.from_array(as_pairs(y)), B, y.shape[1], DeviceBuf.from_array(tr.astype(np.int32)),
                                          True, nt, nf, nb, algorithm, bufs.get('step'), True, bufs.get('forgetting'), True,
                                          bufs.get('delta'), True, d_ff0=DeviceBuf.from_array(as_pairs(ff0)), ff0_batched=True,
                                          d_fb0=DeviceBuf.from_array(as_pairs(fb0)), fb0_batched=True, want=EVERYTHING, **fixed)
    _lib.check(_lib.load().cpx_stream_sync(None))
    shapes = {key: (v.shape, v.dtype) for key, v in ref.items()}
    got = tuple(o.to_array(*shapes[key]) for o, key in zip(out, EVERYTHING))
    same(got, ref)
    same(tuple(g[9:] for g in got), {key: v[9:] for key, v in clean.items()})


@pytest.mark.parametrize("algorithm", ['lms', 'rls'])
def test_same_bits_whatever_the_call(gpu, algorithm):
    """Batch size, row position, stream, host or device form and the subset of ``want`` -- each of the 63 -- change no bit, those of a
    row that is rejected at step 20, after twenty of its results have been stored, included."""
    modem, nf, nb, n, nt, B = QAMModem(16), 7, 3, 70, 30, 11
    idx, y = draw(modem, n, B, 31)
    tr = idx[:, :nt].copy()
    tr[2, 20] = 16                                                 # out of range: row 2 is rewritten at its end
    kw = dict(PARAMS[algorithm], n=n)
    ref = model(y, modem, tr, nf, nb, algorithm, **kw)
    assert ref['bad'].tolist() == [False, False, True] + [False] * 8
    call = lambda yy, tt, names: adaptive_equalize_batch(yy, modem, tt, nf, nb, algorithm, want=names, **kw)
    same(call(y, tr, EVERYTHING), ref)
    same(call(y[::-1], tr[::-1], EVERYTHING), {key: v[::-1] for key, v in ref.items()})
    for r in range(1, len(EVERYTHING) + 1):
        for names in itertools.combinations(EVERYTHING, r):
            same(call(y, tr, names), ref, names, names)
    one = call(y[4], tr[4], EVERYTHING)
    same(tuple(np.asarray(v)[None] for v in one), {key: v[4:5] for key, v in ref.items()})
    lib = _lib.load()
    streams = []
    for _ in range(2):
        st = ctypes.c_void_p()
        _lib.check(lib.cpx_stream_create(ctypes.byref(st)))
        streams.append(st)
    try:
        d_y, d_tr = DeviceBuf.from_array(as_pairs(y)), DeviceBuf.from_array(np.ascontiguousarray(tr, dtype=np.int32))
        par = {key: DeviceBuf.from_array(np.array([v])) for key, v in PARAMS[algorithm].items()}
        dev = lambda names, st: deviceops.adaptive_equalize_dev(modem, d_y, B, y.shape[1], d_tr, True, nt, nf, nb, algorithm, par.get('step'),
                                                                False, par.get('forgetting'), False, par.get('delta'), False, n=n,
                                                                want=names, stream=st)
        outs = [dev(EVERYTHING, st) for st in streams]
        shapes = {key: (v.shape, v.dtype) for key, v in ref.items()}
        for st, out in zip(streams, outs):
            _lib.check(lib.cpx_stream_sync(st))
            same(tuple(o.to_array(*shapes[key]) for o, key in zip(out, EVERYTHING)), ref)
        d_idx = dev(('indices',), streams[0])
        _lib.check(lib.cpx_stream_sync(streams[0]))
        assert np.array_equal(d_idx.to_array((B, n), np.int32), ref['indices'])
    finally:
        for st in streams:
            lib.cpx_stream_destroy(st)


def test_channel_b_end_to_end(gpu):
    """modulate -> multipath_batch -> awgn -> adaptive_equalize_batch on Proakis' channel B, QPSK at 14 dB, 300 symbols of which 100
    train: the error counts of the linear and the feedback equaliser equal the model's for every algorithm."""
    modem = QAMModem(4)
    rs = np.random.RandomState(3)
    B, n, nt = 8, 300, 100
    bits = rs.randint(0, 2, (B, 2 * n))
    x = modem.modulate(bits.reshape(-1)).reshape(B, n)
    idx = (bits.reshape(B, n, 2) * [2, 1]).sum(2)
    assert np.array_equal(modem.constellation[idx], x)
    np.random.seed(5)
    y = np.stack([awgn(row, 14.0) for row in multipath_batch(x, np.array([0.407, 0.815, 0.407]))])
    counts = {}
    for algorithm, kw in (('lms', dict(step=0.005)), ('nlms', dict(step=0.1)), ('rls', dict(forgetting=0.999, delta=0.01))):
        for nb, delay in ((0, 8), (2, 15)):
            ref = model(y, modem, idx[:, :nt], 16, nb, algorithm, delay=delay, n=n, **kw)
            out = adaptive_equalize_batch(y, modem, idx[:, :nt], 16, nb, algorithm, delay=delay, n=n, want='bits', **kw)
            assert np.array_equal(out, ref['bits'])
            counts[algorithm, nb] = int((out[:, 2 * nt:] != bits[:, 2 * nt:]).sum())
            assert counts[algorithm, nb] == int((ref['bits'][:, 2 * nt:] != bits[:, 2 * nt:]).sum())
    print("channel B on the device, bit errors of %d after training: %s" % (B * 2 * (n - nt), counts))


def test_engine_refuses_the_limits(gpu):
    lib = _lib.load()
    h4, h64 = QAMModem(4)._device_handle(), QAMModem(64)._device_handle()
    buf, out = DeviceBuf.from_array(np.full(1 << 10, 0.5)), DeviceBuf(1 << 12)
    labels = DeviceBuf.from_array(np.zeros(64, dtype=np.int32))

    def call(md, alg=0, nf=4, nb=0, n=10, sps=1, nt=2, delay=0, step=buf.ptr, fg=None, dl=None, eps=1e-6, idx=out.ptr, bits=None, B=1):
        return lib.cpx_adaptive_equalize_dev(md, buf.ptr, B, 10 * sps, n, sps, labels.ptr, 0, nt, nf, nb, delay, alg, step, 0, fg, 0, dl, 0, eps,
                                             None, 0, None, 0, idx, bits, None, None, None, None, None)
    for kw, limit in ((dict(alg=3), "algorithm = 3"), (dict(nf=0), "1 <= nf <= 64"), (dict(nf=65), "1 <= nf <= 64"), (dict(nb=65), "0 <= nb <= 64"),
                      (dict(nb=-1), "0 <= nb <= 64"), (dict(alg=2, nf=32, nb=1, step=None, fg=buf.ptr, dl=buf.ptr), "nf + nb <= 32"),
                      (dict(delay=-1), "0 <= delay"), (dict(sps=0), "1 <= sps <= 8"), (dict(sps=9), "1 <= sps <= 8"), (dict(n=0), "1 <= n"),
                      (dict(nt=11), "0 <= nt <= n"), (dict(step=None), "step is required"),
                      (dict(alg=2, fg=buf.ptr, dl=buf.ptr), "step is given with 'rls'"), (dict(alg=2, step=None, fg=buf.ptr), "forgetting and delta"),
                      (dict(eps=-1.0), "eps >= 0"), (dict(idx=None), "no output requested"), (dict(B=-1), "B = -1")):
        assert call(h4, **kw) == _lib.CPX_EINVAL and limit in _lib.last_error(), (limit, _lib.last_error())
    assert call(h64) == _lib.CPX_OK                                # 64-QAM is within the limits
    assert out.to_array((10,), np.int32).max() < 64
    assert call(h4, alg=2, nf=31, nb=1, step=None, fg=buf.ptr, dl=buf.ptr) == _lib.CPX_OK
