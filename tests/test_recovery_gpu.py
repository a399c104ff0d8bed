"""Timing and carrier recovery on the GPU against tests/recovery_model.py: every output equals the model's bit for bit (floats by their
bit pattern, NaNs by position) -- both detectors, both interpolators, the carrier loop on and off, every sps from 2 to 8 that the
ring's bounds depend on, strobe counts below and above the ring's refill period, clock offsets that make the position advance by
sps - 1, sps and sps + 1 samples, rows that start at sample 0 and rows that end early, batches on both sides of a wave and above the
grid cap, and every kind of rejected row between good ones."""
import ctypes
import itertools
import re

import numpy as np
import pytest

import recovery_model as R
from commpy_amd import _lib, deviceops
from commpy_amd.deviceops import DeviceBuf
from commpy_amd.modulation import Modem, PSKModem, QAMModem
from commpy_amd.recovery import RECOVERY_WANT, timing_recover_batch

pytestmark = pytest.mark.gpu
CUSTOM = np.array([1.0 + 0.2j, -0.7 + 1.0j, 0.1 - 1.1j, -1.2 - 0.3j])          # four points, labels in no Gray order
MODEMS = {None: lambda: None, 2: lambda: PSKModem(2), 4: lambda: QAMModem(4), 16: lambda: QAMModem(16), 64: lambda: QAMModem(64),
          256: lambda: QAMModem(256), 'custom': lambda: Modem(CUSTOM, reorder_as_gray=False)}
# (ted, interp, carrier, M, sps, nt ('none', 'one', 'all' = n), n)
CASES = [('gardner', 'cubic', False, None, 2, 'none', 1), ('gardner', 'linear', False, None, 3, 'none', 2),
         ('gardner', 'cubic', True, 4, 4, 'one', 65), ('gardner', 'linear', True, 16, 8, 'all', 130),
         ('mm', 'cubic', True, 16, 2, 'all', 130), ('mm', 'linear', False, 2, 3, 'none', 65), ('mm', 'cubic', False, 64, 8, 'one', 65),
         ('mm', 'linear', True, 256, 4, 'all', 65), ('gardner', 'cubic', False, 'custom', 3, 'one', 130),
         ('mm', 'cubic', True, 'custom', 2, 'none', 1), ('gardner', 'cubic', True, 64, 2, 'none', 130),
         ('mm', 'linear', True, 4, 8, 'one', 2), ('gardner', 'linear', False, 256, 2, 'all', 65), ('mm', 'cubic', False, 4, 4, 'none', 130)]


def names_for(modem, carrier):
    return tuple(key for key in RECOVERY_WANT if (modem is not None or key not in ('indices', 'bits')) and (carrier or key != 'phase'))


def same(got, ref, names, what=None):
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


def points(modem):
    return CUSTOM[:2] if modem is None else modem.constellation


def draw(modem, n, B, seed, sps, clock=1.0004, n_y=None):
    """``(labels [B, n + 4], y [B, n_y])``: raised-cosine rows with their own timing offset, phase and frequency offset each."""
    rs = np.random.RandomState(seed)
    rows = [R.rc_burst(points(modem), n + 4, sps, seed * 1000 + b, tau=rs.uniform(0.0, 0.9), clock=clock, phase=rs.uniform(-0.1, 0.1),
                       cfo=rs.uniform(-1e-3, 1e-3), n_y=(n + 2) * sps if n_y is None else n_y) for b in range(B)]
    return np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])


def gains(modem, sps, B=None, rs=None):
    """Loop gains scaled to the constellation's energy (the detectors' gain grows with it); per row with ``B``."""
    es = 1.0 if modem is None else float(modem.Es)
    spread = 1.0 if B is None else 1.0 + 0.2 * rs.rand(B)
    return dict(k1=0.05 * sps / es * spread, k2=2e-3 * sps / es * spread), (0.05 / es * spread, 0.002 / es * spread)


def model(y, sps, modem, ted, interp, **kw):
    return R.recover(y, sps, None if modem is None else modem.constellation, ted, interp, **kw)


def kernel_name(ted, interp, carrier, sps, modem):
    return "tr_loop_kernel %s %s carrier=%d sps=%d M=%d " % (ted, interp, carrier, sps, 0 if modem is None else modem.m)


@pytest.mark.parametrize("k", range(len(CASES)))
def test_equals_the_model(gpu, k):
    ted, interp, carrier, M_, sps, kind, n = CASES[k]
    modem, B = MODEMS[M_](), 3
    per_row_tr, per_row_par, per_row_start = ((k >> 0) & 1) == 0, ((k >> 1) & 1) == 0, ((k >> 2) & 1) == 0
    idx, y = draw(modem, n, B, 200 + k, sps)
    rs = np.random.RandomState(300 + k)
    kw, pll = gains(modem, sps, B if per_row_par else None, rs)
    kw.update(n=n, carrier=pll if carrier else None)
    nt = {'none': 0, 'one': 1, 'all': n}[kind]
    if kind != 'none':
        kw['training'] = idx[:, :nt] if per_row_tr else idx[0, :nt]
    if k % 3:                                                      # else the defaults: m0 = 0, so that the cubic reads index -1
        kw.update(m0=rs.randint(0, sps + 1, B) if per_row_start else 1, mu0=rs.rand(B) if per_row_start else 0.625,
                  phase0=rs.uniform(-0.5, 0.5, B) if per_row_start and carrier else 0.0)
    ref = model(y, sps, modem, ted, interp, **kw)
    assert not ref['bad'].any()
    names = names_for(modem, carrier)
    got = timing_recover_batch(y, sps, modem, ted, interp, want=names, **kw)
    assert _lib.last_kernel().startswith(kernel_name(ted, interp, carrier, sps, modem)), _lib.last_kernel()
    same(got, ref, names, CASES[k])
    same(timing_recover_batch(y, sps, modem, ted, interp, **kw), ref, ('symbols',))


@pytest.mark.parametrize("ted,interp", [('gardner', 'cubic'), ('mm', 'linear')])
def test_clock_offsets_step_the_window_both_ways(gpu, ted, interp):
    """Sample clocks 2 % fast and slow at sps = 2: the position advances by 1, 2 and 3 samples -- the steps at which the ring's refill
    and the interpolator's window can slip."""
    modem, sps, n, B = QAMModem(4), 2, 130, 3
    kw, pll = gains(modem, sps)
    steps = set()
    for clock in (1.02, 0.98):
        idx, y = draw(modem, n, B, 41, sps, clock, n_y=int((n + 2) * sps / clock))
        ref = model(y, sps, modem, ted, interp, n=n, carrier=pll, training=idx[:, :16], **kw)
        assert not ref['bad'].any()
        steps |= set(np.diff(ref['m'], axis=1).reshape(-1).tolist())
        names = names_for(modem, True)
        same(timing_recover_batch(y, sps, modem, ted, interp, n=n, carrier=pll, training=idx[:, :16], want=names, **kw), ref, names, clock)
    assert steps == {sps - 1, sps, sps + 1}, steps


@pytest.mark.parametrize("ted,interp,sps", [('gardner', 'cubic', 2), ('gardner', 'linear', 8), ('mm', 'cubic', 4)])
def test_rows_that_end_early(gpu, ted, interp, sps):
    """Rows too short for n strobes: the reads run off the end, read 0.0, and ``count`` stays below n."""
    modem, n, B = QAMModem(4), 65, 3
    kw, pll = gains(modem, sps)
    idx, y = draw(modem, n, B, 43, sps, n_y=40 * sps + 1)
    ref = model(y, sps, modem, ted, interp, n=n, carrier=pll, **kw)
    assert not ref['bad'].any() and (ref['count'] < n).all() and (ref['count'] > 30).all()
    names = names_for(modem, True)
    same(timing_recover_batch(y, sps, modem, ted, interp, n=n, carrier=pll, want=names, **kw), ref, names)
    # the last sample of the row as the start: every strobe but the first reads past the end
    ref = model(y, sps, modem, ted, interp, n=n, carrier=pll, m0=y.shape[1] - 1, **kw)
    assert not ref['bad'].any() and (ref['count'] == 0).all()
    same(timing_recover_batch(y, sps, modem, ted, interp, n=n, carrier=pll, m0=y.shape[1] - 1, want=names, **kw), ref, names)


@pytest.mark.parametrize("ted,interp,carrier", [('gardner', 'cubic', True), ('mm', 'linear', False)])
def test_batch_sizes_round_a_wave(gpu, ted, interp, carrier):
    """One row, one short of a wave of 64 rows, a wave, one over, two waves and two rows: every row equals the same row computed alone
    (the model computes every row on its own)."""
    modem, sps, n = QAMModem(16), 2, 20
    idx, y = draw(modem, n, 130, 17, sps)
    kw, pll = gains(modem, sps)
    kw.update(n=n, carrier=pll if carrier else None)
    names = names_for(modem, carrier)
    ref = model(y, sps, modem, ted, interp, training=idx[:, :4], **kw)
    assert not ref['bad'].any()
    for B in (1, 63, 64, 65, 130):
        sub = {key: v[:B] for key, v in ref.items()}
        same(timing_recover_batch(y[:B], sps, modem, ted, interp, training=idx[:B, :4], want=names, **kw), sub, names, B)
    alone = timing_recover_batch(y[77], sps, modem, ted, interp, training=idx[77, :4], want=names, **kw)
    same(tuple(np.asarray(v)[None] for v in alone), {key: v[77:78] for key, v in ref.items()}, names)


def test_batch_above_the_grid_cap(gpu):
    """Every workgroup takes a second group of rows."""
    modem, sps, n = PSKModem(2), 2, 2
    idx, y = draw(modem, n, 70, 19, sps)
    kw, pll = gains(modem, sps)
    kw.update(n=n, carrier=pll)
    names = names_for(modem, True)
    ref = model(y, sps, modem, 'mm', 'cubic', **kw)
    same(timing_recover_batch(y, sps, modem, 'mm', 'cubic', want=names, **kw), ref, names)
    cap = int(re.search(r"tr_cap=(\d+)", _lib.last_kernel()).group(1))
    B = cap * 64 + 1
    tile = lambda v: np.resize(v, (B,) + v.shape[1:])
    same(timing_recover_batch(tile(y), sps, modem, 'mm', 'cubic', want=names, **kw), {key: tile(v) for key, v in ref.items()}, names)


def as_pairs(v):
    return np.ascontiguousarray(v, dtype=np.complex128).view(np.float64)


@pytest.mark.parametrize("ted", ['gardner', 'mm'])
def test_rejected_rows_stay_in_their_row(gpu, ted):
    modem, sps, n, nt, B = QAMModem(4), 2, 30, 6, 12
    idx, y = draw(modem, n, B, 23, sps)
    kw, pll = gains(modem, sps)
    par = dict(k1=np.full(B, kw['k1']), k2=np.full(B, kw['k2']), kc1=np.full(B, pll[0]), kc2=np.full(B, pll[1]), m0=np.zeros(B, np.int64),
               mu0=np.full(B, 0.25), phase0=np.full(B, 0.125))
    run = lambda f, yy, tr, p, **more: f(yy, sps, k1=p['k1'], k2=p['k2'], carrier=(p['kc1'], p['kc2']), training=tr, n=n, m0=p['m0'],
                                         mu0=p['mu0'], phase0=p['phase0'], **more)
    mdl = lambda yy, tr, p: run(lambda *a, **k: model(a[0], a[1], modem, ted, 'cubic', **k), yy, tr, p)
    names = names_for(modem, True)
    clean = mdl(y, idx[:, :nt], par)
    assert not clean['bad'].any()
    y, tr = y.copy(), idx[:, :nt].copy()
    y[0, 3] = np.nan
    y[1, y.shape[1] - 1] = complex(0.0, np.inf)                    # behind the last sample any strobe reads: the scan finds it
    tr[2, 4] = 4                                                   # a label out of range
    par['k1'][3] = 1e6                                             # the period leaves (0.5 sps, 1.5 sps) at the first error
    par['k2'][4], par['kc1'][5], par['kc2'][6] = np.nan, np.inf, np.nan
    par['kc2'][7] = 1.7e308                                        # f overflows: phi is a NaN, |phi| <= 0.5 fails
    ref = mdl(y, tr, par)
    assert ref['bad'].tolist() == [True] * 8 + [False] * 4
    got = run(timing_recover_batch, y, tr, par, modem=modem, ted=ted, interp='cubic', want=names)
    same(got, ref, names)
    for g in got:
        assert not g[:8].any() if g.dtype.kind in 'iu' else np.isnan(g[:8].view(np.float64)).all()
    same(tuple(g[8:] for g in got), {key: v[8:] for key, v in clean.items()}, names)
    # the device form, which hands every value on as it is: a negative label, and starts outside their ranges
    tr[8, 0] = -1
    par['mu0'][9], par['phase0'][10], par['m0'][11] = 1.0, -0.75, y.shape[1]
    ref = mdl(y, tr, par)
    assert ref['bad'].all()
    par['mu0'][9] = 0.25                                           # the model's row 9 is good again, and so must the device's be
    ref = mdl(y, tr, par)
    assert ref['bad'].tolist() == [True] * 9 + [False] + [True] * 2
    buf = {key: DeviceBuf.from_array(v) for key, v in par.items()}
    out = deviceops.timing_recover_dev(DeviceBuf.from_array(as_pairs(y)), B, y.shape[1], sps, buf['k1'], True, buf['k2'], True, buf['m0'], True,
                                       buf['mu0'], True, buf['phase0'], True, modem, ted, 'cubic', buf['kc1'], True, buf['kc2'], True,
                                       DeviceBuf.from_array(tr.astype(np.int32)), True, nt, n, want=names)
    _lib.check(_lib.load().cpx_stream_sync(None))
    got = tuple(o.to_array(ref[key].shape, ref[key].dtype) for o, key in zip(out, names))
    same(got, ref, names)
    same(tuple(g[9:10] for g in got), {key: v[9:10] for key, v in clean.items()}, names)


def test_same_bits_whatever_the_call(gpu):
    """Row order, stream, host or device form and the subset of ``want`` -- each of the 127 -- change no bit, those of a row that is
    rejected at strobe 20, after twenty of its results have been stored, included."""
    modem, sps, n, nt, B = QAMModem(16), 3, 40, 30, 5
    idx, y = draw(modem, n, B, 31, sps)
    tr = idx[:, :nt].copy()
    tr[2, 20] = 16                                                 # out of range: row 2 is rewritten at its end
    kw, pll = gains(modem, sps)
    kw.update(n=n, carrier=pll, mu0=0.5)
    ref = model(y, sps, modem, 'mm', 'cubic', training=tr, **kw)
    assert ref['bad'].tolist() == [False, False, True, False, False]
    call = lambda yy, tt, names: timing_recover_batch(yy, sps, modem, 'mm', 'cubic', training=tt, want=names, **kw)
    same(call(y, tr, RECOVERY_WANT), ref, RECOVERY_WANT)
    same(call(y[::-1], tr[::-1], RECOVERY_WANT), {key: v[::-1] for key, v in ref.items()}, RECOVERY_WANT)
    for r in range(1, len(RECOVERY_WANT) + 1):
        for names in itertools.combinations(RECOVERY_WANT, r):
            same(call(y, tr, names), ref, names, names)
    one = call(y[4], tr[4], RECOVERY_WANT)
    same(tuple(np.asarray(v)[None] for v in one), {key: v[4:5] for key, v in ref.items()}, RECOVERY_WANT)
    lib = _lib.load()
    streams = []
    for _ in range(2):
        st = ctypes.c_void_p()
        _lib.check(lib.cpx_stream_create(ctypes.byref(st)))
        streams.append(st)
    try:
        put = lambda v: DeviceBuf.from_array(np.atleast_1d(np.asarray(v)))
        d_y, d_tr = put(as_pairs(y)), put(np.ascontiguousarray(tr, dtype=np.int32))
        d = dict(k1=put(kw['k1']), k2=put(kw['k2']), kc1=put(pll[0]), kc2=put(pll[1]), m0=put(np.int64(0)), mu0=put(0.5), phase0=put(0.0))
        dev = lambda names, st: deviceops.timing_recover_dev(d_y, B, y.shape[1], sps, d['k1'], False, d['k2'], False, d['m0'], False,
                                                             d['mu0'], False, d['phase0'], False, modem, 'mm', 'cubic', d['kc1'], False,
                                                             d['kc2'], False, d_tr, True, nt, n, want=names, stream=st)
        outs = [dev(RECOVERY_WANT, st) for st in streams]
        for st, out in zip(streams, outs):
            _lib.check(lib.cpx_stream_sync(st))
            same(tuple(o.to_array(ref[key].shape, ref[key].dtype) for o, key in zip(out, RECOVERY_WANT)), ref, RECOVERY_WANT)
        d_count = dev(('count',), streams[0])
        _lib.check(lib.cpx_stream_sync(streams[0]))
        assert np.array_equal(d_count.to_array((B,), np.int32), ref['count'])
    finally:
        for st in streams:
            lib.cpx_stream_destroy(st)


def test_chain_from_the_matched_filter(gpu):
    """pulse_shape -> a fractional delay by interpolation -> matched_filter -> timing_recover_batch: 16-QAM at 4 samples per symbol
    with a 32-symbol training prefix; the decisions equal the model's and, once settled, the symbols sent."""
    from commpy_amd.filters import matched_filter_batch, pulse_shape_batch, rrcosfilter
    modem, sps, n, B = QAMModem(16), 4, 400, 4
    rs = np.random.RandomState(5)
    idx = rs.randint(0, 16, (B, n))
    taps = rrcosfilter(8 * sps, 0.35, 1.0, sps)[1]                 # symmetric about tap 4 sps: a group delay of 4 symbols
    taps = taps / np.sqrt(np.sum(taps ** 2))
    tx = pulse_shape_batch(modem.constellation[idx], taps, sps)
    at, grid = np.arange(tx.shape[1] - 2) + 0.3 * sps, np.arange(tx.shape[1])      # 0.3 symbol early, by linear interpolation
    rx = np.stack([np.interp(at, grid, row.real) + 1j * np.interp(at, grid, row.imag) for row in tx])
    rx = rx * np.exp(2j * np.pi * 0.04) + 0.02 * (rs.randn(*rx.shape) + 1j * rs.randn(*rx.shape))
    y = matched_filter_batch(rx, taps)
    delay = 8 * sps - 2                                            # both filters' group delay less the advance, rounded down
    kw, pll = gains(modem, sps)
    kw.update(n=n - 8, carrier=pll, training=idx[:, :32], m0=delay)
    ref = model(y, sps, modem, 'mm', 'cubic', **kw)
    got = timing_recover_batch(y, sps, modem, 'mm', 'cubic', want=('indices', 'position'), **kw)
    same(got, ref, ('indices', 'position'))
    assert not ref['bad'].any() and np.array_equal(got[0][:, 100:], idx[:, 100:n - 8])
