"""Host side of the multipath channel and the pilot-aided OFDM channel estimator: the NumPy model against brute-force loops, the two
interpolation-matrix builders, every refusal (ValueError before any device is touched) and the loud failure without a device."""
import ctypes

import numpy as np
import pytest

import ofdm_chan_model as M
from commpy_amd import _lib
from commpy_amd.channels import multipath_batch
from commpy_amd.modulation import OfdmPilots, ofdm_estimate_batch, ofdm_map_batch, ofdm_subcarrier_frequencies


def cplx(rs, *shape):
    return rs.randn(*shape) + 1j * rs.randn(*shape)


def frame_of(p):
    return M.Frame(p.nsc, p.nsym, p.nt, p.pil_sym, p.pil_sc, p.pil_tx, p.pil_val, p.W)


def test_model_multipath_against_loops():
    rs = np.random.RandomState(0)
    B, nt, nr, n, L = 2, 2, 3, 5, 4
    x, g = cplx(rs, B, nt, n), cplx(rs, B, nr, nt, L)
    want = np.zeros((B, nr, n + L - 1), complex)
    for b in range(B):
        for r in range(nr):
            for m in range(n + L - 1):
                for t in range(nt):
                    for l in range(L):
                        if 0 <= m - l < n:
                            want[b, r, m] += g[b, r, t, l] * x[b, t, m - l]
    assert np.max(np.abs(M.multipath(x, g) - want)) < 1e-13
    assert np.array_equal(M.multipath(x, g[0]), M.multipath(x, np.stack([g[0], g[0]])))


def test_model_frame_against_loops():
    """A 6 x 3 frame of 2 antennas with scattered pilots, two of them sharing a subcarrier: map, LS, W LS and demap by loops."""
    rs = np.random.RandomState(1)
    nsc, nsym, nt, nr, B = 6, 3, 2, 2, 2
    pil = [(0, 0, 0), (2, 0, 0), (0, 3, 0), (1, 5, 0), (0, 1, 1), (1, 4, 1), (2, 4, 1)]          # (symbol, subcarrier, antenna)
    sym, sc, tx = (np.array(v) for v in zip(*pil))
    val = cplx(rs, len(pil))
    pk = [[0, 3, 5], [1, 4]]
    W = [cplx(rs, nsc, 3), cplx(rs, nsc, 2)]
    fr = M.Frame(nsc, nsym, nt, sym, sc, tx, val, W)
    assert fr.pk == pk and fr.ndata == nsc * nsym - len(pil) and fr.max_count == 2
    assert fr.data[:6] == [(0, 2), (0, 4), (0, 5), (1, 0), (1, 1), (1, 2)]
    data = cplx(rs, B, fr.ndata, nt)
    grid = M.map_grid(fr, data)
    for b in range(B):
        for t in range(nt):
            d = 0
            for s in range(nsym):
                for k in range(nsc):
                    hit = [i for i, q in enumerate(pil) if q[:2] == (s, k)]
                    if hit:
                        assert grid[b, t, s, k] == (val[hit[0]] if pil[hit[0]][2] == t else 0)
                    else:
                        assert grid[b, t, s, k] == data[b, d, t]
                        d += 1
    Y = cplx(rs, B, nr, nsym, nsc)
    y_data, h_data, h_sc, ls = M.estimate(fr, Y)
    for b in range(B):
        for r in range(nr):
            for t in range(nt):
                lsq = []
                for kj in pk[t]:
                    terms = [Y[b, r, s, k] / val[i] for i, (s, k, a) in enumerate(pil) if a == t and k == kj]
                    lsq.append(sum(terms) / len(terms))
                assert np.allclose(ls[t][b, r], lsq, rtol=1e-13, atol=0)
                for k in range(nsc):
                    assert abs(h_sc[b, k, r, t] - sum(W[t][k, j] * lsq[j] for j in range(len(lsq)))) < 1e-13
            for d, (s, k) in enumerate(fr.data):
                assert y_data[b, d, r] == Y[b, r, s, k]
                assert np.array_equal(h_data[b, d, r], h_sc[b, k, r])


def test_package_bookkeeping_matches_the_model():
    for p in (OfdmPilots.comb(52, 4, 2, 4, [0, 2], 'linear'), OfdmPilots.block(52, 5, 3), OfdmPilots.comb(12, 3, 1, 4, [1], 'linear'),
              OfdmPilots(2, 1, 1, [0], [1], [0], [1j])):
        fr = frame_of(p)
        assert p.ndata == fr.ndata and list(zip(p.data_sym, p.data_sc)) == fr.data
        assert [list(k) for k in p.pilot_subcarriers] == fr.pk
        assert np.allclose(np.abs(p.pil_val), 1.0)
    p = OfdmPilots.comb(52, 4, 2, 4, [0, 2], 'linear')
    assert list(p.pilot_subcarriers[1][:3]) == [1, 5, 9] and set(p.pil_sym) == {0, 2}
    p = OfdmPilots.block(52, 5, 3)
    assert p.ndata == 2 * 52 and all(np.array_equal(k, np.arange(52)) for k in p.pilot_subcarriers)


def test_frequencies_follow_the_bin_map():
    assert list(ofdm_subcarrier_frequencies(6)) == [-3, -2, -1, 1, 2, 3]
    assert np.array_equal(ofdm_subcarrier_frequencies(52), M.frequencies(52))


@pytest.mark.parametrize("nsc, pk", [(52, list(range(0, 52, 4))), (52, list(range(3, 52, 7))), (12, [5]), (8, [3, 4]), (64, [0, 63])])
def test_linear_rows(nsc, pk):
    p = OfdmPilots(nsc, 1, 1, np.zeros(len(pk), int), np.array(pk), np.zeros(len(pk), int), np.ones(len(pk)), 'linear')
    W = p.W[0]
    assert W.shape == (nsc, len(pk)) and np.all(W.imag == 0)
    assert np.all(np.count_nonzero(W, axis=1) <= 2)
    assert np.allclose(W.sum(axis=1), 1.0, rtol=0, atol=1e-15) and np.all(W.real >= 0)
    assert np.allclose(W, M.w_linear(nsc, pk), rtol=0, atol=1e-15)
    assert np.array_equal(W[pk], np.eye(len(pk)))                                  # a pilot subcarrier keeps its own estimate
    f = M.frequencies(nsc)
    assert np.allclose(W @ (2.0 * f[pk] + 1), np.clip(2.0 * f + 1, 2.0 * f[pk[0]] + 1, 2.0 * f[pk[-1]] + 1))   # exact on a line


@pytest.mark.parametrize("nsc, nfft, spacing, first, Lmax", [(52, 64, 4, 0, 8), (52, 64, 4, 1, 13), (200, 256, 8, 3, 16), (12, 16, 3, 2, 1)])
def test_taps_reproduce_the_channel(nsc, nfft, spacing, first, Lmax):
    rs = np.random.RandomState(Lmax)
    pk = list(range(first, nsc, spacing))
    p = OfdmPilots(nsc, 1, 1, np.zeros(len(pk), int), np.array(pk), np.zeros(len(pk), int), np.ones(len(pk)), ('taps', Lmax, nfft))
    W = p.W[0]
    assert np.allclose(W, M.w_taps(nsc, pk, Lmax, nfft), rtol=0, atol=1e-9)
    bins = M.frequencies(nsc) % nfft
    for L in {1, Lmax}:
        g = cplx(rs, L)
        H = np.fft.fft(g, nfft)[bins]
        assert np.max(np.abs(W @ H[pk] - H)) <= 1e-9 * np.sqrt(np.mean(np.abs(H) ** 2))


@pytest.fixture
def no_device(monkeypatch):
    """Any attempt to load the engine fails the test: the refusals below must come from the host-side checks."""
    def boom(*a, **k):
        raise AssertionError("the engine was touched")
    monkeypatch.setattr(_lib, "load", boom)


GOOD = dict(nsc=8, nsym=2, nt=2, pil_sym=[0, 0, 1], pil_sc=[0, 1, 4], pil_tx=[0, 1, 0], pil_val=[1, 1j, -1], interp='linear')


@pytest.mark.parametrize("change", [
    dict(nsc=7), dict(nsc=0), dict(nsc=2.5), dict(nsym=0), dict(nt=0), dict(nt=5000),
    dict(pil_sym=[], pil_sc=[], pil_tx=[], pil_val=[]),
    dict(pil_sym=[0, 0, 2]), dict(pil_sym=[0, 0, -1]), dict(pil_sc=[0, 1, 8]), dict(pil_tx=[0, 2, 0]),
    dict(pil_sym=[0, 0, 0], pil_sc=[0, 1, 1]),                                      # a repeated resource element
    dict(pil_tx=[0, 0, 0]),                                                         # antenna 1 without a pilot
    dict(pil_val=[1, 0, 1]), dict(pil_val=[1, np.nan, 1]), dict(pil_val=[1, np.inf, 1]), dict(pil_val=[1, 1]),
    dict(pil_val=['a', 'b', 'c']), dict(pil_sc=[0.0, 1.0, 4.0]), dict(pil_sym=[[0, 0, 1]]),
    dict(interp='cubic'), dict(interp=('taps', 3, 16)), dict(interp=('taps', 0, 16)), dict(interp=('taps', 2)),
    dict(interp=[np.ones((8, 2))]), dict(interp=[np.ones((8, 2)), np.ones((8, 2))]), dict(interp=[np.ones((8, 2)), np.full((8, 1), np.nan)]),
    dict(interp=[np.ones((8, 2)), np.array([['x']] * 8)]),
])
def test_pilot_patterns_refused(no_device, change):
    with pytest.raises(ValueError):
        OfdmPilots(**dict(GOOD, **change))


def test_builders_and_calls_refused(no_device):
    p = OfdmPilots(**GOOD)
    assert p.ndata == 13 and [list(k) for k in p.pilot_subcarriers] == [[0, 4], [1]]
    OfdmPilots(**dict(GOOD, interp=[np.ones((8, 2)), np.ones((8, 1))]))
    OfdmPilots(**dict(GOOD, interp=('taps', 1, 16)))
    for bad in (lambda: OfdmPilots.comb(52, 4, 4, 3, [0], 'linear'), lambda: OfdmPilots.comb(52, 4, 2, 4, [], 'linear'),
                lambda: OfdmPilots.comb(52, 4, 2, 4, [4], 'linear'), lambda: OfdmPilots.comb(51, 4, 2, 4, [0], 'linear'),
                lambda: OfdmPilots.comb(52, 4, 2, 4, [0], ('taps', 14, 64)), lambda: OfdmPilots.comb(52, 4, 2, 4, [0], 'linear', values=[1, 1]),
                lambda: OfdmPilots.block(52, 2, 3), lambda: OfdmPilots.block(52, 3, 0),
                lambda: ofdm_map_batch(np.zeros((1, 13, 2)), None), lambda: ofdm_map_batch(np.zeros((1, 12, 2)), p),
                lambda: ofdm_map_batch(np.zeros((13, 2)), p), lambda: ofdm_map_batch(np.zeros((1, 13, 2), dtype='U1'), p),
                lambda: ofdm_estimate_batch(np.zeros((1, 2, 2, 7)), p), lambda: ofdm_estimate_batch(np.zeros((2, 2, 8)), p),
                lambda: ofdm_estimate_batch(np.zeros((1, 0, 2, 8)), p), lambda: ofdm_estimate_batch(np.zeros((1, 2, 2, 8)), p, want=()),
                lambda: ofdm_estimate_batch(np.zeros((1, 2, 2, 8)), p, want=('y', 'H')),
                lambda: ofdm_estimate_batch(np.zeros((1, 2, 2, 8), dtype=object), p),
                lambda: multipath_batch(np.zeros(4), np.ones(2)), lambda: multipath_batch(np.zeros((1, 2, 4)), np.ones((2, 3, 2))),
                lambda: multipath_batch(np.zeros((2, 1, 4)), np.ones((3, 1, 1, 2))), lambda: multipath_batch(np.zeros((2, 4)), np.ones((3, 2))),
                lambda: multipath_batch(np.zeros((2, 4)), np.ones((2, 1, 2))), lambda: multipath_batch(np.zeros((1, 1, 4)), np.ones(2)),
                lambda: multipath_batch(np.zeros((1, 1, 0)), np.ones((1, 1, 2))), lambda: multipath_batch(np.zeros((1, 1, 4)), np.ones((1, 1, 0))),
                lambda: multipath_batch(np.zeros((1, 4)), np.ones(1025)), lambda: multipath_batch(np.zeros((1, 2, 4)), np.ones((2, 2, 513))),
                lambda: multipath_batch(np.zeros((1, 4), dtype='U1'), np.ones(2)), lambda: multipath_batch(np.zeros((1, 4)), np.array(['a']))):
        with pytest.raises(ValueError):
            bad()
    # empty batches need no device either
    assert ofdm_map_batch(np.zeros((0, 13, 2)), p).shape == (0, 2, 2, 8)
    assert [a.shape for a in ofdm_estimate_batch(np.zeros((0, 3, 2, 8)), p, want=('h_sc', 'y'))] == [(0, 13, 3), (0, 8, 3, 2)]
    assert multipath_batch(np.zeros((0, 2, 4)), np.ones((3, 2, 5))).shape == (0, 3, 8)
    assert multipath_batch(np.zeros((0, 4)), np.ones(5)).shape == (0, 8)


def test_want_names_outputs_alike_in_every_call(no_device):
    """One name may come as a bare string, the members come back in the documented order whatever the order asked in, and every call
    refuses an empty or unknown ``want`` before anything else, in its own fixed words."""
    from commpy_amd import deviceops
    from commpy_amd.channels import fading_multipath_batch
    from commpy_amd.sync import sync_metric_batch
    p = OfdmPilots(**GOOD)
    Y0 = np.zeros((0, 3, 2, 8))
    assert [a.shape for a in ofdm_estimate_batch(Y0, p, want='h_sc')] == [(0, 8, 3, 2)]
    assert [a.shape for a in ofdm_estimate_batch(Y0, p, want=['h_sc', 'h', 'y'])] == [(0, 13, 3), (0, 13, 3, 2), (0, 8, 3, 2)]
    assert [a.dtype for a in sync_metric_batch(np.zeros((0, 8)), 2, 2, want=('p', 'e', 'm'))] == [np.float64, np.float64, np.complex128]
    assert [a.dtype for a in sync_metric_batch(np.zeros((0, 8)), 2, 2, want='p')] == [np.complex128]
    x0 = np.zeros((0, 2, 4))
    assert [a.shape for a in fading_multipath_batch(x0, 3, np.ones(5), 0.01, want=('g', 'y'))] == [(0, 3, 8), (0, 1, 3, 2, 5)]
    assert [a.shape for a in fading_multipath_batch(x0, 3, np.ones(5), 0.01, want='g')] == [(0, 1, 3, 2, 5)]
    assert fading_multipath_batch(x0, 3, np.ones(5), 0.01, want='y').shape == (0, 3, 8)
    calls = [(lambda w: ofdm_estimate_batch(Y0, p, want=w), "'y', 'h', 'h_sc'"),
             (lambda w: deviceops.ofdm_estimate_dev(p, None, 1, 3, want=w), "'y', 'h', 'h_sc'"),
             (lambda w: sync_metric_batch(np.zeros((0, 8)), 2, 2, want=w), "'m', 'e', 'p'"),
             (lambda w: fading_multipath_batch(x0, 3, np.ones(5), 0.01, want=w), "'y', 'g'"),
             (lambda w: deviceops.fading_channel_dev(None, 1, 2, 3, 4, np.ones(5), 0.01, want=w), "'y', 'g'")]
    for call, names in calls:
        for bad in ((), [], '', 'x', ('y', 'x'), (None,), 'h_sym'):
            with pytest.raises(ValueError) as e:
                call(bad)
            assert str(e.value) == "want must name at least one of " + names


def test_engine_checks_without_device():
    """The C entry points: argument errors are reported before the device is looked for; a valid call fails loudly without one."""
    lib = _lib.load()
    x = np.zeros(64)
    i32 = lambda *v: np.array(v, np.int32)
    h = ctypes.c_void_p()
    P = _lib.ptr

    def create(nsc, nsym, nt, sym, sc, tx, val, w):
        val, w = np.asarray(val, complex), np.asarray(w, complex)
        return lib.cpx_pilots_create(nsc, nsym, nt, len(sym), P(i32(*sym)), P(i32(*sc)), P(i32(*tx)), P(val), P(w), ctypes.byref(h))
    ones = np.ones(64)
    for args in ((3, 1, 1, [0], [0], [0], [1], ones), (0, 1, 1, [0], [0], [0], [1], ones), (4, 0, 1, [0], [0], [0], [1], ones),
                 (4, 1, 0, [0], [0], [0], [1], ones), (4, 1, 1, [1], [0], [0], [1], ones), (4, 1, 1, [0], [4], [0], [1], ones),
                 (4, 1, 1, [0], [0], [1], [1], ones), (4, 1, 1, [0, 0], [2, 2], [0, 0], [1, 1], ones),
                 (4, 1, 2, [0, 0], [1, 2], [0, 0], [1, 1], ones), (4, 1, 1, [0], [0], [0], [0], ones),
                 (4, 1, 1, [0], [0], [0], [np.nan], ones), (4, 1, 1, [0], [0], [0], [1], [1, 1, np.inf, 1])):
        assert create(*args) == _lib.CPX_EINVAL, args
        assert _lib.last_error().startswith("ofdm_pilots:") and not h.value
    assert lib.cpx_pilots_create(4, 1, 1, 0, P(x), P(x), P(x), P(x), P(x), ctypes.byref(h)) == _lib.CPX_EINVAL
    assert create(4, 1, 2000, [0], [0], [0], [1], ones) == _lib.CPX_ELIMIT
    # multipath: sizes, then limits, then the empty batch, then null pointers
    mp = lib.cpx_multipath
    for nt, nr, n, L in ((0, 1, 4, 1), (1, 0, 4, 1), (1, 1, 4, 0), (1, 1, 0, 1)):
        assert mp(P(x), P(x), 0, 1, nt, nr, n, L, P(x)) == _lib.CPX_EINVAL
    assert mp(P(x), P(x), 2, 1, 1, 1, 4, 1, P(x)) == _lib.CPX_EINVAL and mp(P(x), P(x), 0, -1, 1, 1, 4, 1, P(x)) == _lib.CPX_EINVAL
    assert mp(P(x), P(x), 0, 1, 1, 1, 4, 1025, P(x)) == _lib.CPX_ELIMIT and mp(P(x), P(x), 0, 1, 2, 2, 4, 513, P(x)) == _lib.CPX_ELIMIT
    assert mp(None, None, 0, 0, 1, 1, 0, 1, None) == _lib.CPX_OK
    assert mp(None, P(x), 0, 1, 1, 1, 4, 1, P(x)) == _lib.CPX_EINVAL and _lib.last_error() == "multipath: null pointer"
    assert lib.cpx_pilots_map(None, P(x), 1, P(x)) == _lib.CPX_EINVAL and _lib.last_error() == "ofdm_map: null plan"
    assert lib.cpx_pilots_estimate(None, P(x), 1, 1, P(x), None, None) == _lib.CPX_EINVAL and _lib.last_error() == "ofdm_estimate: null plan"
    assert lib.cpx_pilots_destroy(None) == _lib.CPX_OK
    if _lib.device_count() > 0:
        return
    assert create(4, 1, 1, [0], [0], [0], [1], ones) == _lib.CPX_ENODEV and _lib.last_error().startswith("no HIP device available")
    assert mp(P(x), P(x), 0, 1, 1, 1, 4, 1, P(x)) == _lib.CPX_ENODEV


def test_entry_points_fail_loudly_without_device():
    if _lib.device_count() > 0:
        pytest.skip("a HIP device is present")
    p = OfdmPilots.comb(52, 4, 2, 4, [0, 2], 'linear')
    with pytest.raises(_lib.EngineError):
        ofdm_map_batch(np.zeros((1, p.ndata, 2)), p)
    with pytest.raises(_lib.EngineError):
        ofdm_estimate_batch(np.zeros((1, 2, 4, 52)), p)
    with pytest.raises(_lib.EngineError):
        multipath_batch(np.zeros((1, 2, 8)), np.ones((2, 2, 3)))
    with pytest.raises(_lib.EngineError):
        multipath_batch(np.zeros((1, 8)), np.ones(3))
