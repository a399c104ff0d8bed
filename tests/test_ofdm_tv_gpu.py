"""The pilot-aided estimator that follows a channel moving inside the frame (cpx_pilots_create_tv / cpx_pilots_estimate_tv,
csrc/ofdm_chan.hip) on the MI355X against the NumPy model of ofdm_tv_model.py.

Tolerance, derived rather than tuned: ofdm_tv_model.h_tv_bound (its module docstring) for H^; copies (y_data, h_data against h_sym)
are exact.  The end-to-end cases are first decided on the CPU, with the fading model's gains and the estimator's model."""
import ctypes

import numpy as np
import pytest

import fading_model as FM
import ofdm_chan_model as M
import ofdm_tv_model as T
from commpy_amd import _lib, modulation
from commpy_amd.channels import fading_multipath_batch, tap_frequency_response
from commpy_amd.deviceops import DeviceBuf, fading_channel_dev, ofdm_estimate_tv_dev, ofdm_map_dev
from commpy_amd.modulation import (OfdmPilots, QAMModem, _linear_run, linear_batch, ofdm_estimate_batch, ofdm_estimate_tv_batch,
                                   ofdm_map_batch, ofdm_rx_batch, ofdm_tx_batch)

pytestmark = pytest.mark.gpu

ALL = ('y', 'h', 'h_sym')
TV_KERNELS = "ofdm_ls_kernel+ofdm_interp_kernel<tv>+ofdm_tv_kernel<%s>"
TV_NS = 4                       # pilot symbols the fused kernel keeps in registers (csrc/ofdm_chan.hip)


def cplx(rs, *shape):
    return rs.randn(*shape) + 1j * rs.randn(*shape)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def frame_of(p):
    return T.Frame(p.nsc, p.nsym, p.nt, p.pil_sym, p.pil_sc, p.pil_tx, p.pil_val, p.W, p.V)


def random_v(make):
    """The pattern of make(time_interp) with complex random V: negative entries, and every fifth one an exact zero."""
    rs = np.random.RandomState(77)
    V = []
    for ps in make('hold').pilot_symbols:
        v = cplx(rs, make('hold').nsym, len(ps))
        v.reshape(-1)[::5] = 0
        V.append(v)
    return make(V)


@pytest.fixture(scope="module")
def user_stream(gpu):
    lib = _lib.load()
    st = ctypes.c_void_p()
    _lib.check(lib.cpx_stream_create(ctypes.byref(st)))
    yield st
    lib.cpx_stream_sync(st)
    lib.cpx_stream_destroy(st)


# name: (pattern, nr, B).  Shapes for the kernels' edges: nsc = 52 (a partial tile of 64 subcarriers) and 130 (two tiles and a remainder);
# one pilot and one data element; ns_t = 1, 2, TV_NS, TV_NS + 1 and nsym; antennas with different pilot symbols and different ns_t;
# symbols without data for all or part of the band; V in the LDS and (above 1024 entries) in global memory
PATTERNS = {
    "one": (lambda: OfdmPilots(2, 1, 1, [0], [1], [0], [0.6 - 0.8j], 'linear', 'linear'), 1, 3),
    "comb52": (lambda: OfdmPilots.comb(52, 6, 2, 4, [0, 3], 'linear', time_interp='linear'), 3, 3),
    "comb130": (lambda: random_v(lambda ti: OfdmPilots.comb(130, 14, 4, 8, [0, 4, 9, 13], ('taps', 8, 256), time_interp=ti)), 2, 2),
    "ns5": (lambda: random_v(lambda ti: OfdmPilots.comb(52, 7, 3, 4, list(range(0, 7, 2)) + [5], 'linear', time_interp=ti)), 5, 3),
    "nsall": (lambda: OfdmPilots.comb(12, 6, 1, 4, list(range(6)), 'linear', time_interp=('doppler', 0.05, 1e-3)), 1, 3),
    "block": (lambda: OfdmPilots.block(52, 5, 3, time_interp='hold'), 2, 3),
    "full": (lambda: OfdmPilots.comb(52, 4, 4, 4, [0, 2], 'linear', time_interp='linear'), 2, 3),
    "mixed": (lambda: random_v(lambda ti: OfdmPilots(8, 5, 2, [0, 0, 3, 3, 2, 2, 2], [0, 4, 0, 4, 1, 5, 7], [0, 0, 0, 0, 1, 1, 1],
                                                     [1, 1j, -1, 0.6 - 0.8j, 1, -1j, 1], 'linear', ti)), 3, 3),
    "vglobal": (lambda: random_v(lambda ti: OfdmPilots.comb(16, 40, 4, 4, list(range(0, 40, 6)), 'linear', time_interp=ti)), 1, 2),
}
_cache = {}


def pattern(name):
    """(pilots, model frame, nr, B, Y, model outputs): built once and shared by the tests, never changed."""
    if name not in _cache:
        make, nr, B = PATTERNS[name]
        p = make()
        fr = frame_of(p)
        Y = cplx(np.random.RandomState(len(name) + ord(name[0])), B, nr, p.nsym, p.nsc)
        _cache[name] = (p, fr, nr, B, Y, T.estimate_tv(fr, Y))
    return _cache[name]


def test_patterns_cover_the_edges():
    ns = {name: [len(s) for s in pattern(name)[0].pilot_symbols] for name in PATTERNS}
    assert ns["one"] == [1] and ns["comb52"] == [2, 2] and ns["comb130"] == [TV_NS] * 4 and ns["ns5"] == [TV_NS + 1] * 3
    assert ns["nsall"] == [pattern("nsall")[0].nsym] and ns["block"] == [1, 1, 1] and ns["mixed"] == [2, 1]
    assert pattern("one")[0].ndata == 1 and sum(v.size for v in pattern("vglobal")[0].V) > 1024
    assert {(pattern(n)[2], pattern(n)[0].nt) for n in PATTERNS} >= {(1, 1), (3, 2), (2, 4), (5, 3)}
    assert not np.any(pattern("full")[0].data_sym == 0) and set(pattern("block")[0].data_sym) == {3, 4}


# ---- 1. against the model -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(PATTERNS))
def test_estimate_tv_against_model(gpu, name):
    p, fr, nr, B, Y, (y_m, h_m, hs_m, lsp, hp) = pattern(name)
    y, h, hs = ofdm_estimate_tv_batch(Y, p, want=ALL)
    assert _lib.last_kernel() == TV_KERNELS % ("global" if name == "vglobal" else "lds") + "+ofdm_ydemap_kernel"
    assert y.shape == (B, p.ndata, nr) and h.shape == (B, p.ndata, nr, p.nt) and hs.shape == (B, p.nsym, p.nsc, nr, p.nt)
    assert same_bits(y, y_m)
    bound = T.h_tv_bound(fr, lsp, hp)
    err = np.abs(hs - hs_m)
    pos = bound > 0
    print("estimate_tv", name, "largest share of the bound: %.3f" % np.max(err[pos] / bound[pos]))
    assert np.all(err <= bound)
    assert same_bits(h, hs[:, p.data_sym, p.data_sc])                               # h_data = h_sym at the data elements, bit for bit
    assert np.all(np.abs(h - h_m) <= bound[:, p.data_sym, p.data_sc])


# ---- 2. one pilot symbol and V = 1: the per-frame estimator's values ---------------------------------------------------------------
@pytest.mark.parametrize("which", ["comb", "block"])
def test_single_pilot_symbol_equals_per_frame_estimate(gpu, which):
    if which == "comb":
        make = lambda ti: OfdmPilots.comb(52, 4, 2, 4, [1], ('taps', 8, 64), time_interp=ti)
        p_tv, nr = make([np.ones((4, 1))] * 2), 3
    else:
        make = lambda ti: OfdmPilots.block(52, 5, 3, time_interp=ti)
        p_tv, nr = make('hold'), 2
    assert all(np.array_equal(v, np.ones((p_tv.nsym, 1))) for v in p_tv.V)
    Y = cplx(np.random.RandomState(21), 3, nr, p_tv.nsym, p_tv.nsc)
    y, h, hs = ofdm_estimate_tv_batch(Y, p_tv, want=ALL)
    y0, h0, hsc0 = ofdm_estimate_batch(Y, make(None), want=('y', 'h', 'h_sc'))
    assert same_bits(y, y0)
    assert np.array_equal(h, h0)                                                    # ==, so that +0 and -0 are alike
    for s in range(p_tv.nsym):
        assert np.array_equal(hs[:, s], hsc0)


# ---- 3. invariance ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["comb52", "ns5", "block", "mixed"])
def test_bit_identity(gpu, user_stream, name):
    p, fr, nr, B, Y, _ = pattern(name)
    rs = np.random.RandomState(11)
    alone = ofdm_estimate_tv_batch(Y[:1], p, want=ALL)                              # B = 1
    Y5, Y8 = cplx(rs, 5, nr, p.nsym, p.nsc), cplx(rs, 8, nr, p.nsym, p.nsc)
    Y5[3], Y8[7] = Y[0], Y[0]
    for batch, pos in ((Y5, 3), (Y8, 7), (Y8[[7, 0, 1]], 0), (Y5[2:4], 1)):
        out = ofdm_estimate_tv_batch(batch, p, want=ALL)
        assert all(same_bits(a[pos], b[0]) for a, b in zip(out, alone))
    # every subset of the outputs
    full = ofdm_estimate_tv_batch(Y5, p, want=ALL)
    for want in (('y',), ('h',), ('h_sym',), ('y', 'h'), ('y', 'h_sym'), ('h', 'h_sym')):
        out = ofdm_estimate_tv_batch(Y5, p, want=want)
        assert len(out) == len(want) and all(same_bits(a, full[ALL.index(w)]) for a, w in zip(out, want)), want
    # the device form, on a user stream and on the library's
    shapes = ((5, p.ndata, nr), (5, p.ndata, nr, p.nt), (5, p.nsym, p.nsc, nr, p.nt))
    d_Y5 = DeviceBuf.from_array(Y5)
    for st in (user_stream, None):
        bufs = ofdm_estimate_tv_dev(p, d_Y5, 5, nr, want=ALL, stream=st)
        _lib.check(_lib.load().cpx_stream_sync(st))
        assert all(same_bits(d.to_array(s, np.complex128), f) for d, s, f in zip(bufs, shapes, full))
    (d_h,) = ofdm_estimate_tv_dev(p, d_Y5, 5, nr, want='h', stream=user_stream)
    _lib.check(_lib.load().cpx_stream_sync(user_stream))
    assert same_bits(d_h.to_array(shapes[1], np.complex128), full[1])


@pytest.mark.parametrize("name", ["comb52", "block"])
def test_nan_isolation(gpu, name):
    p, fr, nr, B, Y, _ = pattern(name)
    clean = ofdm_estimate_tv_batch(Y, p, want=ALL)
    for s, k, bad in ((int(p.pil_sym[0]), int(p.pil_sc[0]), np.nan), (int(p.data_sym[5]), int(p.data_sc[5]), np.inf)):
        Yb = Y.copy()
        Yb[1, 0, s, k] = bad
        out = ofdm_estimate_tv_batch(Yb, p, want=ALL)
        for a, b in zip(out, clean):
            assert same_bits(a[[0, 2]], b[[0, 2]])
        if np.isnan(bad):
            assert np.isnan(out[2][1]).any() and np.isnan(out[1][1]).any()
        else:
            assert same_bits(out[1][1], clean[1][1]) and not same_bits(out[0][1], clean[0][1])      # a data element: y only


@pytest.mark.parametrize("name", ["comb52", "block"])
def test_tv_handle_serves_map_and_per_frame_estimate(gpu, name):
    p, fr, nr, B, Y, _ = pattern(name)
    plain = OfdmPilots(p.nsc, p.nsym, p.nt, p.pil_sym, p.pil_sc, p.pil_tx, p.pil_val, p.W)
    data = cplx(np.random.RandomState(3), B, p.ndata, p.nt)
    assert same_bits(ofdm_map_batch(data, p), ofdm_map_batch(data, plain))
    for a, b in zip(ofdm_estimate_batch(Y, p, want=('y', 'h', 'h_sc')), ofdm_estimate_batch(Y, plain, want=('y', 'h', 'h_sc'))):
        assert same_bits(a, b)


# ---- 4. more workgroups than the grid -------------------------------------------------------------------------------------------------
def test_grid_cap(gpu):
    """70 001 frames of two subcarriers and two symbols: one workgroup of the fused kernel per frame, more than the grid of 65 535."""
    B = 70001
    p = OfdmPilots(2, 2, 1, [0, 1], [1, 1], [0, 0], [0.6 - 0.8j, 1j], 'linear', 'linear')
    fr = frame_of(p)
    Y = cplx(np.random.RandomState(4), B, 1, 2, 2)
    y, h, hs = ofdm_estimate_tv_batch(Y, p, want=ALL)
    ends = [0, 1, 65534, 65535, 65536, B - 2, B - 1]
    y_m, h_m, hs_m, lsp, hp = T.estimate_tv(fr, Y[ends])
    assert same_bits(y[ends], y_m) and same_bits(y[:, :, 0], Y[:, 0, :, 0])
    assert np.all(np.abs(hs[ends] - hs_m) <= T.h_tv_bound(fr, lsp, hp))
    assert same_bits(h, hs[:, p.data_sym, p.data_sc])
    # all frames: the pilot subcarrier's estimate, held over the band by W, is Y c on its own symbol (V = identity there)
    assert np.allclose(hs[:, :, 1, 0, 0], Y[:, 0, :, 1] * np.conj(p.pil_val) / np.abs(p.pil_val) ** 2, rtol=1e-15, atol=0)
    assert same_bits(hs[:, :, 0], hs[:, :, 1])


# ---- 4b. frames without a data element -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("time_interp", [None, 'hold'])
@pytest.mark.parametrize("shape", [(2, 1, 1, 1), (4, 2, 2, 3)])
def test_frames_of_pilots_only(gpu, shape, time_interp):
    """Every resource element is a pilot (ndata = 0): y_data and h_data are empty and no demap kernel is launched, by either estimator
    (the time-tracking one needs a plan made with time_interp); the estimates on the grid are the models'."""
    nsc, nsym, nt, nr = shape
    B = 2
    p = OfdmPilots.block(nsc, nsym, nt, time_interp=time_interp)
    assert p.ndata == 0
    Y = cplx(np.random.RandomState(8 + nsc), B, nr, nsym, nsc)
    fr0 = M.Frame(p.nsc, p.nsym, p.nt, p.pil_sym, p.pil_sc, p.pil_tx, p.pil_val, p.W)
    y_m, h_m, hsc_m, ls = M.estimate(fr0, Y)
    assert y_m.shape == (B, 0, nr) and h_m.shape == (B, 0, nr, nt)
    y, h, hsc = ofdm_estimate_batch(Y, p, want=('y', 'h', 'h_sc'))
    assert _lib.last_kernel() == "ofdm_ls_kernel+ofdm_interp_kernel"
    assert same_bits(y, y_m) and same_bits(h, h_m)
    err, bound = np.abs(hsc - hsc_m), M.h_bound(fr0, ls)
    print("pilots only", shape, time_interp, "per frame: largest share of the bound %.3f" % np.max(err / bound))
    assert hsc.shape == (B, nsc, nr, nt) and np.all(err <= bound)
    assert [a.shape for a in ofdm_estimate_batch(Y, p, want=('y', 'h'))] == [(B, 0, nr), (B, 0, nr, nt)]
    if time_interp is None:
        return
    fr = frame_of(p)
    y_m, h_m, hs_m, lsp, hp = T.estimate_tv(fr, Y)
    assert y_m.shape == (B, 0, nr) and h_m.shape == (B, 0, nr, nt)
    y, h, hs = ofdm_estimate_tv_batch(Y, p, want=ALL)
    assert _lib.last_kernel() == TV_KERNELS % "lds"
    assert same_bits(y, y_m) and same_bits(h, h_m)
    err, bound = np.abs(hs - hs_m), T.h_tv_bound(fr, lsp, hp)
    pos = bound > 0
    print("pilots only", shape, time_interp, "time tracking: largest share of the bound %.3f" % np.max(err[pos] / bound[pos]))
    assert hs.shape == (B, nsym, nsc, nr, nt) and np.all(err <= bound)
    assert [a.shape for a in ofdm_estimate_tv_batch(Y, p, want=('y', 'h'))] == [(B, 0, nr), (B, 0, nr, nt)]


# ---- 5. errors on the device path -----------------------------------------------------------------------------------------------------
def test_device_path_errors(gpu):
    lib = _lib.load()
    p, _, nr, B, Y, _ = pattern("comb52")
    plain = OfdmPilots.comb(52, 6, 2, 4, [0, 3], 'linear')
    buf = DeviceBuf(Y.nbytes * p.nt)
    d = buf.ptr
    tv = lib.cpx_pilots_estimate_tv_dev
    assert tv(plain.handle(), d, B, nr, d, None, None, None) == _lib.CPX_EINVAL
    assert _lib.last_error() == "ofdm_estimate_tv: the plan has no time matrices (it was made by cpx_pilots_create, not cpx_pilots_create_tv)"
    assert tv(plain.handle(), d, 0, nr, d, None, None, None) == _lib.CPX_EINVAL     # ... whatever the batch size
    assert tv(p.handle(), d, B, nr, None, None, None, None) == _lib.CPX_EINVAL and _lib.last_error() == "ofdm_estimate_tv: no output requested"
    assert tv(p.handle(), d, B, 0, d, None, None, None) == _lib.CPX_EINVAL and "nr = 0" in _lib.last_error()
    assert tv(p.handle(), d, B, 1025, d, None, None, None) == _lib.CPX_ELIMIT
    assert tv(p.handle(), d, -1, nr, d, None, None, None) == _lib.CPX_EINVAL
    assert tv(p.handle(), None, B, nr, d, None, None, None) == _lib.CPX_EINVAL and _lib.last_error() == "ofdm_estimate_tv: null pointer"
    assert tv(p.handle(), None, 0, nr, d, None, None, None) == _lib.CPX_OK          # an empty batch: no launch, nothing read
    assert lib.cpx_pilots_estimate_tv(p.handle(), None, 0, nr, None, _lib.ptr(np.zeros(2)), None) == _lib.CPX_OK
    _lib.check(lib.cpx_stream_sync(None))
    with pytest.raises(ValueError):
        ofdm_estimate_tv_batch(Y, plain)


# ---- 6. end to end through the real chain ---------------------------------------------------------------------------------------------
E2E = {"qam16_1x1": (16, 1, 1, 64, 52, 16, 4), "qam16_2x2": (16, 2, 2, 64, 52, 16, 4), "qam64_2x3": (64, 2, 3, 256, 200, 32, 8)}
E2E_MODES = {"linear": (0.005, 'linear'), "doppler": (0.02, ('doppler', 0.02, 1e-8))}   # cycles per OFDM symbol, time_interp


def zf_model(y, H, constellation):
    """Zero forcing and the nearest constellation point, in NumPy: y [V, nr], H [V, nr, nt] -> indices [V, nt]."""
    Hh = np.conj(H.transpose(0, 2, 1))
    x = np.linalg.solve(Hh @ H, Hh @ y[..., None])[..., 0]
    return np.argmin(np.abs(x[..., None] - constellation), axis=-1)


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("mode", sorted(E2E_MODES))
@pytest.mark.parametrize("case", sorted(E2E))
def test_end_to_end_noise_free(gpu, case, mode, seed):
    """map -> ofdm_tx -> fading channel (one block per OFDM symbol) -> ofdm_rx -> estimate -> ZF, no noise: the time-tracking estimate
    detects every index, the per-frame estimate does not.  Both statements are first made on the CPU models."""
    m, nt, nr, nfft, nsc, cp, spacing = E2E[case]
    fd_sym, time_interp = E2E_MODES[mode]
    B, nsym, L, Ns = 3, 14, 8, 16
    hold = nfft + cp
    fd = fd_sym / hold
    pdp = np.exp(-0.5 * np.arange(L))
    pdp /= pdp.sum()
    p = OfdmPilots.comb(nsc, nsym, nt, spacing, [0, 4, 9, 13], ('taps', 8, nfft), time_interp=time_interp)
    md = QAMModem(m)
    idx = np.random.RandomState(seed).randint(0, m, size=(B, p.ndata, nt))
    V = B * p.ndata
    # the CPU: the fading model's gains, the channel applied per subcarrier (L - 1 <= cp), the two estimators' models
    fr, fr0 = frame_of(p), M.Frame(p.nsc, p.nsym, p.nt, p.pil_sym, p.pil_sc, p.pil_tx, p.pil_val, p.W)
    nblk = -(-(nsym * hold + L - 1) // hold)
    Gm = FM.gains(B, nr, nt, pdp, fd, nblk, hold, 0, Ns, None, 0.0, seed, 17)[:, :nsym]
    Hm = tap_frequency_response(Gm, nfft, nsc).transpose(0, 1, 4, 2, 3)             # [B, nsym, nsc, nr, nt]
    kappa = float(np.max(np.linalg.cond(Hm)))
    assert kappa < 1e6
    Ym = np.einsum('bskrt,btsk->brsk', Hm, M.map_grid(fr0, md.constellation[idx]))
    y_m, h_m = T.estimate_tv(fr, Ym)[:2]
    wrong_m = int(np.count_nonzero(zf_model(y_m.reshape(V, nr), h_m.reshape(V, nr, nt), md.constellation).reshape(idx.shape) != idx))
    y_0, h_0 = M.estimate(fr0, Ym)[:2]
    wrong_m0 = int(np.count_nonzero(zf_model(y_0.reshape(V, nr), h_0.reshape(V, nr, nt), md.constellation).reshape(idx.shape) != idx))
    print("tv end to end", case, mode, seed, "model: kappa %.3g, wrong %d (tracking) and %d (per frame) of %d" % (kappa, wrong_m, wrong_m0, idx.size))
    assert wrong_m == 0 and wrong_m0 >= 1
    # the device
    grid = ofdm_map_batch(md.constellation[idx], p)
    tx = ofdm_tx_batch(grid.reshape(B * nt, nsym, nsc), nfft, cp).reshape(B, nt, nsym * hold)
    rx, G = fading_multipath_batch(tx, nr, pdp, fd, hold=hold, n_sin=Ns, seed=seed, stream_id=17, want=('y', 'g'))
    Y = ofdm_rx_batch(rx.reshape(B * nr, -1), nfft, nsc, cp).reshape(B, nr, nsym, nsc)
    y, h, hs = ofdm_estimate_tv_batch(Y, p, want=ALL)
    sent = md.constellation[idx]
    det = linear_batch(y.reshape(V, nr), h.reshape(V, nr, nt), md, 0, method='zf', output_type='hard')
    wrong = int(np.count_nonzero(det.reshape(sent.shape) != sent))
    y0, h0 = ofdm_estimate_batch(Y, p)
    det0 = linear_batch(y0.reshape(V, nr), h0.reshape(V, nr, nt), md, 0, method='zf', output_type='hard')
    wrong0 = int(np.count_nonzero(det0.reshape(sent.shape) != sent))
    H = tap_frequency_response(G[:, :nsym], nfft, nsc).transpose(0, 1, 4, 2, 3)
    err, rms = np.max(np.abs(hs - H)), np.sqrt(np.mean(np.abs(H) ** 2))
    print("tv end to end", case, mode, seed, "device: wrong %d (tracking) and %d (per frame) of %d, max|H^ - H| = %.2e rms" %
          (wrong, wrong0, idx.size, err / rms))
    assert wrong == 0
    assert wrong0 >= 1


# ---- 7. the chain on the device -------------------------------------------------------------------------------------------------------
def test_device_chain_matches_staged_host_calls(gpu, user_stream):
    """map -> ofdm_tx -> fading channel -> ofdm_rx -> time-tracking estimate -> ZF detection on one stream, nothing copied to the host
    in between, against the same stages called one by one on host arrays."""
    lib = _lib.load()
    st = user_stream
    B, nt, nr, L, nfft, nsc, cp, nsym, Ns, seed = 4, 2, 2, 8, 64, 52, 16, 14, 16, 5
    hold = nfft + cp
    per, fd = nsym * hold, 0.005 / hold
    n_rx = per + L - 1
    pdp = np.exp(-0.5 * np.arange(L))
    pdp /= pdp.sum()
    p = OfdmPilots.comb(nsc, nsym, nt, 4, [0, 4, 9, 13], ('taps', 8, nfft), time_interp='linear')
    md = QAMModem(16)
    data = md.constellation[np.random.RandomState(9).randint(0, 16, size=(B, p.ndata, nt))]
    plan = modulation._ofdm_plan(nfft, nsc, cp).handle()
    V = B * p.ndata
    # staged: every stage on host arrays
    grid = ofdm_map_batch(data, p)
    tx = ofdm_tx_batch(grid.reshape(B * nt, nsym, nsc), nfft, cp).reshape(B, nt, per)
    rx = fading_multipath_batch(tx, nr, pdp, fd, hold=hold, n_sin=Ns, seed=seed, stream_id=17)
    Y = ofdm_rx_batch(rx.reshape(B * nr, n_rx), nfft, nsc, cp).reshape(B, nr, nsym, nsc)
    y, h = ofdm_estimate_tv_batch(Y, p)
    idx = _linear_run(y.reshape(V, nr), h.reshape(V, nr, nt), md, 0.0, 0.0, ('idx',))['idx']
    # the chain
    d_data = DeviceBuf.from_array(data)
    d_tx, d_Y, d_idx = DeviceBuf(tx.nbytes), DeviceBuf(Y.nbytes), DeviceBuf(V * nt * 4)
    d_grid = ofdm_map_dev(p, d_data, B, stream=st)
    _lib.check(lib.cpx_ofdm_tx_dev(plan, d_grid.ptr, B * nt, nsym, d_tx.ptr, st))
    d_rx = fading_channel_dev(d_tx, B, nt, nr, per, pdp, fd, hold=hold, n_sin=Ns, seed=seed, stream_id=17, stream=st)
    _lib.check(lib.cpx_ofdm_rx_dev(plan, d_rx.ptr, B * nr, n_rx, d_Y.ptr, st))
    d_y, d_h = ofdm_estimate_tv_dev(p, d_Y, B, nr, stream=st)
    _lib.check(lib.cpx_mimo_linear_dev(md._device_handle(), d_y.ptr, d_h.ptr, 1, V, nr, nt, 0.0, 0.0, d_idx.ptr, None, None, None, st))
    _lib.check(lib.cpx_stream_sync(st))
    assert same_bits(d_Y.to_array(Y.shape, np.complex128), Y)
    assert same_bits(d_y.to_array(y.shape, np.complex128), y) and same_bits(d_h.to_array(h.shape, np.complex128), h)
    assert same_bits(d_idx.to_array(idx.shape, np.int32), idx)
    assert np.count_nonzero(md.constellation[idx].reshape(data.shape) != data) == 0
