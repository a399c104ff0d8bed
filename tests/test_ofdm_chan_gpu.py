"""The multipath channel, the resource mapping and the pilot-aided channel estimator on the MI355X (csrc/ofdm_chan.hip) against the
NumPy model of ofdm_chan_model.py.

Tolerances, derived rather than tuned: two float64 sums of T products of the same operands differ by at most
2 (T + 2) 2^-53 sqrt(2) sum|g| max|x| -- T = nt L for the channel, and for the estimator T + 2 = np_t + c + 8 with sum_j |W_t[k][j]|
max_j |LS_j| as the operands' size (ofdm_chan_model.h_bound).  Copies (map, y_data, h_data against h_sc) are exact."""
import ctypes

import numpy as np
import pytest

import ofdm_chan_model as M
from commpy_amd import _lib, modulation
from commpy_amd.channels import multipath_batch
from commpy_amd.deviceops import DeviceBuf, multipath_dev, ofdm_estimate_dev, ofdm_map_dev
from commpy_amd.modulation import (OfdmPilots, QAMModem, _linear_run, linear_batch, ofdm_estimate_batch, ofdm_map_batch, ofdm_rx_batch,
                                   ofdm_tx_batch)

pytestmark = pytest.mark.gpu


def cplx(rs, *shape):
    return rs.randn(*shape) + 1j * rs.randn(*shape)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def frame_of(p):
    return M.Frame(p.nsc, p.nsym, p.nt, p.pil_sym, p.pil_sc, p.pil_tx, p.pil_val, p.W)


@pytest.fixture(scope="module")
def user_stream(gpu):
    lib = _lib.load()
    st = ctypes.c_void_p()
    _lib.check(lib.cpx_stream_create(ctypes.byref(st)))
    yield st
    lib.cpx_stream_sync(st)
    lib.cpx_stream_destroy(st)


def on_stream(fn, st):
    """fn() queues work on the stream `st`; its DeviceBufs are read once the stream has finished."""
    out = fn()
    _lib.check(_lib.load().cpx_stream_sync(st))
    return out


# ---- multipath ----------------------------------------------------------------------------------------------------------------
def mp_bound(x, g):
    """[B, nr, 1]: 2 (nt L + 2) 2^-53 sqrt(2) sum|g[b][r]| max|x[b]|."""
    B, nt, _ = x.shape
    g4 = np.broadcast_to(g, (B,) + g.shape[-3:])
    T = nt * g.shape[-1]
    return (2 * (T + 2) * 2.0 ** -53 * np.sqrt(2) * np.sum(np.abs(g4), axis=(2, 3)) * np.max(np.abs(x), axis=(1, 2))[:, None])[:, :, None]


# the issue's cases, then the tiled kernel with nr = 4 (one group), nr = 5 (two groups, the second partly empty), nr = 2, and taps in two chunks
MP_CASES = [(1, 1, 1, 1, 1), (3, 1, 1, 257, 5), (1, 1, 2, 3, 8), (2, 2, 3, 1000, 17), (2, 4, 4, 323, 16), (1, 3, 2, 5000, 64),
            (2, 4, 4, 1500, 16), (1, 1, 5, 700, 3), (2, 2, 2, 1100, 7), (1, 1, 1, 2100, 600)]


@pytest.mark.parametrize("B, nt, nr, n, L", MP_CASES)
@pytest.mark.parametrize("batched", [False, True])
def test_multipath_against_model(gpu, B, nt, nr, n, L, batched):
    rs = np.random.RandomState(B * 1000 + n + L)
    x = cplx(rs, B, nt, n)
    g = cplx(rs, B, nr, nt, L) if batched else cplx(rs, nr, nt, L)
    got = multipath_batch(x, g)
    kernel = _lib.last_kernel()
    assert kernel == ("multipath_kernel<%d>" % (4 if nr >= 3 else nr) if 2 * (n + L - 1) >= 1024 else "multipath_direct")
    assert got.shape == (B, nr, n + L - 1) and got.dtype == np.complex128
    err, bound = np.abs(got - M.multipath(x, g)), mp_bound(x, g)
    print("multipath", (B, nt, nr, n, L), kernel, "largest share of the bound: %.3f" % np.max(err / bound))
    assert np.all(err <= bound)


def test_multipath_identity_and_siso_forms(gpu):
    rs = np.random.RandomState(5)
    for n in (1, 300, 3000):
        x = cplx(rs, 3, n)
        assert same_bits(multipath_batch(x, np.ones(1)), x)
        assert same_bits(multipath_batch(x[:, None, :], np.ones((1, 1, 1)))[:, 0], x)
    x, g = cplx(rs, 3, 700), cplx(rs, 3, 4)
    assert same_bits(multipath_batch(x, g), multipath_batch(x[:, None], g[:, None, None])[:, 0])
    assert same_bits(multipath_batch(x, g[1]), multipath_batch(x[:, None], g[1][None, None])[:, 0])


def test_multipath_limits(gpu):
    lib = _lib.load()
    buf = DeviceBuf(64 * 1024)
    p = buf.ptr
    mp = lambda *a: lib.cpx_multipath_dev(*a)
    assert mp(p, p, 0, 1, 1, 1, 4, 1025, p, None) == _lib.CPX_ELIMIT
    assert mp(p, p, 0, 1, 2, 2, 4, 513, p, None) == _lib.CPX_ELIMIT and "2052 taps" in _lib.last_error()
    assert mp(p, p, 0, 1, 2, 2, 4, 512, p, None) == _lib.CPX_OK and mp(p, p, 0, 1, 1, 1, 4, 1024, p, None) == _lib.CPX_OK
    for nt, nr, n, L in ((0, 1, 4, 1), (1, 0, 4, 1), (1, 1, 4, 0), (1, 1, 0, 1), (-1, 1, 4, 1)):
        assert mp(p, p, 0, 1, nt, nr, n, L, p, None) == _lib.CPX_EINVAL
    for args in ((None, p, p), (p, None, p), (p, p, None)):
        assert mp(args[0], args[1], 0, 1, 1, 1, 4, 2, args[2], None) == _lib.CPX_EINVAL and _lib.last_error() == "multipath: null pointer"
    assert mp(None, None, 0, 0, 1, 1, 0, 1, None, None) == _lib.CPX_OK
    _lib.check(lib.cpx_stream_sync(None))
    with pytest.raises(ValueError):
        multipath_batch(np.zeros((1, 2, 4)), np.ones((2, 2, 513)))


@pytest.mark.parametrize("nt, nr, n, L", [(2, 3, 1000, 17), (2, 2, 300, 9)])          # the tiled and the direct kernel
def test_multipath_bit_identity(gpu, user_stream, nt, nr, n, L):
    rs = np.random.RandomState(7)
    x, g = cplx(rs, 5, nt, n), cplx(rs, nr, nt, L)
    alone = multipath_batch(x[3:4], g)[0]
    assert same_bits(multipath_batch(x, g)[3], alone)
    assert same_bits(multipath_batch(x[[3, 0, 1, 2, 4]], g)[0], alone)
    gb = cplx(rs, 5, nr, nt, L)
    gb[3] = g
    assert same_bits(multipath_batch(x, gb)[3], alone)                               # g replicated per row
    assert same_bits(multipath_batch(x[2:4], gb[2:4])[1], alone)
    d_x, d_g, d_gb = DeviceBuf.from_array(x), DeviceBuf.from_array(g), DeviceBuf.from_array(gb)
    d_y = on_stream(lambda: multipath_dev(d_x, d_gb, 1, 5, nt, nr, n, L, stream=user_stream), user_stream)
    assert same_bits(d_y.to_array((5, nr, n + L - 1), np.complex128)[3], alone)
    d_y = multipath_dev(d_x, d_g, 0, 5, nt, nr, n, L)
    assert same_bits(d_y.to_array((5, nr, n + L - 1), np.complex128)[3], alone)


def _peek(buf, start, count):
    out = np.zeros(count, complex)
    _lib.check(_lib.load().cpx_memcpy_d2h(_lib.ptr(out), ctypes.c_void_p(buf.ptr.value + start * 16), count * 16))
    return out


def test_multipath_large_row(gpu):
    """One row of 2^27 + 5 samples (2 GB in, 2 GB out): 131 073 tiles, more than the grid, and offsets past 2^31 bytes."""
    lib = _lib.load()
    n, L = 2 ** 27 + 5, 2
    md = QAMModem(4)
    g = np.array([0.75 - 0.5j, 0.25 + 1.5j])
    bits, x, y, d_g = DeviceBuf(2 * n), DeviceBuf(16 * n), DeviceBuf(16 * (n + 1)), DeviceBuf.from_array(g)
    _lib.check(lib.cpx_random_bits_dev(bits.ptr, 2 * n, 3, 0, None))
    _lib.check(lib.cpx_modulate_dev(md._device_handle(), bits.ptr, n, x.ptr, None))
    _lib.check(lib.cpx_multipath_dev(x.ptr, d_g.ptr, 0, 1, 1, 1, n, L, y.ptr, None))
    _lib.check(lib.cpx_stream_sync(None))
    assert _lib.last_kernel() == "multipath_kernel<1>"
    for m0 in (0, 1024 - 50, 65535 * 1024 - 50, 2 ** 26 - 50, 2 ** 27 - 50, n + 1 - 100):   # ends, tile boundaries, the grid's wrap
        cnt = min(100, n + 1 - m0)
        got = _peek(y, m0, cnt)
        lo, hi = max(0, m0 - 1), min(n, m0 + cnt)
        seg = _peek(x, lo, hi - lo)
        want = np.convolve(seg, g)[m0 - lo:][:cnt]
        assert len(want) == cnt
        assert np.max(np.abs(got - want)) <= 2 * (L + 2) * 2.0 ** -53 * np.sqrt(2) * np.sum(np.abs(g)) * np.max(np.abs(seg))
    for b in (bits, x, y):
        b.free()


# ---- map and estimate ---------------------------------------------------------------------------------------------------------
PATTERNS = {
    "a": (lambda: OfdmPilots(2, 1, 1, [0], [1], [0], [0.6 - 0.8j]), 1, 3),
    "b": (lambda: OfdmPilots.comb(52, 4, 2, 4, [0, 2], 'linear'), 2, 3),
    "c": (lambda: OfdmPilots.comb(52, 4, 2, 4, [0, 2], ('taps', 8, 64)), 2, 3),
    "d": (lambda: OfdmPilots.block(52, 5, 3), 2, 3),
    "e": (lambda: OfdmPilots.comb(1200, 14, 4, 8, [0, 4, 7, 11], ('taps', 16, 2048)), 4, 2),
    "f": (lambda: OfdmPilots(2, 1, 1, [0], [1], [0], [0.6 - 0.8j]), 1, 70001),
}
_cache = {}


def pattern(name):
    """(pilots, model frame, nr, B, Y, model outputs): built once and shared by the tests, never changed."""
    if name not in _cache:
        make, nr, B = PATTERNS[name]
        p = make()
        fr = frame_of(p)
        Y = cplx(np.random.RandomState(ord(name)), B, nr, p.nsym, p.nsc)
        _cache[name] = (p, fr, nr, B, Y, M.estimate(fr, Y))
    return _cache[name]


@pytest.mark.parametrize("name", sorted(PATTERNS))
def test_map_is_exact(gpu, name):
    p, fr, nr, B, _, _ = pattern(name)
    data = cplx(np.random.RandomState(3), B, p.ndata, p.nt)
    grid = ofdm_map_batch(data, p)
    assert _lib.last_kernel() == "ofdm_map_kernel"
    assert same_bits(grid, M.map_grid(fr, data))
    d_data = DeviceBuf.from_array(data)
    d_grid = ofdm_map_dev(p, d_data, B)
    assert same_bits(d_grid.to_array(grid.shape, np.complex128), grid)


@pytest.mark.parametrize("name", sorted(PATTERNS))
def test_estimate_against_model(gpu, name):
    p, fr, nr, B, Y, (y_m, h_m, hsc_m, ls) = pattern(name)
    y, h, hsc = ofdm_estimate_batch(Y, p, want=('y', 'h', 'h_sc'))
    assert _lib.last_kernel() == "ofdm_ls_kernel+ofdm_interp_kernel+ofdm_hdemap_kernel+ofdm_ydemap_kernel"
    assert y.shape == (B, p.ndata, nr) and h.shape == (B, p.ndata, nr, p.nt) and hsc.shape == (B, p.nsc, nr, p.nt)
    assert same_bits(y, y_m)
    bound = M.h_bound(fr, ls)
    err = np.abs(hsc - hsc_m)
    print("estimate", name, "largest share of the bound: %.3f" % np.max(err / bound))
    assert np.all(err <= bound)
    assert same_bits(h, hsc[:, p.data_sc])                                          # h_data = the matching rows of h_sc, bit for bit
    assert np.all(np.abs(h - h_m) <= bound[:, p.data_sc])
    # whichever outputs are requested
    for want, ref in ((('y',), (y,)), (('h',), (h,)), (('h_sc',), (hsc,)), (('y', 'h'), (y, h)), (('h', 'h_sc'), (h, hsc))):
        out = ofdm_estimate_batch(Y, p, want=want)
        assert len(out) == len(ref) and all(same_bits(a, b) for a, b in zip(out, ref)), want
    assert _lib.last_kernel() == "ofdm_ls_kernel+ofdm_interp_kernel+ofdm_hdemap_kernel"


@pytest.mark.parametrize("name", ["b", "d", "e"])
def test_estimate_bit_identity(gpu, user_stream, name):
    p, fr, nr, B, Y, _ = pattern(name)
    rs = np.random.RandomState(11)
    Y5 = cplx(rs, 5, nr, p.nsym, p.nsc)
    Y5[3] = Y[0]
    alone = ofdm_estimate_batch(Y[:1], p, want=('y', 'h', 'h_sc'))
    for batch, pos in ((Y5, 3), (Y5[[3, 0, 1]], 0), (Y5[2:4], 1)):
        out = ofdm_estimate_batch(batch, p, want=('y', 'h', 'h_sc'))
        assert all(same_bits(a[pos], b[0]) for a, b in zip(out, alone))
    shapes = ((5, p.ndata, nr), (5, p.ndata, nr, p.nt), (5, p.nsc, nr, p.nt))
    d_Y5 = DeviceBuf.from_array(Y5)
    for st in (user_stream, None):
        bufs = ofdm_estimate_dev(p, d_Y5, 5, nr, want=('y', 'h', 'h_sc'), stream=st)
        _lib.check(_lib.load().cpx_stream_sync(st))
        assert all(same_bits(d.to_array(s, np.complex128)[3], b[0]) for d, s, b in zip(bufs, shapes, alone))
    (d_h,) = on_stream(lambda: ofdm_estimate_dev(p, d_Y5, 5, nr, want='h', stream=user_stream), user_stream)
    assert same_bits(d_h.to_array(shapes[1], np.complex128)[3], alone[1][0])


@pytest.mark.parametrize("name", ["b", "d"])
def test_estimate_nan_isolation(gpu, name):
    p, fr, nr, B, Y, _ = pattern(name)
    clean = ofdm_estimate_batch(Y, p, want=('y', 'h', 'h_sc'))
    for s, k, bad in ((int(p.pil_sym[0]), int(p.pil_sc[0]), np.nan), (int(p.data_sym[5]), int(p.data_sc[5]), np.inf)):
        Yb = Y.copy()
        Yb[1, 0, s, k] = bad
        out = ofdm_estimate_batch(Yb, p, want=('y', 'h', 'h_sc'))
        for a, b in zip(out, clean):
            assert same_bits(a[[0, 2]], b[[0, 2]])
        if np.isnan(bad):
            assert np.isnan(out[2][1]).any() and np.isnan(out[1][1]).any()
        else:
            assert same_bits(out[1][1], clean[1][1]) and not same_bits(out[0][1], clean[0][1])      # a data element: y only


# ---- end to end ---------------------------------------------------------------------------------------------------------------
E2E = {
    "i": dict(nfft=64, nsc=52, cp=16, nsym=4, nt=2, nr=2, L=4, decay=0.7, spacing=4, psym=[0, 2], interp=('taps', 8, 64), m=16, count=936),
    "ii": dict(nfft=256, nsc=200, cp=32, nsym=4, nt=4, nr=4, L=6, decay=0.3, spacing=8, psym=[0, 2], interp=('taps', 16, 256), m=64, count=7200),
    "iii": dict(nfft=64, nsc=52, cp=16, nsym=3, nt=1, nr=1, L=1, decay=0.0, spacing=4, psym=[1], interp='linear', m=16, count=429),
}


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("case", sorted(E2E))
def test_end_to_end_noise_free(gpu, case, seed):
    c = E2E[case]
    B, nt, nr, L, nfft, nsc, cp = 3, c["nt"], c["nr"], c["L"], c["nfft"], c["nsc"], c["cp"]
    rs = np.random.RandomState(seed)
    p = OfdmPilots.comb(nsc, c["nsym"], nt, c["spacing"], c["psym"], c["interp"])
    md = QAMModem(c["m"])
    idx = rs.randint(0, c["m"], size=(B, p.ndata, nt))
    assert idx.size == c["count"]
    g = (rs.randn(B, nr, nt, L) + 1j * rs.randn(B, nr, nt, L)) * np.sqrt(0.5) * np.exp(-c["decay"] * np.arange(L))
    grid = ofdm_map_batch(md.constellation[idx], p)
    tx = ofdm_tx_batch(grid.reshape(B * nt, c["nsym"], nsc), nfft, cp).reshape(B, nt, -1)
    rx = multipath_batch(tx, g)
    Y = ofdm_rx_batch(rx.reshape(B * nr, -1), nfft, nsc, cp).reshape(B, nr, c["nsym"], nsc)
    y, h, hsc = ofdm_estimate_batch(Y, p, want=('y', 'h', 'h_sc'))
    det = linear_batch(y.reshape(-1, nr), h.reshape(-1, nr, nt), md, 0, method='zf', output_type='hard')
    wrong = int(np.count_nonzero(det.reshape(B, p.ndata, nt) != md.constellation[idx]))
    bins = M.frequencies(nsc) % nfft
    Htrue = np.fft.fft(g, nfft, axis=-1)[..., bins].transpose(0, 3, 1, 2)           # [B, nsc, nr, nt]
    err, rms = np.max(np.abs(hsc - Htrue)), np.sqrt(np.mean(np.abs(Htrue) ** 2))
    print("end to end", case, seed, "wrong %d of %d, max|H^ - H| = %.2e rms" % (wrong, idx.size, err / rms))
    assert wrong == 0
    assert err <= 1e-10 * rms


def test_device_chain_matches_staged_host_calls(gpu, user_stream):
    """map -> ofdm_tx -> multipath -> awgn -> ofdm_rx -> estimate -> ZF detection on one stream, nothing copied to the host in
    between, against the same stages called one by one on host arrays."""
    lib = _lib.load()
    st = user_stream
    B, nt, nr, L, nfft, nsc, cp, nsym = 4, 2, 2, 4, 64, 52, 16, 4
    rs = np.random.RandomState(9)
    p = OfdmPilots.comb(nsc, nsym, nt, 4, [0, 2], ('taps', 8, 64))
    md = QAMModem(16)
    data = md.constellation[rs.randint(0, 16, size=(B, p.ndata, nt))]
    g = cplx(rs, B, nr, nt, L) * np.sqrt(0.5) * np.exp(-0.7 * np.arange(L))
    plan = modulation._ofdm_plan(nfft, nsc, cp).handle()
    per = nsym * (cp + nfft)
    n_rx = per + L - 1
    sigma, seed, sid, V = 1e-4, 5, 3, B * p.ndata

    def awgn(d_in, d_out, stream):
        _lib.check(lib.cpx_awgn_dev(d_in.ptr, B * nr * n_rx, sigma, sigma, seed, sid, d_out.ptr, stream))

    # staged: every stage on host arrays
    grid = ofdm_map_batch(data, p)
    tx = ofdm_tx_batch(grid.reshape(B * nt, nsym, nsc), nfft, cp).reshape(B, nt, per)
    rx = multipath_batch(tx, g)
    d_clean, d_noisy = DeviceBuf.from_array(rx), DeviceBuf(rx.nbytes)
    awgn(d_clean, d_noisy, None)
    noisy = d_noisy.to_array(rx.shape, np.complex128)
    assert not same_bits(noisy, rx)
    Y = ofdm_rx_batch(noisy.reshape(B * nr, n_rx), nfft, nsc, cp).reshape(B, nr, nsym, nsc)
    y, h = ofdm_estimate_batch(Y, p)
    idx = _linear_run(y.reshape(V, nr), h.reshape(V, nr, nt), md, 0.0, sigma * sigma * 2, ('idx',))['idx']
    # the chain
    d_data, d_g = DeviceBuf.from_array(data), DeviceBuf.from_array(g)
    d_tx, d_rxn, d_Y, d_idx = DeviceBuf(tx.nbytes), DeviceBuf(rx.nbytes), DeviceBuf(Y.nbytes), DeviceBuf(V * nt * 4)
    d_grid = ofdm_map_dev(p, d_data, B, stream=st)
    _lib.check(lib.cpx_ofdm_tx_dev(plan, d_grid.ptr, B * nt, nsym, d_tx.ptr, st))
    d_rx = multipath_dev(d_tx, d_g, 1, B, nt, nr, per, L, stream=st)
    awgn(d_rx, d_rxn, st)
    _lib.check(lib.cpx_ofdm_rx_dev(plan, d_rxn.ptr, B * nr, n_rx, d_Y.ptr, st))
    d_y, d_h = ofdm_estimate_dev(p, d_Y, B, nr, stream=st)
    _lib.check(lib.cpx_mimo_linear_dev(md._device_handle(), d_y.ptr, d_h.ptr, 1, V, nr, nt, 0.0, sigma * sigma * 2, d_idx.ptr, None, None,
                                       None, st))
    _lib.check(lib.cpx_stream_sync(st))
    assert same_bits(d_y.to_array(y.shape, np.complex128), y) and same_bits(d_h.to_array(h.shape, np.complex128), h)
    assert same_bits(d_idx.to_array(idx.shape, np.int32), idx)
    assert np.count_nonzero(md.constellation[idx].reshape(data.shape) != data) == 0
