"""The Doppler-fading multipath channel on the MI355X (csrc/fading.hip) against the NumPy model of fading_model.py.

Tolerances, derived rather than tuned (fading_model.py writes them out): the drawn phases are exact; nu is held to twice the measured
deviation of the device's cospi (FADING_ULP, capped at 16 ulp); a gain, against the model evaluated on the device's own (nu, phi), to
gain_bound (the rounding of the kernel's phase, twice the measured deviation of its sincospi, the sum's own roundings); the convolution
to 2 (nt L + 2) 2^-53 sqrt(2) sum|G| max|x|; everything said to be bit-identical is compared byte for byte."""
import ctypes

import numpy as np
import pytest
from scipy.special import j0

import fading_model as M
import rng_model as R
from commpy_amd import _lib
from commpy_amd.channels import (FADING_SCRATCH_BYTES, fading_convolve_batch, fading_gains_batch, fading_multipath_batch,
                                 fading_params_batch, multipath_batch, tap_frequency_response)
from commpy_amd.deviceops import DeviceBuf, fading_channel_dev, fading_convolve_dev, fading_gains_dev, fading_params_dev
from commpy_amd.modulation import QAMModem, linear_batch, ofdm_rx_batch, ofdm_tx_batch

pytestmark = pytest.mark.gpu


def cplx(rs, *shape):
    return rs.randn(*shape) + 1j * rs.randn(*shape)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


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


def taps_of(L):
    """(pdp, kf) of the gain tests: a decaying profile with a tap without power in the middle (L >= 3) and Rician taps (0, 3, 0, 1e6, ...)."""
    pdp = np.exp(-0.3 * np.arange(L))
    if L >= 3:
        pdp[L // 2] = 0.0
    pdp /= pdp.sum()
    kf = np.resize(np.array([0.0, 3.0, 0.0, 1e6]), L) if L >= 2 else None
    return pdp, kf


# ---- 1. params ------------------------------------------------------------------------------------------------------------------------
def nu_deviation(got, want):
    """Largest |got - want| / (2^-52 |want|); where the model is exactly zero the device must be too."""
    nz = want != 0.0
    assert np.array_equal(got[~nz] == 0.0, np.ones(np.count_nonzero(~nz), bool))
    return float(np.max(np.abs(got[nz] - want[nz]) / (R.ULP * np.abs(want[nz]))))


@pytest.mark.parametrize("seed, stream", R.KEYS)
def test_params_against_model(gpu, seed, stream):
    """2^21 draws per key at fd = 1/2 (the multiply rounds nothing): phi bit for bit, nu within FADING_ULP."""
    B, nr, nt, L, Ns = 512, 2, 2, 16, 63
    first = 5 if seed == 7 else 0
    got = fading_params_batch(B, nr, nt, L, 0.5, n_sin=Ns, fd_los=-0.25, seed=seed, stream_id=stream, first_row=first)
    assert _lib.last_kernel() == "fading_params_kernel"
    want = M.params(B, nr, nt, L, Ns, 0.5, -0.25, seed, stream, first_row=first)
    assert got.shape == want.shape == (B, nr, nt, L, Ns + 1, 2)
    assert same_bits(got[..., 1], want[..., 1])                                  # the drawn integers, exactly
    assert same_bits(got[..., Ns, 0], want[..., Ns, 0])
    dev = nu_deviation(got[..., :Ns, 0], want[..., :Ns, 0])
    print("fading params", (seed, stream), "largest deviation of nu: %.3f ulp (FADING_ULP_MEASURED %.2f)" % (dev, M.FADING_ULP_MEASURED))
    assert M.FADING_ULP <= M.FADING_ULP_CAP
    assert dev <= M.FADING_ULP


def test_params_other_dopplers(gpu):
    """fd = 0 gives nu = +-0; a Doppler that is no power of two adds the product's own rounding on both sides: one more ulp."""
    z = fading_params_batch(3, 1, 2, 5, 0.0, n_sin=7, fd_los=0.0, seed=1, stream_id=2)
    assert np.all(z[..., 0] == 0.0)
    assert same_bits(z[..., 1], M.params(3, 1, 2, 5, 7, 0.0, 0.0, 1, 2)[..., 1])
    got = fading_params_batch(64, 1, 2, 16, 0.01, n_sin=16, seed=3, stream_id=4)
    want = M.params(64, 1, 2, 16, 16, 0.01, 0.0, 3, 4)
    assert nu_deviation(got[..., :16, 0], want[..., :16, 0]) <= M.FADING_ULP + 1.0
    assert np.all(np.abs(got[..., :16, 0]) <= 0.01)


# ---- 2. gains -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed, stream", R.KEYS)
def test_sincospi_constant(gpu, seed, stream):
    """Ns = 1, pdp = 1, tau = 0: G is the bare (cos, sin) of 2 pi phi.  2^21 paths per key; the measurement behind FADING_SINCOS_ULP."""
    B, L = 2048, 1024
    pdp = np.ones(L)
    prm = fading_params_batch(B, 1, 1, L, 0.5, n_sin=1, seed=seed, stream_id=stream)
    G = fading_gains_batch(B, 1, 1, pdp, 0.5, 1, n_sin=1, seed=seed, stream_id=stream)
    assert _lib.last_kernel() == "fading_gains_kernel"
    want = M.gains_from_params(prm, pdp, None, [0])
    dev = max(np.max(np.abs(G.real - want.real)), np.max(np.abs(G.imag - want.imag))) / R.ULP
    print("fading sincospi", (seed, stream), "largest deviation: %.3f (FADING_SINCOS_ULP_MEASURED %.2f)" % (dev, M.FADING_SINCOS_ULP_MEASURED))
    assert M.FADING_SINCOS_ULP <= M.FADING_ULP_CAP
    assert dev <= M.FADING_SINCOS_ULP


GAIN_SHAPES = [(1, 1, 1, 1, 1, 1, 1, 0), (3, 2, 2, 5, 8, 7, 3, 0), (2, 1, 3, 16, 16, 300, 1, 12345), (1, 4, 4, 16, 64, 5, 80, 2 ** 40),
               (2, 1, 1, 1024, 2, 2, 1000, 0), (1, 2, 1, 3, 256, 4, 1, 0)]


@pytest.mark.parametrize("B, nr, nt, L, Ns, nblk, hold, t0", GAIN_SHAPES)
def test_gains_against_model(gpu, B, nr, nt, L, Ns, nblk, hold, t0):
    pdp, kf = taps_of(L)
    fd, fd_los = 0.0123, -0.004
    kw = dict(n_sin=Ns, fd_los=fd_los, seed=11, stream_id=3, first_row=2)
    prm = fading_params_batch(B, nr, nt, L, fd, **kw)
    G = fading_gains_batch(B, nr, nt, pdp, fd, nblk, hold=hold, t0=t0, k_factor=kf, **kw)
    assert G.shape == (B, nblk, nr, nt, L) and G.dtype == np.complex128
    taus = M.block_times(t0, hold, nblk)
    want = M.gains_from_params(prm, pdp, kf, taus)
    bound = M.gain_bound(pdp, kf, Ns, fd, fd_los, taus, M.FADING_SINCOS_ULP)[None, :, None, None, :]
    err = np.maximum(np.abs(G.real - want.real), np.abs(G.imag - want.imag))
    print("fading gains", (B, nr, nt, L, Ns, nblk, hold, t0), "largest share of the bound: %.3f" % np.max(err / np.where(bound > 0, bound, np.inf)))
    assert np.all(err <= bound)
    if L >= 3:                                                                   # a tap without power: exact +0
        z = G[..., L // 2]
        assert np.all(z == 0) and not np.any(np.signbit(z.real) | np.signbit(z.imag))
    # the whole model, from its own draws: the deviation of nu, amplified by tau, on top
    full = M.gains(B, nr, nt, pdp, fd, nblk, hold, t0, Ns, kf, fd_los, 11, 3, 2)
    a, c, _ = M.tap_scales(pdp, kf, Ns)
    slack = 2 * np.pi * (M.FADING_ULP + 1) * R.ULP * fd * taus[None, :, None, None, None] * (a * Ns)
    assert np.all(np.abs(G - full) <= np.sqrt(2) * (bound + slack) + 1e-300)


# ---- 3. purity ------------------------------------------------------------------------------------------------------------------------
def test_gains_are_pure(gpu, user_stream):
    pdp, kf = taps_of(6)
    nr, nt, hold = 2, 3, 7
    kw = dict(hold=hold, n_sin=9, k_factor=kf, fd_los=0.02, seed=21, stream_id=4)
    all_rows = fading_gains_batch(8, nr, nt, pdp, 0.03, 10, **kw)
    assert same_bits(all_rows[5:8], fading_gains_batch(3, nr, nt, pdp, 0.03, 10, first_row=5, **kw))
    assert same_bits(all_rows[:, 4:10], fading_gains_batch(8, nr, nt, pdp, 0.03, 6, t0=4 * hold, **kw))
    # the forms: host, device on a user stream, and the channel's own G
    d_G = on_stream(lambda: fading_gains_dev(8, nr, nt, pdp, 0.03, 10, stream=user_stream, **kw), user_stream)
    assert same_bits(d_G.to_array(all_rows.shape, np.complex128), all_rows)
    n = 10 * hold - 6 + 1                                                       # n + L - 1 = 10 blocks
    x = cplx(np.random.RandomState(0), 8, nt, n)
    y, G = fading_multipath_batch(x, nr, pdp, 0.03, want=('y', 'g'), **kw)
    assert same_bits(G, all_rows)
    assert same_bits(y, fading_convolve_batch(x, all_rows, hold))
    d_x = DeviceBuf.from_array(x)
    d_y, d_G2 = on_stream(lambda: fading_channel_dev(d_x, 8, nt, nr, n, pdp, 0.03, want=('y', 'g'), stream=user_stream, **kw), user_stream)
    assert same_bits(d_G2.to_array(all_rows.shape, np.complex128), all_rows) and same_bits(d_y.to_array(y.shape, np.complex128), y)
    (G_only,) = fading_multipath_batch(x, nr, pdp, 0.03, want=('g',), **kw)
    assert same_bits(G_only, all_rows)
    # other keys draw other channels
    for other in (dict(seed=22), dict(stream_id=5)):
        diff = fading_gains_batch(8, nr, nt, pdp, 0.03, 10, **{**kw, **other})
        assert not np.any((diff == all_rows) & (all_rows != 0))
    # the params agree between their forms too
    p_host = fading_params_batch(4, nr, nt, 6, 0.03, n_sin=9, fd_los=0.02, seed=21, stream_id=4, first_row=3)
    d_p = on_stream(lambda: fading_params_dev(4, nr, nt, 6, 0.03, n_sin=9, fd_los=0.02, seed=21, stream_id=4, first_row=3, stream=user_stream),
                    user_stream)
    assert same_bits(d_p.to_array(p_host.shape, np.float64), p_host)
    assert same_bits(p_host[2:], fading_params_batch(2, nr, nt, 6, 0.03, n_sin=9, fd_los=0.02, seed=21, stream_id=4, first_row=5))


def test_gains_workgroup_wrap(gpu):
    """70 001 rows of one block with L = 1, Ns = 1 (rows far past a 16-bit grid), then the shape whose workgroup tiles outnumber the grid."""
    B, pdp = 70001, np.ones(1)
    G = fading_gains_batch(B, 1, 1, pdp, 0.1, 1, t0=77, n_sin=1, seed=2, stream_id=9)
    tail = fading_gains_batch(B - 65530, 1, 1, pdp, 0.1, 1, t0=77, n_sin=1, seed=2, stream_id=9, first_row=65530)
    assert same_bits(G[65530:], tail)
    prm = fading_params_batch(B, 1, 1, 1, 0.1, n_sin=1, seed=2, stream_id=9)
    want = M.gains_from_params(prm, pdp, None, [77])
    bound = M.gain_bound(pdp, None, 1, 0.1, 0.0, [77], M.FADING_SINCOS_ULP)[0, 0]
    assert np.all(np.maximum(np.abs(G.real - want.real), np.abs(G.imag - want.imag)) <= bound)
    # a workgroup takes up to 256 consecutive paths, across rows: the shape above is 274 workgroup tiles.  With Ns = 256 a group holds 7
    # paths, so 70 001 rows of 7 paths are 70 001 tiles: the grid of 65 535 wraps
    pdp = np.full(7, 1.0 / 7)
    kw = dict(t0=5, n_sin=256, seed=2, stream_id=9)
    G = fading_gains_batch(B, 1, 1, pdp, 0.1, 1, **kw)
    assert same_bits(G[65530:], fading_gains_batch(B - 65530, 1, 1, pdp, 0.1, 1, first_row=65530, **kw))
    prm = fading_params_batch(40, 1, 1, 7, 0.1, n_sin=256, seed=2, stream_id=9, first_row=B - 40)
    want = M.gains_from_params(prm, pdp, None, [5])
    bound = M.gain_bound(pdp, None, 256, 0.1, 0.0, [5], M.FADING_SINCOS_ULP)[0]
    assert np.all(np.maximum(np.abs(G[B - 40:].real - want.real), np.abs(G[B - 40:].imag - want.imag)) <= bound)


# ---- 4. / 5. the convolution ----------------------------------------------------------------------------------------------------------
CONV_SHAPES = [(1, 1, 1, 1, 1), (2, 2, 3, 1000, 17), (1, 1, 5, 700, 3), (2, 4, 4, 1500, 16), (1, 1, 1, 2100, 600)]
CONV_HOLDS = [1, 3, 4, 80, 81, 1000, 1024, 1025, "n+L"]          # the issue's, and 81: threads that straddle a block edge in the tiled kernel
G_LIMIT = 64 * 10 ** 6                                           # combinations whose G is larger are dropped (none of these is)
CONV_CASES = [(B, nt, nr, n, L, n + L if h == "n+L" else h) for (B, nt, nr, n, L) in CONV_SHAPES for h in CONV_HOLDS]
CONV_CASES = [c for c in CONV_CASES if c[0] * -(-(c[3] + c[4] - 1) // c[5]) * c[2] * c[1] * c[4] * 16 <= G_LIMIT]


def conv_case(B, nt, nr, n, L, hold):
    nblk = -(-(n + L - 1) // hold)
    rs = np.random.RandomState(B * 1000 + n + L + hold)
    return nblk, cplx(rs, B, nt, n), cplx(rs, B, nblk, nr, nt, L)


@pytest.mark.parametrize("B, nt, nr, n, L, hold", CONV_CASES)
def test_convolve_against_model(gpu, B, nt, nr, n, L, hold):
    nblk, x, G = conv_case(B, nt, nr, n, L, hold)
    for g in (G, G[0]):                                                          # batched, then shared by all rows
        got = fading_convolve_batch(x, g, hold)
        kernel = _lib.last_kernel()
        assert kernel == M.conv_kernel(B, nt, nr, n, L, hold)
        assert got.shape == (B, nr, n + L - 1) and got.dtype == np.complex128
        err, bound = np.abs(got - M.convolve(x, g, hold)), M.convolve_bound(x, g, hold)
        print("fading convolve", (B, nt, nr, n, L, hold), "batched" if g.ndim == 5 else "shared", kernel,
              "largest share of the bound: %.3f" % np.max(err / bound))
        assert np.all(err <= bound)


@pytest.mark.parametrize("B, nt, nr, n, L, hold", CONV_CASES)
def test_convolve_static_equivalence(gpu, B, nt, nr, n, L, hold):
    """Gains that do not change from block to block: cpx_multipath, bit for bit."""
    nblk, x, G = conv_case(B, nt, nr, n, L, hold)
    for g in (G, G[0]):
        static = multipath_batch(x, g[..., 0, :, :, :])
        assert same_bits(fading_convolve_batch(x, np.repeat(g[..., :1, :, :, :], nblk, axis=-4), hold), static)


@pytest.mark.parametrize("hold", [1, 80, 5000])
def test_channel_without_doppler_is_static(gpu, hold):
    rs = np.random.RandomState(4)
    pdp, kf = taps_of(8)
    x = cplx(rs, 3, 2, 1200)
    y, G = fading_multipath_batch(x, 3, pdp, 0.0, hold=hold, t0=99, n_sin=12, k_factor=kf, seed=6, want=('y', 'g'))
    assert np.all(G == G[:, :1]) and np.any(G != 0)
    assert same_bits(y, multipath_batch(x, G[:, 0]))
    xs = x[:, 0]
    ys, Gs = fading_multipath_batch(xs, 1, pdp, 0.0, hold=hold, seed=6, want=('y', 'g'))
    assert ys.shape == (3, 1207) and same_bits(ys, multipath_batch(xs, Gs[:, 0, 0, 0]))
    assert same_bits(ys, fading_convolve_batch(xs, Gs[:, :, 0, 0], hold))


# ---- 6. isolation and invariance ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nt, nr, n, L, hold", [(2, 3, 1000, 17, 1024), (2, 2, 300, 9, 50), (2, 2, 600, 9, 50), (1, 4, 1500, 16, 81)])   # tiled<4>, direct, tiled<2> with 13 sets, tiled<4> with 14
def test_convolve_isolation_and_invariance(gpu, user_stream, nt, nr, n, L, hold):
    rs = np.random.RandomState(7)
    nblk = -(-(n + L - 1) // hold)
    x, G = cplx(rs, 5, nt, n), cplx(rs, 5, nblk, nr, nt, L)
    whole = fading_convolve_batch(x, G, hold)
    assert _lib.last_kernel() == M.conv_kernel(5, nt, nr, n, L, hold)
    assert np.all(np.abs(whole - M.convolve(x, G, hold)) <= M.convolve_bound(x, G, hold))
    alone = fading_convolve_batch(x[3:4], G[3:4], hold)[0]
    assert same_bits(whole[3], alone)
    order = [3, 0, 1, 2, 4]
    assert same_bits(fading_convolve_batch(x[order], G[order], hold)[0], alone)
    assert same_bits(fading_convolve_batch(x, G[3], hold)[3], alone)                # shared against replicated
    d_x, d_G = DeviceBuf.from_array(x), DeviceBuf.from_array(G)
    d_y = on_stream(lambda: fading_convolve_dev(d_x, d_G, 1, 5, nt, nr, n, L, hold, stream=user_stream), user_stream)
    assert same_bits(d_y.to_array(whole.shape, np.complex128), whole)
    bad = x.copy()
    bad[1, nt - 1, n // 2] = np.nan
    out = fading_convolve_batch(bad, G, hold)
    assert np.any(np.isnan(out[1])) and not np.any(np.isnan(out[[0, 2, 3, 4]]))
    assert same_bits(out[[0, 2, 3, 4]], whole[[0, 2, 3, 4]])


# ---- 7. chunking ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B, L, n", [(2, 128, FADING_SCRATCH_BYTES // (2048 * 16) + 300),      # one row's gains above the budget
                                     (7, 16, 5000)])                                           # three rows per chunk
def test_channel_chunks_change_nothing(gpu, B, L, n):
    nr = nt = 4
    hold, Ns = 1, 4
    nblk = n + L - 1
    row_bytes = nblk * nr * nt * L * 16
    assert (row_bytes > FADING_SCRATCH_BYTES) == (L == 128) and B * row_bytes > FADING_SCRATCH_BYTES
    pdp = np.exp(-0.05 * np.arange(L))
    kw = dict(hold=hold, t0=31, n_sin=Ns, seed=8, stream_id=1, first_row=9)
    d_x = DeviceBuf.from_array(cplx(np.random.RandomState(1), B, nt, n))
    d_y = fading_channel_dev(d_x, B, nt, nr, n, pdp, 0.02, **kw)
    kernel = _lib.last_kernel()
    y = d_y.to_array((B, nr, nblk), np.complex128)
    chunks = B * -(-row_bytes // FADING_SCRATCH_BYTES) if L == 128 else -(-B // (FADING_SCRATCH_BYTES // row_bytes))
    assert kernel == "fading_gains_kernel+fading_direct_kernel (%d chunks)" % chunks
    d_G = fading_gains_dev(B, nr, nt, pdp, 0.02, nblk, **kw)
    d_ref = fading_convolve_dev(d_x, d_G, 1, B, nt, nr, n, L, hold)
    assert same_bits(y, d_ref.to_array(y.shape, np.complex128))
    assert np.all(np.isfinite(y.view(np.float64))) and np.any(y != 0)


# ---- 8. statistics --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed, stream", [(0, 0), (7, 1)])
def test_device_statistics(gpu, seed, stream):
    B, L, Ns, fd, t0 = 1024, 16, 16, 0.01, 1000
    pdp = np.full(L, 1.0 / L)
    tol = 6 / np.sqrt(B * L)
    G = fading_gains_batch(B, 1, 1, pdp, fd, 201, hold=1, t0=t0, n_sin=Ns, seed=seed, stream_id=stream)
    for d in M.STAT_DELTAS:
        ac = M.autocorrelation(G[:, 0], G[:, d], pdp)
        assert abs(ac - j0(2 * np.pi * fd * d)) <= tol, (d, ac)
    assert abs(np.mean(np.abs(G[:, 0]) ** 2 / pdp) - 1) <= tol


# ---- 9. end to end --------------------------------------------------------------------------------------------------------------------
E2E = {"qam16_1x1": (16, 1, 1, 64, 52, 16), "qam16_2x2": (16, 2, 2, 64, 52, 16), "qam64_2x3": (64, 2, 3, 256, 200, 32)}
E2E_SEEDS = [1, 2, 3]


def e2e_run(case, seed, fd):
    """(sent symbols [B, nsym, nsc, nt], Y [B, nsym, nsc, nr], device G, model G, modem) of one noise-free frame per row."""
    m, nt, nr, nfft, nsc, cp = E2E[case]
    B, nsym, L, Ns = 3, 6, 8, 16
    hold = nfft + cp
    pdp = np.exp(-0.5 * np.arange(L))
    pdp /= pdp.sum()
    md = QAMModem(m)
    idx = np.random.RandomState(seed).randint(0, m, size=(B, nt, nsym, nsc))
    tx = ofdm_tx_batch(md.constellation[idx].reshape(B * nt, nsym, nsc), nfft, cp).reshape(B, nt, nsym * hold)
    y, G = fading_multipath_batch(tx, nr, pdp, fd, hold=hold, n_sin=Ns, seed=seed, stream_id=17, want=('y', 'g'))
    Y = ofdm_rx_batch(y.reshape(B * nr, -1), nfft, nsc, cp).reshape(B, nr, nsym, nsc)
    Gm = M.gains(B, nr, nt, pdp, fd, G.shape[1], hold, 0, Ns, None, 0.0, seed, 17)
    sent = md.constellation[idx].transpose(0, 2, 3, 1)
    return sent, Y.transpose(0, 2, 3, 1), G[:, :nsym], Gm[:, :nsym], md


def zf(Y, H, md):
    nr, nt = H.shape[-2:]
    return linear_batch(Y.reshape(-1, nr), np.ascontiguousarray(H).reshape(-1, nr, nt), md, 0, method='zf', output_type='hard').reshape(Y.shape[:3] + (nt,))


@pytest.mark.parametrize("seed", E2E_SEEDS)
@pytest.mark.parametrize("case", sorted(E2E))
def test_end_to_end_noise_free(gpu, case, seed):
    """ofdm_tx -> fading channel (one block per OFDM symbol) -> ofdm_rx -> perfect CSI per symbol -> ZF: every index is detected."""
    nfft, nsc = E2E[case][3:5]
    sent, Y, G, Gm, md = e2e_run(case, seed, 0.002)
    Hm = tap_frequency_response(Gm, nfft, nsc).transpose(0, 1, 4, 2, 3)           # the MODEL's H [B, nsym, nsc, nr, nt]
    kappa = float(np.max(np.linalg.cond(Hm)))
    print("fading end to end", case, seed, "largest condition number of the model's H: %.3g" % kappa)
    assert kappa < 1e6                                                          # the seeds were chosen for this, on the CPU
    H = tap_frequency_response(G, nfft, nsc).transpose(0, 1, 4, 2, 3)
    assert np.max(np.abs(H - Hm)) <= 1e-9
    wrong = int(np.count_nonzero(zf(Y, H, md) != sent))
    assert wrong == 0


@pytest.mark.parametrize("case", sorted(E2E))
def test_end_to_end_channel_moves(gpu, case):
    """fd ten times larger and the channel state of the frame's FIRST symbol for the whole frame: there are errors."""
    nfft, nsc = E2E[case][3:5]
    sent, Y, G, _, md = e2e_run(case, E2E_SEEDS[0], 0.02)
    H = tap_frequency_response(G, nfft, nsc).transpose(0, 1, 4, 2, 3)
    assert int(np.count_nonzero(zf(Y, H, md) != sent)) == 0                       # per-symbol CSI still detects everything
    stale = np.broadcast_to(H[:, :1], H.shape)
    wrong = int(np.count_nonzero(zf(Y, stale, md) != sent))
    print("fading end to end", case, "per-frame CSI at fd = 0.02: %d of %d wrong" % (wrong, sent.size))
    assert wrong >= 1
