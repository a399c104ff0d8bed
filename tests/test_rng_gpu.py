"""The random stages on the device against tests/rng_model.py: the kernels that draw from csrc/cpx_rng.h (random_bits_kernel,
binary_channel_kernel, awgn_kernel, mimo_channel_kernel, link_front_kernel) compute the exactly specified function of
(seed, stream id, element index) that include/commpy_amd.h documents.  The integer stages are equalities; the Gaussian stage is held
to the ulp bound below.  No statistics here: the distribution of the contract is tested on the host model
(tests/test_rng_model_host.py).

The AWGN bound (rng_model.AWGN_ULP).  No accuracy table of the HIP math functions ships with the toolkit, so the bound is the
measured one: the largest deviation between ``cpx_awgn_dev`` and the mpmath-validated model on zeros, in ulps of the noise term
(relative: 2^-52 |term|), over the 2^21 + 5 draws of each of the four (seed, stream) pairs was 2.84 ulp
(rng_model.AWGN_ULP_MEASURED).  The tests assert twice that, 5.68 ulp, per component as ``AWGN_ULP 2^-52 |scale n|`` plus
``2^-53 |y|`` for the kernel's final add, and in any case less than the cap of 16 ulp (another algorithm; a float32 intermediate
would be near 2^29 ulp).  The model itself is within 2 ulp of
the 50-digit value."""
import functools
import math

import numpy as np
import pytest

import rng_model as R
from commpy_amd import _lib
from commpy_amd.devicelink import DeviceBuf

pytestmark = pytest.mark.gpu

GUARD = 64
FILL = 0xA5


def _sync():
    _lib.check(_lib.load().cpx_stream_sync(None))


def _guarded(nbytes):
    """A device buffer of ``nbytes`` + GUARD pre-filled bytes."""
    return DeviceBuf.from_array(np.full(nbytes + GUARD, FILL, np.uint8))


def _payload(buf, n, dtype):
    """The first ``n`` items of a guarded buffer, after checking that the guard behind them is untouched."""
    raw = buf.to_array((n * np.dtype(dtype).itemsize + GUARD,), np.uint8)
    assert np.all(raw[-GUARD:] == FILL), "wrote past the end"
    return raw[:-GUARD].view(dtype)


@functools.lru_cache(maxsize=8)
def _polar(n, key, first=0):
    """(rad, cos, sin) of the model for counters first .. first + n - 1 of ``key`` = (seed, stream): computed once per module."""
    out = R.box_muller(*R.gauss_uniforms(R.counters(first, n), *key))
    for a in out:
        a.setflags(write=False)
    return out


def _model_noise(n, key, scale_re, scale_im):
    rad, cs, sn = _polar(n, key)
    return (scale_re * rad) * cs + 1j * ((scale_im * rad) * sn)


def _within_bound(y, x, noise):
    assert R.AWGN_ULP_MEASURED <= R.AWGN_ULP <= R.AWGN_ULP_CAP
    excess = R.awgn_excess(y, x, noise, R.AWGN_ULP)
    assert np.all(excess <= 0.0), (float(excess.max()), np.unravel_index(int(np.argmax(excess)), excess.shape))


# ---- message bits --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 15, 16, 17, 4095, 65537, 2 ** 25 + 17])
def test_random_bits_equal_the_model(gpu, n):
    """2^25 + 17 is one past the grid cap (8192 blocks x 256 lanes x 16 bits): the grid-stride second pass and a ragged last counter."""
    lib = _lib.load()
    for seed, stream in R.KEYS:
        buf = _guarded(n)
        _lib.check(lib.cpx_random_bits_dev(buf.ptr, n, seed, stream, None))
        _sync()
        got = _payload(buf, n, np.uint8)
        assert np.array_equal(got, R.message_bits(n, seed, stream)), (seed, stream)
        buf.free()


# ---- binary channels -----------------------------------------------------------------------------------------------------------

def _binary(which, d_bits, n, p, seed, stream, want_i8, want_f64):
    """One launch of cpx_bsc_dev / cpx_bec_dev with the chosen outputs -> (int8 or None, float64 or None), guards checked."""
    lib = _lib.load()
    b_i8 = _guarded(n) if want_i8 else None
    b_f = _guarded(8 * n) if want_f64 else None
    _lib.check(getattr(lib, which)(d_bits.ptr, n, p, seed, stream, b_i8.ptr if b_i8 else None, b_f.ptr if b_f else None, None))
    _sync()
    out = (_payload(b_i8, n, np.int8) if b_i8 else None, _payload(b_f, n, np.float64) if b_f else None)
    for b in (b_i8, b_f):
        if b:
            b.free()
    return out


@pytest.mark.parametrize("n", [1, 2, 3, 511, 512, 513, 2 ** 22 + 3])
def test_bsc_bec_equal_the_model(gpu, n):
    """2^22 + 3: the grid wrap at two draws per counter, with an odd n.  Below it every output combination of both channels runs for
    every (p, seed, stream); at it, per (p, seed, stream): the BSC's int8 alone, its float64 alone, and the BEC with both."""
    bits = np.random.RandomState(n % 1000).randint(0, 2, n).astype(np.uint8)
    d_bits = DeviceBuf.from_array(bits)
    small = n < 2 ** 20
    for seed, stream in R.KEYS:
        m = R.binary_draws(n, seed, stream)
        for p in (0.0, 0.05, 0.5, 1.0):
            hits = (m - np.uint64(1)).astype(np.float64) <= p * R.TWO53
            assert np.array_equal(hits, R.binary_hits(n, p, seed, stream)) if small else True
            flipped = (bits ^ hits).astype(np.int8)
            erased = np.where(hits, -1, bits).astype(np.int8)
            plan = [("cpx_bsc_dev", flipped, True, False), ("cpx_bsc_dev", flipped, False, True), ("cpx_bec_dev", erased, True, True)]
            if small:
                plan += [("cpx_bsc_dev", flipped, True, True), ("cpx_bec_dev", erased, True, False), ("cpx_bec_dev", erased, False, True)]
            for which, want, i8, f64 in plan:
                got_i8, got_f = _binary(which, d_bits, n, p, seed, stream, i8, f64)
                if i8:
                    assert np.array_equal(got_i8, want), (which, p, seed, stream)
                if f64:
                    assert np.array_equal(got_f, want.astype(np.float64)), (which, p, seed, stream)
            # the BEC erases exactly where the BSC flips
            assert np.array_equal(erased == -1, flipped != bits.astype(np.int8))
    d_bits.free()


@pytest.mark.parametrize("k", [4, 5, 512])
def test_binary_channel_threshold_is_inclusive(gpu, k):
    """p equal to the draw of position k hits it (`<=`); the next float64 towards 0 does not.  A strict `<` fails the first, a draw
    without the 2^-53 shift onto [0, 1) fails it too."""
    n, (seed, stream) = 513, R.KEYS[2]
    m = R.binary_draws(n, seed, stream)
    u_k = float(int(m[k]) - 1) / R.TWO53
    assert 0.0 < u_k < 1.0
    bits = np.zeros(n, np.uint8)
    d_bits = DeviceBuf.from_array(bits)
    for which in ("cpx_bsc_dev", "cpx_bec_dev"):
        at = _binary(which, d_bits, n, u_k, seed, stream, True, False)[0] != 0
        below = _binary(which, d_bits, n, float(np.nextafter(u_k, 0.0)), seed, stream, True, False)[0] != 0
        assert at[k] and not below[k]
        assert np.array_equal(at, R.binary_hits(n, u_k, seed, stream))
        assert np.array_equal(below, R.binary_hits(n, float(np.nextafter(u_k, 0.0)), seed, stream))
    d_bits.free()


# ---- AWGN ----------------------------------------------------------------------------------------------------------------------

def _awgn_dev(x, scale_re, scale_im, seed, stream, in_place=False):
    lib = _lib.load()
    n = x.size
    d_x = DeviceBuf.from_array(np.concatenate([x.view(np.uint8), np.full(GUARD, FILL, np.uint8)])) if in_place else DeviceBuf.from_array(x)
    d_y = d_x if in_place else _guarded(16 * n)
    _lib.check(lib.cpx_awgn_dev(d_x.ptr, n, scale_re, scale_im, seed, stream, d_y.ptr, None))
    _sync()
    y = _payload(d_y, n, np.complex128)
    d_x.free()
    d_y.free()
    return y


def _check_awgn(n, key, rs):
    seed, stream = key
    zero = np.zeros(n, np.complex128)
    x = np.exp(2j * math.pi * rs.rand(n)) * (0.5 + rs.rand(n))          # magnitude about 1
    worst = 0.0
    for xin in (zero, x):
        for s_re, s_im in ((2.0, 0.5), (0.0, 0.5), (2.0, 0.0)):
            noise = _model_noise(n, key, s_re, s_im)
            y = _awgn_dev(xin, s_re, s_im, seed, stream)
            _within_bound(y, xin, noise)
            if s_re == 0.0:
                assert np.array_equal(y.real.view(np.uint64), xin.real.copy().view(np.uint64))      # untouched, bit for bit
            if s_im == 0.0:
                assert np.array_equal(y.imag.view(np.uint64), xin.imag.copy().view(np.uint64))
            y2 = _awgn_dev(xin, s_re, s_im, seed, stream, in_place=True)
            assert np.array_equal(y2.view(np.uint64), y.view(np.uint64))
            if xin is zero and (s_re, s_im) == (2.0, 0.5):
                worst = R.ulp_deviation(y, noise)
    return worst


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_awgn_equals_the_model(gpu, n):
    rs = np.random.RandomState(n)
    for key in R.KEYS:
        _check_awgn(n, key, rs)


@pytest.mark.parametrize("key", R.KEYS)
def test_awgn_grid_wrap_and_far_tail(gpu, key):
    """2^21 + 5 elements: past the grid cap of 8192 blocks x 256 lanes.  The deviation printed here, over the four keys, is what
    rng_model.AWGN_ULP_MEASURED records.  The element with the model's largest |n| (beyond 5 sigma in 2 10^6 draws) is asserted on
    its own: the tail is what a uniform of fewer than 53 bits changes."""
    n = 2 ** 21 + 5
    worst = _check_awgn(n, key, np.random.RandomState(11))
    print("cpx_awgn_dev vs model, key %r: max deviation %.3f ulp of the noise term (asserted %.3f)" % (key, worst, R.AWGN_ULP))
    assert worst <= R.AWGN_ULP
    rad, cs, sn = _polar(n, key)
    far = int(np.argmax(rad))
    assert rad[far] > 5.0
    y = _awgn_dev(np.zeros(n, np.complex128), 1.0, 1.0, *key)
    for got, want in ((y.real[far], rad[far] * cs[far]), (y.imag[far], rad[far] * sn[far])):
        assert abs(got - want) <= R.AWGN_ULP * R.ULP * abs(want), (far, got, want)
    assert abs(abs(y[far]) - rad[far]) <= R.AWGN_ULP * R.ULP * rad[far]


# ---- the MIMO channel: a counter with a high word ------------------------------------------------------------------------------------

def test_mimo_channel_counter_high_word(gpu):
    """first_vector = 2^33 + 5 puts a non-zero high word into the counters of the fading (gv nr nt + r nt + a) and of the noise
    (gv nr + r); V = 70 is past one 64-lane wave."""
    from commpy_amd.channels import MIMOFlatChannel
    from commpy_amd.devicelink import _channel_handles
    from commpy_amd.modulation import QAMModem
    from test_mimo_link_gpu import _host_hx
    lib, md = _lib.load(), QAMModem(4)
    nr, nt, V, scale = 2, 3, 70, 0.3
    seed, s_fade, s_noise = 2 ** 32 + 3, 2 ** 32 + 5, 6
    ch = MIMOFlatChannel(nt, nr)
    ch.uncorr_rayleigh_fading(complex)
    hs = _channel_handles(ch)
    bits = np.random.RandomState(8).randint(0, 2, V * nt * 2).astype(np.uint8)
    d_bits = DeviceBuf.from_array(bits)

    def run(first):
        d_y, d_h = _guarded(V * nr * 16), _guarded(V * nr * nt * 16)
        _lib.check(lib.cpx_mimo_channel_run_dev(hs.get(), md._device_handle(), d_bits.ptr, V, first, scale, seed, s_fade, s_noise,
                                                d_y.ptr, d_h.ptr, None))
        _sync()
        out = _payload(d_y, V * nr, np.complex128).reshape(V, nr), _payload(d_h, V * nr * nt, np.complex128).reshape(V, nr, nt)
        d_y.free()
        d_h.free()
        return out

    first = 2 ** 33 + 5
    y, H = run(first)
    _within_bound(H, np.zeros_like(H), R.mimo_fading(first, V, nr, nt, seed, s_fade))
    hx = _host_hx(H, md.modulate(bits).reshape(V, nt))
    _within_bound(y, hx, R.mimo_noise(first, V, nr, seed, s_noise, scale))
    y5, H5 = run(5)
    assert not np.any(H5 == H) and not np.any(y5 == y)
    _within_bound(H5, np.zeros_like(H5), R.mimo_fading(5, V, nr, nt, seed, s_fade))
    hs.drop()
    d_bits.free()


# ---- the links draw the streams their docstrings state ----------------------------------------------------------------------------------

def test_bsc_link_streams(gpu):
    from commpy_amd.devicelink import DeviceBscLink
    from helpers import make_trellis
    seed, B, p = 2 ** 32 + 9, 37, 0.05
    link = DeviceBscLink(make_trellis("t57"), 64, tb_depth=10, seed=seed)
    for c in (1, 2):
        link.run_batch(p, B)
        bufs = link.buffers(B)
        msg = bufs['msg'].to_array((B * 64,), np.uint8)
        coded = bufs['coded'].to_array((B * link.ncoded,), np.uint8)
        rx = bufs['rx'].to_array((B * link.ncoded,), np.float64)
        assert np.array_equal(msg, R.message_bits(B * 64, seed, 2 * c))
        assert np.array_equal(rx != coded, R.binary_hits(B * link.ncoded, p, seed, 2 * c + 1))


@pytest.mark.parametrize("fused", [True, False])
def test_wifi_link_streams(gpu, fused):
    from commpy_amd.channelcoding import conv_encode_batch
    from commpy_amd.channelcoding.convcode import puncture_keep_mask
    from commpy_amd.devicelink import DeviceWifiLink
    seed, T, snr = 17, 5, 12.0
    link = DeviceWifiLink(4, 600, generator_matrix=[[0o133, 0o171]], seed=seed, fused=fused)       # 16-QAM, rate 3/4: punctured
    link.keep_rx = True
    assert (link._front is not None) == fused, link.front_reason
    pvec = link.wifi._get_puncture_matrix(*link.coding)
    assert pvec is not None
    s = link.noise_std(snr) * 0.5
    for c in (1, 2):
        link.run_batch(snr, T)
        assert ("link_front_kernel" in link.front_last_kernel) == fused
        msg = link._bufs['msg'].to_array((T, link.nbits), np.uint8)
        rx = link._bufs['rx'].to_array((T * link.nsym,), np.complex128)
        assert np.array_equal(msg.reshape(-1), R.message_bits(T * link.nbits, seed, 2 * c))
        coded = conv_encode_batch(msg, link.trellis, 'cont')
        coded = coded[:, puncture_keep_mask(coded.shape[1], pvec)]
        sym = link.modem.modulate(coded.reshape(-1))
        assert sym.shape == rx.shape
        _within_bound(rx, sym, R.noise_terms(rx.size, s, s, seed, 2 * c + 1))


def test_mimo_link_streams(gpu):
    from commpy_amd.channels import MIMOFlatChannel
    from commpy_amd.devicelink import DeviceMimoLink
    from commpy_amd.modulation import QAMModem
    from test_mimo_link_gpu import _host_hx
    ch = MIMOFlatChannel(4, 4)
    ch.uncorr_rayleigh_fading(complex)
    ch.noise_std = 0.0
    md, seed, T = QAMModem(16), 5, 7
    link = DeviceMimoLink(md, ch, detector='kbest', seed=seed)
    link.keep_rx = True
    for c in (1, 2):
        link.run_batch(12.0, T)
        rx = link.last_rx
        V = T * link.vectors_per_tx
        assert np.array_equal(rx['msg'].reshape(-1), R.message_bits(T * link.send_chunk, seed, 3 * c))
        _within_bound(rx['h'], np.zeros_like(rx['h']), R.mimo_fading(0, V, 4, 4, seed, 3 * c + 1))
        hx = _host_hx(rx['h'], md.modulate(rx['msg'].reshape(-1)).reshape(V, 4))
        _within_bound(rx['y'], hx, R.mimo_noise(0, V, 4, seed, 3 * c + 2, rx['noise_std'] * 0.5))
