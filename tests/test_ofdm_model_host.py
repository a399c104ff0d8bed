"""The extended-precision OFDM model (ofdm_model.py) checked on its own, and its bounds checked on numpy.fft (CPU only).

The last three tests run the bounds the GPU tests assert over the suite's float64 model: an implementation known to be good has
to pass them, with the inputs the GPU tests use, before they say anything about a kernel."""
import numpy as np
import pytest

import ofdm_model as om
from ofdm_model import CLD, EPS_LD, LD, U
from test_ofdm_host import model_rx, model_rx_batch, model_tx, model_tx_batch

pytestmark = om.requires_longdouble


def cplx(rs, *shape):
    return rs.randn(*shape) + 1j * rs.randn(*shape)


def test_twiddles_are_exact_on_the_axes_and_symmetric():
    for N in (2, 3, 8, 12, 100, 4096):
        w = om.twiddles_ld(N)
        assert w.dtype == CLD and w[0] == 1
        if N % 4 == 0:
            assert w[N // 4] == -1j and w[N // 2] == -1 and w[3 * N // 4] == 1j
        assert float(np.max(np.abs(w[1:] - np.conj(w[1:][::-1])))) <= 2 * EPS_LD      # W^(N - k) = conj(W^k)
        assert float(np.max(np.abs(np.abs(w) - 1))) <= 2 * EPS_LD
    w = om.twiddles_ld(12)
    assert abs(w[1].real - np.sqrt(LD(3)) / 2) <= EPS_LD and abs(w[1].imag + LD(1) / 2) <= EPS_LD
    assert abs(w[2].real - LD(1) / 2) <= EPS_LD


@pytest.mark.parametrize("N", [2, 8, 64, 256])
def test_fft_ld_equals_dft_ld(N):
    rs = np.random.RandomState(N)
    x = cplx(rs, 3, N)
    for inverse in (False, True):
        a, b = om.fft_ld(x, inverse), om.dft_ld(x, inverse=inverse)
        assert a.dtype == CLD and b.dtype == CLD and a.shape == b.shape == (3, N)
        l1 = np.sum(np.abs(x), axis=-1, keepdims=True) / (N if inverse else 1)
        assert np.all(np.abs(a - b) <= 64 * EPS_LD * l1), float(np.max(np.abs(a - b) / l1)) / EPS_LD
    # a subset of bins is those bins; a sparse input takes the other loop and gives the same
    bins = np.arange(0, N, 3)
    assert np.array_equal(om.dft_ld(x, bins), om.dft_ld(x)[:, bins])
    xs = np.zeros((2, N), complex)
    xs[0, N - 1], xs[1, 0] = 1 - 2j, 3j
    want = np.stack([(1 - 2j) * om.twiddles_ld(N)[(np.arange(N) * (N - 1)) % N], np.full(N, 3j, CLD)])
    assert np.array_equal(om.dft_ld(xs), want)
    assert float(np.max(np.abs(om.fft_ld(xs) - want))) <= 64 * EPS_LD * 3


def test_ref_single_tone():
    nfft, nsc, cp = 16, 8, 4
    h = nsc // 2
    n = np.arange(nfft)
    for sc in range(nsc):
        x = np.zeros((1, 1, nsc), complex)
        x[0, 0, sc] = 1.0
        k = sc - h + 1 if sc >= h else nfft - h + sc                   # the bin that carries subcarrier sc
        tone = np.conj(om.twiddles_ld(nfft))[(k * n) % nfft] / nfft
        got = om.ref_tx_batch(x, nfft, cp)
        assert got.shape == (1, cp + nfft) and got.dtype == CLD
        assert float(np.max(np.abs(got[0, cp:] - tone))) <= 8 * EPS_LD
        assert np.array_equal(got[0, :cp], got[0, nfft:])
        back = om.ref_rx_batch(got.astype(complex), nfft, nsc, cp)
        assert back.shape == (1, 1, nsc)
        assert float(np.max(np.abs(back[0, 0] - x[0, 0]))) <= 1e-15   # the tone went through float64 on its way back
        some = om.ref_tx_batch(x, nfft, cp, samples=[0, 5])
        assert some.shape == (1, 1, 2) and float(np.max(np.abs(some[0, 0] - got[0, [cp, cp + 5]]))) <= 8 * EPS_LD


def test_ref_second_write_wins():
    nfft = 8
    x = (np.arange(nfft) + 1.0).reshape(1, 1, nfft)
    F = om.fft_ld(om.ref_tx_batch(x, nfft, 2)[0, 2:])
    assert float(np.max(np.abs(F - np.array([0, 5, 6, 7, 1, 2, 3, 4])))) <= 64 * EPS_LD * 8
    nsc = 2 * (nfft - 1)
    x = (np.arange(nsc) + 1.0).reshape(1, 1, nsc)
    F = om.fft_ld(om.ref_tx_batch(x, nfft, 2)[0, 2:])
    assert float(np.max(np.abs(F - np.arange(8)))) <= 64 * EPS_LD * 8
    assert np.array_equal(om.tx_bins(x, nfft)[0, 0], [0, 1, 2, 3, 4, 5, 6, 7])
    assert np.array_equal(om.rx_bin_of(nfft, nsc), [1, 2, 3, 4, 5, 6, 7, 1, 2, 3, 4, 5, 6, 7])
    assert np.array_equal(om.rx_bin_of(8, 4), [6, 7, 1, 2])


def test_ref_whole_symbol_prefix_and_leftover():
    rs = np.random.RandomState(1)
    x = cplx(rs, 1, 3, 6)
    for nfft in (8, 12):                                                # fft_ld and dft_ld
        for cp in (0, nfft, nfft + 3):
            got = om.ref_tx_batch(x, nfft, cp).reshape(3, 2 * nfft)
            assert np.array_equal(got[:, :nfft], got[:, nfft:])
        assert om.ref_tx_batch(x, nfft, 3).shape == (1, 3 * (nfft + 3))
        y = cplx(rs, 2, 2 * (nfft + 4) + 7)
        full = om.ref_rx_batch(y, nfft, 6, 4)
        assert full.shape == (2, 2, 6)
        assert np.array_equal(full, om.ref_rx_batch(y[:, :2 * (nfft + 4)], nfft, 6, 4))
        assert om.ref_rx_batch(y[:, :nfft + 3], nfft, 6, 4).shape == (2, 0, 6)
        junk = y.copy()
        junk.reshape(2, -1)[:, 2 * (nfft + 4):] = np.nan               # the leftover and the prefixes are never read
        junk[:, :4] = np.nan
        assert np.array_equal(full, om.ref_rx_batch(junk, nfft, 6, 4))
        some = om.ref_rx_batch(y, nfft, 6, 4, bins=[1, 3])
        assert float(np.max(np.abs(some - om.dft_ld(om.rx_bodies(y, nfft, 4), [1, 3])))) <= 64 * EPS_LD * nfft * 4


@pytest.mark.parametrize("nfft, nsc, cp", [(64, 52, 16), (8, 8, 1), (12, 8, 3), (100, 60, 10)])
def test_ref_agrees_with_the_float64_model(nfft, nsc, cp):
    rs = np.random.RandomState(nfft)
    x = cplx(rs, 2, 3, nsc)
    t = model_tx_batch(x, nfft, cp)
    rt = om.ref_tx_batch(x, nfft, cp)
    assert rt.shape == t.shape
    assert float(np.max(np.abs(rt - t))) <= 1e-14 * float(np.max(np.abs(t)))
    y = np.concatenate([t, cplx(rs, 2, 5)], axis=1)
    r = model_rx_batch(y, nfft, nsc, cp)
    rr = om.ref_rx_batch(y, nfft, nsc, cp)
    assert rr.shape == r.shape
    assert float(np.max(np.abs(rr - r))) <= 1e-14 * float(np.max(np.abs(r)))
    assert np.array_equal(model_tx(x[0].T, nfft, nsc, cp), t[0]) and np.array_equal(model_rx(y[0], nfft, nsc, cp), r[0].T)


def test_pass_structure_and_bound_values():
    assert om.fast_passes(2) == [1] and om.fast_passes(8) == [3] and om.fast_passes(16) == [1, 3]
    assert om.fast_passes(64) == [3, 3] and om.fast_passes(4096) == [3, 3, 3, 3] and om.fast_passes(8192) == [1, 4, 4, 4]
    assert [om.fast_factors(n) for n in (2, 8, 16, 64, 512, 4096, 8192)] == [0, 1, 4, 5, 9, 13, 15]
    s5 = 5 ** 0.5
    assert om.fast_bound(2) == 1 and om.fast_bound(8) == 3 + (1 + s5)
    assert abs(om.fast_bound(8192) - (13 + 6 * (1 + s5) + 9 * (1 + s5))) < 1e-12
    for k in range(1, 14):
        assert om.fast_bound(2 ** k) <= 12 * k
    assert om.sparse_bound(1, 1) == 1 + s5 and om.sparse_bound(3, 1, True) == 1 + s5 + 2 + 2
    assert om.dense_bound(65536) == 65539


@pytest.mark.parametrize("nfft", [2 ** k for k in range(1, 14)])
def test_numpy_fft_is_inside_the_fast_bound(nfft):
    rs = np.random.RandomState(nfft)
    x = cplx(rs, max(2, 4096 // nfft), nfft)
    for inverse in (False, True):
        got = np.fft.ifft(x, axis=-1) if inverse else np.fft.fft(x, axis=-1)
        ref = om.fft_ld(x, inverse)
        err = om.norm2(got - ref) / (LD(U) * om.norm2(ref))
        assert np.all(err <= om.fast_bound(nfft)), (float(np.max(err)), om.fast_bound(nfft))


def dense_check(got, ref, walk, l1, N):
    """Both assertions of (c) over the bins given (last axis, all symbols together); returns the ratio of the second."""
    assert np.all(np.abs(got - ref) <= om.dense_bound(N) * LD(U) * l1)
    e_got = float(np.sqrt(np.sum(om.norm2(got - ref) ** 2)))
    e_walk = float(np.sqrt(np.sum(om.norm2(walk - ref) ** 2)))
    assert e_got <= om.DENSE_RATIO_LIMIT * e_walk, (e_got, e_walk)
    return e_got / e_walk


@pytest.mark.parametrize("N, bins", [(1536, None), (65536, range(0, 65536, 1024))])
def test_numpy_fft_passes_the_dense_dft_checks(N, bins):
    rs = np.random.RandomState(N)
    x = cplx(rs, 1, N)
    bins = np.arange(N) if bins is None else np.asarray(bins)
    assert bins.size >= 64
    l1 = LD(np.sum(np.abs(x)))
    for inverse in (False, True):
        got = (np.fft.ifft(x, axis=-1) if inverse else np.fft.fft(x, axis=-1))[:, bins]
        ref = om.dft_ld(x, bins, inverse)
        walk = om.dft_f64_index_order(x, bins, inverse)
        ratio = dense_check(got, ref, walk, l1 / (N if inverse else 1), N)
        assert ratio < 1                                               # an FFT's error grows with log N, a direct sum's with sqrt N
        # the yardstick is itself a float64 DFT: far inside the rigorous bound, far outside the reference's own error
        assert np.all(np.abs(walk - ref) <= om.dense_bound(N) * LD(U) * l1 / (N if inverse else 1))
        assert float(np.sqrt(np.sum(om.norm2(walk - ref) ** 2))) > 1e3 * EPS_LD * float(np.sqrt(np.sum(om.norm2(ref) ** 2)))
