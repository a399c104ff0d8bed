"""OFDM transmit / receive: argument checks, the C-ABI's names, and this suite's NumPy model of the semantics (CPU only).

The model is the contract of ofdm_tx / ofdm_rx (commpy/modulation.py:265-296) written as a bin-index map plus numpy.fft: with
h = nsc // 2, TX puts x[h:] on bins 1..h and x[:h] on bins nfft-h.. (the second write wins), takes the ifft and prefixes the last P
samples, P = cp if 0 < cp < nfft else nfft; RX takes the fft after cp samples of every block of nfft + cp and reads the same bins
back, the top ones first."""
import os
import re

import numpy as np
import pytest

from commpy_amd import _lib, modulation

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["cpx_ofdm_create", "cpx_ofdm_destroy", "cpx_ofdm_tx", "cpx_ofdm_tx_dev", "cpx_ofdm_rx", "cpx_ofdm_rx_dev"]


def prefix_len(nfft, cp):
    return cp if 0 < cp < nfft else nfft


def bin_map(nfft, nsc):
    """bins[k] = the subcarrier index that bin k carries after both writes of TX, -1 for an empty bin."""
    h = nsc // 2
    bins = np.full(nfft, -1)
    bins[1:h + 1] = np.arange(h, 2 * h)
    bins[nfft - h:] = np.arange(h)
    return bins


def model_tx_batch(x, nfft, cp):
    """x [B, nsym, nsc] -> [B, nsym * (P + nfft)]."""
    x = np.asarray(x, dtype=complex)
    B, nsym, nsc = x.shape
    bins = bin_map(nfft, nsc)
    F = np.zeros((B, nsym, nfft), complex)
    used = bins >= 0
    F[:, :, used] = x[:, :, bins[used]]
    t = np.fft.ifft(F, axis=-1)
    P = prefix_len(nfft, cp)
    return np.concatenate([t[:, :, nfft - P:], t], axis=-1).reshape(B, -1)


def model_rx_batch(y, nfft, nsc, cp):
    """y [B, n] -> [B, n // (nfft + cp), nsc]."""
    y = np.asarray(y, dtype=complex)
    B, n = y.shape
    S = nfft + cp
    nsym = n // S
    X = np.fft.fft(y[:, :nsym * S].reshape(B, nsym, S)[:, :, cp:cp + nfft], axis=-1)
    h = nsc // 2
    return np.concatenate([X[:, :, nfft - h:], X[:, :, 1:h + 1]], axis=-1)


def model_tx(x, nfft, nsc, cp):
    return model_tx_batch(np.asarray(x).T[None], nfft, cp)[0]


def model_rx(y, nfft, nsc, cp):
    return model_rx_batch(np.asarray(y)[None], nfft, nsc, cp)[0].T


# ---- refused arguments: ValueError before any device is touched -------------------------------------------------------------
@pytest.mark.parametrize("nfft, nsc, cp", [
    (1, 2, 0), (0, 2, 0), (-4, 2, 0),            # nfft < 2
    (64, 3, 16), (64, 0, 16), (64, -2, 16),       # nsc odd or < 2
    (64, 130, 16), (2, 4, 0),                     # h > nfft - 1
    (64, 52, -1),                                 # negative prefix
    (64.5, 52, 16), (64, 52.5, 16), (64, 52, 1.5), (64, 52, float("nan")), ("64", 52, 16),
])
def test_refused_arguments(nfft, nsc, cp):
    x = np.ones((nsc if isinstance(nsc, int) and nsc > 0 else 2, 3), complex)
    with pytest.raises(ValueError):
        modulation.ofdm_tx(x, nfft, nsc, cp)
    with pytest.raises(ValueError):
        modulation.ofdm_rx(np.ones(300, complex), nfft, nsc, cp)
    with pytest.raises(ValueError):
        modulation.ofdm_rx_batch(np.ones((2, 300), complex), nfft, nsc, cp)


def test_limit_names_65536():
    with pytest.raises(ValueError, match="65536"):
        modulation.ofdm_tx(np.ones((4, 1), complex), 65537, 4, 0)
    with pytest.raises(ValueError, match="65536"):
        modulation.ofdm_rx(np.ones(10, complex), 131072, 4, 0)


def test_refused_shapes():
    with pytest.raises(ValueError):
        modulation.ofdm_tx(np.ones(52, complex), 64, 52, 16)            # x not 2-D
    with pytest.raises(ValueError):
        modulation.ofdm_tx(np.ones((52, 2, 2), complex), 64, 52, 16)
    with pytest.raises(ValueError):
        modulation.ofdm_tx(np.ones((50, 2), complex), 64, 52, 16)       # rows != nsc
    with pytest.raises(ValueError):
        modulation.ofdm_rx(np.ones((2, 80), complex), 64, 52, 16)       # y not 1-D
    with pytest.raises(ValueError):
        modulation.ofdm_tx_batch(np.ones((52, 2), complex), 64, 16)
    with pytest.raises(ValueError):
        modulation.ofdm_rx_batch(np.ones(80, complex), 64, 52, 16)


def test_whole_number_floats_are_accepted():
    assert modulation._ofdm_sizes(64.0, 52.0, 16.0) == (64, 52, 16)
    assert modulation._ofdm_sizes(np.int64(64), np.float32(52), np.uint8(16)) == (64, 52, 16)
    assert all(type(v) is int for v in modulation._ofdm_sizes(64.0, 52.0, 16.0))


def test_prefix_length_rule():
    assert [modulation.ofdm_prefix_length(64, cp) for cp in (0, 1, 16, 63, 64, 67)] == [64, 1, 16, 63, 64, 64]


# ---- the names agree across header, ctypes table and __all__ -------------------------------------------------------------
def test_header_symbols_and_all_agree():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "commpy_amd.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(cpx_ofdm_[a-z0-9_]+)\s*\(", text))
    assert declared == set(NEW)
    assert {s for s in _lib.SYMBOLS if s.startswith("cpx_ofdm_")} == set(NEW)
    for name in ("ofdm_tx", "ofdm_rx", "ofdm_tx_batch", "ofdm_rx_batch"):
        assert name in modulation.__all__
        assert callable(getattr(modulation, name))
    assert "out of scope" not in modulation.__doc__


# ---- the model on cases checked by hand --------------------------------------------------------------------------------------
def test_model_single_tone():
    nfft, nsc, cp = 16, 8, 4
    h = nsc // 2
    n = np.arange(nfft)
    for sc in range(nsc):
        x = np.zeros((nsc, 1), complex)
        x[sc, 0] = 1.0
        k = sc - h + 1 if sc >= h else nfft - h + sc                   # the bin that carries subcarrier sc
        tone = np.exp(2j * np.pi * k * n / nfft) / nfft
        got = model_tx(x, nfft, nsc, cp)
        assert got.shape == (cp + nfft,)
        assert np.allclose(got[cp:], tone, rtol=0, atol=1e-15)
        assert np.allclose(got[:cp], tone[nfft - cp:], rtol=0, atol=1e-15)
        back = model_rx(got, nfft, nsc, cp)
        assert back.shape == (nsc, 1)
        assert np.allclose(back[:, 0], x[:, 0], rtol=0, atol=1e-14)


def test_model_second_write_wins():
    # nsc == nfft: bin nfft/2 is written twice, and carries x[0] (the second write)
    nfft = 8
    x = (np.arange(nfft) + 1.0).reshape(nfft, 1)
    F = np.fft.fft(model_tx(x, nfft, nfft, 2)[2:])
    assert np.allclose(F, [0, 5, 6, 7, 1, 2, 3, 4], atol=1e-13)
    # nsc = 2 (nfft - 1): bins 1..nfft-1 from both writes, the second covering all of them
    nsc = 2 * (nfft - 1)
    x = (np.arange(nsc) + 1.0).reshape(nsc, 1)
    F = np.fft.fft(model_tx(x, nfft, nsc, 2)[2:])
    assert np.allclose(F, [0, 1, 2, 3, 4, 5, 6, 7], atol=1e-13)
    assert np.array_equal(bin_map(nfft, nsc), [-1, 0, 1, 2, 3, 4, 5, 6])


def test_model_whole_symbol_prefix():
    rs = np.random.RandomState(1)
    x = rs.randn(6, 3) + 1j * rs.randn(6, 3)
    for cp in (0, 8, 11):
        got = model_tx(x, 8, 6, cp).reshape(3, 16)
        assert np.array_equal(got[:, :8], got[:, 8:])
    assert model_tx(x, 8, 6, 3).size == 3 * 11


def test_model_rx_ignores_leftover_and_short_input():
    rs = np.random.RandomState(2)
    y = rs.randn(2 * 20 + 7) + 1j * rs.randn(2 * 20 + 7)
    assert np.array_equal(model_rx(y, 16, 8, 4), model_rx(y[:40], 16, 8, 4))
    assert model_rx(y[:19], 16, 8, 4).shape == (8, 0)


def test_empty_input_needs_no_device():
    out = modulation.ofdm_tx(np.zeros((52, 0), complex), 64, 52, 16)
    assert out.shape == (0,) and out.dtype == np.complex128
    rx = modulation.ofdm_rx(np.zeros(79, complex), 64, 52, 16)
    assert rx.shape == (52, 0) and rx.dtype == np.complex128
