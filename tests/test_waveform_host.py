"""Waveform modules on the host (CPU only): the tap and sequence generators against goldens recorded from the reference
(tests/golden/make_golden_waveform.py), argument checks of the GPU entry points, the C-ABI's names, and the copy check."""
import ctypes
import os
import re

import numpy as np
import pytest

import commpy_amd
import test_no_verbatim_copies as nv
from commpy_amd import _lib, filters, impairments, sequences
from golden.make_golden_waveform_shared import FO_STRIDE, fo_input

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "waveform.npz"))
NEW = ["cpx_fir_create", "cpx_fir_destroy", "cpx_fir_interp", "cpx_fir_interp_dev", "cpx_fir_decim", "cpx_fir_decim_dev",
       "cpx_freq_offset", "cpx_freq_offset_dev"]
KINDS = {0: filters.rcosfilter, 1: filters.rrcosfilter, 2: filters.gaussianfilter, 3: None}


def test_taps_match_the_reference():
    cases = GOLD["tap_cases"]
    assert len(cases) >= 576
    equal = 0
    for i, (kind, N, alpha, Ts, Fs) in enumerate(cases):
        N = int(N)
        if kind == 3:
            t, h = filters.rectfilter(N, Ts, Fs)
        else:
            t, h = KINDS[int(kind)](N, alpha, Ts, Fs)
        want = GOLD["tap_h_%d" % i]
        assert np.array_equal(t, GOLD["tap_t_%d_%r" % (N, float(Fs))]), (kind, N, alpha, Ts, Fs)
        assert h.shape == want.shape and h.dtype == np.float64
        assert np.max(np.abs(h - want)) <= 1e-12 * np.max(np.abs(want)), (kind, N, alpha, Ts, Fs)
        equal += bool(np.array_equal(h, want))
    print("taps bit-equal to the reference: %d of %d" % (equal, len(cases)))


def test_singular_points_are_hit():
    # N = 32, alpha = 0.25, Ts = 1, Fs = 4: t = +-1 is Ts / (4 alpha) and t = +-2 is Ts / (2 alpha), exactly
    t, h = filters.rrcosfilter(32, 0.25, 1, 4)
    assert t[16] == 0.0 and h[16] == 1.0 - 0.25 + 4 * 0.25 / np.pi
    assert t[20] == 1.0 and h[20] == h[12] == (0.25 / np.sqrt(2)) * ((1 + 2 / np.pi) * np.sin(np.pi) + (1 - 2 / np.pi) * np.cos(np.pi))
    t, h = filters.rcosfilter(32, 0.25, 1, 4)
    assert t[24] == 2.0 and h[24] == h[8] == (np.pi / 4) * (np.sin(2 * np.pi) / (2 * np.pi)) and h[16] == 1.0
    assert np.all(np.isfinite(h))
    t, _ = filters.rcosfilter(33, 0.5, 1, 4)
    assert not np.any(t == 0.0)                      # an odd N never samples t = 0


def test_pnsequence():
    for order, seed, mask in GOLD["pn_cases"]:
        s, m = format(seed, "0%db" % order), format(mask, "0%db" % order)
        want = GOLD["pn_%d_str" % order]
        for a, b in ((s, m), ([int(c) for c in s], tuple(int(c) for c in m)), (np.array([int(c) for c in s]), np.array([int(c) for c in m]))):
            got = sequences.pnsequence(order, a, b, len(want))
            assert got.dtype == np.int8 and np.array_equal(got, want)
        assert np.array_equal(GOLD["pn_%d_list" % order], want) and np.array_equal(GOLD["pn_%d_arr" % order], want)
    # the reference's own test vectors
    assert np.array_equal(sequences.pnsequence(4, '0011', [1, 1, 0, 1], 7), [1, 1, 0, 0, 1, 0, 1])
    assert np.array_equal(sequences.pnsequence(4, (0, 0, 1, 1), np.array((1, 1, 0, 1)), 7), [1, 1, 0, 0, 1, 0, 1])
    with pytest.raises(ValueError):
        sequences.pnsequence(4, '001', '1101', 2 ** 4 - 1)
    with pytest.raises(ValueError):
        sequences.pnsequence(4, '0011', '110', 2 ** 4 - 1)


def test_zcsequence():
    ulp = 2.0 ** -52
    for i, (u, L, q) in enumerate(GOLD["zc_cases"]):
        got, want = sequences.zcsequence(int(u), int(L), int(q)), GOLD["zc_%d" % i]
        assert got.dtype == np.complex128 and got.shape == want.shape
        assert np.max(np.abs(got.real - want.real)) <= 4 * ulp and np.max(np.abs(got.imag - want.imag)) <= 4 * ulp
    # constant amplitude, zero autocorrelation (the reference's own test)
    seq = sequences.zcsequence(3, 20)
    assert np.allclose(np.abs(seq), 1.0, atol=1e-12)
    for shift in range(1, 20):
        assert abs(np.vdot(seq, np.roll(seq, shift))) < 1e-10
    for args in ((0, 20), (-1, 20), (20, 20), (20, 0), (21, 20), (4, 20), (3, 18), (3.1, 11), (3, 20.5), (3, 20, 0.5)):
        with pytest.raises(ValueError):
            sequences.zcsequence(*args)


def test_refused_arguments_need_no_device():
    x, h = np.ones(8, complex), np.ones(5)
    for sps in (0, -1, 1.5, "2", True, None):
        with pytest.raises(ValueError):
            filters.pulse_shape(x, h, sps)
        with pytest.raises(ValueError):
            filters.matched_filter_batch(x[None], h, sps)
    for off in (-1, 12, 100, 0.5):                       # the full convolution has 8 + 5 - 1 = 12 samples
        with pytest.raises(ValueError):
            filters.matched_filter(x, h, 1, off)
    for taps in ([], np.ones((2, 3)), np.ones(filters.FIR_MAX_TAPS + 1), 1.0):
        with pytest.raises(ValueError):
            filters.pulse_shape(x, taps, 2)
        with pytest.raises(ValueError):
            filters.matched_filter(x, taps)
    with pytest.raises(ValueError, match=str(filters.FIR_MAX_TAPS)):
        filters.pulse_shape_batch(x[None], np.ones(filters.FIR_MAX_TAPS + 1), 2)
    for bad in (np.zeros(0), np.ones((2, 4))):
        with pytest.raises(ValueError):
            filters.pulse_shape(bad, h, 2)
        with pytest.raises(ValueError):
            filters.matched_filter(bad, h)
    for bad in (np.ones(4), np.zeros((3, 0))):
        with pytest.raises(ValueError):
            filters.pulse_shape_batch(bad, h, 2)
        with pytest.raises(ValueError):
            filters.matched_filter_batch(bad, h)
    with pytest.raises(ValueError):
        impairments.add_frequency_offset(np.ones((2, 4)), 1.0, 0.1)
    with pytest.raises(ValueError):
        impairments.add_frequency_offset(np.ones(4), 1.0, [0.1, 0.2])
    with pytest.raises(ValueError):
        impairments.add_frequency_offset_batch(np.ones(4), 1.0, 0.1)
    with pytest.raises(ValueError):
        impairments.add_frequency_offset_batch(np.ones((3, 4)), 1.0, [0.1, 0.2])
    # empty batches need no device either
    assert filters.pulse_shape_batch(np.zeros((0, 4)), h, 2).shape == (0, 12)
    assert filters.matched_filter_batch(np.zeros((0, 8)), h, 2, 1).shape == (0, 6)
    assert impairments.add_frequency_offset(np.zeros(0), 1.0, 0.1).shape == (0,)


def test_header_symbols_and_all_agree():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "commpy_amd.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(cpx_(?:fir|freq)_[a-z0-9_]+)\s*\(", text))
    assert declared == set(NEW)
    assert {s for s in _lib.SYMBOLS if s.startswith(("cpx_fir_", "cpx_freq_"))} == set(NEW)
    assert not any(s.startswith("cpx_ofdm_") for s in NEW)
    for mod, names in ((filters, ["rcosfilter", "rrcosfilter", "gaussianfilter", "rectfilter", "pulse_shape", "pulse_shape_batch",
                                  "matched_filter", "matched_filter_batch"]),
                       (sequences, ["pnsequence", "zcsequence"]),
                       (impairments, ["add_frequency_offset", "add_frequency_offset_batch"])):
        for name in names:
            assert name in mod.__all__ and callable(getattr(mod, name))
        assert "out of scope" not in mod.__doc__
    for name in ("filters", "sequences", "impairments"):
        assert name in commpy_amd.__all__
    assert "out of scope" not in commpy_amd.__doc__


def test_host_forms_without_a_device():
    lib = _lib.load()
    nodev = _lib.device_count() <= 0            # with a device present only the argument codes can be observed
    buf = np.zeros(64)
    step = np.zeros(1)
    p = _lib.ptr(buf)
    assert lib.cpx_fir_interp(None, p, 1, 4, 2, p) == _lib.CPX_EINVAL and "null plan" in _lib.last_error()
    assert lib.cpx_fir_decim(None, p, 1, 4, 2, 0, p) == _lib.CPX_EINVAL and "null plan" in _lib.last_error()
    h = ctypes.c_void_p()
    assert lib.cpx_fir_create(None, 4, 0, ctypes.byref(h)) == _lib.CPX_EINVAL and _lib.last_error() == "fir: null pointer"
    assert lib.cpx_fir_create(p, 4, 0, None) == _lib.CPX_EINVAL
    assert lib.cpx_fir_create(p, 0, 0, ctypes.byref(h)) == _lib.CPX_EINVAL
    assert lib.cpx_fir_create(p, filters.FIR_MAX_TAPS + 1, 0, ctypes.byref(h)) == _lib.CPX_ELIMIT
    if nodev:
        assert lib.cpx_fir_create(p, 4, 0, ctypes.byref(h)) == _lib.CPX_ENODEV and not h.value
    assert lib.cpx_freq_offset(None, 1, 4, _lib.ptr(step), 0, p) == _lib.CPX_EINVAL and _lib.last_error() == "freq_offset: null pointer"
    assert lib.cpx_freq_offset(p, 1, 4, None, 0, p) == _lib.CPX_EINVAL
    if nodev:
        assert lib.cpx_freq_offset(p, 1, 4, _lib.ptr(step), 0, p) == _lib.CPX_ENODEV
    assert lib.cpx_freq_offset(None, 0, 4, None, 0, None) == _lib.CPX_OK
    assert lib.cpx_freq_offset_dev(None, 0, 4, None, 0, None, None) == _lib.CPX_OK
    assert lib.cpx_fir_destroy(None) == _lib.CPX_OK


PAIRS = [("filters.py",) * 2, ("sequences.py",) * 2, ("impairments.py",) * 2]


@pytest.mark.parametrize("ours,theirs", PAIRS)
def test_no_verbatim_copies(ours, theirs, monkeypatch):
    monkeypatch.setattr(nv, "FINGERPRINTS", os.path.join(ROOT, "tests", "golden", "reference_fingerprints_waveform.json"))
    nv.test_no_run_of_identical_statements(ours, theirs)
    nv.test_same_named_functions_share_under_30_percent(ours, theirs)


def test_frequency_offset_goldens_are_consistent():
    """The stored outputs against the NumPy expression on the regenerated inputs (host only; the GPU test uses the same data)."""
    for i, (n, Fs, df) in enumerate(GOLD["fo_cases"]):
        n = int(n)
        x = fo_input(i, n)
        y = x * np.exp(1j * 2 * np.pi * (df / Fs) * np.arange(n))
        want = GOLD["fo_y_%d" % i]
        got = y if n <= 5000 else y[::FO_STRIDE]
        assert np.max(np.abs(got - want)) <= 16 * 2.0 ** -52 * np.max(np.abs(x))
