"""Host side of the timing / frequency-offset synchroniser: the NumPy model against brute-force loops and exact integers, the
Schmidl-Cox preamble, the C-ABI's names, every refusal (ValueError before any device is touched) and the loud failure without a
device."""
import os
import re

import numpy as np
import pytest

import sync_model as M
from commpy_amd import _lib, deviceops, sync
from commpy_amd.sync import frame_sync_batch, schmidl_cox_preamble, sync_align_batch, sync_estimate_batch, sync_metric_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["cpx_sync_metric", "cpx_sync_metric_dev", "cpx_sync_estimate", "cpx_sync_estimate_dev", "cpx_sync_align", "cpx_sync_align_dev"]
I64MAX = 2 ** 63 - 1


def cplx(rs, *shape):
    return rs.randn(*shape) + 1j * rs.randn(*shape)


def test_model_against_loops():
    rs = np.random.RandomState(0)
    B, nr, n, D, W = 2, 3, 23, 4, 5
    y = cplx(rs, B, nr, n)
    P, E, Mm = M.metric(y, D, W)
    nd = n - D - W + 1
    assert P.shape == E.shape == Mm.shape == (B, nd)
    for b in range(B):
        for d in range(nd):
            p, e = 0, 0
            for i in range(d, d + W):
                for r in range(nr):
                    p += np.conj(y[b, r, i]) * y[b, r, i + D]
                    e += (abs(y[b, r, i]) ** 2 + abs(y[b, r, i + D]) ** 2) / 2
            assert abs(P[b, d] - p) <= 1e-14 * e and abs(E[b, d] - e) <= 1e-14 * e
            assert abs(Mm[b, d] - abs(p) ** 2 / e ** 2) <= 1e-14
    assert np.all(Mm <= 1 + 1e-14)                           # Cauchy-Schwarz and AM-GM
    bp, be = M.bound(y, D, W)
    a = np.sum(np.abs(y[:, :, :n - D]) * np.abs(y[:, :, D:]), axis=1)
    assert np.allclose(bp, 2 * (W + 2056) * 2.0 ** -53 * np.sqrt(2) * a.sum(axis=1, keepdims=True), rtol=1e-13)   # the row is all within 2048
    assert np.all(be >= bp)


def test_model_exact_on_integers():
    rs = np.random.RandomState(1)
    B, nr, n, D, W = 2, 2, 40, 3, 7
    re, im = rs.randint(-64, 65, (B, nr, n)), rs.randint(-64, 65, (B, nr, n))
    P, E, Mm = M.metric(re + 1j * im, D, W)
    for b in range(B):
        for d in range(n - D - W + 1):
            pr = pi = e2 = 0                                # Python integers; e2 = 2 e
            for i in range(d, d + W):
                for r in range(nr):
                    ar, ai, br, bi = int(re[b, r, i]), int(im[b, r, i]), int(re[b, r, i + D]), int(im[b, r, i + D])
                    pr += ar * br + ai * bi
                    pi += ar * bi - ai * br
                    e2 += ar * ar + ai * ai + br * br + bi * bi
            assert (P[b, d].real, P[b, d].imag, 2 * E[b, d]) == (pr, pi, e2)
    # zeros: M is +0 where the window holds no energy, sums never give -0
    z = np.zeros((1, 1, 12), complex)
    z[0, 0, 9:] = [-3, 0, 2j]
    P, E, Mm = M.metric(z, 2, 3)
    assert E[0, 0] == 0 and Mm[0, 0] == 0 and not np.signbit(Mm[0, 0])
    assert not np.any((np.signbit(P.real) & (P.real == 0)) | (np.signbit(P.imag) & (P.imag == 0)))
    assert np.isnan(M.metric_of(np.array([1 + 0j]), np.array([np.nan])))[0]


def test_model_first_argmax():
    m = np.array([[0.5, np.nan, 0.9, 0.9, 0.1], [np.nan] * 5, [0.0] * 5])
    assert list(M.first_argmax(m)) == [2, -1, 0]
    assert list(M.first_argmax(m, 3, 5)) == [3, -1, 3] and list(M.first_argmax(m, 1, 2)) == [-1, -1, 1]


@pytest.mark.parametrize("nfft, nsc", [(64, 52), (256, 200), (64, 62)])
def test_preamble_has_two_equal_halves(nfft, nsc):
    row = schmidl_cox_preamble(nfft, nsc)
    assert row.shape == (nsc,) and row.dtype == np.complex128
    bins = M.preamble_bins(nfft, nsc)
    used = bins % 2 == 0
    assert np.all(row[~used] == 0) and np.allclose(np.abs(row[used]), np.sqrt(2.0), rtol=0, atol=1e-15)
    body = M.ofdm_tx(row[None], nfft, 16)[16:]
    assert np.max(np.abs(body[:nfft // 2] - body[nfft // 2:])) <= 1e-15
    assert np.max(np.abs(body)) > 0.01
    # the caller's values, and the bin rule against the model's
    vals = cplx(np.random.RandomState(nfft), nsc)
    assert np.array_equal(schmidl_cox_preamble(nfft, nsc, vals), M.preamble(nfft, nsc, vals))
    assert np.array_equal(schmidl_cox_preamble(nfft, nsc), schmidl_cox_preamble(nfft, nsc))        # seeded


def test_abi_names():
    text = open(os.path.join(ROOT, "include", "commpy_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(cpx_sync_[a-z0-9_]+)\s*\(", text))
    assert declared == set(NAMES) == {s for s in _lib.SYMBOLS if s.startswith("cpx_sync_")}
    lib = _lib.load()
    assert all(hasattr(lib, s) for s in NAMES)
    assert set(sync.__all__) >= {"sync_metric_batch", "sync_estimate_batch", "sync_align_batch", "schmidl_cox_preamble", "frame_sync_batch"}
    assert {"sync_estimate_dev", "sync_align_dev"} <= set(deviceops.__all__)


@pytest.fixture
def no_device(monkeypatch):
    """Any attempt to load the engine fails the test: the refusals below must come from the host-side checks."""
    def boom(*a, **k):
        raise AssertionError("the engine was touched")
    monkeypatch.setattr(_lib, "load", boom)


def test_python_refusals(no_device):
    y = np.zeros((2, 100), complex)
    y3 = np.zeros((2, 3, 100), complex)
    for bad in (lambda: sync_metric_batch(y, 0, 4), lambda: sync_metric_batch(y, 4, 0), lambda: sync_metric_batch(y, -1, 4),
                lambda: sync_metric_batch(y, 50, 51), lambda: sync_metric_batch(y, 4.0, 4), lambda: sync_metric_batch(y, 4, True),
                lambda: sync_metric_batch(y, 4, 4, want=()), lambda: sync_metric_batch(y, 4, 4, want=('m', 'x')),
                lambda: sync_metric_batch(y[0], 4, 4), lambda: sync_metric_batch(np.zeros((1, 1, 1, 9)), 4, 4),
                lambda: sync_metric_batch(np.zeros((2, 0, 100)), 4, 4), lambda: sync_metric_batch(np.zeros((1, 1025, 20)), 4, 4),
                lambda: sync_metric_batch(np.zeros((1, 100), dtype='U1'), 4, 4),
                lambda: sync_metric_batch(np.zeros((1, 3 << 20)), (1 << 20) + 1, 4), lambda: sync_metric_batch(np.zeros((1, 3 << 20)), 4, (1 << 20) + 1),
                lambda: sync_estimate_batch(y, 0, 4), lambda: sync_estimate_batch(y, 4, 0), lambda: sync_estimate_batch(y, 60, 60),
                lambda: sync_estimate_batch(y3, 4, 4, search=(5, 5)), lambda: sync_estimate_batch(y3, 4, 4, search=(7, 3)),
                lambda: sync_estimate_batch(y, 4, 4, search=(93, 200)), lambda: sync_estimate_batch(y, 4, 4, search=(-9, 0)),
                lambda: sync_estimate_batch(y, 4, 4, search=(1,)), lambda: sync_estimate_batch(y, 4, 4, search=(0.0, 5)),
                lambda: sync_estimate_batch(y, 4, 4, search=3),
                lambda: sync_align_batch(y, 0, None, 0), lambda: sync_align_batch(y, [0], None, 5), lambda: sync_align_batch(y, 0.5, None, 5),
                lambda: sync_align_batch(y, [0, 1], [0.1], 5), lambda: sync_align_batch(y, [0, 1], 1j, 5), lambda: sync_align_batch(y, 0, None, 2.0),
                lambda: sync_align_batch(y[0], 0, None, 5), lambda: sync_align_batch(np.zeros((1, 2000, 4)), 0, None, 5),
                lambda: frame_sync_batch(y, 63, 4, 10), lambda: frame_sync_batch(y, 0, 4, 10), lambda: frame_sync_batch(y, 16, -1, 10),
                lambda: frame_sync_batch(y, 16, 4, 0), lambda: frame_sync_batch(y, 128, 4, 10),
                lambda: schmidl_cox_preamble(63, 52), lambda: schmidl_cox_preamble(64, 51), lambda: schmidl_cox_preamble(64, 52, np.ones(51)),
                lambda: schmidl_cox_preamble(64, 52, np.array(['a'] * 52)), lambda: schmidl_cox_preamble(16, 52)):
        with pytest.raises(ValueError):
            bad()
    # the largest lag and window the issue asks for are accepted, and empty batches need no device either
    e = np.zeros((0, 2, 50))
    assert [a.shape for a in sync_metric_batch(e, 8, 8, want=('p', 'm'))] == [(0, 35), (0, 35)]
    assert sync_metric_batch(np.zeros((0, 40000)), 8192, 8192)[0].shape == (0, 40000 - 16384 + 1)
    assert [a.shape for a in sync_estimate_batch(e, 8, 8)] == [(0,)] * 3 and sync_estimate_batch(e, 8, 8)[0].dtype == np.int64
    assert sync_align_batch(e, 0, None, 7).shape == (0, 2, 7) and sync_align_batch(np.zeros((0, 50)), 0, 0.1, 7).shape == (0, 7)
    out = frame_sync_batch(e, 16, 4, 30)
    assert out[0].shape == (0, 2, 30) and len(out) == 4


def test_engine_checks_without_device():
    """The C entry points: argument errors are reported before the device is looked for; a valid call fails loudly without one."""
    lib = _lib.load()
    x = np.zeros(4096)
    i64 = np.zeros(8, np.int64)
    P = _lib.ptr
    met, est, ali = lib.cpx_sync_metric, lib.cpx_sync_estimate, lib.cpx_sync_align
    for nr, n, D, W in ((0, 64, 4, 4), (1, 64, 0, 4), (1, 64, 4, 0), (-1, 64, 4, 4), (1, 7, 4, 4), (1, 0, 1, 1)):
        assert met(P(x), 1, nr, n, D, W, None, None, P(x)) == _lib.CPX_EINVAL and _lib.last_error().startswith("sync_metric:")
        assert est(P(x), 1, nr, n, D, W, 0, I64MAX, P(i64), P(x), P(x)) == _lib.CPX_EINVAL and _lib.last_error().startswith("sync_estimate:")
    for nr, n, D, W in ((1025, 64, 4, 4), (1, 1 << 22, (1 << 20) + 1, 4), (1, 1 << 22, 4, (1 << 20) + 1)):
        assert met(P(x), 1, nr, n, D, W, None, None, P(x)) == _lib.CPX_ELIMIT
        assert est(P(x), 1, nr, n, D, W, 0, I64MAX, P(i64), P(x), P(x)) == _lib.CPX_ELIMIT
        assert lib.cpx_sync_metric_dev(P(x), 1, nr, n, D, W, None, None, P(x), None) == _lib.CPX_ELIMIT
    assert met(P(x), -1, 1, 64, 4, 4, None, None, P(x)) == _lib.CPX_EINVAL
    assert met(P(x), 1, 1, 64, 4, 4, None, None, None) == _lib.CPX_EINVAL and _lib.last_error() == "sync_metric: no output requested"
    assert met(P(x), 0, 1, 64, 4, 4, None, None, None) == _lib.CPX_EINVAL
    assert met(None, 1, 1, 64, 4, 4, P(x), None, None) == _lib.CPX_EINVAL and _lib.last_error() == "sync_metric: null pointer"
    for lo, hi in ((5, 5), (9, 3), (57, 100), (-5, 0)):
        assert est(P(x), 1, 1, 64, 4, 4, lo, hi, P(i64), P(x), P(x)) == _lib.CPX_EINVAL and "search range" in _lib.last_error()
    assert est(P(x), 0, 1, 64, 4, 4, 5, 5, P(i64), P(x), P(x)) == _lib.CPX_EINVAL
    for args in ((None, P(i64), P(x), P(x)), (P(x), None, P(x), P(x)), (P(x), P(i64), None, P(x)), (P(x), P(i64), P(x), None)):
        assert est(args[0], 1, 1, 64, 4, 4, 0, I64MAX, *args[1:]) == _lib.CPX_EINVAL and _lib.last_error() == "sync_estimate: null pointer"
    assert ali(P(x), 1, 0, 64, P(i64), None, 0, 8, P(x[64:])) == _lib.CPX_EINVAL and ali(P(x), 1, 1, 64, P(i64), None, 0, 0, P(x[64:])) == _lib.CPX_EINVAL
    assert ali(P(x), 1, 1025, 1, P(i64), None, 0, 8, P(x[2048:])) == _lib.CPX_ELIMIT
    assert ali(P(x), -1, 1, 64, P(i64), None, 0, 8, P(x[64:])) == _lib.CPX_EINVAL
    for args in ((None, P(i64), P(x)), (P(x), None, P(x[64:])), (P(x), P(i64), None)):
        assert ali(args[0], 1, 1, 16, args[1], None, 0, 8, args[2]) == _lib.CPX_EINVAL and _lib.last_error() == "sync_align: null pointer"
    assert ali(P(x), 1, 1, 16, P(i64), None, 0, 8, P(x)) == _lib.CPX_EINVAL and "alias" in _lib.last_error()
    # empty batches succeed without a device, in both forms
    assert met(None, 0, 1, 64, 4, 4, None, None, P(x)) == _lib.CPX_OK and est(None, 0, 1, 64, 4, 4, 0, I64MAX, None, None, None) == _lib.CPX_OK
    assert ali(None, 0, 1, 64, None, None, 0, 8, None) == _lib.CPX_OK
    assert lib.cpx_sync_metric_dev(None, 0, 1, 64, 4, 4, None, None, P(x), None) == _lib.CPX_OK
    assert lib.cpx_sync_estimate_dev(None, 0, 1, 64, 4, 4, 0, I64MAX, None, None, None, None) == _lib.CPX_OK
    assert lib.cpx_sync_align_dev(None, 0, 1, 64, None, None, 0, 8, None, None) == _lib.CPX_OK
    # an nfft = 8192 Schmidl-Cox search passes the size checks (it fails for want of a device, or runs)
    big = np.zeros(2 * 20000)
    rc = est(P(big), 1, 1, 20000, 4096, 4096, 0, I64MAX, P(i64), P(x), P(x))
    assert rc == (_lib.CPX_OK if _lib.device_count() > 0 else _lib.CPX_ENODEV)
    if _lib.device_count() > 0:
        return
    assert met(P(x), 1, 1, 64, 4, 4, None, None, P(x)) == _lib.CPX_ENODEV and _lib.last_error().startswith("no HIP device available")
    assert ali(P(x), 1, 1, 16, P(i64), None, 0, 8, P(x[64:])) == _lib.CPX_ENODEV


def test_entry_points_fail_loudly_without_device():
    if _lib.device_count() > 0:
        pytest.skip("a HIP device is present")
    y = np.zeros((2, 2, 300), complex)
    for call in (lambda: sync_metric_batch(y, 16, 16), lambda: sync_estimate_batch(y, 16, 16), lambda: sync_estimate_batch(y[:, 0], 16, 16, (3, 9)),
                 lambda: sync_align_batch(y, [0, -4], [0.1, 0.2], 64), lambda: sync_align_batch(y, 3, None, 64),
                 lambda: frame_sync_batch(y, 32, 8, 200)):
        with pytest.raises(_lib.EngineError):
            call()
