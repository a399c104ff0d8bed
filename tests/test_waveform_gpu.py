"""Pulse shaping, matched filtering and frequency offset on the MI355X (csrc/fir.hip).  The model is numpy.convolve per row.

Tolerance of the filters, derived rather than tuned: two float64 sums of T products of the same operands differ by at most
2 (T + 2) 2^-53 sum|h| max|x| sqrt(2), T = ceil(ntaps / sps) for the interpolator and ntaps for the decimator."""
import ctypes
import os

import numpy as np
import pytest

from commpy_amd import _lib, filters, impairments, sequences
from commpy_amd.filters import matched_filter, matched_filter_batch, pulse_shape, pulse_shape_batch, rrcosfilter
from commpy_amd.modulation import QAMModem
from commpy_amd.utilities import upsample
from golden.make_golden_waveform_shared import FO_STRIDE, fo_input

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT = filters.FIR_MAX_TAPS


def cplx(rs, *shape):
    return rs.randn(*shape) + 1j * rs.randn(*shape)


def bound(T, h, x):
    return 2 * (T + 2) * 2.0 ** -53 * np.sum(np.abs(h)) * np.max(np.abs(x)) * np.sqrt(2)


def model_interp(x, h, sps):
    """numpy.convolve(upsample(x, sps), h).  Above 2e8 multiply-adds the zero-stuffed convolution takes minutes on the host; the
    same sums are then taken phase by phase: output q sps + p is numpy.convolve(x, h[p::sps])[q], the terms left once the zeros are
    dropped (test_polyphase_model_is_the_zero_stuffed_convolution compares the two forms)."""
    if len(x) * sps * len(h) <= 2e8:
        return np.convolve(upsample(x, sps), h)
    return model_interp_polyphase(x, h, sps)


def model_interp_polyphase(x, h, sps):
    out = np.zeros(len(x) * sps + len(h) - 1, complex)
    for p in range(min(sps, len(h))):
        c = np.convolve(x, h[p::sps])
        out[p::sps][:len(c)] = c
    return out


def model_decim(y, h, sps, off):
    return np.convolve(y, h)[off::sps]


def taps_of(rs, ntaps, cx):
    return cplx(rs, ntaps) if cx else rs.randn(ntaps)


def ntaps_values(sps):
    return sorted({v for v in (1, 2, sps - 1, sps, sps + 1, 49, 97, 129, 1000, LIMIT) if v >= 1})


# outputs above this many bytes are not brought to the host whole (the largest cell of the grid, B = 257 rows of 100 003 symbols at
# sps = 64, is 26 GB of output): the call then goes through the _dev form and only the rows that are compared are read back
HOST_OUTPUT_LIMIT = 2 ** 28


class Rows:
    """A batch x [B, n] with a device copy made once and shared by the calls that need it."""

    def __init__(self, x):
        self.x = x
        self._dev = None

    def dev(self):
        if self._dev is None:
            self._dev = DevBuf(self.x.view(float)).__enter__()
        return self._dev.p

    def close(self):
        if self._dev is not None:
            self._dev.__exit__()


def run_fir(rows, h, sps, off, picks):
    """{b: output row b} of the interpolator (off is None) or the decimator, for b in picks; the whole batch is computed."""
    lib = _lib.load()
    x = rows.x
    B, n = x.shape
    full = n + len(h) - 1
    lout = n * sps + len(h) - 1 if off is None else -(-(full - off) // sps)
    if B * lout * 16 <= HOST_OUTPUT_LIMIT:
        out = pulse_shape_batch(x, h, sps) if off is None else matched_filter_batch(x, h, sps, off)
        assert out.shape == (B, lout) and out.dtype == np.complex128
        return {b: out[b] for b in picks}
    hh, cx = filters._taps(h)
    plan = filters._fir_plan(hh, cx).handle()
    d_out = ctypes.c_void_p()
    _lib.check(lib.cpx_malloc(ctypes.byref(d_out), B * lout * 16))
    try:
        if off is None:
            _lib.check(lib.cpx_fir_interp_dev(plan, rows.dev(), B, n, sps, d_out, None))
        else:
            _lib.check(lib.cpx_fir_decim_dev(plan, rows.dev(), B, n, sps, off, d_out, None))
        _lib.check(lib.cpx_stream_sync(None))
        return {b: _peek(d_out, b * lout, lout) for b in picks}
    finally:
        lib.cpx_free(d_out)


def check_row(got, want, T, h, xrow):
    assert got.shape == want.shape
    err = np.max(np.abs(got - want))
    assert err <= bound(T, h, xrow), (err, bound(T, h, xrow))


def test_polyphase_model_is_the_zero_stuffed_convolution():
    rs = np.random.RandomState(1)
    for sps, ntaps, n in ((1, 5, 7), (3, 1, 4), (4, 3, 9), (5, 49, 64), (8, 97, 300), (64, 1000, 50), (16, 129, 1)):
        x, h = cplx(rs, n), cplx(rs, ntaps)
        a, b = np.convolve(upsample(x, sps), h), model_interp_polyphase(x, h, sps)
        assert a.shape == b.shape and np.max(np.abs(a - b)) <= bound(-(-ntaps // sps), h, x)


@pytest.mark.parametrize("sps", [1, 2, 3, 4, 5, 8, 16, 64])
def test_interpolator_matches_convolve(gpu, sps):
    """The whole grid: ntaps x n x real / complex taps x B, rows 0, B // 2 and B - 1 of every case against the model, whole rows."""
    rs = np.random.RandomState(sps)
    for n in (1, 2, 63, 64, 65, 1000, 100003):
        for B in (1, 3, 257):
            rows = Rows(cplx(rs, B, n))
            try:
                for ntaps in ntaps_values(sps):
                    for cx in (False, True):
                        h = taps_of(rs, ntaps, cx)
                        picks = sorted({0, B // 2, B - 1})
                        got = run_fir(rows, h, sps, None, picks)
                        for b in picks:
                            check_row(got[b], model_interp(rows.x[b], h, sps), -(-ntaps // sps), h, rows.x[b])
            finally:
                rows.close()


@pytest.mark.parametrize("sps", [1, 2, 3, 4, 5, 8, 16, 64])
def test_decimator_matches_convolve(gpu, sps):
    """The whole grid and every offset of it; rows 0 and B - 1 of every case against the full convolution subsampled."""
    rs = np.random.RandomState(100 + sps)
    for n in (1, 2, 63, 64, 65, 1000, 100003):
        for B in (1, 3, 257):
            rows = Rows(cplx(rs, B, n))
            try:
                for ntaps in ntaps_values(sps):
                    for cx in (False, True):
                        h = taps_of(rs, ntaps, cx)
                        picks = sorted({0, B - 1})
                        conv = {b: np.convolve(rows.x[b], h) for b in picks}
                        full = n + ntaps - 1
                        for off in sorted({o for o in (0, 1, sps - 1, (ntaps - 1) // 2, full - 1) if 0 <= o < full}):
                            got = run_fir(rows, h, sps, off, picks)
                            for b in picks:
                                want = conv[b][off::sps]
                                assert len(want) == -(-(full - off) // sps)       # the last kept sample is there
                                check_row(got[b], want, ntaps, h, rows.x[b])
            finally:
                rows.close()


def test_tap_limit(gpu):
    lib = _lib.load()
    h = np.ones(LIMIT + 1)
    p = ctypes.c_void_p()
    assert lib.cpx_fir_create(_lib.ptr(h), LIMIT + 1, 0, ctypes.byref(p)) == _lib.CPX_ELIMIT
    assert str(LIMIT) in _lib.last_error()
    assert lib.cpx_fir_create(_lib.ptr(h), LIMIT, 0, ctypes.byref(p)) == 0
    assert lib.cpx_fir_destroy(p) == 0


def test_equivalences(gpu):
    rs = np.random.RandomState(5)
    for ntaps, cx in ((1, False), (49, False), (97, True), (839, True), (1000, False)):
        h = taps_of(rs, ntaps, cx)
        x = cplx(rs, 3, 5000)
        a = pulse_shape_batch(x, h, 1)
        b = matched_filter_batch(x, h, 1, 0)
        assert a.tobytes() == b.tobytes()                 # sps = 1: the same chain, bit for bit
        for sps, off in ((4, 3), (8, 0), (5, 2)):
            sub = matched_filter_batch(x, h, sps, off)
            for r in range(3):
                assert np.max(np.abs(sub[r] - a[r][off::sps])) <= bound(ntaps, h, x[r])
    # RRC shaping, then the matched RRC sampled at offset ntaps - 1: the symbols plus the model's inter-symbol interference
    for sps, span, alpha in ((8, 12, 0.22), (4, 12, 0.22), (5, 8, 0.35)):
        ntaps = span * sps + 1
        _, h = rrcosfilter(ntaps, alpha, 1.0, sps)
        h = h / np.sqrt(np.sum(h * h))
        sym = QAMModem(16).modulate(rs.randint(0, 2, 4 * 2000))
        w = pulse_shape(sym, h, sps)
        got = matched_filter(w, h, sps, ntaps - 1)
        want = model_decim(model_interp(sym, h, sps), h, sps, ntaps - 1)
        assert got.shape == want.shape
        assert np.max(np.abs(got - want)) <= bound(ntaps, h, w) + np.sum(np.abs(h)) * bound(span + 1, h, sym)
        isi = np.max(np.abs(want[:len(sym)] - sym))
        assert np.max(np.abs(got[:len(sym)] - sym)) <= isi + 1e-12


def test_bit_identity(gpu):
    lib = _lib.load()
    rs = np.random.RandomState(6)
    _, h = rrcosfilter(97, 0.22, 1.0, 8)
    for n, sps in ((64, 8), (1000, 8), (5000, 1)):
        for hh in (h, cplx(rs, 839)):
            x = cplx(rs, 257, n)
            row = x[100].copy()
            alone_i = pulse_shape(row, hh, sps)
            alone_d = matched_filter(row, hh, sps, 3)
            for pos in (0, 100, 256):
                xb = x.copy()
                xb[pos] = row
                assert pulse_shape_batch(xb, hh, sps)[pos].tobytes() == alone_i.tobytes()
                assert matched_filter_batch(xb, hh, sps, 3)[pos].tobytes() == alone_d.tobytes()
            xb = x.copy()
            both = pulse_shape_batch(xb, hh, sps)
            halves = np.concatenate([pulse_shape_batch(xb[:130], hh, sps), pulse_shape_batch(xb[130:], hh, sps)])
            assert both.tobytes() == halves.tobytes()
            bothd = matched_filter_batch(xb, hh, sps, 3)
            halvesd = np.concatenate([matched_filter_batch(xb[:57], hh, sps, 3), matched_filter_batch(xb[57:], hh, sps, 3)])
            assert bothd.tobytes() == halvesd.tobytes()
    # a created stream, through the _dev forms
    x = cplx(rs, 5, 1000)
    hh = np.ascontiguousarray(h)
    plan = filters._fir_plan(hh, False).handle()
    want_i, want_d = pulse_shape_batch(x, hh, 8), matched_filter_batch(x, hh, 8, 3)
    st = ctypes.c_void_p()
    _lib.check(lib.cpx_stream_create(ctypes.byref(st)))
    try:
        with DevBuf(x.view(float)) as dx, DevBuf(np.zeros(want_i.shape + (2,))) as di, DevBuf(np.zeros(want_d.shape + (2,))) as dd:
            _lib.check(lib.cpx_fir_interp_dev(plan, dx.p, 5, 1000, 8, di.p, st))
            _lib.check(lib.cpx_fir_decim_dev(plan, dx.p, 5, 1000, 8, 3, dd.p, st))
            _lib.check(lib.cpx_stream_sync(st))
            assert di.get().tobytes() == want_i.tobytes() and dd.get().tobytes() == want_d.tobytes()
    finally:
        _lib.check(lib.cpx_stream_destroy(st))


class DevBuf:
    """A device copy of a host array for the _dev entry points."""

    def __init__(self, host):
        self.host = np.ascontiguousarray(host)
        self.p = ctypes.c_void_p()

    def __enter__(self):
        lib = _lib.load()
        _lib.check(lib.cpx_malloc(ctypes.byref(self.p), max(self.host.nbytes, 8)))
        _lib.check(lib.cpx_memcpy_h2d(self.p, _lib.ptr(self.host), self.host.nbytes))
        return self

    def get(self):
        out = np.empty_like(self.host)
        _lib.check(_lib.load().cpx_memcpy_d2h(_lib.ptr(out), self.p, out.nbytes))
        return out

    def __exit__(self, *exc):
        _lib.load().cpx_free(self.p)
        return False


def test_frequency_offset(gpu):
    lib = _lib.load()
    gold = np.load(os.path.join(ROOT, "tests", "golden", "waveform.npz"))
    tol = 16 * 2.0 ** -52
    for i, (n, Fs, df) in enumerate(gold["fo_cases"]):
        n = int(n)
        x = fo_input(i, n)
        got = impairments.add_frequency_offset(x, Fs, df)
        assert got.shape == (n,) and got.dtype == np.complex128
        want = gold["fo_y_%d" % i]
        sel = slice(None) if n <= 5000 else slice(None, None, FO_STRIDE)
        assert np.all(np.abs(got[sel] - want) <= tol * np.abs(x[sel]))
        model = x * np.exp(1j * 2 * np.pi * (df / Fs) * np.arange(n))
        assert np.all(np.abs(got - model) <= tol * np.abs(x))
    rs = np.random.RandomState(8)
    x = cplx(rs, 4, 3001)
    assert np.array_equal(impairments.add_frequency_offset_batch(x, 1e3, 0.0), x)
    dfs = np.array([10.0, -250.0, 0.0, 499.0])
    got = impairments.add_frequency_offset_batch(x, 1e3, dfs)
    for b in range(4):
        assert np.array_equal(got[b], impairments.add_frequency_offset(x[b], 1e3, dfs[b]))
        model = x[b] * np.exp(1j * 2 * np.pi * (dfs[b] / 1e3) * np.arange(3001))
        assert np.all(np.abs(got[b] - model) <= tol * np.abs(x[b]))
    # k up to 1e7 with a step near pi: the argument reduction
    n = 10 ** 7 + 3
    x = np.ones(n, complex)
    step = (2 * np.pi) * (0.49999 / 1.0)
    got = impairments.add_frequency_offset(x, 1.0, 0.49999)
    k = np.concatenate([np.arange(0, n, 9973), np.arange(n - 50, n)])
    want = np.exp(1j * (step * k))
    assert np.all(np.abs(got[k] - want) <= tol)
    # in place, through the _dev form
    x = cplx(rs, 2, 5000)
    st = np.array([0.3, -2.9])
    with DevBuf(x.view(float)) as dx, DevBuf(st) as ds:
        _lib.check(lib.cpx_freq_offset_dev(dx.p, 2, 5000, ds.p, 1, dx.p, None))
        _lib.check(lib.cpx_stream_sync(None))
        got = dx.get().view(complex)
    for b in range(2):
        assert np.all(np.abs(got[b] - x[b] * np.exp(1j * (st[b] * np.arange(5000)))) <= tol * np.abs(x[b]))


def test_zadoff_chu_correlator(gpu):
    rs = np.random.RandomState(9)
    zc = sequences.zcsequence(25, 839)
    h = np.conj(zc[::-1])
    delay = 1234
    w = 0.01 * cplx(rs, 5000)
    clean = np.zeros(5000, complex)
    clean[delay:delay + 839] = zc
    corr = matched_filter(clean + w, h)
    peak = int(np.argmax(np.abs(corr)))
    assert peak == delay + 838
    want = np.convolve(clean + w, h)
    assert np.max(np.abs(corr - want)) <= bound(839, h, clean + w)
    assert abs(abs(matched_filter(clean, h)[peak]) - 839) <= bound(839, h, clean)
    assert "fir_decim_kernel<complex" in _lib.last_kernel()


def test_device_chain(gpu):
    """bits -> 16-QAM -> RRC shaping (sps 8) -> +delta, -delta frequency offset -> AWGN -> matched filter -> soft demodulation."""
    import oracle
    lib = _lib.load()
    md = QAMModem(16)
    sps, span, B, n = 8, 12, 3, 500
    ntaps = span * sps + 1
    _, h = rrcosfilter(ntaps, 0.22, 1.0, sps)
    h = np.ascontiguousarray(h / np.sqrt(np.sum(h * h)))
    plan = filters._fir_plan(h, False).handle()
    nbits, lw = B * n * 4, n * sps + ntaps - 1
    # the reference's time axis (k - N / 2) / Fs centres an N = 97 pulse on sample 48.5, so shaping + matched filter peak at sample N
    off = ntaps
    ld = -(-(lw + ntaps - 1 - off) // sps)
    step = np.array([(2 * np.pi) * (123.0 / 8000.0)])
    with DevBuf(np.zeros(nbits, np.uint8)) as bits, DevBuf(np.zeros((B * n, 2))) as sym, DevBuf(np.zeros((B * lw, 2))) as w, \
            DevBuf(np.zeros((B * lw, 2))) as w2, DevBuf(np.zeros((B * lw, 2))) as noisy, DevBuf(np.zeros((B * ld, 2))) as rx, \
            DevBuf(np.zeros(B * ld * 4)) as llr, DevBuf(np.zeros(B * ld * 4, np.int8)) as hard, DevBuf(step) as sp, DevBuf(-step) as sm:
        _lib.check(lib.cpx_random_bits_dev(bits.p, nbits, 21, 0, None))
        _lib.check(lib.cpx_modulate_dev(md._device_handle(), bits.p, B * n, sym.p, None))
        _lib.check(lib.cpx_fir_interp_dev(plan, sym.p, B, n, sps, w.p, None))
        _lib.check(lib.cpx_freq_offset_dev(w.p, B, lw, sp.p, 0, w2.p, None))
        _lib.check(lib.cpx_freq_offset_dev(w2.p, B, lw, sm.p, 0, w2.p, None))
        _lib.check(lib.cpx_fir_decim_dev(plan, w2.p, B, lw, sps, off, rx.p, None))
        _lib.check(lib.cpx_demod_hard_dev(md._device_handle(), rx.p, B * ld, hard.p, None))
        _lib.check(lib.cpx_stream_sync(None))
        b = bits.get()
        s = sym.get().view(complex).reshape(B, n)
        assert np.array_equal(s.reshape(-1), md.modulate(b))
        dec = hard.get().reshape(B, ld, 4)[:, :n].reshape(-1)
        assert np.array_equal(dec.astype(np.uint8), b)                # noiseless: the hard decisions are the bits
        n_eff = 0.05
        scale = np.sqrt(n_eff / 2)
        _lib.check(lib.cpx_awgn_dev(w2.p, B * lw, scale, scale, 22, 1, noisy.p, None))
        _lib.check(lib.cpx_fir_decim_dev(plan, noisy.p, B, lw, sps, off, rx.p, None))
        _lib.check(lib.cpx_demod_soft_dev(md._device_handle(), rx.p, B * ld, n_eff, llr.p, None))
        _lib.check(lib.cpx_stream_sync(None))
        y = noisy.get().view(complex).reshape(B, lw)
        got = rx.get().view(complex).reshape(B, ld)
        want = np.stack([model_decim(y[r], h, sps, off) for r in range(B)])
        for r in range(B):
            assert np.max(np.abs(got[r] - want[r])) <= bound(ntaps, h, y[r])
        want_llr = oracle.demodulate(md.constellation, want.reshape(-1), "soft", n_eff)
        assert np.max(np.abs(llr.get() - want_llr)) <= 1e-9 * max(1.0, float(np.max(np.abs(want_llr))))


def _peek(ptr, start, count):
    out = np.zeros((count, 2))
    _lib.check(_lib.load().cpx_memcpy_d2h(_lib.ptr(out), ctypes.c_void_p(ptr.value + start * 16), count * 16))
    return out.view(complex).reshape(-1)


def test_large_sizes(gpu):
    """One row of 2^27 + 5 samples through the decimator, and more than 2^32 output bytes through the interpolator."""
    lib = _lib.load()
    md = QAMModem(4)
    _, h = rrcosfilter(97, 0.22, 1.0, 8)
    h = np.ascontiguousarray(h)
    plan = filters._fir_plan(h, False).handle()
    n = 2 ** 27 + 5
    ptrs = {}
    try:
        for name, nbytes in (("bits", n * 2), ("x", n * 16), ("out", (2 ** 28 + 4096) * 16 + 97 * 16 * 64)):
            ptrs[name] = ctypes.c_void_p()
            _lib.check(lib.cpx_malloc(ctypes.byref(ptrs[name]), nbytes))
        _lib.check(lib.cpx_random_bits_dev(ptrs["bits"], n * 2, 3, 0, None))
        _lib.check(lib.cpx_modulate_dev(md._device_handle(), ptrs["bits"], n, ptrs["x"], None))
        off, sps = 5, 8
        lo = -(-(n + 96 - off) // sps)
        _lib.check(lib.cpx_fir_decim_dev(plan, ptrs["x"], 1, n, sps, off, ptrs["out"], None))
        _lib.check(lib.cpx_stream_sync(None))
        for i0 in (0, 250, 2 ** 23 - 40, lo // 2, lo - 100):          # ends, a tile boundary (256 outputs), the middle
            cnt = min(100, lo - i0)
            got = _peek(ptrs["out"], i0, cnt)
            lo_s = max(0, off + i0 * sps - 96)
            hi_s = min(n, off + (i0 + cnt) * sps)
            seg = _peek(ptrs["x"], lo_s, hi_s - lo_s)
            full = np.convolve(seg, h)
            first = off + i0 * sps - lo_s
            want = full[first::sps][:cnt]                # the segment holds every input these outputs touch
            assert np.max(np.abs(got - want)) <= bound(97, h, seg)
        # interpolator: B n sps 16 > 2^32 bytes
        B, nn = 64, 2 ** 19
        lw = nn * sps + 96
        assert B * lw * 16 > 2 ** 32
        _lib.check(lib.cpx_fir_interp_dev(plan, ptrs["x"], B, nn, sps, ptrs["out"], None))
        _lib.check(lib.cpx_stream_sync(None))
        for b in (0, 31, 63):
            row = _peek(ptrs["x"], b * nn, nn)
            for q0 in (0, 120, nn // 2, nn - 300):                 # the ends and a tile boundary (128 symbols)
                cnt = 280
                seg = row[max(0, q0 - 12):q0 + cnt]
                full = model_interp(seg, h, sps)
                skip = (q0 - max(0, q0 - 12)) * sps
                hi = lw if q0 + cnt >= nn else (q0 + cnt) * sps
                want = full[skip:skip + hi - q0 * sps]
                got = _peek(ptrs["out"], b * lw + q0 * sps, hi - q0 * sps)
                assert np.max(np.abs(got - want)) <= bound(13, h, seg)
    finally:
        for p in ptrs.values():
            lib.cpx_free(p)


def test_c_abi_errors(gpu):
    lib = _lib.load()
    h = np.ones(5)
    plan = filters._fir_plan(h, False).handle()
    buf = np.zeros((64, 2))
    p = _lib.ptr(buf)
    step = np.zeros(1)

    def refused(rc, text, code=_lib.CPX_EINVAL):
        assert rc == code and text in _lib.last_error(), (rc, _lib.last_error())

    refused(lib.cpx_fir_interp(None, p, 1, 4, 2, p), "fir_interp: null plan")
    refused(lib.cpx_fir_decim(None, p, 1, 4, 2, 0, p), "fir_decim: null plan")
    refused(lib.cpx_fir_interp(plan, None, 1, 4, 2, p), "fir_interp: null pointer")
    refused(lib.cpx_fir_interp(plan, p, 1, 4, 2, None), "fir_interp: null pointer")
    refused(lib.cpx_fir_decim(plan, None, 1, 4, 2, 0, p), "fir_decim: null pointer")
    refused(lib.cpx_fir_interp_dev(plan, None, 1, 4, 2, None, None), "fir_interp: null pointer")
    refused(lib.cpx_fir_decim_dev(plan, None, 1, 4, 2, 0, None, None), "fir_decim: null pointer")
    refused(lib.cpx_fir_interp(plan, p, 1, 4, 0, p), "sps = 0")
    refused(lib.cpx_fir_decim(plan, p, 1, 4, -1, 0, p), "sps = -1")
    refused(lib.cpx_fir_decim(plan, p, 1, 4, 2, 8, p), "offset = 8")
    refused(lib.cpx_fir_decim(plan, p, 1, 4, 2, -1, p), "offset = -1")
    refused(lib.cpx_fir_interp(plan, p, 1, 0, 2, p), "n = 0")
    refused(lib.cpx_fir_decim(plan, p, 1, 0, 2, 0, p), "n = 0")
    refused(lib.cpx_freq_offset(None, 1, 4, _lib.ptr(step), 0, p), "freq_offset: null pointer")
    refused(lib.cpx_freq_offset(p, 1, 4, None, 0, p), "freq_offset: null pointer")
    refused(lib.cpx_freq_offset(p, 1, 4, _lib.ptr(step), 2, p), "step_batched = 2")
    refused(lib.cpx_freq_offset(p, -1, 4, _lib.ptr(step), 0, p), "negative size")
    # empty batches succeed without touching the buffers
    assert lib.cpx_fir_interp(plan, None, 0, 4, 2, None) == 0
    assert lib.cpx_fir_decim(plan, None, 0, 4, 2, 0, None) == 0
    assert lib.cpx_freq_offset(None, 0, 4, None, 0, None) == 0
