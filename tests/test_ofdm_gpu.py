"""OFDM transmit / receive on the MI355X (csrc/ofdm.hip) against this suite's NumPy model (test_ofdm_host.py)."""
import ctypes

import numpy as np
import pytest

from commpy_amd import _lib
from commpy_amd.modulation import QAMModem, ofdm_rx, ofdm_rx_batch, ofdm_tx, ofdm_tx_batch
from test_ofdm_host import model_rx, model_rx_batch, model_tx, model_tx_batch

pytestmark = pytest.mark.gpu


def rms(a):
    return float(np.sqrt(np.mean(np.abs(a) ** 2))) if a.size else 0.0


def close(got, want, rel):
    assert got.shape == want.shape and got.dtype == np.complex128
    if want.size:
        err = float(np.max(np.abs(got - want)))
        assert err <= rel * rms(want), (err, rms(want))


def cplx(rs, *shape):
    return rs.randn(*shape) + 1j * rs.randn(*shape)


def nsc_values(nfft):
    return sorted({v for v in (2, 2 * int(0.4 * nfft), nfft - 2, nfft, 2 * (nfft - 1)) if v >= 2 and v % 2 == 0})


@pytest.mark.parametrize("nfft", [2 ** k for k in range(1, 14)])
def test_fast_path_matches_model(gpu, nfft):
    rs = np.random.RandomState(nfft)
    for nsym in (1, 7, 1000):
        for nsc in nsc_values(nfft):
            x = cplx(rs, nsc, nsym)
            for cp in sorted({0, 1, nfft // 4, nfft, nfft + 3}):
                t = ofdm_tx(x, nfft, nsc, cp)
                close(t, model_tx(x, nfft, nsc, cp), 1e-12)
                y = t + 0.1 * cplx(rs, t.size)
                close(ofdm_rx(y, nfft, nsc, cp), model_rx(y, nfft, nsc, cp), 1e-12)
    assert "ofdm_fast_kernel<%d,rx>" % nfft in _lib.last_kernel()


@pytest.mark.parametrize("nfft", [3, 12, 100, 1536, 12288])
def test_general_path_matches_model(gpu, nfft):
    rs = np.random.RandomState(nfft)
    for nsc in nsc_values(nfft):
        nsym = 5 if nfft < 10000 else 2
        x = cplx(rs, nsc, nsym)
        for cp in (0, 1, nfft // 4, nfft + 3):
            t = ofdm_tx(x, nfft, nsc, cp)
            close(t, model_tx(x, nfft, nsc, cp), 1e-10)
            assert "ofdm_dft_kernel<%d,tx>" % nfft in _lib.last_kernel()
            close(ofdm_rx(t, nfft, nsc, cp), model_rx(t, nfft, nsc, cp), 1e-10)


def test_edge_cases(gpu):
    rs = np.random.RandomState(3)
    y = cplx(rs, 3 * 80 + 50)
    full = ofdm_rx(y, 64, 52, 16)
    assert full.shape == (52, 3)
    assert np.array_equal(full, ofdm_rx(y[:240], 64, 52, 16))
    assert ofdm_rx(y[:79], 64, 52, 16).shape == (52, 0)
    assert ofdm_tx(np.zeros((52, 0), complex), 64, 52, 16).shape == (0,)
    assert ofdm_tx(np.ones((4, 2)), 8.0, 4.0, 2.0).dtype == np.complex128       # real input, whole-number floats


@pytest.mark.parametrize("nfft, nsc, cp", [(64, 52, 16), (2048, 1200, 144), (8, 6, 1), (8192, 8190, 7), (1536, 900, 108)])
def test_round_trip(gpu, nfft, nsc, cp):
    rs = np.random.RandomState(nfft)
    x = cplx(rs, nsc, 9)
    close(ofdm_rx(ofdm_tx(x, nfft, nsc, cp), nfft, nsc, cp), x, 1e-12 if nfft != 1536 else 1e-10)


@pytest.mark.parametrize("nfft, nsc, cp", [(64, 52, 16), (2048, 1200, 144), (8192, 6000, 100), (100, 60, 10)])
def test_batched_forms_are_bit_identical(gpu, nfft, nsc, cp):
    rs = np.random.RandomState(5)
    xb = cplx(rs, 5, 11, nsc)
    tb = ofdm_tx_batch(xb, nfft, cp)
    close(tb, model_tx_batch(xb, nfft, cp), 1e-10)
    rb = ofdm_rx_batch(tb, nfft, nsc, cp)
    close(rb, model_rx_batch(tb, nfft, nsc, cp), 1e-10)
    for b in (0, 3, 4):
        assert np.array_equal(tb[b], ofdm_tx(xb[b].T, nfft, nsc, cp))
        assert np.array_equal(rb[b], ofdm_rx(tb[b], nfft, nsc, cp).T)
    # one symbol alone, and at another place of another batch size
    assert np.array_equal(ofdm_tx_batch(xb[3:4, 7:8], nfft, cp)[0], tb[3].reshape(11, -1)[7])
    shuffled = np.concatenate([xb[1:2, 7:8], cplx(rs, 1, 2, nsc), xb[3:4, 7:8]], axis=1)
    assert np.array_equal(ofdm_tx_batch(shuffled, nfft, cp)[0].reshape(4, -1)[3], tb[3].reshape(11, -1)[7])
    # the same call on a stream of its own (the _dev entry points)
    lib = _lib.load()
    plan = _plan(nfft, nsc, cp)
    st = ctypes.c_void_p()
    _lib.check(lib.cpx_stream_create(ctypes.byref(st)))
    try:
        with DevBuf(xb) as dx, DevBuf(np.zeros_like(tb)) as dt, DevBuf(np.zeros_like(rb)) as dr:
            _lib.check(lib.cpx_ofdm_tx_dev(plan, dx.p, 5, 11, dt.p, st))
            _lib.check(lib.cpx_ofdm_rx_dev(plan, dt.p, 5, tb.shape[1], dr.p, st))
            _lib.check(lib.cpx_stream_sync(st))
            assert np.array_equal(dt.get(), tb) and np.array_equal(dr.get(), rb)
    finally:
        lib.cpx_stream_destroy(st)


class DevBuf:
    """A device copy of a NumPy array (freed on exit)."""

    def __init__(self, arr):
        self.arr = np.ascontiguousarray(arr)
        self.p = ctypes.c_void_p()

    def __enter__(self):
        lib = _lib.load()
        _lib.check(lib.cpx_malloc(ctypes.byref(self.p), max(self.arr.nbytes, 8)))
        if self.arr.nbytes:
            _lib.check(lib.cpx_memcpy_h2d(self.p, _lib.ptr(self.arr), self.arr.nbytes))
        return self

    def get(self, out=None):
        out = np.empty_like(self.arr) if out is None else out
        _lib.check(_lib.load().cpx_memcpy_d2h(_lib.ptr(out), self.p, out.nbytes))
        return out

    def __exit__(self, *exc):
        _lib.load().cpx_free(self.p)


def _plan(nfft, nsc, cp):
    from commpy_amd.modulation import _ofdm_plan
    return _ofdm_plan(nfft, nsc, cp).handle()


def test_device_chain(gpu):
    """bits -> 64-QAM -> OFDM TX -> AWGN -> OFDM RX -> soft demodulation, all on the device."""
    import oracle
    lib = _lib.load()
    md = QAMModem(64)
    nfft, nsc, cp, B, nsym = 256, 200, 32, 3, 20
    P = cp
    nbits = B * nsym * nsc * 6
    nt = B * nsym * (P + nfft)
    plan = _plan(nfft, nsc, cp)
    n_eff = 1.0
    with DevBuf(np.zeros(nbits, np.uint8)) as bits, DevBuf(np.zeros((B * nsym * nsc, 2))) as sym, \
            DevBuf(np.zeros((nt, 2))) as tx, DevBuf(np.zeros((nt, 2))) as noisy, \
            DevBuf(np.zeros((B * nsym * nsc, 2))) as rx, DevBuf(np.zeros(nbits)) as llr, \
            DevBuf(np.zeros(nbits, np.int8)) as hard:
        _lib.check(lib.cpx_random_bits_dev(bits.p, nbits, 11, 0, None))
        _lib.check(lib.cpx_modulate_dev(md._device_handle(), bits.p, B * nsym * nsc, sym.p, None))
        _lib.check(lib.cpx_ofdm_tx_dev(plan, sym.p, B, nsym, tx.p, None))
        # noiseless: RX gives the symbols back, and hard decisions give the bits exactly
        _lib.check(lib.cpx_ofdm_rx_dev(plan, tx.p, B, nsym * (P + nfft), rx.p, None))
        _lib.check(lib.cpx_demod_hard_dev(md._device_handle(), rx.p, B * nsym * nsc, hard.p, None))
        _lib.check(lib.cpx_stream_sync(None))
        b = bits.get()
        assert np.array_equal(hard.get().astype(np.uint8), b)
        s = sym.get().view(complex).reshape(B, nsym, nsc)
        assert np.array_equal(s.reshape(-1), md.modulate(b))
        close(rx.get().view(complex).reshape(B, nsym, nsc), s, 1e-12)
        # with noise: per-sample variance n_eff / nfft in the time domain is n_eff per subcarrier after the fft
        scale = np.sqrt(n_eff / (2 * nfft))
        _lib.check(lib.cpx_awgn_dev(tx.p, nt, scale, scale, 12, 1, noisy.p, None))
        _lib.check(lib.cpx_ofdm_rx_dev(plan, noisy.p, B, nsym * (P + nfft), rx.p, None))
        _lib.check(lib.cpx_demod_soft_dev(md._device_handle(), rx.p, B * nsym * nsc, n_eff, llr.p, None))
        _lib.check(lib.cpx_stream_sync(None))
        y = noisy.get().view(complex).reshape(B, -1)
        want_sym = model_rx_batch(y, nfft, nsc, cp).reshape(-1)
        close(rx.get().view(complex).reshape(-1), want_sym, 1e-12)
        want = oracle.demodulate(md.constellation, want_sym, "soft", n_eff)
        got = llr.get()
        assert np.max(np.abs(got - want)) <= 1e-9 * max(1.0, float(np.max(np.abs(want))))


def test_large_batch_64bit_offsets(gpu):
    """(64, 52, 16) with 2^21 + 5 OFDM symbols made on the device; 200 symbols checked against the model, TX and RX."""
    lib = _lib.load()
    md = QAMModem(64)
    nfft, nsc, cp = 64, 52, 16
    B, nsym = 2, 2 ** 20 + 3
    S = nsym * B
    per = cp + nfft
    plan = _plan(nfft, nsc, cp)
    rs = np.random.RandomState(7)
    picks = np.sort(np.concatenate([rs.choice(S, 196, replace=False), [0, S - 1, S // 2, nsym]]))
    x = np.zeros((nsc, 2))
    t = np.zeros((per, 2))
    ptrs = {}
    try:
        for name, nbytes in (("bits", S * nsc * 6), ("sym", S * nsc * 16), ("tx", S * per * 16), ("rx", S * nsc * 16)):
            ptrs[name] = ctypes.c_void_p()
            _lib.check(lib.cpx_malloc(ctypes.byref(ptrs[name]), nbytes))
        _lib.check(lib.cpx_random_bits_dev(ptrs["bits"], S * nsc * 6, 5, 0, None))
        _lib.check(lib.cpx_modulate_dev(md._device_handle(), ptrs["bits"], S * nsc, ptrs["sym"], None))
        _lib.check(lib.cpx_ofdm_tx_dev(plan, ptrs["sym"], B, nsym, ptrs["tx"], None))
        _lib.check(lib.cpx_ofdm_rx_dev(plan, ptrs["tx"], B, nsym * per, ptrs["rx"], None))
        _lib.check(lib.cpx_stream_sync(None))
        r = np.zeros((nsc, 2))
        for s in picks:
            s = int(s)
            _lib.check(lib.cpx_memcpy_d2h(_lib.ptr(x), ctypes.c_void_p(ptrs["sym"].value + s * nsc * 16), nsc * 16))
            _lib.check(lib.cpx_memcpy_d2h(_lib.ptr(t), ctypes.c_void_p(ptrs["tx"].value + s * per * 16), per * 16))
            _lib.check(lib.cpx_memcpy_d2h(_lib.ptr(r), ctypes.c_void_p(ptrs["rx"].value + s * nsc * 16), nsc * 16))
            xs = x.view(complex).reshape(1, 1, nsc)
            close(t.view(complex).reshape(-1), model_tx_batch(xs, nfft, cp)[0], 1e-12)
            close(r.view(complex).reshape(-1), xs.reshape(-1), 1e-12)
    finally:
        for p in ptrs.values():
            lib.cpx_free(p)


def test_c_abi_argument_errors(gpu):
    lib = _lib.load()
    h = ctypes.c_void_p()
    assert lib.cpx_ofdm_create(65537, 4, 0, ctypes.byref(h)) == _lib.CPX_ELIMIT
    assert "65536" in _lib.last_error()
    for args in ((1, 2, 0), (64, 3, 0), (64, 0, 0), (64, 130, 0), (64, 52, -1)):
        assert lib.cpx_ofdm_create(*args, ctypes.byref(h)) == _lib.CPX_EINVAL
        assert _lib.last_error()
    assert lib.cpx_ofdm_create(64, 52, 16, None) == _lib.CPX_EINVAL
    x = np.zeros((3, 52), complex)
    out = np.zeros(3 * 80, complex)
    assert lib.cpx_ofdm_tx(None, _lib.ptr(x), 1, 3, _lib.ptr(out)) == _lib.CPX_EINVAL
    assert lib.cpx_ofdm_rx(None, _lib.ptr(out), 1, 240, _lib.ptr(x)) == _lib.CPX_EINVAL
    assert lib.cpx_ofdm_tx_dev(None, None, 1, 3, None, None) == _lib.CPX_EINVAL
    assert lib.cpx_ofdm_rx_dev(None, None, 1, 240, None, None) == _lib.CPX_EINVAL
    plan = _plan(64, 52, 16)
    assert lib.cpx_ofdm_tx(plan, None, 1, 3, _lib.ptr(out)) == _lib.CPX_EINVAL
    assert lib.cpx_ofdm_tx(plan, _lib.ptr(x), 1, 3, None) == _lib.CPX_EINVAL
    assert lib.cpx_ofdm_rx(plan, None, 1, 240, _lib.ptr(x)) == _lib.CPX_EINVAL
    assert lib.cpx_ofdm_tx_dev(plan, None, 1, 3, None, None) == _lib.CPX_EINVAL
    assert lib.cpx_ofdm_rx_dev(plan, None, 1, 240, None, None) == _lib.CPX_EINVAL
    assert lib.cpx_ofdm_tx(plan, _lib.ptr(x), -1, 3, _lib.ptr(out)) == _lib.CPX_EINVAL
    assert lib.cpx_ofdm_tx(plan, None, 1, 0, None) == _lib.CPX_OK                # nothing to do
    assert lib.cpx_ofdm_destroy(None) == _lib.CPX_OK
