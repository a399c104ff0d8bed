"""The MIMO link on the device (csrc/mimo_channel.hip, commpy_amd/devicelink.py: mimo_channel_gpu, DeviceMimoLink).

Channel structure bit for bit (host loops in the documented summation order, the documented Philox keys, split launches),
channel statistics over 2^20 vectors with bounds derived from the sample count, plumbing parity against the per-vector
detectors and a host recount / host LDPC decode of a kept batch, and BER: the reference's test_links.py targets and a
two-sample test against the host LinkModel for the uncoded K-best and the LDPC-coded best-first link."""
import ctypes
import math

import numpy as np
import pytest

from commpy_amd import _lib
from commpy_amd.channelcoding.ldpc import ldpc_bp_decode
from commpy_amd.channels import MIMOFlatChannel
from commpy_amd.devicelink import DeviceBuf, DeviceMimoLink, _channel_handles, _fading_matrices, mimo_channel_gpu
from commpy_amd.links import LinkModel, mimo_receiver
from commpy_amd.modulation import QAMModem, best_first_detector, kbest, mimo_ml
from helpers import ldpc_params

pytestmark = pytest.mark.gpu
SQRT_HALF = math.sqrt(0.5)


def _rayleigh(nr=4, nt=4, noise_std=0.0):
    ch = MIMOFlatChannel(nt, nr)
    ch.uncorr_rayleigh_fading(complex)
    ch.noise_std = noise_std
    return ch


def _rician(nr=4, nt=4, noise_std=0.0):
    ch = MIMOFlatChannel(nt, nr)
    mean = np.exp(1j * np.add.outer(np.arange(nr) * 0.7, np.arange(nt) * -0.4))
    ch.expo_corr_rician_fading(mean, 2.0, np.exp(0.3j), np.exp(-0.5j), betat=0.2, betar=0.4)
    ch.noise_std = noise_std
    return ch


def _cmac(acc, a, b):
    """acc + a * b with the complex product written out, element-wise over float64 arrays (no contraction)."""
    pr = a.real * b.real - a.imag * b.imag
    pi = a.real * b.imag + a.imag * b.real
    return (acc.real + pr) + 1j * (acc.imag + pi)


def _host_hx(H, x):
    """y[v][r] = 0 + sum_a H[v][r][a] x[v][a], a ascending (the kernel's order)."""
    y = np.zeros(H.shape[:2], complex)
    for a in range(H.shape[2]):
        y = _cmac(y, H[:, :, a], x[:, a][:, None])
    return y


def _host_kron(A, G, Bt, mean):
    """H = (A G) Bt + mean, every sum from 0 in ascending index order (the kernel's order)."""
    V, nr, nt = G.shape
    T = np.zeros_like(G)
    for q in range(nr):
        T = _cmac(T, A[None, :, q][:, :, None], G[:, q, :][:, None, :])
    H = np.zeros_like(G)
    for p in range(nt):
        H = _cmac(H, T[:, :, p][:, :, None], Bt[None, p, :][:, None, :])
    return H + mean[None]


def _awgn_dev(x, scale, seed, stream):
    """cpx_awgn_dev over a flat complex array: the documented draws of the channel's G and noise."""
    flat = np.ascontiguousarray(x, dtype=np.complex128).reshape(-1)
    d_in, d_out = DeviceBuf.from_array(flat), DeviceBuf(flat.nbytes)
    _lib.check(_lib.load().cpx_awgn_dev(d_in.ptr, flat.size, scale, scale, seed, stream, d_out.ptr, None))
    _lib.check(_lib.load().cpx_stream_sync(None))
    return d_out.to_array(flat.shape, np.complex128).reshape(np.shape(x))


def _bits(rs, V, nt, nb):
    return rs.randint(0, 2, V * nt * nb).astype(np.uint8)


# ---- channel structure, exact -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nr,nt", [(4, 4), (3, 2), (2, 5)])
def test_noise_free_output_is_h_times_x(gpu, nr, nt):
    md, rs = QAMModem(16), np.random.RandomState(1)
    V = 3000
    bits = _bits(rs, V, nt, 4)
    for ch in (_rayleigh(nr, nt), _rician(nr, nt)):
        y, H = mimo_channel_gpu(ch, md, bits, seed=5, stream_id=3)
        x = md.modulate(bits).reshape(V, nt)
        assert np.array_equal(y, _host_hx(H, x))


def test_fading_is_the_documented_stream_and_kronecker_product(gpu):
    md, rs = QAMModem(4), np.random.RandomState(2)
    nr, nt, V = 4, 3, 2500
    bits = _bits(rs, V, nt, 2)
    _, G = mimo_channel_gpu(_rayleigh(nr, nt), md, bits, seed=9, stream_id=4)
    # uncorrelated, mean 0: H is G itself, the N(0, 1/2)-per-component draws of cpx_awgn_dev on stream 2 * stream_id
    assert np.array_equal(G, _awgn_dev(np.zeros((V, nr, nt), complex), SQRT_HALF, 9, 8))
    ch = _rician(nr, nt)
    _, H = mimo_channel_gpu(ch, md, bits, seed=9, stream_id=4)
    A, Bt, mean = _fading_matrices(ch)
    assert not np.allclose(A, np.eye(nr)) and not np.allclose(Bt, np.eye(nt))
    assert np.array_equal(H, _host_kron(A, G, Bt, mean))


def test_noise_is_the_documented_stream(gpu):
    md, rs = QAMModem(16), np.random.RandomState(3)
    V, s = 1 << 16, 0.8
    bits = _bits(rs, V, 4, 4)
    y, H = mimo_channel_gpu(_rayleigh(noise_std=s), md, bits, seed=2, stream_id=1)
    _, H0 = mimo_channel_gpu(_rayleigh(), md, bits, seed=2, stream_id=1)
    assert np.array_equal(H, H0)
    hx = _host_hx(H, md.modulate(bits).reshape(V, 4))
    assert np.array_equal(y, _awgn_dev(hx, s * 0.5, 2, 3))             # noise_std / 2 per component (quirk B7)
    n = (y - hx).reshape(-1)
    N = n.size
    for comp in (n.real, n.imag):
        assert abs(comp.mean()) <= 5 * (s * 0.5) / math.sqrt(N)
        assert abs(comp.std() / (s * 0.5) - 1) <= 5 / math.sqrt(2 * N)


def test_split_launch_and_streams(gpu):
    lib, md = _lib.load(), QAMModem(16)
    nr = nt = 4
    V, V1 = 5000, 1777
    ch = _rician(nr, nt)
    bits = _bits(np.random.RandomState(4), V, nt, 4)
    hs = _channel_handles(ch)

    def run(seed, s_fade, s_noise, parts):
        d_bits, d_y, d_h = DeviceBuf.from_array(bits), DeviceBuf(V * nr * 16), DeviceBuf(V * nr * nt * 16)
        for lo, hi in parts:
            at = lambda buf, stride: ctypes.c_void_p(buf.ptr.value + lo * stride)  # noqa: E731
            _lib.check(lib.cpx_mimo_channel_run_dev(hs.get(), md._device_handle(), at(d_bits, nt * 4), hi - lo, lo, 0.3, seed,
                                                    s_fade, s_noise, at(d_y, nr * 16), at(d_h, nr * nt * 16), None))
        _lib.check(lib.cpx_stream_sync(None))
        return d_y.to_array((V, nr), np.complex128).tobytes() + d_h.to_array((V, nr, nt), np.complex128).tobytes()

    whole = run(7, 10, 11, [(0, V)])
    assert whole == run(7, 10, 11, [(0, V1), (V1, V)])
    assert whole == run(7, 10, 11, [(0, V)])
    other = run(7, 12, 13, [(0, V)])
    assert other != whole
    assert np.mean(np.frombuffer(other, np.float64) != np.frombuffer(whole, np.float64)) > 0.99
    hs.drop()


def test_channel_refusals(gpu):
    md = QAMModem(16)
    with pytest.raises(ValueError):
        mimo_channel_gpu(_rayleigh(), md, np.zeros(15, np.uint8))        # not a whole vector
    real = MIMOFlatChannel(2, 2)
    real.uncorr_rayleigh_fading(float)
    real.noise_std = 0.0
    with pytest.raises(ValueError):
        mimo_channel_gpu(real, md, np.zeros(16, np.uint8))


def test_large_shape_takes_the_workspace(gpu):
    md, rs = QAMModem(4), np.random.RandomState(5)
    nr = nt = 12                                                          # 64 lanes x (2 nt + nr nt) x 16 B > 64 KB
    ch = MIMOFlatChannel(nt, nr)
    ch.expo_corr_rayleigh_fading(np.exp(0.2j), np.exp(0.1j), betat=0.3, betar=0.3)
    ch.noise_std = 0.0
    V = 700
    bits = _bits(rs, V, nt, 2)
    y, H = mimo_channel_gpu(ch, md, bits, seed=1)
    assert "mimo_channel_kernel<global>" in _lib.last_kernel()
    _, G = mimo_channel_gpu(_rayleigh(nr, nt), md, bits, seed=1)
    A, Bt, mean = _fading_matrices(ch)
    assert np.array_equal(H, _host_kron(A, G, Bt, mean))
    assert np.array_equal(y, _host_hx(H, md.modulate(bits).reshape(V, nt)))


# ---- channel statistics ------------------------------------------------------------------------------------------------------

def test_rayleigh_statistics(gpu):
    md = QAMModem(4)
    V = 1 << 20
    bits = np.zeros(V * 4 * 2, np.uint8)
    _, H = mimo_channel_gpu(_rayleigh(), md, bits, seed=11)
    h = H.reshape(V, 16)
    N = V
    bound = 5 / math.sqrt(N)
    m = h.mean(axis=0)
    assert np.all(np.abs(m.real) <= 5 * SQRT_HALF / math.sqrt(N)) and np.all(np.abs(m.imag) <= 5 * SQRT_HALF / math.sqrt(N))
    p = (np.abs(h) ** 2).mean(axis=0)                                     # Var |h|^2 = 1 for CN(0, 1)
    assert np.all(np.abs(p - 1) <= bound)
    s = (h ** 2).mean(axis=0)                                             # E h^2 = 0; each component of h^2 has variance 1/2
    assert np.all(np.abs(s.real) <= 5 * SQRT_HALF / math.sqrt(N)) and np.all(np.abs(s.imag) <= 5 * SQRT_HALF / math.sqrt(N))
    C = h.T @ h.conj() / N                                                # cross-entry E h_i conj(h_j): variance 1/N (1/2 per component)
    off = C[~np.eye(16, dtype=bool)]
    assert np.all(np.abs(off.real) <= 5 * SQRT_HALF / math.sqrt(N)) and np.all(np.abs(off.imag) <= 5 * SQRT_HALF / math.sqrt(N))
    lag = (h[1:] * h[:-1].conj()).mean(axis=0)                            # neighbouring vectors
    lim = 5 * SQRT_HALF / math.sqrt(N - 1)
    assert np.all(np.abs(lag.real) <= lim) and np.all(np.abs(lag.imag) <= lim)


def test_correlated_rician_statistics(gpu):
    md = QAMModem(4)
    V = 1 << 20
    ch = _rician()
    mean, rt, rr = ch.fading_param
    _, H = mimo_channel_gpu(ch, md, np.zeros(V * 4 * 2, np.uint8), seed=12)
    vec = H.transpose(0, 2, 1).reshape(V, 16)                            # vec(H): column after column
    C_true = np.kron(rt, rr)
    d = np.real(np.diag(C_true))
    m = vec.mean(axis=0)
    want = np.asarray(mean).T.reshape(-1)
    lim = 5 * np.sqrt(d / 2 / V)
    assert np.all(np.abs(m.real - want.real) <= lim) and np.all(np.abs(m.imag - want.imag) <= lim)
    c = vec - want
    C = c.T @ c.conj() / V
    lim = 5 * np.sqrt(np.outer(d, d) / 2 / V) + 1e-12                   # var of a sample E[x conj(y)] ~ E|x|^2 E|y|^2 / N
    assert np.all(np.abs(C.real - C_true.real) <= lim) and np.all(np.abs(C.imag - C_true.imag) <= lim)


# ---- plumbing parity ---------------------------------------------------------------------------------------------------------

def _recount(rx, nb):
    shifts = np.arange(nb - 1, -1, -1)
    bits = ((rx['idx'].reshape(-1)[:, None] >> shifts) & 1).reshape(rx['msg'].shape)
    return (bits != rx['msg']).sum(axis=1)


@pytest.mark.parametrize("detector", ["kbest", "ml"])
def test_hard_link_parity(gpu, detector):
    md = QAMModem(16)
    link = DeviceMimoLink(md, _rayleigh(), detector=detector, K=16)
    link.keep_rx = True
    errs = link.run_batch(12.0, 300)
    rx = link.last_rx
    assert errs.dtype == np.int32 and errs.shape == (300,) and errs.sum() > 0
    assert np.array_equal(errs, _recount(rx, 4))
    x = md.modulate(rx['msg'].reshape(-1)).reshape(-1, 4)
    assert np.max(np.abs(rx['y'] - _host_hx(rx['h'], x))) < 5 * rx['noise_std']   # the kept arrays belong together
    for v in np.random.RandomState(6).choice(len(rx['y']), 40, replace=False):
        if detector == 'kbest':
            want = kbest(rx['y'][v], rx['h'][v], md.constellation, 16)
        else:
            want = mimo_ml(rx['y'][v], rx['h'][v], md.constellation)
        assert np.array_equal(want, md.constellation[rx['idx'][v]])


def test_batches_use_fresh_streams(gpu):
    link = DeviceMimoLink(QAMModem(16), _rayleigh(), detector='kbest')
    link.keep_rx = True
    link.run_batch(10.0, 20)
    first = link.last_rx
    link.run_batch(10.0, 20)
    assert not np.array_equal(first['msg'], link.last_rx['msg'])
    assert not np.array_equal(first['h'], link.last_rx['h'])


def test_best_first_ldpc_link_parity(gpu):
    md, ldpc = QAMModem(16), ldpc_params("wimax1440")
    link = DeviceMimoLink(md, _rayleigh(), detector='best_first', ldpc_params=ldpc, send_chunk=1440)
    assert link.codewords_per_tx == 2 and link.vectors_per_tx == 180
    link.keep_rx = True
    errs = link.run_batch(18.0, 64)
    rx = link.last_rx
    k, n, vpt = 720, 1440, link.vectors_per_tx
    noise_var = rx['noise_std'] ** 2
    demode = lambda s: md.demodulate(s, 'hard')  # noqa: E731
    for v in np.random.RandomState(7).choice(len(rx['y']), 24, replace=False):
        want = best_first_detector(rx['y'][v], rx['h'][v], md.constellation, (1, 3, 5), noise_var, demode, 500)
        assert np.array_equal(want, rx['llr'][v])
    for t in np.random.RandomState(8).choice(64, 12, replace=False):
        llr = rx['llr'][t * vpt:(t + 1) * vpt].reshape(-1).copy()
        dec = ldpc_bp_decode(llr, ldpc, 'MSA', 15)[0]
        assert np.array_equal(dec.T, rx['dec'][2 * t:2 * t + 2])
        got = dec[:k].reshape(-1, order='F')
        assert int((got != rx['msg'][t]).sum()) == errs[t]
    # the transmitted bits are the systematic code words, block after block
    assert np.array_equal(rx['tx'].reshape(64, 2, n)[:, :, :k].reshape(64, -1), rx['msg'])


def test_kbest_soft_ldpc_link_runs(gpu):
    from commpy_amd.modulation import kbest_batch
    md, ldpc = QAMModem(16), ldpc_params("wimax1440")
    link = DeviceMimoLink(md, _rayleigh(), detector='kbest', output_type='soft', ldpc_params=ldpc)
    link.keep_rx = True
    errs = link.run_batch(16.0, 32)
    rx = link.last_rx
    llr = kbest_batch(rx['y'][:200], rx['h'][:200], md, 16, rx['noise_std'] ** 2, 'soft')
    assert np.array_equal(llr, rx['llr'][:200], equal_nan=True)
    assert errs.shape == (32,)


def test_refusals_on_device(gpu):
    md = QAMModem(16)
    with pytest.raises(ValueError):
        DeviceMimoLink(md, _rayleigh(4, 5), detector='kbest')
    with pytest.raises(ValueError):
        DeviceMimoLink(md, _rayleigh(), detector='best_first')


# ---- link_performance stop rule ----------------------------------------------------------------------------------------------

def _reference_rule(per_point_counts, n_snr, send_max, err_min, chunk):
    """links.py:269-343 restated one transmission at a time over recorded counts."""
    out = np.zeros(n_snr)
    for i in range(n_snr):
        it = iter(per_point_counts[i])
        sent = wrong = 0
        while sent < send_max and wrong < err_min:
            wrong += next(it)
            sent += chunk
        out[i] = wrong / sent
        if wrong < err_min:
            break
    return out


def test_link_performance_stop_rule_on_device(gpu):
    link = DeviceMimoLink(QAMModem(16), _rayleigh(), detector='kbest')
    link.tx_batch = 50
    record = {}
    run = link.run_batch

    def recording(snr, T):
        e = run(snr, T)
        record.setdefault(snr, []).extend(int(v) for v in e)
        return e
    link.run_batch = recording
    snrs = np.array([6.0, 12.0, 30.0])
    got = link.link_performance(snrs, 5e4, 200)
    want = _reference_rule([record.get(s, []) for s in snrs], len(snrs), 5e4, 200, link.send_chunk)
    assert np.array_equal(got, want)
    assert got[0] > 0


# ---- BER ---------------------------------------------------------------------------------------------------------------------

def test_kbest_link_meets_reference_targets(gpu):
    """test_links.py:48-59 with 20x its bit budget (5e5 -> 1e7 bits per point)."""
    md = QAMModem(16)
    link = DeviceMimoLink(md, _rayleigh(), detector='kbest', K=16, send_chunk=720)
    snrs = np.arange(0, 21, 5) + 10 * np.log10(md.num_bits_symbol)
    bers = link.ber_sweep(snrs, 10 ** 7)
    np.testing.assert_allclose(bers, (2e-1, 1e-1, 3e-2, 2e-3, 4e-5), rtol=1.25)


def test_kbest_device_and_host_links_agree(gpu):
    """Two-sample 5-sigma test on per-transmission error counts: device link vs LinkModel + mimo_receiver (NumPy channel)."""
    md = QAMModem(16)
    link = DeviceMimoLink(md, _rayleigh(), detector='kbest', K=16, send_chunk=720)
    host = LinkModel(md.modulate, _rayleigh(), mimo_receiver(md, 'kbest', 16), md.num_bits_symbol, md.constellation, md.Es)
    np.random.seed(20261015)
    for snr in 10 * np.log10(4) + np.array([5.0, 10.0]):
        _, BEs, _, _ = host.link_performance_full_metrics([snr], 600, 10 ** 12, 720, 1)
        h = BEs[0].astype(float)
        d = np.concatenate([link.run_batch(snr, 4000) for _ in range(2)]).astype(float)
        z = (h.mean() - d.mean()) / math.sqrt(h.var(ddof=1) / h.size + d.var(ddof=1) / d.size)
        assert abs(z) <= 5, (snr, h.mean(), d.mean(), z)


@pytest.mark.slow
def test_best_first_ldpc_link_meets_reference_targets(gpu):
    """test_links.py:61-86, :92-99: the third link, through link_performance with the reference's float send_max."""
    md, ldpc = QAMModem(16), ldpc_params("wimax1440")
    link = DeviceMimoLink(md, _rayleigh(), detector='best_first', stack_size=(1, 3, 5), llr_max=500, ldpc_params=ldpc,
                          ldpc_alg='MSA', ldpc_iters=15, send_chunk=720)
    snrs = np.arange(17, 20, 1)
    np.testing.assert_allclose(link.link_performance(snrs, 5e5, 200), (1.7e-1, 1e-1, 2.5e-3), rtol=2)
    np.testing.assert_allclose(link.ber_sweep(snrs, 2 * 10 ** 6), (1.7e-1, 1e-1, 2.5e-3), rtol=2)


def test_best_first_device_and_host_links_agree(gpu):
    """The same two-sample test for the LDPC-coded best-first link: LinkModel + mimo_receiver + host ldpc_bp_decode."""
    from commpy_amd.channelcoding.ldpc import triang_ldpc_systematic_encode
    md, ldpc = QAMModem(16), ldpc_params("wimax1440")
    link = DeviceMimoLink(md, _rayleigh(), detector='best_first', ldpc_params=ldpc, send_chunk=720)

    def modulate(bits):
        return md.modulate(triang_ldpc_systematic_encode(bits, ldpc, False).reshape(-1, order='F'))

    def decoder(llrs):
        return ldpc_bp_decode(llrs, ldpc, 'MSA', 15)[0][:720].reshape(-1, order='F')
    host = LinkModel(modulate, _rayleigh(), mimo_receiver(md, 'best_first'), md.num_bits_symbol, md.constellation, md.Es,
                     decoder, 0.5)
    np.random.seed(20261016)
    for snr in (17.0, 18.0):
        _, BEs, _, _ = host.link_performance_full_metrics([snr], 800, 10 ** 12, 720, 0.5)
        h = BEs[0].astype(float)
        d = link.run_batch(snr, 8000).astype(float)
        z = (h.mean() - d.mean()) / math.sqrt(h.var(ddof=1) / h.size + d.var(ddof=1) / d.size)
        assert abs(z) <= 5, (snr, h.mean(), d.mean(), z)
