"""Iterative detection and decoding on the MI355X (csrc/mimo_idd.hip, DeviceMimoLink(idd_iters=...)): the list detector with
priors against the reference's max_log_approx and the NumPy model (tests/golden/idd.npz), its edge semantics, bit-identity across
batch sizes, positions and streams, the fused exchange against the staged composition, the loop against the reference's
idd_decoder, the device link against links.idd_decoder one transmission at a time, and the bit errors with and without IDD."""
import ctypes

import numpy as np
import pytest

from commpy_amd import _lib
from commpy_amd.channelcoding.ldpc import ldpc_bp_decode
from commpy_amd.channels import MIMOFlatChannel
from commpy_amd.devicelink import DeviceBuf, DeviceMimoLink
from commpy_amd.links import idd_decoder
from commpy_amd.modulation import Modem, QAMModem, apriori_detector, kbest_batch, list_apriori_batch
from helpers import ldpc_params
from test_idd_host import DET_CASES, G, list_model

pytestmark = pytest.mark.gpu
Q16 = QAMModem(16)


def _rayleigh(nr=4, nt=4):
    ch = MIMOFlatChannel(nt, nr)
    ch.uncorr_rayleigh_fading(complex)
    return ch


def _assert_llr(got, want):
    """The bound tests/test_mimo_gpu.py uses for K-best soft LLRs."""
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.array_equal(np.where(np.isfinite(want), 0, got), np.where(np.isfinite(want), 0, want), equal_nan=True)
    fin = np.isfinite(want)
    assert np.all(np.abs(got[fin] - want[fin]) <= 1e-9 * np.maximum(1, np.abs(want[fin])))


def _same_bits(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _case(case):
    g = lambda k: G["det_%s_%s" % (case, k)]  # noqa: E731
    return g, Modem(g("const"), reorder_as_gray=False), int(g("K")), float(g("noise_var")), float(g("clip"))


def _vectors(rs, n, nr=4, nt=4, md=Q16, noise=0.5):
    h = (rs.randn(n, nr, nt) + 1j * rs.randn(n, nr, nt)) / np.sqrt(2)
    x = md.constellation[rs.randint(0, md.m, (n, nt))]
    y = np.einsum('vrt,vt->vr', h, x) + noise * (rs.randn(n, nr) + 1j * rs.randn(n, nr)) / np.sqrt(2)
    return y, h


class _Dev:
    """The device entry points on explicit buffers: search the list, compute its distances, then any number of passes."""

    def __init__(self, md, y, h, K, stream=None):
        self.lib, self.md, self.stream = _lib.load(), md, stream
        self.B, self.nr = y.shape
        self.nt = h.shape[-1]
        self.nbt = self.nt * md.num_bits_symbol
        self.Ke = min(K, md.m ** self.nt)
        self.bufs = [DeviceBuf.from_array(np.ascontiguousarray(y, dtype=np.complex128)),
                     DeviceBuf.from_array(np.ascontiguousarray(h, dtype=np.complex128))]
        self.cand, self.count = DeviceBuf(self.B * self.Ke * self.nt * 4), DeviceBuf(self.B * 4)
        self.dist = DeviceBuf(self.B * self.Ke * 8)
        hd = md._device_handle()
        _lib.check(self.lib.cpx_kbest_list_dev(hd, self.bufs[0].ptr, self.bufs[1].ptr, 1, self.B, self.nr, self.nt, K, self.cand.ptr,
                                               self.count.ptr, stream))
        _lib.check(self.lib.cpx_mimo_list_dist_dev(hd, self.bufs[0].ptr, self.bufs[1].ptr, 1, self.B, self.nr, self.nt, self.cand.ptr,
                                                   self.count.ptr, self.Ke, self.dist.ptr, stream))

    def llr(self, prior, nv, clip):
        d_prior = None if prior is None else DeviceBuf.from_array(np.ascontiguousarray(prior, dtype=np.float64))
        out = DeviceBuf(self.B * self.nbt * 8)
        _lib.check(self.lib.cpx_mimo_list_llr_dev(self.md._device_handle(), self.cand.ptr, self.count.ptr, self.dist.ptr, self.B, self.nt,
                                                  self.Ke, None if d_prior is None else d_prior.ptr, nv, clip, out.ptr, self.stream))
        _lib.check(self.lib.cpx_stream_sync(self.stream))
        return out.to_array((self.B, self.nbt), np.float64)

    def exchange(self, a, dec_out, nv, clip, last):
        d_a, d_o = DeviceBuf.from_array(np.ascontiguousarray(a)), DeviceBuf.from_array(np.ascontiguousarray(dec_out))
        _lib.check(self.lib.cpx_mimo_idd_exchange_dev(self.md._device_handle(), self.cand.ptr, self.count.ptr, self.dist.ptr, self.B,
                                                      self.nt, self.Ke, d_a.ptr, d_o.ptr, nv, clip, int(last), self.stream))
        _lib.check(self.lib.cpx_stream_sync(self.stream))
        return d_a.to_array((self.B, self.nbt), np.float64)


# ---- 1. zero prior, clip = inf: max_log_approx and cpx_kbest_soft ------------------------------------------------------------------

@pytest.mark.parametrize("case", DET_CASES)
def test_zero_prior_is_kbest_soft(gpu, case):
    g, md, K, nv, _ = _case(case)
    y, h = g("y"), g("h")
    with np.errstate(divide="ignore", invalid="ignore"):
        none = list_apriori_batch(y, h, md, K, nv, None, np.inf)
        zero = list_apriori_batch(y, h, md, K, nv, np.zeros_like(g("ref")), np.inf)
        soft = kbest_batch(y, h, md, K, nv, 'soft')
    _assert_llr(none, g("ref"))
    assert _same_bits(none, soft) and _same_bits(zero, soft)


# ---- 2. priors ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", DET_CASES)
def test_priors_match_the_model(gpu, case):
    g, md, K, nv, clip = _case(case)
    got = list_apriori_batch(g("y"), g("h"), md, K, nv, g("prior"), clip)
    _assert_llr(got, g("post"))
    # the device's own list is the reference's (as sets: the order within a list does not enter the LLRs)
    dev = _Dev(md, g("y"), g("h"), K)
    cand, count = dev.cand.to_array((dev.B, dev.Ke, dev.nt), np.int32), dev.count.to_array((dev.B,), np.int32)
    assert np.array_equal(count, g("count"))
    for i in range(dev.B):
        assert sorted(map(tuple, cand[i, :count[i]])) == sorted(map(tuple, g("cand")[i, :count[i]].astype(int)))
    # +-clip where a bit value has no candidate, and only there or where the model clips too
    labels = g("labels")
    for i in range(dev.B):
        bits = labels[cand[i, :count[i]]].reshape(count[i], -1)
        assert np.all(got[i][bits.all(axis=0)] == -clip) and np.all(got[i][~bits.any(axis=0)] == clip)
    if case == "qam16_4x4":
        assert any((labels[cand[i, :count[i]]].reshape(count[i], -1).all(axis=0)).any() for i in range(dev.B))


def test_priors_beyond_the_clip_act_as_the_clip(gpu):
    g, md, K, nv, clip = _case("qam16_4x4")
    prior = g("prior") * 10
    assert (np.abs(prior) > clip).mean() > 0.2
    assert _same_bits(list_apriori_batch(g("y"), g("h"), md, K, nv, prior, clip),
                      list_apriori_batch(g("y"), g("h"), md, K, nv, np.clip(prior, -clip, clip), clip))
    inf = np.where(prior > 0, np.inf, -np.inf)
    assert _same_bits(list_apriori_batch(g("y"), g("h"), md, K, nv, inf, clip),
                      list_apriori_batch(g("y"), g("h"), md, K, nv, np.where(prior > 0, clip, -clip), clip))


def test_nan_vectors_stay_alone(gpu):
    g, md, K, nv, clip = _case("qam16_4x4")
    y, h, prior = g("y").copy(), g("h").copy(), g("prior").copy()
    clean = list_apriori_batch(y, h, md, K, nv, prior, clip)
    y[3, 1] = np.nan
    h[10, 2, 3] = np.nan + 0j
    prior[17, 5] = np.nan
    h[40, 0, 0] = complex(0.0, np.nan)
    got = list_apriori_batch(y, h, md, K, nv, prior, clip)
    bad = np.zeros(len(y), bool)
    bad[[3, 10, 17, 40]] = True
    assert np.isnan(got[bad]).all()
    assert _same_bits(got[~bad], clean[~bad])


def test_full_list_is_brute_force_max_log_map(gpu):
    rs = np.random.RandomState(11)
    md = QAMModem(4)
    nr = nt = 4
    y, h = _vectors(rs, 50, nr, nt, md, 0.7)
    prior = rs.randn(50, 8) * 3
    nv, clip = 0.4, 500.0
    got = list_apriori_batch(y, h, md, 4 ** nt, nv, prior, clip)
    again = list_apriori_batch(y, h, md, 10 ** 6, nv, prior, clip)                   # K above m^nt is m^nt
    assert _same_bits(got, again)
    hyp = np.stack(np.meshgrid(*[np.arange(4)] * nt, indexing='ij'), axis=-1).reshape(-1, nt)
    labels = ((np.arange(4)[:, None] >> np.arange(1, -1, -1)) & 1).astype(np.uint8)
    want = np.array([list_model(y[i], h[i], md.constellation, labels, hyp, prior[i], nv, clip) for i in range(50)])
    _assert_llr(got, want)
    assert np.all(np.abs(got) < clip)                                                 # every bit value has a candidate


# ---- 3. bit-identity across batch sizes, positions and streams -----------------------------------------------------------------------

def test_bit_identical_across_batches_positions_and_streams(gpu):
    rs = np.random.RandomState(12)
    n = 270000                # above 16384 workgroups of 4 vectors and of 16 lists: both kernels stride over their grids
    y, h = _vectors(rs, n)
    prior = rs.randn(n, 16) * 20
    nv, clip, K = 0.3, 500.0, 16
    whole = list_apriori_batch(y, h, Q16, K, nv, prior, clip)
    assert "4 vectors per wave" in _lib.last_kernel()
    for B in (1, 3, 4, 5, 63, 64, 65, 1000):                                          # a wave holds 4 vectors here
        for lo in (0, 7, 65537, n - B):
            part = list_apriori_batch(y[lo:lo + B], h[lo:lo + B], Q16, K, nv, prior[lo:lo + B], clip)
            assert _same_bits(part, whole[lo:lo + B]), (B, lo)
    perm = rs.permutation(n)[:2000]
    assert _same_bits(list_apriori_batch(y[perm], h[perm], Q16, K, nv, prior[perm], clip), whole[perm])
    lib = _lib.load()
    stream = ctypes.c_void_p()
    _lib.check(lib.cpx_stream_create(ctypes.byref(stream)))
    try:
        assert _same_bits(_Dev(Q16, y[:5000], h[:5000], K, stream).llr(prior[:5000], nv, clip), whole[:5000])
        assert _same_bits(_Dev(Q16, y, h, K, stream).llr(prior, nv, clip), whole)
    finally:
        _lib.check(lib.cpx_stream_destroy(stream))
    # other group widths: 8 bits with a 256-candidate list (one vector per wave), 4 bits with 4 candidates (16 per wave)
    for md, nr, nt, K2, per_wave in ((QAMModem(4), 4, 4, 256, 1), (QAMModem(4), 2, 2, 4, 16)):
        y2, h2 = _vectors(rs, 300, nr, nt, md)
        p2 = rs.randn(300, nt * 2) * 5
        full = list_apriori_batch(y2, h2, md, K2, nv, p2, clip)
        assert "%d vectors per wave" % per_wave in _lib.last_kernel()
        for lo, B in ((0, 1), (per_wave - 1, 2), (100, per_wave + 1), (299, 1)):
            assert _same_bits(list_apriori_batch(y2[lo:lo + B], h2[lo:lo + B], md, K2, nv, p2[lo:lo + B], clip), full[lo:lo + B])


# ---- 4. the fused exchange is the staged composition ---------------------------------------------------------------------------------

@pytest.mark.parametrize("last", [0, 1])
def test_exchange_is_the_staged_composition(gpu, last):
    rs = np.random.RandomState(13)
    n = 3001
    y, h = _vectors(rs, n)
    a = np.clip(rs.randn(n, 16) * 200, -500, 500)
    dec_out = a + rs.randn(n, 16) * rs.choice([1.0, 50.0, 600.0], (n, 1))
    nv, clip = 0.3, 500.0
    dev = _Dev(Q16, y, h, 16)
    ext = dec_out - a
    post = dev.llr(ext, nv, clip)
    want = post if last else post - ext
    assert _same_bits(dev.exchange(a, dec_out, nv, clip, last), want)
    assert "idd_exchange_kernel" in _lib.last_kernel()


def test_llr_hard_is_signbit(gpu):
    """cpx_mimo_llr_hard_dev, the 'hard' decision of the link: np.signbit of every LLR, -0.0 and NaNs of either sign included."""
    lib = _lib.load()
    rs = np.random.RandomState(14)
    llr = rs.randn(5 * 10 ** 6 + 3) * 10                                              # above 16384 workgroups of 256
    llr[:8] = [0.0, -0.0, np.inf, -np.inf, np.nan, -np.nan, 5e-324, -5e-324]
    d_llr, d_bits = DeviceBuf.from_array(llr), DeviceBuf(llr.size)
    _lib.check(lib.cpx_mimo_llr_hard_dev(d_llr.ptr, llr.size, d_bits.ptr, None))
    _lib.check(lib.cpx_stream_sync(None))
    assert np.array_equal(d_bits.to_array((llr.size,), np.int8), np.signbit(llr).astype(np.int8))
    assert lib.cpx_mimo_llr_hard_dev(d_llr.ptr, -1, d_bits.ptr, None) == _lib.CPX_EINVAL
    assert lib.cpx_mimo_llr_hard_dev(None, 4, d_bits.ptr, None) == _lib.CPX_EINVAL


def test_noise_var_must_be_positive_and_finite(gpu):
    g, md, K, nv, clip = _case("qpsk_2x2")
    dev = _Dev(md, g("y"), g("h"), K)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            dev.llr(g("prior"), bad, clip)


# ---- 5. the loop against the reference's idd_decoder -------------------------------------------------------------------------------

def _device_loop(y, h, md, K, nv, clip, code, n_it, ldpc_iters=15):
    """The sequence DeviceMimoLink runs, on given y [V, nr] and h [V, nr, nt] holding whole codewords: final LLRs [V, nt nb]."""
    lib, dev = _lib.load(), _Dev(md, y, h, K)
    n = code['n_vnodes']
    B = dev.B * dev.nbt // n
    from commpy_amd.channelcoding.ldpc import _device_code
    a, out, dec = DeviceBuf(B * n * 8), DeviceBuf(B * n * 8), DeviceBuf(B * n)
    hd = md._device_handle()
    _lib.check(lib.cpx_mimo_list_llr_dev(hd, dev.cand.ptr, dev.count.ptr, dev.dist.ptr, dev.B, dev.nt, dev.Ke, None, nv, clip, a.ptr, None))
    for it in range(n_it):
        _lib.check(lib.cpx_ldpc_bp_decode_batch_bm_dev(_device_code(code), a.ptr, B, 1, ldpc_iters, dec.ptr, out.ptr, None, None))
        _lib.check(lib.cpx_mimo_idd_exchange_dev(hd, dev.cand.ptr, dev.count.ptr, dev.dist.ptr, dev.B, dev.nt, dev.Ke, a.ptr, out.ptr,
                                                 nv, clip, int(it == n_it - 1), None))
    _lib.check(lib.cpx_stream_sync(None))
    return a.to_array((dev.B, dev.nbt), np.float64)


@pytest.mark.parametrize("n_it", [1, 2, 3])
def test_loop_matches_the_reference_chain(gpu, n_it):
    y, h, want = G["loop_y"], G["loop_h"], G["loop_final_it%d" % n_it]
    T, V = y.shape[:2]
    nv, clip, K, sens = float(G["loop_noise_var"]), float(G["loop_clip"]), int(G["loop_K"]), float(G["idd_llr_sensitivity"])
    got = _device_loop(y.reshape(T * V, -1), h.reshape(T * V, 4, 4), Q16, K, nv, clip, ldpc_params("wimax1440"), n_it,
                       int(G["loop_ldpc_iters"])).reshape(T, -1)
    dev = np.abs(got - want)
    print("n_it %d: max |LLR - golden| %.3e (sensitivity %.3e)" % (n_it, dev.max(), sens))
    assert np.array_equal(np.signbit(got), np.signbit(want))                          # the decisions, exactly
    assert np.all(dev <= 4 * sens + 1e-9 * np.abs(want))


# ---- 6. the device link against links.idd_decoder --------------------------------------------------------------------------------

@pytest.mark.parametrize("n_it,decision", [(1, 'hard'), (2, 'decode'), (3, 'hard')])
def test_link_equals_idd_decoder_one_by_one(gpu, n_it, decision):
    ldpc = ldpc_params("wimax1440")
    link = DeviceMimoLink(Q16, _rayleigh(), detector='kbest', K=16, output_type='soft', ldpc_params=ldpc, send_chunk=1440, seed=5,
                          idd_iters=n_it, idd_decision=decision)
    link.keep_rx = True
    T = 6
    errs = link.run_batch(15.0, T)
    rx = link.last_rx
    assert rx['idd_llr'].shape == (T * 180, 16) and rx['cand'].shape == (T * 180, 16, 4) and np.all(rx['count'] == 16)
    nv, vpt, k, n = rx['noise_std'] ** 2, link.vectors_per_tx, 720, 1440
    det = apriori_detector(Q16, 16)

    def decoder(llrs):
        return ldpc_bp_decode(llrs, ldpc, 'MSA', 15)[1].reshape(-1, order='F')

    for t in range(T):
        y, h = rx['y'][t * vpt:(t + 1) * vpt], rx['h'][t * vpt:(t + 1) * vpt]
        first = list_apriori_batch(y, h, Q16, 16, nv, None, 500.0).reshape(-1)
        final = []
        idd_decoder(det, decoder, lambda llrs: final.append(llrs.copy()), n_it)(y, h, Q16.constellation, nv, first, 16)
        if decision == 'decode':
            dec = np.asarray(ldpc_bp_decode(final[0].copy(), ldpc, 'MSA', 15)[0]).T.reshape(-1, n)
        else:
            dec = np.signbit(final[0]).reshape(-1, n)
        got = dec[:, :k].reshape(-1)
        assert int((got != rx['msg'][t]).sum()) == errs[t], t
        np.testing.assert_allclose(rx['idd_llr'][t * vpt:(t + 1) * vpt].reshape(-1), final[0], rtol=1e-9, atol=1e-9)
    assert errs.sum() > 0


# ---- 7. idd_iters = 0 is the link as it was ----------------------------------------------------------------------------------------

def test_zero_rounds_is_the_one_pass_link(gpu):
    ldpc = ldpc_params("wimax1440")
    kw = dict(detector='kbest', K=16, output_type='soft', ldpc_params=ldpc, seed=3)
    plain = DeviceMimoLink(Q16, _rayleigh(), **kw)
    zero = DeviceMimoLink(Q16, _rayleigh(), idd_iters=0, idd_clip=7.0, idd_decision='hard', **kw)
    for snr in (14.0, 16.0):
        assert np.array_equal(plain.run_batch(snr, 200), zero.run_batch(snr, 200))


# ---- 8. IDD does not lose to one pass ----------------------------------------------------------------------------------------------

def test_three_rounds_do_not_lose_to_one_pass(gpu):
    """4x4 16-QAM, K = 16, WiMAX (1440, 720), MSA 15 iterations, 18 dB, seed 1, 2048 codewords, the same channel draws for both
    links.  18 dB is where the one-pass link's block error rate lies between 0.1 and 0.9 (asserted below; the reference's own
    chain on the host gave 24 of 40 blocks in error at 18 dB, 36 of 40 at 17 dB, 14 of 40 at 19 dB).

    The IDD link runs with ``idd_clip=inf``, for a reason that does not depend on the device code: the exchange writes
    ``a = posterior - ext`` with the UNCLIPPED ext while the detector saw ext clipped to +-clip, so wherever the decoder's
    extrinsic exceeds the clip (min-sum sums reach several times its own +-500) ``a`` is off by ``|ext| - clip`` against the
    decoder's own opinion.  Only a clip above every extrinsic makes ``posterior - ext`` the detector's extrinsic.  On the
    reference's chain (NumPy model + the reference's ldpc_bp_decode, 40 codewords at 18 dB) three rounds gave 3747 bit errors
    with clip 500 and 296 with clip inf against 1177 for one pass."""
    ldpc = ldpc_params("wimax1440")
    kw = dict(detector='kbest', K=16, output_type='soft', ldpc_params=ldpc, seed=1)
    one = DeviceMimoLink(Q16, _rayleigh(), **kw).run_batch(18.0, 2048)
    idd = DeviceMimoLink(Q16, _rayleigh(), idd_iters=3, idd_clip=float('inf'), idd_decision='decode', **kw).run_batch(18.0, 2048)
    bler = float(np.mean(one > 0))
    print("18 dB, 2048 codewords: one pass %d bit errors (BLER %.3f), idd_iters=3 %d bit errors (BLER %.3f)"
          % (one.sum(), bler, idd.sum(), float(np.mean(idd > 0))))
    assert 0.1 <= bler <= 0.9
    assert idd.sum() <= one.sum()
