"""GPU-resident coded link: the whole Monte-Carlo chain of BASELINE config 5 on the device.

``DeviceWifiLink`` runs, per batch of transmissions and without leaving HBM,

    random bits -> conv_encode('cont') -> puncturing -> modulate -> AWGN -> soft demodulation
                -> depuncturing -> soft Viterbi -> per-chunk error count

with the semantics of the reference's ``Wifi80211.link_performance`` chain
(/root/reference/commpy/wifi80211.py:132-216, links.py:155-267, channels.py:37-74), including quirk B7
(complex noise of per-component std ``noise_std/2`` while the demodulator is told ``noise_std**2``) and
quirk B1 (decimal generators) unless ``generator_matrix`` is given.  Only the error counters come back
to the host.  The random streams are not NumPy's MT19937 draws: they are an exactly specified function of
(seed, stream id, element index) (Philox4x32-10; include/commpy_amd.h, "Random streams"), tested against the NumPy
model tests/rng_model.py, so BERs agree with the reference's in distribution, not bit for bit.  Call number c of a link
(1, 2, ...) draws its message bits on stream 2 c and its noise on stream 2 c + 1; the deterministic stages are
bit-exact (tests/test_devicelink_gpu.py).

``DeviceMimoLink`` does the same for a MIMO link over a ``MIMOFlatChannel`` (bits -> [LDPC encode] -> Kronecker fading channel ->
ML / K-best / best-first detector -> [LDPC decode] -> error count), the device counterpart of ``LinkModel`` with ``mimo_receiver``;
with ``idd_iters`` it closes the loop between a list detector with priors and the LDPC decoder (``links.idd_decoder`` on the device).

``DeviceBscLink`` is BASELINE config 1 (hard-decision Viterbi over a BSC).  The two sweep rules the links share are
``_fixed_budget_ber`` and ``_sequential_ber``.  ``DeviceBuf``, the one-shot ``*_gpu`` host conveniences and ``LdpcEncoder`` live in
``commpy_amd.deviceops`` and are re-exported here.
"""
import ctypes
import math
import operator
from fractions import Fraction

import numpy as np

from commpy_amd import _lib
from commpy_amd.deviceops import (DeviceBuf, LdpcEncoder, _channel_handles, _encoded_length, _fading_matrices,  # noqa: F401
                                  _OneShot, _require_complex, bec_gpu, bsc_gpu, conv_encode_gpu, depuncture_indices,
                                  depuncturing_gpu, gf2_generator, mimo_channel_gpu, modulate_gpu, puncture_indices,
                                  puncturing_gpu, triang_ldpc_systematic_encode_gpu, turbo_encode_gpu)
from commpy_amd.wifi80211 import Wifi80211

__all__ = ['DeviceBuf', 'DeviceWifiLink', 'DeviceBscLink', 'DeviceMimoLink', 'conv_encode_gpu', 'modulate_gpu', 'bsc_gpu', 'bec_gpu',
           'mimo_channel_gpu', 'puncturing_gpu', 'depuncturing_gpu', 'puncture_indices', 'depuncture_indices', 'turbo_encode_gpu',
           'LdpcEncoder', 'gf2_generator', 'triang_ldpc_systematic_encode_gpu']


def _viterbi_geometry(length, trellis, tb_depth=None):
    """(L, n_steps, tb_depth) of a ``cpx_viterbi_decode_batch_dev`` call on codewords of ``length`` received values
    (convcode.py:694-702, 721).  ``L`` is ``int(length * k / n)``, a product and a quotient: ``convcode._viterbi_sizes`` multiplies
    by the rounded ``k / n`` instead, which is one less for some lengths when n = 3, and the links keep the sizes they always had."""
    k, n, m = trellis.k, trellis.n, trellis.total_memory
    L = int(length * k / n)
    n_steps = int((L + m) / k) - 1
    return L, n_steps, min(5 * m, L) if tb_depth is None else int(tb_depth)


def _buffer_set(link, key, build):
    """``link._bufs`` for the batch shape ``key``: kept when it was built for that key; otherwise its ``DeviceBuf``s are freed
    and ``build()``'s dict takes its place."""
    if link._bufs.get('key') != key:
        for b in link._bufs.values():
            if isinstance(b, DeviceBuf):
                b.free()
        link._bufs = dict(build(), key=key)
    return link._bufs


class DeviceBscLink:
    """BASELINE config 1 end to end in HBM: random messages -> conv_encode('term') -> BSC(p) -> hard-decision Viterbi -> bit errors
    (the loop of /root/reference/commpy/channelcoding/tests/test_convcode.py:133-178 with channels.py:652-673 as the channel).
    Call number c draws its messages on stream 2 c and its flips on stream 2 c + 1 of ``seed`` (tests/rng_model.py)."""

    def __init__(self, trellis, block_bits=64, tb_depth=None, seed=1):
        self.lib = _lib.load()
        _lib.require_device()
        if trellis.k != 1:
            raise ValueError('DeviceBscLink: k = 1 codes')
        self.trellis, self.nbits, self.seed = trellis, int(block_bits), int(seed)
        self.ncoded = _encoded_length(self.nbits, trellis, 'term')
        self.L, self.n_steps, self.tb = _viterbi_geometry(self.ncoded, trellis, tb_depth)
        self._calls = 0
        self._bufs = {}

    def buffers(self, B):
        return _buffer_set(self, B, lambda: {
            'msg': DeviceBuf(B * self.nbits), 'coded': DeviceBuf(B * self.ncoded), 'rx': DeviceBuf(B * self.ncoded * 8),
            'dec': DeviceBuf(B * self.L), 'errs': DeviceBuf(B * 4)})

    def generate(self, p_t, B):
        """Messages, codewords and the channel output (float64 0.0 / 1.0) of ``B`` blocks, left on the device."""
        lib, bufs, ck = self.lib, self.buffers(B), _lib.check
        self._calls += 1
        rsc = self.trellis.code_type == 'rsc'
        ck(lib.cpx_random_bits_dev(bufs['msg'].ptr, B * self.nbits, self.seed, 2 * self._calls, None))
        ck(lib.cpx_conv_encode_batch_dev(self.trellis._device_handle(), bufs['msg'].ptr, B, self.nbits, 1, int(rsc),
                                         bufs['coded'].ptr, self.ncoded, None))
        ck(lib.cpx_bsc_dev(bufs['coded'].ptr, B * self.ncoded, float(p_t), self.seed, 2 * self._calls + 1, None, bufs['rx'].ptr, None))
        return bufs

    def decode(self, B):
        lib, bufs = self.lib, self.buffers(B)
        _lib.check(lib.cpx_viterbi_decode_batch_dev(self.trellis._device_handle(), bufs['rx'].ptr, B, self.ncoded, self.L,
                                                    self.n_steps, self.tb, 0, bufs['dec'].ptr, None))

    def run_batch(self, p_t, B):
        """Bit errors per block (int32 ``[B]``) of ``B`` transmissions over a BSC with transition probability ``p_t``."""
        lib, bufs = self.lib, self.generate(p_t, B)
        self.decode(B)
        _lib.check(lib.cpx_count_errors_dev(bufs['msg'].ptr, self.nbits, bufs['dec'].ptr, self.L, B, 1, self.nbits,
                                            bufs['errs'].ptr, None))
        _lib.check(lib.cpx_stream_sync(None))
        return bufs['errs'].to_array((B,), np.int32)


class DeviceWifiLink:
    """BER of an 802.11 MCS over AWGN, simulated entirely on the GPU.

    Parameters mirror ``Wifi80211``: ``mcs`` 0..9, optional ``generator_matrix`` (default: the reference's
    decimal ``(133, 171)``, quirk B1).  ``send_chunk`` is the frame length in information bits (rounded
    like links.py:212-214), ``frame_aggregation`` the number of frames per transmission.
    """

    def __init__(self, mcs, send_chunk=600, frame_aggregation=1, generator_matrix=None, seed=1, fused=None):
        """``fused``: None = use the fused front-end kernel (``cpx_link_front_*``: bits ... depuncturing in one launch per point)
        where the library supports the combination, the staged kernels otherwise; False = staged kernels only; True = fused or
        ``ValueError``.  Both produce the same bits and LLRs (same counter-based streams, same arithmetic)."""
        self._plan(mcs, send_chunk, frame_aggregation, generator_matrix)
        self.seed = int(seed)
        self._calls = 0
        self._bufs = {}
        self._front = None
        self.keep_rx = False                                          # tests: the fused launch also stores the noisy symbols (bufs['rx'])
        self.front_reason = 'fused=False'
        # device state, only once every argument has been accepted
        self.lib = _lib.load()
        _lib.require_device()
        if fused is None or fused:
            self._make_front(bool(fused))

    # -- the plan: every size and index map, no device --------------------------------------------------------------------------
    def _plan(self, mcs, send_chunk, frame_aggregation, generator_matrix):
        self.wifi = Wifi80211(mcs, generator_matrix=generator_matrix)
        self.trellis = self.wifi._get_trellis()
        self.modem = self.wifi.get_modem()
        self.coding = self.wifi._get_coding()
        self.rate = self.coding[0] / self.coding[1]
        divider = (Fraction(1, self.modem.num_bits_symbol) * 1 / Fraction(self.rate).limit_denominator(100)).denominator
        self.send_chunk = max(divider, send_chunk // divider * divider)
        self.agg = int(frame_aggregation)
        self.nbits = self.send_chunk * self.agg                       # information bits per transmission
        # index maps of puncturing / depuncturing (vector form of convcode.py:752-804)
        self.ncoded = 2 * self.nbits                                  # rate-1/2 mother code, 'cont'
        pvec = Wifi80211._get_puncture_matrix(*self.coding)
        if pvec is None:
            self.keep_idx = self.de_idx = None
            self.ntx = self.nde = self.ncoded
        else:
            self.keep_idx = puncture_indices(self.ncoded, pvec)
            self.ntx = len(self.keep_idx)
            self.nde = math.ceil(self.ntx * self.coding[0] / self.coding[1] * 2)
            self.de_idx = depuncture_indices(self.nde, pvec, self.ntx)
        if self.ntx % self.modem.num_bits_symbol:
            raise ValueError('send_chunk does not give an integer number of symbols')
        self.nsym = self.ntx // self.modem.num_bits_symbol

    def noise_std(self, snr_db):
        """channels.py:74 for a complex channel: sqrt(2 Es / (rate 10^(SNR/10))); the noise has per-component std ``noise_std / 2``."""
        return math.sqrt(2.0 * self.modem.Es / (self.rate * 10 ** (float(snr_db) / 10.0)))

    def _make_front(self, required):
        """The plan of the fused front end (``_front``: its handles, one per device), or the reason why the staged kernels stay
        (``front_reason``).  The plan of the current device is created here: whether the library takes the combination at all
        (CPX_ELIMIT) is known only then."""
        pos = None
        if self.de_idx is not None:
            pos = np.flatnonzero(self.de_idx >= 0).astype(np.int32)         # decoder-input position of transmitted bit t
            if len(pos) != self.ntx:
                self.front_reason = 'depuncturing leaves %d of %d transmitted bits unused' % (self.ntx - len(pos), self.ntx)
                if required:
                    raise ValueError(self.front_reason)
                return
        keep = self.keep_idx                                                # int32, like pos: what cpx_link_front_create reads
        lib, trellis, modem, nbits, ntx, nde = self.lib, self.trellis, self.modem, self.nbits, self.ntx, self.nde
        rc = [_lib.CPX_OK]

        def create():                     # no reference to the link: its buffers are freed when the last reference to it goes
            h = ctypes.c_void_p()
            rc[:] = [lib.cpx_link_front_create(trellis._device_handle(), modem._device_handle(), nbits,
                                               None if keep is None else _lib.ptr(keep), ntx,
                                               None if pos is None else _lib.ptr(pos), nde, ctypes.byref(h))]
            _lib.check(rc[0])
            return h
        front = _lib.DeviceHandles(create, 'cpx_link_front_destroy')
        try:
            front.get()
        except ValueError:
            if rc[0] != _lib.CPX_ELIMIT or required:
                raise
            self.front_reason = _lib.last_error()
            return
        self._front = front
        self.front_reason = None

    def _front_end(self, T, noise_std, calls, d_msg, d_llr, d_rx=None):
        """One launch for the stages in front of the decoder; False when this call has to take the staged kernels (a
        non-default demodulator mode or precision)."""
        self.front_last_kernel = 'staged'
        if self._front is None:
            return False
        rc = self.lib.cpx_link_front_run_dev(self._front.get(), T, noise_std ** 2, noise_std * 0.5, noise_std * 0.5, 1.0, self.seed,
                                             2 * calls, 2 * calls + 1, d_msg, d_llr, d_rx, None)
        if rc == _lib.CPX_ELIMIT:
            return False
        _lib.check(rc)
        self.front_last_kernel = _lib.last_kernel()
        return True

    def _staged_front(self, T, noise_std, calls, d_msg, d_llr, d_rx):
        """The stages in front of the decoder as one kernel each (what the fused kernel replaces): messages to ``d_msg``, noisy
        symbols to ``d_rx`` (which may be ``bufs['sym']`` itself: the noise is then added in place), the decoder's LLRs to ``d_llr``."""
        lib, ck, bufs = self.lib, _lib.check, self._bufs
        h_tr, h_md = self.trellis._device_handle(), self.modem._device_handle()
        punctured = self.keep_idx is not None
        ck(lib.cpx_random_bits_dev(d_msg, T * self.nbits, self.seed, 2 * calls, None))
        ck(lib.cpx_conv_encode_batch_dev(h_tr, d_msg, T, self.nbits, 0, 0, bufs['coded'].ptr, self.ncoded, None))
        tx = bufs['coded']
        if punctured:
            ck(lib.cpx_gather_u8_dev(bufs['coded'].ptr, T, self.ncoded, bufs['keep_idx'].ptr, self.ntx, bufs['tx'].ptr, None))
            tx = bufs['tx']
        ck(lib.cpx_modulate_dev(h_md, tx.ptr, T * self.nsym, bufs['sym'].ptr, None))
        ck(lib.cpx_awgn_dev(bufs['sym'].ptr, T * self.nsym, noise_std * 0.5, noise_std * 0.5, self.seed, 2 * calls + 1, d_rx, None))
        ck(lib.cpx_demod_soft_dev(h_md, d_rx, T * self.nsym, noise_std ** 2, bufs['llr'].ptr if punctured else d_llr, None))
        if punctured:
            ck(lib.cpx_gather_f64_dev(bufs['llr'].ptr, T, self.ntx, bufs['de_idx'].ptr, self.nde, d_llr, None))

    def front_sample(self, nf, snr_db, calls):
        """Tests / benchmarks: the first ``nf`` transmissions of the point that was generated with call number ``calls`` at ``snr_db``,
        once more, this time with the noisy symbols stored -- (msg [nf, nbits] uint8, rx [nf, nsym] complex, llr [nf, nde] float64).
        The streams are counter based, so these are the values the sweep's own launch produced for those transmissions."""
        if self._front is None:
            raise ValueError('no fused front end: ' + str(self.front_reason))
        with _OneShot() as dev:
            d_msg, d_llr, d_rx = dev.alloc(nf * self.nbits), dev.alloc(nf * self.nde * 8), dev.alloc(nf * self.nsym * 16)
            if not self._front_end(nf, self.noise_std(snr_db), calls, d_msg.ptr, d_llr.ptr, d_rx.ptr):
                raise ValueError('the fused front end refused this call: ' + _lib.last_error())
            return (dev.download(d_msg, (nf, self.nbits), np.uint8), dev.download(d_rx, (nf, self.nsym), np.complex128),
                    dev.download(d_llr, (nf, self.nde), np.float64))

    # -- buffers --------------------------------------------------------------------------------------------
    def _stage_bufs(self, T):
        """What the staged front end needs besides its three pointers, for ``T`` transmissions."""
        bufs = {'coded': DeviceBuf(T * self.ncoded), 'sym': DeviceBuf(T * self.nsym * 16), 'llr': DeviceBuf(T * self.ntx * 8)}
        if self.keep_idx is not None:
            bufs.update(tx=DeviceBuf(T * self.ntx), keep_idx=DeviceBuf.from_array(self.keep_idx),
                        de_idx=DeviceBuf.from_array(self.de_idx))
        return bufs

    def _batch_bufs(self, T):
        bufs = dict(self._stage_bufs(T), msg=DeviceBuf(T * self.nbits), rx=DeviceBuf(T * self.nsym * 16),
                    dec=DeviceBuf(T * self.nbits), errs=DeviceBuf(T * self.agg * 4))
        if self.keep_idx is not None:
            bufs['llr_de'] = DeviceBuf(T * self.nde * 8)
        return bufs

    def _decode_and_count(self, R, d_llr, length, mark=lambda k, start: None):
        """Soft Viterbi over ``R`` frames of ``length`` LLRs at ``d_llr``, then the errors per frame against ``bufs['msg']``."""
        lib, ck, bufs = self.lib, _lib.check, self._bufs
        L, n_steps, tb = _viterbi_geometry(length, self.trellis)
        mark(1, True)
        ck(lib.cpx_viterbi_decode_batch_dev(self.trellis._device_handle(), d_llr, R, length, L, n_steps, tb, 1, bufs['dec'].ptr, None))
        mark(1, False)
        mark(2, True)
        ck(lib.cpx_count_errors_dev(bufs['msg'].ptr, self.nbits, bufs['dec'].ptr, L, R, self.agg, self.send_chunk,
                                    bufs['errs'].ptr, None))
        mark(2, False)
        ck(lib.cpx_stream_sync(None))

    # -- one batch of T transmissions at one SNR ----------------------------------------------------------------
    def run_batch(self, snr_db, T):
        """Simulate ``T`` transmissions; returns int32 ``[T, frame_aggregation]`` bit errors per frame."""
        bufs = _buffer_set(self, T, lambda: self._batch_bufs(T))
        noise_std = self.noise_std(snr_db)
        self._calls += 1
        msg, rx = bufs['msg'].ptr, bufs['rx'].ptr
        llr, length = (bufs['llr_de'], self.nde) if self.keep_idx is not None else (bufs['llr'], self.ntx)
        if not self._front_end(T, noise_std, self._calls, msg, llr.ptr, rx if self.keep_rx else None):
            self._staged_front(T, noise_std, self._calls, msg, llr.ptr, rx)
        self._decode_and_count(T, llr.ptr, length)
        return bufs['errs'].to_array((T, self.agg), np.int32)

    def ber_sweep(self, snrs_db, n_bits, tx_batch=4096):
        """BER per SNR over at least ``n_bits`` information bits each (no early stopping)."""
        return _fixed_budget_ber(snrs_db, n_bits, self.nbits, tx_batch, self.run_batch)

    def ber_sweep_batched(self, snrs_db, n_bits, mark=None):
        """Same result statistics as :meth:`ber_sweep`, with ONE Viterbi call for the whole sweep.
        ``mark(k, start)`` (benchmarks): called around stage k = 0 front end, 1 decoder, 2 error count -- e.g. to record HIP events.

        The element-wise stages (bits, encode, puncture, modulate, AWGN, demod, depuncture) run per SNR point on their
        slice of sweep-sized buffers; the decoder and the error counter then see all ``len(snrs) * T`` frames at once,
        which is what gives the large-batch Viterbi kernel (one codeword per lane, csrc/viterbi_cw.hip) its batch.
        """
        T = int(math.ceil(n_bits / self.nbits))
        P = len(snrs_db)
        R = P * T
        bufs = _buffer_set(self, ('sweep', R), lambda: dict(
            self._stage_bufs(T), msg=DeviceBuf(R * self.nbits), llr_all=DeviceBuf(R * self.nde * 8), dec=DeviceBuf(R * self.nbits),
            errs=DeviceBuf(R * self.agg * 4)))
        mark = mark or (lambda k, start: None)
        mark(0, True)
        for i, snr_db in enumerate(snrs_db):
            noise_std = self.noise_std(snr_db)
            self._calls += 1
            msg = ctypes.c_void_p(bufs['msg'].ptr.value + i * T * self.nbits)
            llr_out = ctypes.c_void_p(bufs['llr_all'].ptr.value + i * T * self.nde * 8)
            if not self._front_end(T, noise_std, self._calls, msg, llr_out):
                self._staged_front(T, noise_std, self._calls, msg, llr_out, bufs['sym'].ptr)
        mark(0, False)
        self._decode_and_count(R, bufs['llr_all'].ptr, self.nde, mark)
        errs = bufs['errs'].to_array((P, T * self.agg), np.int32)
        return errs.sum(axis=1) / float(T * self.nbits)


# ---- MIMO links ---------------------------------------------------------------------------------------------------------------

_ML_LDS = 64 * 1024            # mimo_ml_kernel's LDS budget for H, y and the per-lane residuals (mimo.hip)
_VECTORS_PER_LAUNCH = 1 << 20  # detector batch the default tx_batch aims at


class DeviceMimoLink:
    """BER of a MIMO link over a ``MIMOFlatChannel``, simulated entirely on the GPU.

    The detector arguments mean what they mean in ``mimo_receiver``: 'ml' or 'kbest' with 'hard' output make an uncoded link
    (bits -> channel -> detector -> hard-decision error count); with ``ldpc_params``, 'kbest' with 'soft' output or 'best_first'
    make an LDPC-coded one (bits -> systematic encode -> channel -> soft detector -> block-major decode -> errors in the first k
    bits of each block).  A transmission carries ``send_chunk`` message bits, rounded like ``LinkModel._prepare``; coded, that is
    ``send_chunk / k`` codewords sent one after another, as ``triang_ldpc_systematic_encode(...).reshape(-1, order='F')`` lays them
    out.  The SNR convention is channels.py's: ``noise_std = sqrt(2 nt Es / (rate 10^(SNR/10)))``, noise of per-component std
    ``noise_std / 2`` while the detector is told ``noise_std**2`` (quirk B7).  The random streams are not NumPy's MT19937 draws
    but an exactly specified function of (seed, stream id, element index), tested against tests/rng_model.py: call number c draws
    its message bits on stream 3 c, its fading on 3 c + 1 and its noise on 3 c + 2, so BERs are the host link's in distribution,
    not bit for bit.

    ``detector`` 'zf' or 'mmse' is the linear detector (``cpx_mimo_linear_dev`` on the link's buffers): 'hard' output makes an
    uncoded link, 'soft' output with ``ldpc_params`` an LDPC-coded one.  Because of quirk B7 the true N0 is ``noise_std**2 / 2``:
    'mmse' regularises with ``noise_std**2 / (2 Es)``, and the LLRs are scaled with ``noise_std**2`` itself, exactly as the K-best
    soft path is.  ``idd_iters > 0`` with a linear detector is refused.

    ``idd_iters >= 1`` (LDPC-coded 'kbest' with 'soft' output only) runs iterative detection and decoding, ``links.idd_decoder``
    with a list detector: the K-best list is searched once and its distances computed once, a first detector pass without prior
    (LLRs clipped to ``idd_clip``) fills the decoder's input, then ``idd_iters`` rounds of LDPC decode and detector / decoder
    exchange (``cpx_mimo_idd_exchange_dev``) follow.  ``idd_decision``: 'hard' takes the sign of the final LLRs, 'decode' one more
    LDPC decode of them; the first k bits of each block are counted.  ``idd_iters=0`` is the one-pass link.
    The exchange subtracts the decoder's extrinsic LLRs unclipped (links.py:404) while the detector reads them clipped to
    ``idd_clip``: a clip below the extrinsic magnitudes (min-sum sums reach several times the decoder's own 500) makes the
    detector's output disagree with the decoder by the difference, and the default 500 then loses to one pass on this link;
    ``idd_clip=float('inf')`` keeps ``posterior - ext`` the detector's extrinsic.

    Refusals (``ValueError``, before anything is launched): other detector / code combinations, a real channel, a shape the
    detector refuses, a ``send_chunk`` that does not fill whole vectors (or whole codewords).
    """

    def __init__(self, modem, channel, detector='kbest', K=16, output_type='hard', stack_size=(1, 3, 5), llr_max=500,
                 ldpc_params=None, ldpc_alg='MSA', ldpc_iters=15, send_chunk=720, seed=1, idd_iters=0, idd_clip=500.0,
                 idd_decision='decode'):
        self.modem, self.channel = modem, channel
        self.detector, self.output_type = detector, output_type
        self.K, self.llr_max = int(K), float(llr_max)
        self.seed = int(seed)
        self.ldpc_params, self.ldpc_iters = ldpc_params, int(ldpc_iters)
        self._plan(detector, output_type, stack_size, ldpc_params, ldpc_alg, send_chunk, idd_iters, idd_clip, idd_decision)
        self.tx_batch = max(1, _VECTORS_PER_LAUNCH // self.vectors_per_tx)
        self.keep_rx = False               # tests: keep the last batch's y, H, detector output and messages (self.last_rx);
                                           # an IDD link also keeps its final LLRs and the candidate list
        self.last_rx = None
        self._calls = 0
        self._bufs = {}
        # device state, only once every argument has been accepted
        self.lib = _lib.load()
        _lib.require_device()
        self._chan = _channel_handles(channel)
        self.encoder = None
        if self.coded:
            from commpy_amd.channelcoding.ldpc import _device_code
            self.encoder = LdpcEncoder(ldpc_params)
            self._code = _device_code(ldpc_params)

    # -- the plan: every check that needs no device ------------------------------------------------------------------------------
    def _plan(self, detector, output_type, stack_size, ldpc_params, ldpc_alg, send_chunk, idd_iters=0, idd_clip=500.0,
              idd_decision='decode'):
        from commpy_amd.channels import MIMOFlatChannel
        from commpy_amd.modulation import _bf_stacks, _list_checks
        if not isinstance(self.channel, MIMOFlatChannel):
            raise ValueError('DeviceMimoLink needs a MIMOFlatChannel')
        _require_complex(self.channel)
        nr, nt, nb = self.channel.nb_rx, self.channel.nb_tx, self.modem.num_bits_symbol
        m = int(np.size(self.modem.constellation))
        if m != 1 << nb:
            raise ValueError('the modem must have 2^num_bits_symbol points')
        self.coded = ldpc_params is not None
        linear = detector in ('zf', 'mmse')
        uncoded_ok = detector in ('ml', 'kbest', 'zf', 'mmse') and output_type == 'hard'
        coded_ok = detector in ('kbest', 'zf', 'mmse') and output_type == 'soft' or detector == 'best_first'
        if not (coded_ok if self.coded else uncoded_ok):
            raise ValueError("detector %r with output %r %s an LDPC code is not a device MIMO link: uncoded links take 'ml', "
                             "'kbest', 'zf' or 'mmse' with 'hard' output, coded ones 'kbest', 'zf' or 'mmse' with 'soft' output or "
                             "'best_first'"
                             % (detector, output_type, 'and' if self.coded else 'without'))
        self.idd_iters, self.idd_clip, self.idd_decision = _whole(idd_iters), float(idd_clip), idd_decision
        if self.idd_iters < 0:
            raise ValueError('idd_iters must be 0 (one detection pass) or a positive number of rounds')
        if self.idd_iters:
            if not (self.coded and detector == 'kbest' and output_type == 'soft'):
                raise ValueError("iterative detection and decoding needs an LDPC code and detector='kbest' with output_type='soft'")
            if idd_decision not in ('hard', 'decode'):
                raise ValueError("idd_decision must be 'hard' or 'decode'")
        self.stacks = None
        if detector == 'ml':
            if nb * nt > 31:
                raise ValueError('mimo_ml: m^nt above 2^31 hypotheses per vector')
            if 16 * (nr * nt + nr + 64 * nr) > _ML_LDS:
                raise ValueError('mimo_ml: %d receive antennas exceed the kernel\'s LDS' % nr)
        elif detector == 'kbest':
            if nt > nr:
                raise ValueError('h has more columns than rows')
            if self.K < 1:
                raise ValueError('kbest: K must be a positive integer')
            if min(self.K, m ** nt) * m >= 2 ** 31:
                raise ValueError('kbest: K * m above 2^31 children')
            if self.idd_iters:
                _list_checks(self.modem, self.K, self.idd_clip, nr, nt)
                self.Ke = min(self.K, m ** nt)
        elif linear:
            if nt > 8 and 16 * (m + nr * nt + nr + 2 * nt * nt + 4 * nt) > _ML_LDS:
                raise ValueError('mimo_linear: the state of one %dx%d vector exceeds the kernel\'s LDS' % (nr, nt))
        else:
            self.stacks = _bf_stacks(nr, nt, stack_size)
            if nr > 64:
                raise ValueError('best_first: %d receive antennas above the engine\'s 64' % nr)
            if nr != nt:
                raise ValueError('best_first gives nr * num_bits_symbol LLRs per vector: the link needs nr == nt (got %dx%d)' % (nr, nt))
        if self.coded:
            if ldpc_alg not in ('SPA', 'MSA'):
                raise ValueError("ldpc_alg must be 'SPA' or 'MSA'")
            self.alg = 0 if ldpc_alg == 'SPA' else 1
            self.n = int(ldpc_params['n_vnodes'])
            self.k = self.n - int(ldpc_params['n_cnodes'])
            self.rate = Fraction(self.k, self.n)
        else:
            self.k = self.n = None
            self.rate = Fraction(1)
        divider = (Fraction(1, nb * nt) / self.rate).denominator          # LinkModel._prepare (links.py:203-214)
        chunk = _whole(send_chunk)
        self.send_chunk = max(divider, chunk // divider * divider)
        if self.coded:
            if self.send_chunk % self.k:
                raise ValueError('send_chunk %d is not a whole number of %d-bit LDPC messages' % (self.send_chunk, self.k))
            self.codewords_per_tx = self.send_chunk // self.k
            self.tx_bits = self.codewords_per_tx * self.n
        else:
            self.codewords_per_tx = 0
            self.tx_bits = self.send_chunk
        if self.tx_bits % (nt * nb):
            raise ValueError('%d transmitted bits per transmission do not fill whole vectors of %d x %d bits' % (self.tx_bits, nt, nb))
        self.vectors_per_tx = self.tx_bits // (nt * nb)
        self.nr, self.nt, self.nb = nr, nt, nb

    def noise_std(self, snr_db):
        """channels.py:74 for a complex channel: sqrt(2 nt Es / (rate 10^(SNR/10)))."""
        return math.sqrt(2.0 * self.nt * self.modem.Es / (float(self.rate) * 10 ** (float(snr_db) / 10.0)))

    # -- buffers ---------------------------------------------------------------------------------------------------------------
    def _batch_bufs(self, T):
        V = T * self.vectors_per_tx
        bufs = {'msg': DeviceBuf(T * self.send_chunk), 'y': DeviceBuf(V * self.nr * 16),
                'h': DeviceBuf(V * self.nr * self.nt * 16), 'errs': DeviceBuf(T * 4)}
        if self.coded:
            B = T * self.codewords_per_tx
            bufs.update(code=DeviceBuf(B * self.n), llr=DeviceBuf(B * self.n * 8), dec=DeviceBuf(B * self.n),
                        out=DeviceBuf(B * self.n * 8), blk_errs=DeviceBuf(B * 4))
            if self.idd_iters:
                bufs.update(cand=DeviceBuf(V * self.Ke * self.nt * 4), count=DeviceBuf(V * 4), dist=DeviceBuf(V * self.Ke * 8))
        else:
            bufs['idx'] = DeviceBuf(V * self.nt * 4)
        return bufs

    # -- one batch -------------------------------------------------------------------------------------------------------------
    def run_batch(self, snr_db, T, mark=None):
        """Bit errors per transmission (int32 ``[T]``) of ``T`` transmissions at ``snr_db``; every call draws from fresh
        streams.  ``mark(stage, start)`` (benchmarks) is called around the stages 'source' (bits, encoder), 'channel', 'detector',
        'decoder' (coded links) and 'count'; an IDD link has 'list' (search, distances, first pass) and 'idd' (the rounds) in place of
        'detector', and 'decoder' only for the 'decode' decision."""
        T = _whole(T)
        if T < 1:
            raise ValueError('T must be at least 1')
        lib, ck, bufs = self.lib, _lib.check, _buffer_set(self, T, lambda: self._batch_bufs(T))
        mark = mark or (lambda stage, start: None)
        md = self.modem._device_handle()
        noise_std = self.noise_std(snr_db)
        self._calls += 1
        s_bits, s_fade, s_noise = 3 * self._calls, 3 * self._calls + 1, 3 * self._calls + 2
        V, nr, nt = T * self.vectors_per_tx, self.nr, self.nt
        B = T * self.codewords_per_tx
        mark('source', True)
        ck(lib.cpx_random_bits_dev(bufs['msg'].ptr, T * self.send_chunk, self.seed, s_bits, None))
        tx = bufs['msg']
        if self.coded:
            self.encoder.encode_dev(bufs['msg'].ptr, B, bufs['code'].ptr)
            tx = bufs['code']
        mark('source', False)
        mark('channel', True)
        ck(lib.cpx_mimo_channel_run_dev(self._chan.get(), md, tx.ptr, V, 0, noise_std * 0.5, self.seed, s_fade, s_noise,
                                        bufs['y'].ptr, bufs['h'].ptr, None))
        mark('channel', False)
        if self.idd_iters:
            return self._run_idd(bufs, T, noise_std, snr_db, mark)
        mark('detector', True)
        if self.detector == 'ml':
            ck(lib.cpx_mimo_ml_dev(md, bufs['y'].ptr, bufs['h'].ptr, 1, V, nr, nt, bufs['idx'].ptr, None))
        elif self.detector == 'kbest' and not self.coded:
            ck(lib.cpx_kbest_hard_dev(md, bufs['y'].ptr, bufs['h'].ptr, 1, V, nr, nt, self.K, bufs['idx'].ptr, None))
        elif self.detector == 'kbest':
            ck(lib.cpx_kbest_soft_dev(md, bufs['y'].ptr, bufs['h'].ptr, 1, V, nr, nt, self.K, noise_std ** 2, bufs['llr'].ptr, None))
        elif self.detector in ('zf', 'mmse'):
            # the true N0 is noise_std^2 / 2 (quirk B7); the LLR scale is what the K-best soft path is given
            reg = 0.0 if self.detector == 'zf' else noise_std ** 2 / (2.0 * self.modem.Es)
            ck(lib.cpx_mimo_linear_dev(md, bufs['y'].ptr, bufs['h'].ptr, 1, V, nr, nt, reg, noise_std ** 2,
                                       None if self.coded else bufs['idx'].ptr, bufs['llr'].ptr if self.coded else None, None, None,
                                       None))
        else:
            ck(lib.cpx_best_first_dev(md, bufs['y'].ptr, bufs['h'].ptr, 1, V, nr, nt, _lib.ptr(self.stacks), self.llr_max, None,
                                      bufs['llr'].ptr, None, None))
        mark('detector', False)
        llr_copy = None
        if self.coded:
            if self.keep_rx:                       # the decoder clips its input in place: keep what the detector gave
                llr_copy = DeviceBuf(B * self.n * 8)
                ck(lib.cpx_memcpy_d2d_async(llr_copy.ptr, bufs['llr'].ptr, B * self.n * 8, None))
            mark('decoder', True)
            ck(lib.cpx_ldpc_bp_decode_batch_bm_dev(self._code, bufs['llr'].ptr, B, self.alg, self.ldpc_iters, bufs['dec'].ptr,
                                                   bufs['out'].ptr, None, None))
            mark('decoder', False)
            mark('count', True)
            ck(lib.cpx_count_errors_dev(bufs['msg'].ptr, self.k, bufs['dec'].ptr, self.n, B, 1, self.k, bufs['blk_errs'].ptr, None))
            mark('count', False)
            ck(lib.cpx_stream_sync(None))
            errs = bufs['blk_errs'].to_array((T, self.codewords_per_tx), np.int32).sum(axis=1, dtype=np.int32)
        else:
            mark('count', True)
            ck(lib.cpx_mimo_hard_errors_dev(bufs['idx'].ptr, self.nb, bufs['msg'].ptr, T, self.send_chunk, bufs['errs'].ptr, None))
            mark('count', False)
            ck(lib.cpx_stream_sync(None))
            errs = bufs['errs'].to_array((T,), np.int32)
        if self.keep_rx:
            rx = {'snr_db': float(snr_db), 'noise_std': noise_std, 'msg': bufs['msg'].to_array((T, self.send_chunk), np.uint8),
                  'y': bufs['y'].to_array((V, nr), np.complex128), 'h': bufs['h'].to_array((V, nr, nt), np.complex128),
                  'errs': errs.copy()}
            if self.coded:
                rx['tx'] = bufs['code'].to_array((T, self.tx_bits), np.uint8)
                rx['llr'] = llr_copy.to_array((V, self.tx_bits // self.vectors_per_tx), np.float64)
                rx['dec'] = bufs['dec'].to_array((B, self.n), np.int8)
                llr_copy.free()
            else:
                rx['tx'] = rx['msg']
                rx['idx'] = bufs['idx'].to_array((V, nt), np.int32)
            self.last_rx = rx
        return errs

    def _run_idd(self, bufs, T, noise_std, snr_db, mark):
        """The receiver of an IDD link on the batch the channel left in ``bufs``: links.py:396-405 with the list detector as
        ``detector`` and the LDPC decoder's out_llrs as ``decoder``, every buffer block-major on the device."""
        lib, ck = self.lib, _lib.check
        md = self.modem._device_handle()
        V, nr, nt, Ke, B = T * self.vectors_per_tx, self.nr, self.nt, self.Ke, T * self.codewords_per_tx
        nv, clip = noise_std ** 2, self.idd_clip
        y, h, a, out = bufs['y'].ptr, bufs['h'].ptr, bufs['llr'].ptr, bufs['out'].ptr
        cand, count, dist = bufs['cand'].ptr, bufs['count'].ptr, bufs['dist'].ptr
        mark('list', True)
        ck(lib.cpx_kbest_list_dev(md, y, h, 1, V, nr, nt, self.K, cand, count, None))
        ck(lib.cpx_mimo_list_dist_dev(md, y, h, 1, V, nr, nt, cand, count, Ke, dist, None))
        ck(lib.cpx_mimo_list_llr_dev(md, cand, count, dist, V, nt, Ke, None, nv, clip, a, None))
        mark('list', False)
        mark('idd', True)
        for it in range(self.idd_iters):
            ck(lib.cpx_ldpc_bp_decode_batch_bm_dev(self._code, a, B, self.alg, self.ldpc_iters, bufs['dec'].ptr, out, None, None))
            ck(lib.cpx_mimo_idd_exchange_dev(md, cand, count, dist, V, nt, Ke, a, out, nv, clip, int(it == self.idd_iters - 1), None))
        mark('idd', False)
        final = None
        if self.keep_rx:                           # the last decode clips its input in place: keep what the loop gave
            final = DeviceBuf(B * self.n * 8)
            ck(lib.cpx_memcpy_d2d_async(final.ptr, a, B * self.n * 8, None))
        if self.idd_decision == 'decode':
            mark('decoder', True)
            ck(lib.cpx_ldpc_bp_decode_batch_bm_dev(self._code, a, B, self.alg, self.ldpc_iters, bufs['dec'].ptr, out, None, None))
            mark('decoder', False)
        else:
            ck(lib.cpx_mimo_llr_hard_dev(a, B * self.n, bufs['dec'].ptr, None))
        mark('count', True)
        ck(lib.cpx_count_errors_dev(bufs['msg'].ptr, self.k, bufs['dec'].ptr, self.n, B, 1, self.k, bufs['blk_errs'].ptr, None))
        mark('count', False)
        ck(lib.cpx_stream_sync(None))
        errs = bufs['blk_errs'].to_array((T, self.codewords_per_tx), np.int32).sum(axis=1, dtype=np.int32)
        if self.keep_rx:
            self.last_rx = {
                'snr_db': float(snr_db), 'noise_std': noise_std, 'msg': bufs['msg'].to_array((T, self.send_chunk), np.uint8),
                'y': bufs['y'].to_array((V, nr), np.complex128), 'h': bufs['h'].to_array((V, nr, nt), np.complex128),
                'errs': errs.copy(), 'tx': bufs['code'].to_array((T, self.tx_bits), np.uint8),
                'idd_llr': final.to_array((V, nt * self.nb), np.float64), 'dec': bufs['dec'].to_array((B, self.n), np.int8),
                'cand': bufs['cand'].to_array((V, Ke, nt), np.int32), 'count': bufs['count'].to_array((V,), np.int32)}
            final.free()
        return errs

    # -- sweeps ----------------------------------------------------------------------------------------------------------------
    def ber_sweep(self, snrs_db, n_bits, tx_batch=None):
        """BER per SNR over at least ``n_bits`` message bits each (a fixed budget: no early stop)."""
        return _fixed_budget_ber(snrs_db, n_bits, self.send_chunk, self.tx_batch if tx_batch is None else max(1, _whole(tx_batch)),
                                 self.run_batch)

    def link_performance(self, SNRs, send_max, err_min):
        """``LinkModel.link_performance`` on the device: per SNR, transmissions count in order while ``sent < send_max`` and
        ``errors < err_min`` (the surplus of a batch is dropped); the sweep ends after a point that stayed below ``err_min``."""
        return _sequential_ber(SNRs, send_max, err_min, self.send_chunk, self.tx_batch, self.run_batch)


def _whole(v):
    """``int(v)`` for integers and integral floats (what the reference's float arguments such as 5e5 are); ValueError otherwise."""
    if isinstance(v, (float, np.floating)):
        if not float(v).is_integer():
            raise ValueError('%r is not a whole number' % (v,))
        return int(v)
    return operator.index(v)


def _fixed_budget_ber(snrs_db, n_bits, bits_per_tx, tx_batch, run):
    """BER per SNR over at least ``n_bits`` bits each, a fixed budget without early stop: ``run(snr, T)`` returns the bit errors of T
    transmissions of ``bits_per_tx`` bits and is asked for at most ``tx_batch`` of them at a time."""
    out = []
    for snr in snrs_db:
        done = errs = 0
        while done < n_bits:
            T = int(min(tx_batch, math.ceil((n_bits - done) / bits_per_tx)))
            errs += int(run(float(snr), T).sum())
            done += T * bits_per_tx
        out.append(errs / done)
    return np.array(out)


def _sequential_ber(SNRs, send_max, err_min, send_chunk, tx_batch, run):
    """The stop rule of links.py:269-343 over batches: ``run(snr, T)`` returns the bit errors of T transmissions of ``send_chunk``
    bits, which are taken one by one while ``sent < send_max and wrong < err_min``; BER = wrong / sent; the points after the first
    one that ends with fewer than ``err_min`` errors stay 0.  ``send_max`` may be a float."""
    curve = np.zeros(len(SNRs), dtype=float)
    for i, snr in enumerate(SNRs):
        sent = wrong = 0
        while sent < send_max and wrong < err_min:
            T = max(1, min(int(tx_batch), math.ceil((send_max - sent) / send_chunk)))
            for e in run(snr, T):
                if not (sent < send_max and wrong < err_min):
                    break
                sent += send_chunk
                wrong += int(e)
        curve[i] = wrong / sent
        if wrong < err_min:
            break
    return curve
