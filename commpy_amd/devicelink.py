"""GPU-resident coded link: the whole Monte-Carlo chain of BASELINE config 5 on the device.

``DeviceWifiLink`` runs, per batch of transmissions and without leaving HBM,

    random bits -> conv_encode('cont') -> puncturing -> modulate -> AWGN -> soft demodulation
                -> depuncturing -> soft Viterbi -> per-chunk error count

with the semantics of the reference's ``Wifi80211.link_performance`` chain
(/root/reference/commpy/wifi80211.py:132-216, links.py:155-267, channels.py:37-74), including quirk B7
(complex noise of per-component std ``noise_std/2`` while the demodulator is told ``noise_std**2``) and
quirk B1 (decimal generators) unless ``generator_matrix`` is given.  Only the error counters come back
to the host.  The random streams are Philox-based, so results are statistically -- not bit-wise --
comparable with the reference; the deterministic stages are bit-exact (tests/test_devicelink_gpu.py).

``DeviceMimoLink`` does the same for a MIMO link over a ``MIMOFlatChannel`` (bits -> [LDPC encode] -> Kronecker fading channel ->
ML / K-best / best-first detector -> [LDPC decode] -> error count), the device counterpart of ``LinkModel`` with ``mimo_receiver``.

``DeviceBuf`` / the ``*_dev`` helpers are thin wrappers over the C-ABI for callers that keep data in HBM.
"""
import ctypes
import math
import operator
from fractions import Fraction

import numpy as np

from commpy_amd import _lib
from commpy_amd.wifi80211 import Wifi80211

__all__ = ['DeviceBuf', 'DeviceWifiLink', 'DeviceBscLink', 'DeviceMimoLink', 'conv_encode_gpu', 'modulate_gpu', 'bsc_gpu', 'bec_gpu',
           'mimo_channel_gpu', 'puncturing_gpu', 'depuncturing_gpu', 'puncture_indices', 'depuncture_indices', 'turbo_encode_gpu',
           'LdpcEncoder', 'gf2_generator', 'triang_ldpc_systematic_encode_gpu']


class DeviceBuf:
    """A device allocation owned through the C-ABI (cpx_malloc / cpx_free)."""

    def __init__(self, nbytes):
        self.lib = _lib.load()
        self.nbytes = int(nbytes)
        self.ptr = ctypes.c_void_p()
        _lib.check(self.lib.cpx_malloc(ctypes.byref(self.ptr), max(self.nbytes, 8)))

    @classmethod
    def from_array(cls, arr):
        arr = np.ascontiguousarray(arr)
        buf = cls(arr.nbytes)
        if arr.nbytes:
            _lib.check(buf.lib.cpx_memcpy_h2d(buf.ptr, _lib.ptr(arr), arr.nbytes))
        return buf

    def to_array(self, shape, dtype):
        out = np.empty(shape, dtype=dtype)
        if out.nbytes:
            _lib.check(self.lib.cpx_memcpy_d2h(_lib.ptr(out), self.ptr, out.nbytes))
        return out

    def free(self):
        if self.ptr:
            self.lib.cpx_free(self.ptr)
            self.ptr = ctypes.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _encoded_length(nmsg, trellis, termination):
    """number_outbits of conv_encode (convcode.py:505-520)."""
    k, n, m = trellis.k, trellis.n, trellis.total_memory
    rate = float(k) / n
    if termination == 'cont':
        return int(nmsg / rate)
    if trellis.code_type == 'rsc':
        return int((nmsg + k * m) / rate)
    return int((nmsg + m + m % k) / rate)


def conv_encode_gpu(message_bits, trellis, termination='term'):
    """``conv_encode`` for a batch ``[B, nbits]`` on the GPU (no puncturing); returns int64 ``[B, nout]``."""
    lib = _lib.load()
    msgs = np.ascontiguousarray(np.atleast_2d(message_bits), dtype=np.uint8)
    B, nmsg = msgs.shape
    nout = _encoded_length(nmsg, trellis, termination)
    d_msg, d_out = DeviceBuf.from_array(msgs), DeviceBuf(B * nout)
    rsc = trellis.code_type == 'rsc'
    # recursive codes clock a tail for 'term' only (convcode.py:538); other codes append zeros for anything but 'cont'
    terminate = (termination == 'term') if rsc else (termination != 'cont')
    _lib.check(lib.cpx_conv_encode_batch_dev(trellis._device_handle(), d_msg.ptr, B, nmsg, int(terminate),
                                             int(rsc), d_out.ptr, nout, None))
    _lib.check(lib.cpx_stream_sync(None))
    return d_out.to_array((B, nout), np.uint8).astype(np.int64)


def modulate_gpu(modem, input_bits):
    """``Modem.modulate`` on the GPU; returns complex128 symbols."""
    lib = _lib.load()
    bits = np.ascontiguousarray(input_bits, dtype=np.uint8).reshape(-1)
    nsym = bits.size // modem.num_bits_symbol
    d_bits, d_sym = DeviceBuf.from_array(bits), DeviceBuf(nsym * 16)
    _lib.check(lib.cpx_modulate_dev(modem._device_handle(), d_bits.ptr, nsym, d_sym.ptr, None))
    _lib.check(lib.cpx_stream_sync(None))
    return d_sym.to_array((nsym,), np.complex128)


def puncture_indices(n_positions, punct_vec):
    """Index table of ``puncturing(message, punct_vec)`` (convcode.py:752-774) for messages of ``n_positions`` bits:
    ``punctured[j] = message[idx[j]]`` -- what ``cpx_gather_u8_dev`` is given."""
    from commpy_amd.channelcoding.convcode import puncture_keep_mask
    return np.flatnonzero(puncture_keep_mask(n_positions, punct_vec)).astype(np.int32)


def depuncture_indices(shouldbe, punct_vec, n_punctured):
    """Index table of ``depuncturing(punctured, punct_vec, shouldbe)`` (convcode.py:777-804): ``out[j] = punctured[idx[j]]`` where
    ``idx[j] >= 0`` and 0.0 where it is -1 -- what ``cpx_gather_f64_dev`` is given.  ``IndexError`` like the reference's
    ``punctured[idx - shift2]`` when ``n_punctured`` values cannot fill the pattern."""
    from commpy_amd.channelcoding.convcode import puncture_keep_mask
    keep = puncture_keep_mask(shouldbe, punct_vec)
    if keep.sum() > n_punctured:
        raise IndexError('depuncturing: message too short for the puncturing pattern')
    de = -np.ones(int(shouldbe), dtype=np.int32)
    de[keep] = np.arange(keep.sum(), dtype=np.int32)
    return de


def puncturing_gpu(messages, punct_vec):
    """``puncturing`` for a batch ``[B, n]`` of bit rows on the GPU (``cpx_gather_u8_dev``); returns uint8 ``[B, n_kept]``."""
    lib = _lib.load()
    msgs = np.ascontiguousarray(np.atleast_2d(messages), dtype=np.uint8)
    B, n = msgs.shape
    idx = puncture_indices(n, punct_vec)
    d_in, d_idx, d_out = DeviceBuf.from_array(msgs), DeviceBuf.from_array(idx), DeviceBuf(B * len(idx))
    _lib.check(lib.cpx_gather_u8_dev(d_in.ptr, B, n, d_idx.ptr, len(idx), d_out.ptr, None))
    _lib.check(lib.cpx_stream_sync(None))
    return d_out.to_array((B, len(idx)), np.uint8)


def depuncturing_gpu(punctured, punct_vec, shouldbe):
    """``depuncturing`` for a batch ``[B, n_punctured]`` of float rows on the GPU (``cpx_gather_f64_dev``); float64 ``[B, shouldbe]``."""
    lib = _lib.load()
    rows = np.ascontiguousarray(np.atleast_2d(punctured), dtype=np.float64)
    B, n = rows.shape
    idx = depuncture_indices(shouldbe, punct_vec, n)
    d_in, d_idx, d_out = DeviceBuf.from_array(rows), DeviceBuf.from_array(idx), DeviceBuf(B * len(idx) * 8)
    _lib.check(lib.cpx_gather_f64_dev(d_in.ptr, B, n, d_idx.ptr, len(idx), d_out.ptr, None))
    _lib.check(lib.cpx_stream_sync(None))
    return d_out.to_array((B, len(idx)), np.float64)


def _binary_channel_gpu(which, input_bits, p, seed, stream_id):
    lib = _lib.load()
    bits = np.ascontiguousarray(input_bits, dtype=np.uint8)
    d_in, d_out = DeviceBuf.from_array(bits), DeviceBuf(bits.size)
    _lib.check(getattr(lib, which)(d_in.ptr, bits.size, float(p), int(seed), int(stream_id), d_out.ptr, None, None))
    _lib.check(lib.cpx_stream_sync(None))
    return d_out.to_array(bits.shape, np.int8)


def bsc_gpu(input_bits, p_t, seed=0, stream_id=0):
    """``bsc(input_bits, p_t)`` (channels.py:652-673) on the GPU: every bit flipped with probability ``p_t``.  The draws come
    from the Philox stream ``(seed, stream_id)``, not from NumPy's global generator: statistically, not bit-wise, the reference's."""
    return _binary_channel_gpu("cpx_bsc_dev", input_bits, p_t, seed, stream_id)


def bec_gpu(input_bits, p_e, seed=0, stream_id=0):
    """``bec(input_bits, p_e)`` (channels.py:630-649) on the GPU: every bit erased (-1) with probability ``p_e``."""
    return _binary_channel_gpu("cpx_bec_dev", input_bits, p_e, seed, stream_id)


class DeviceBscLink:
    """BASELINE config 1 end to end in HBM: random messages -> conv_encode('term') -> BSC(p) -> hard-decision Viterbi -> bit errors
    (the loop of /root/reference/commpy/channelcoding/tests/test_convcode.py:133-178 with channels.py:652-673 as the channel)."""

    def __init__(self, trellis, block_bits=64, tb_depth=None, seed=1):
        self.lib = _lib.load()
        _lib.require_device()
        if trellis.k != 1:
            raise ValueError('DeviceBscLink: k = 1 codes')
        self.trellis, self.nbits, self.seed = trellis, int(block_bits), int(seed)
        self.ncoded = _encoded_length(self.nbits, trellis, 'term')
        m = trellis.total_memory
        self.L = int(self.ncoded * trellis.k / trellis.n)
        self.n_steps = int((self.L + m) / trellis.k) - 1
        self.tb = min(5 * m, self.L) if tb_depth is None else int(tb_depth)
        self._calls = 0
        self._bufs = None

    def buffers(self, B):
        if self._bufs is None or self._bufs['B'] != B:
            self._bufs = {'B': B, 'msg': DeviceBuf(B * self.nbits), 'coded': DeviceBuf(B * self.ncoded),
                          'rx': DeviceBuf(B * self.ncoded * 8), 'dec': DeviceBuf(B * self.L), 'errs': DeviceBuf(B * 4)}
        return self._bufs

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


def turbo_encode_gpu(msg_bits, trellis1, trellis2, interleaver, mode=0):
    """``turbo_encode`` (turbo.py:14-59) for a batch ``[B, N]`` of messages on the GPU.

    Returns ``[sys, p1, p2]`` as int64 arrays ``[B, N]``, ``[B, N]`` and ``[B, 2(N+m2)-m2]``: row ``b`` of each equals
    what the reference returns for ``msg_bits[b]`` (the second parity stream keeps ``conv_encode``'s
    unpunctured length with a zero tail -- use ``p2[:, :N]``).  ``mode``: 0 auto, 1 walk, 2 scan kernel.
    """
    lib = _lib.load()
    msgs = np.ascontiguousarray(np.atleast_2d(msg_bits), dtype=np.uint8)
    B, N = msgs.shape
    if trellis1.code_type != 'rsc' or trellis2.code_type != 'rsc':
        # a non-recursive trellis makes conv_encode clock a zero tail (convcode.py:516-520) whose outputs the
        # reference leaves in the second parity stream; only the recursive-systematic case is built
        raise ValueError("turbo_encode_gpu needs recursive systematic component codes (code_type='rsc')")
    perm = np.ascontiguousarray(interleaver.p_array, dtype=np.int32)
    if perm.size != N:
        raise ValueError('interleaver length must equal the message length')
    np2 = 2 * (N + trellis2.total_memory) - trellis2.total_memory     # conv_encode's length minus turbo.py:57's cut
    d_msg, d_perm = DeviceBuf.from_array(msgs), DeviceBuf.from_array(perm)
    d_sys, d_p1, d_p2 = DeviceBuf(B * N), DeviceBuf(B * N), DeviceBuf(B * np2)
    _lib.check(lib.cpx_turbo_encode_batch_dev(trellis1._device_handle(), trellis2._device_handle(), d_msg.ptr, B, N,
                                              d_perm.ptr, d_sys.ptr, d_p1.ptr, d_p2.ptr, np2, int(mode), None))
    _lib.check(lib.cpx_stream_sync(None))
    return [d_sys.to_array((B, N), np.uint8).astype(np.int64), d_p1.to_array((B, N), np.uint8).astype(np.int64),
            d_p2.to_array((B, np2), np.uint8).astype(np.int64)]


def gf2_generator(ldpc_code_params):
    """Systematic generator over GF(2): ``P`` (uint8 ``[m, k]``) with ``H[:, k:] @ P = H[:, :k] (mod 2)``.

    ``build_matrix`` (ldpc.py:44-48) inverts the last ``m`` columns of H over the *reals*, which is only a valid GF(2)
    inverse for (approximately) triangular codes; this is the same construction done in GF(2) arithmetic, so it
    also covers codes like the 802.11n (1944,1296) matrix of BASELINE config 4 whose real inverse is not integral.
    """
    from commpy_amd.channelcoding.ldpc import build_matrix
    if ldpc_code_params.get('parity_check_matrix') is None:
        try:
            build_matrix(ldpc_code_params)
        except Exception:       # the real-valued inverse may not exist; H itself is all that is needed here
            pass
    H = ldpc_code_params.get('parity_check_matrix')
    if H is None:
        n_c, deg = ldpc_code_params['n_cnodes'], ldpc_code_params['max_cnode_deg']
        adj = np.asarray(ldpc_code_params['cnode_adj_list']).reshape(n_c, deg)
        Hd = np.zeros((n_c, ldpc_code_params['n_vnodes']), np.uint8)
        for c in range(n_c):
            Hd[c, adj[c, :ldpc_code_params['cnode_deg_list'][c]]] = 1
    else:
        Hd = (np.asarray(H.todense() if hasattr(H, 'todense') else H) != 0).astype(np.uint8)
    m, n = Hd.shape
    k = n - m
    A = np.concatenate([Hd[:, k:], Hd[:, :k]], axis=1)               # [H_sys | H_par], reduce the left block to I
    for col in range(m):
        piv = col + np.flatnonzero(A[col:, col])
        if piv.size == 0:
            raise ValueError('the last n_cnodes columns of H are singular over GF(2)')
        if piv[0] != col:
            A[[col, piv[0]]] = A[[piv[0], col]]
        rows = np.flatnonzero(A[:, col])
        rows = rows[rows != col]
        A[rows] ^= A[col]
    return np.ascontiguousarray(A[:, m:])


class LdpcEncoder:
    """Device-resident systematic LDPC encoder: ``code = [msg, G2 @ msg mod 2]`` per block (ldpc.py:302-354).

    ``generator='reference'`` uses ``ldpc_code_params['generator_matrix']`` exactly as
    ``triang_ldpc_systematic_encode`` does (built by ``build_matrix`` if absent) and requires its entries to be
    integers, so that ``G.dot(msg) % 2`` (ldpc.py:353) is GF(2) arithmetic; ``generator='gf2'`` uses
    :func:`gf2_generator`.
    """

    def __init__(self, ldpc_code_params, generator='reference'):
        from commpy_amd.channelcoding.ldpc import build_matrix
        self.lib = _lib.load()
        if generator == 'gf2':
            G2 = gf2_generator(ldpc_code_params)
        elif generator == 'reference':
            if ldpc_code_params.get('generator_matrix') is None or ldpc_code_params.get('parity_check_matrix') is None:
                build_matrix(ldpc_code_params)
            G = ldpc_code_params['generator_matrix']
            G = np.asarray(G.todense() if hasattr(G, 'todense') else G, dtype=np.float64)
            if not np.all(np.abs(G - np.rint(G)) < 1e-9):
                raise ValueError("generator_matrix is not integer valued (the code is not triangular); "
                                 "use generator='gf2'")
            G2 = (np.rint(G).astype(np.int64) % 2).astype(np.uint8)
        else:
            raise ValueError("generator must be 'reference' or 'gf2'")
        self.G2 = np.ascontiguousarray(G2, dtype=np.uint8)
        self.m, self.k = self.G2.shape
        self.n = self.m + self.k
        self.h = ctypes.c_void_p()
        _lib.require_device()
        _lib.check(self.lib.cpx_ldpc_encoder_create(_lib.ptr(self.G2), self.m, self.k, ctypes.byref(self.h)))

    def encode_dev(self, d_msg, B, d_code, stream=None):
        """msg ``[B][k]`` uint8 (device) -> code ``[B][n]`` uint8 (device); asynchronous on ``stream``."""
        _lib.check(self.lib.cpx_ldpc_encode_batch_dev(self.h, d_msg, int(B), d_code, stream))

    def encode(self, msgs):
        """Host convenience: uint8/int ``[B, k]`` -> int8 ``[B, n]``."""
        msgs = np.ascontiguousarray(np.atleast_2d(msgs), dtype=np.uint8)
        B, k = msgs.shape
        if k != self.k:
            raise ValueError('messages must have %d bits' % self.k)
        d_msg, d_code = DeviceBuf.from_array(msgs), DeviceBuf(B * self.n)
        self.encode_dev(d_msg.ptr, B, d_code.ptr)
        _lib.check(self.lib.cpx_stream_sync(None))
        return d_code.to_array((B, self.n), np.int8)

    def __del__(self):
        try:
            if self.h:
                self.lib.cpx_ldpc_encoder_destroy(self.h)
                self.h = ctypes.c_void_p()
        except Exception:
            pass


def triang_ldpc_systematic_encode_gpu(message_bits, ldpc_code_params, pad=True, generator='reference'):
    """``triang_ldpc_systematic_encode`` (ldpc.py:302-354) on the GPU: same arguments, padding rule, ``ValueError``
    and return layout (int8 ``(n, n_blocks)``, squeezed; block ``j`` = ``message_bits[j*k:(j+1)*k]``)."""
    enc = ldpc_code_params.get('_cpx_ldpc_enc_' + generator)
    if enc is None:
        enc = LdpcEncoder(ldpc_code_params, generator)
        ldpc_code_params['_cpx_ldpc_enc_' + generator] = enc
    message_bits = np.asarray(message_bits)
    modulo = len(message_bits) % enc.k
    if modulo:
        if pad:
            message_bits = np.concatenate((message_bits, np.zeros(enc.k - modulo, message_bits.dtype)))
        else:
            raise ValueError('Padding is disable but message length is not a multiple of block length.')
    return enc.encode(message_bits.reshape(-1, enc.k)).T.squeeze().astype(np.int8)


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
        self.lib = _lib.load()
        _lib.require_device()
        self.wifi = Wifi80211(mcs, generator_matrix=generator_matrix)
        self.trellis = self.wifi._get_trellis()
        self.modem = self.wifi.get_modem()
        self.coding = self.wifi._get_coding()
        self.rate = self.coding[0] / self.coding[1]
        from fractions import Fraction
        divider = (Fraction(1, self.modem.num_bits_symbol) * 1 / Fraction(self.rate).limit_denominator(100)).denominator
        self.send_chunk = max(divider, send_chunk // divider * divider)
        self.agg = int(frame_aggregation)
        self.nbits = self.send_chunk * self.agg                       # information bits per transmission
        self.seed = int(seed)
        self._calls = 0
        # index maps of puncturing / depuncturing (vector form of convcode.py:752-804)
        self.ncoded = 2 * self.nbits                                  # rate-1/2 mother code, 'cont'
        pvec = Wifi80211._get_puncture_matrix(*self.coding)
        if pvec is None:
            self.keep_idx = None
            self.ntx = self.ncoded
            self.nde = self.ncoded
            self.de_idx = None
        else:
            self.keep_idx = puncture_indices(self.ncoded, pvec)
            self.ntx = len(self.keep_idx)
            self.nde = math.ceil(self.ntx * self.coding[0] / self.coding[1] * 2)
            self.de_idx = depuncture_indices(self.nde, pvec, self.ntx)
        nb = self.modem.num_bits_symbol
        if self.ntx % nb:
            raise ValueError('send_chunk does not give an integer number of symbols')
        self.nsym = self.ntx // nb
        self._bufs = {}
        self._front = None
        self.keep_rx = False                                          # tests: the fused launch also stores the noisy symbols (bufs['rx'])
        self.front_reason = 'fused=False'
        if fused is None or fused:
            self._make_front(bool(fused))

    def _make_front(self, required):
        """The plan of the fused front end, or the reason why the staged kernels stay (``front_reason``)."""
        pos = None
        if self.de_idx is not None:
            mapped = np.flatnonzero(self.de_idx >= 0).astype(np.int32)      # decoder-input position of transmitted bit t
            if len(mapped) != self.ntx:
                self.front_reason = 'depuncturing leaves %d of %d transmitted bits unused' % (self.ntx - len(mapped), self.ntx)
                if required:
                    raise ValueError(self.front_reason)
                return
            pos = np.ascontiguousarray(mapped)
        keep = None if self.keep_idx is None else np.ascontiguousarray(self.keep_idx, dtype=np.int32)
        h = ctypes.c_void_p()
        rc = self.lib.cpx_link_front_create(self.trellis._device_handle(), self.modem._device_handle(), self.nbits,
                                            None if keep is None else _lib.ptr(keep), self.ntx,
                                            None if pos is None else _lib.ptr(pos), self.nde, ctypes.byref(h))
        if rc == _lib.CPX_ELIMIT and not required:
            self.front_reason = _lib.last_error()
            return
        _lib.check(rc)
        self._front = h
        self.front_reason = None

    def _front_end(self, T, noise_std, calls, d_msg, d_llr, d_rx=None):
        """One launch for the stages in front of the decoder; False when this call has to take the staged kernels (a
        non-default demodulator mode or precision)."""
        self.front_last_kernel = 'staged'
        if self._front is None:
            return False
        rc = self.lib.cpx_link_front_run_dev(self._front, T, noise_std ** 2, noise_std * 0.5, noise_std * 0.5, 1.0, self.seed,
                                             2 * calls, 2 * calls + 1, d_msg, d_llr, d_rx, None)
        if rc == _lib.CPX_ELIMIT:
            return False
        _lib.check(rc)
        self.front_last_kernel = _lib.last_kernel()
        return True

    def front_sample(self, nf, snr_db, calls):
        """Tests / benchmarks: the first ``nf`` transmissions of the point that was generated with call number ``calls`` at ``snr_db``,
        once more, this time with the noisy symbols stored -- (msg [nf, nbits] uint8, rx [nf, nsym] complex, llr [nf, nde] float64).
        The streams are counter based, so these are the values the sweep's own launch produced for those transmissions."""
        if self._front is None:
            raise ValueError('no fused front end: ' + str(self.front_reason))
        noise_std = math.sqrt(2.0 * self.modem.Es / (self.rate * 10 ** (float(snr_db) / 10.0)))
        d_msg, d_llr, d_rx = DeviceBuf(nf * self.nbits), DeviceBuf(nf * self.nde * 8), DeviceBuf(nf * self.nsym * 16)
        try:
            if not self._front_end(nf, noise_std, calls, d_msg.ptr, d_llr.ptr, d_rx.ptr):
                raise ValueError('the fused front end refused this call: ' + _lib.last_error())
            _lib.check(self.lib.cpx_stream_sync(None))
            return (d_msg.to_array((nf, self.nbits), np.uint8), d_rx.to_array((nf, self.nsym), np.complex128),
                    d_llr.to_array((nf, self.nde), np.float64))
        finally:
            d_msg.free(); d_llr.free(); d_rx.free()

    def __del__(self):
        try:
            if self._front is not None:
                self.lib.cpx_link_front_destroy(self._front)
                self._front = None
        except Exception:
            pass

    # -- buffers --------------------------------------------------------------------------------------------
    def _alloc(self, T):
        if self._bufs.get('T') == T:
            return self._bufs
        for b in self._bufs.values():
            if isinstance(b, DeviceBuf):
                b.free()
        nb = self.modem.num_bits_symbol
        bufs = {'T': T,
                'msg': DeviceBuf(T * self.nbits), 'coded': DeviceBuf(T * self.ncoded),
                'sym': DeviceBuf(T * self.nsym * 16), 'rx': DeviceBuf(T * self.nsym * 16),
                'llr': DeviceBuf(T * self.nsym * nb * 8), 'dec': DeviceBuf(T * self.nbits),
                'errs': DeviceBuf(T * self.agg * 4)}
        if self.keep_idx is not None:
            bufs['tx'] = DeviceBuf(T * self.ntx)
            bufs['llr_de'] = DeviceBuf(T * self.nde * 8)
            bufs['keep_idx'] = DeviceBuf.from_array(self.keep_idx)
            bufs['de_idx'] = DeviceBuf.from_array(self.de_idx)
        self._bufs = bufs
        return bufs

    def _staged_front(self, T, noise_std, calls, bufs):
        """The stages in front of the decoder as one kernel each (what the fused kernel replaces)."""
        lib, ck = self.lib, _lib.check
        h_tr, h_md = self.trellis._device_handle(), self.modem._device_handle()
        ck(lib.cpx_random_bits_dev(bufs['msg'].ptr, T * self.nbits, self.seed, 2 * calls, None))
        ck(lib.cpx_conv_encode_batch_dev(h_tr, bufs['msg'].ptr, T, self.nbits, 0, 0, bufs['coded'].ptr, self.ncoded, None))
        tx = bufs['coded']
        if self.keep_idx is not None:
            ck(lib.cpx_gather_u8_dev(bufs['coded'].ptr, T, self.ncoded, bufs['keep_idx'].ptr, self.ntx, bufs['tx'].ptr, None))
            tx = bufs['tx']
        ck(lib.cpx_modulate_dev(h_md, tx.ptr, T * self.nsym, bufs['sym'].ptr, None))
        ck(lib.cpx_awgn_dev(bufs['sym'].ptr, T * self.nsym, noise_std * 0.5, noise_std * 0.5, self.seed, 2 * calls + 1,
                            bufs['rx'].ptr, None))
        ck(lib.cpx_demod_soft_dev(h_md, bufs['rx'].ptr, T * self.nsym, noise_std ** 2, bufs['llr'].ptr, None))
        llr, length = bufs['llr'], self.ntx
        if self.keep_idx is not None:
            ck(lib.cpx_gather_f64_dev(bufs['llr'].ptr, T, self.ntx, bufs['de_idx'].ptr, self.nde, bufs['llr_de'].ptr, None))
            llr, length = bufs['llr_de'], self.nde
        return llr, length

    # -- one batch of T transmissions at one SNR ----------------------------------------------------------------
    def run_batch(self, snr_db, T):
        """Simulate ``T`` transmissions; returns int32 ``[T, frame_aggregation]`` bit errors per frame."""
        lib, bufs = self.lib, self._alloc(T)
        nb = self.modem.num_bits_symbol
        h_tr, h_md = self.trellis._device_handle(), self.modem._device_handle()
        # channels.py:74 (complex channel): noise_std = sqrt(2 * Es / (rate * snr)); per-component std = noise_std/2
        noise_std = math.sqrt(2.0 * self.modem.Es / (self.rate * 10 ** (snr_db / 10.0)))
        self._calls += 1
        ck = _lib.check
        if self._front_end(T, noise_std, self._calls, bufs['msg'].ptr, (bufs['llr_de'] if self.keep_idx is not None else bufs['llr']).ptr,
                           bufs['rx'].ptr if self.keep_rx else None):
            llr, length = (bufs['llr_de'], self.nde) if self.keep_idx is not None else (bufs['llr'], self.ntx)
        else:
            llr, length = self._staged_front(T, noise_std, self._calls, bufs)
        m = self.trellis.total_memory
        L = int(length * 0.5)
        n_steps = int((L + m) / 1) - 1
        ck(lib.cpx_viterbi_decode_batch_dev(h_tr, llr.ptr, T, length, L, n_steps, min(5 * m, L), 1, bufs['dec'].ptr, None))
        ck(lib.cpx_count_errors_dev(bufs['msg'].ptr, self.nbits, bufs['dec'].ptr, L, T, self.agg, self.send_chunk,
                                    bufs['errs'].ptr, None))
        ck(lib.cpx_stream_sync(None))
        return bufs['errs'].to_array((T, self.agg), np.int32)

    def ber_sweep(self, snrs_db, n_bits, tx_batch=4096):
        """BER per SNR over at least ``n_bits`` information bits each (no early stopping)."""
        out = []
        for snr in snrs_db:
            done, errs = 0, 0
            while done < n_bits:
                T = int(min(tx_batch, math.ceil((n_bits - done) / self.nbits)))
                e = self.run_batch(float(snr), T)
                errs += int(e.sum())
                done += T * self.nbits
            out.append(errs / done)
        return np.array(out)

    def ber_sweep_batched(self, snrs_db, n_bits, mark=None):
        """Same result statistics as :meth:`ber_sweep`, with ONE Viterbi call for the whole sweep.
        ``mark(k, start)`` (benchmarks): called around stage k = 0 front end, 1 decoder, 2 error count -- e.g. to record HIP events.

        The element-wise stages (bits, encode, puncture, modulate, AWGN, demod, depuncture) run per SNR point on their
        slice of sweep-sized buffers; the decoder and the error counter then see all ``len(snrs) * T`` frames at once,
        which is what gives the large-batch Viterbi kernel (one codeword per lane, csrc/viterbi_cw.hip) its batch.
        """
        lib, ck = self.lib, _lib.check
        nb = self.modem.num_bits_symbol
        T = int(math.ceil(n_bits / self.nbits))
        P = len(snrs_db)
        R = P * T
        key = ('sweep', R)
        if self._bufs.get('T') != key:
            for b in self._bufs.values():
                if isinstance(b, DeviceBuf):
                    b.free()
            bufs = {'T': key,
                    'msg': DeviceBuf(R * self.nbits), 'coded': DeviceBuf(T * self.ncoded),
                    'sym': DeviceBuf(T * self.nsym * 16), 'llr': DeviceBuf(T * self.nsym * nb * 8),
                    'llr_all': DeviceBuf(R * self.nde * 8), 'dec': DeviceBuf(R * self.nbits),
                    'errs': DeviceBuf(R * self.agg * 4)}
            if self.keep_idx is not None:
                bufs['tx'] = DeviceBuf(T * self.ntx)
                bufs['keep_idx'] = DeviceBuf.from_array(self.keep_idx)
                bufs['de_idx'] = DeviceBuf.from_array(self.de_idx)
            self._bufs = bufs
        bufs = self._bufs
        h_tr, h_md = self.trellis._device_handle(), self.modem._device_handle()

        def at(buf, nbytes):
            return ctypes.c_void_p(buf.ptr.value + nbytes)

        mark = mark or (lambda k, start: None)
        mark(0, True)
        for i, snr_db in enumerate(snrs_db):
            noise_std = math.sqrt(2.0 * self.modem.Es / (self.rate * 10 ** (float(snr_db) / 10.0)))   # channels.py:74
            self._calls += 1
            msg = at(bufs['msg'], i * T * self.nbits)
            llr_out = at(bufs['llr_all'], i * T * self.nde * 8)
            if self._front_end(T, noise_std, self._calls, msg, llr_out):
                continue
            ck(lib.cpx_random_bits_dev(msg, T * self.nbits, self.seed, 2 * self._calls, None))
            ck(lib.cpx_conv_encode_batch_dev(h_tr, msg, T, self.nbits, 0, 0, bufs['coded'].ptr, self.ncoded, None))
            tx = bufs['coded']
            if self.keep_idx is not None:
                ck(lib.cpx_gather_u8_dev(bufs['coded'].ptr, T, self.ncoded, bufs['keep_idx'].ptr, self.ntx, bufs['tx'].ptr, None))
                tx = bufs['tx']
            ck(lib.cpx_modulate_dev(h_md, tx.ptr, T * self.nsym, bufs['sym'].ptr, None))
            ck(lib.cpx_awgn_dev(bufs['sym'].ptr, T * self.nsym, noise_std * 0.5, noise_std * 0.5, self.seed,
                                2 * self._calls + 1, bufs['sym'].ptr, None))
            if self.keep_idx is not None:
                ck(lib.cpx_demod_soft_dev(h_md, bufs['sym'].ptr, T * self.nsym, noise_std ** 2, bufs['llr'].ptr, None))
                ck(lib.cpx_gather_f64_dev(bufs['llr'].ptr, T, self.ntx, bufs['de_idx'].ptr, self.nde, llr_out, None))
            else:
                ck(lib.cpx_demod_soft_dev(h_md, bufs['sym'].ptr, T * self.nsym, noise_std ** 2, llr_out, None))
        mark(0, False)
        m = self.trellis.total_memory
        length = self.nde
        L = int(length * 0.5)
        n_steps = int((L + m) / 1) - 1
        mark(1, True)
        ck(lib.cpx_viterbi_decode_batch_dev(h_tr, bufs['llr_all'].ptr, R, length, L, n_steps, min(5 * m, L), 1,
                                            bufs['dec'].ptr, None))
        mark(1, False)
        mark(2, True)
        ck(lib.cpx_count_errors_dev(bufs['msg'].ptr, self.nbits, bufs['dec'].ptr, L, R, self.agg, self.send_chunk,
                                    bufs['errs'].ptr, None))
        mark(2, False)
        ck(lib.cpx_stream_sync(None))
        errs = bufs['errs'].to_array((P, T * self.agg), np.int32)
        return errs.sum(axis=1) / float(T * self.nbits)


# ---- MIMO links ---------------------------------------------------------------------------------------------------------------

def _fading_matrices(channel):
    """(sqrtm(Rr) [nr, nr], sqrtm(Rt).T [nt, nt], mean [nr, nt]) as complex128 C arrays: the three matrices
    ``MIMOFlatChannel.propagate`` multiplies G with, computed once on the host."""
    from scipy.linalg import sqrtm
    mean, rt, rr = channel.fading_param
    return (np.ascontiguousarray(sqrtm(rr), dtype=np.complex128), np.ascontiguousarray(sqrtm(rt).T, dtype=np.complex128),
            np.ascontiguousarray(np.broadcast_to(mean, (channel.nb_rx, channel.nb_tx)), dtype=np.complex128))


def _channel_handles(channel):
    """cpx_mimo_channel handles (one per device) of the channel's current fading_param."""
    lib = _lib.load()
    a, bt, mean = _fading_matrices(channel)

    def create():
        h = ctypes.c_void_p()
        _lib.check(lib.cpx_mimo_channel_create(channel.nb_rx, channel.nb_tx, _lib.ptr(a), _lib.ptr(bt), _lib.ptr(mean),
                                               ctypes.byref(h)))
        return h
    return _lib.DeviceHandles(create, 'cpx_mimo_channel_destroy')


def _require_complex(channel):
    if not channel.isComplex:
        raise ValueError('the device MIMO channel is complex valued: call uncorr_rayleigh_fading(complex) or give a complex fading_param')


def mimo_channel_gpu(channel, modem, bits, seed=0, stream_id=0):
    """``MIMOFlatChannel.propagate(modem.modulate(bits))`` on the GPU: returns ``(y [V, nr], H [V, nr, nt])`` for the
    ``V = len(bits) / (nt * num_bits_symbol)`` vectors the bits fill (a partial vector is a ValueError).  The fading G and the noise
    come from the Philox streams ``(seed, 2 stream_id)`` and ``(seed, 2 stream_id + 1)`` instead of NumPy's generator (statistically,
    not bit-wise, the reference's); ``H = sqrtm(Rr) G sqrtm(Rt).T + mean`` and the noise of per-component std ``noise_std / 2``
    follow channels.py (quirk B7)."""
    _require_complex(channel)
    if channel.noise_std is None:
        raise AssertionError('Noise standard deviation must be set before propagation.')
    nr, nt, nb = channel.nb_rx, channel.nb_tx, modem.num_bits_symbol
    flat = np.ascontiguousarray(bits, dtype=np.uint8).reshape(-1)
    if flat.size % (nt * nb):
        raise ValueError('%d bits do not fill whole vectors of %d symbols of %d bits' % (flat.size, nt, nb))
    V = flat.size // (nt * nb)
    lib = _lib.load()
    handles = _channel_handles(channel)
    try:
        d_bits, d_y, d_h = DeviceBuf.from_array(flat), DeviceBuf(V * nr * 16), DeviceBuf(V * nr * nt * 16)
        _lib.check(lib.cpx_mimo_channel_run_dev(handles.get(), modem._device_handle(), d_bits.ptr, V, 0,
                                                float(channel.noise_std) * 0.5, int(seed), 2 * int(stream_id),
                                                2 * int(stream_id) + 1, d_y.ptr, d_h.ptr, None))
        _lib.check(lib.cpx_stream_sync(None))
        return d_y.to_array((V, nr), np.complex128), d_h.to_array((V, nr, nt), np.complex128)
    finally:
        handles.drop()


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
    ``noise_std / 2`` while the detector is told ``noise_std**2`` (quirk B7).  Random streams are Philox (seed, call, stage), so
    BERs are statistically, not bit-wise, the host link's.

    Refusals (``ValueError``, before anything is launched): other detector / code combinations, a real channel, a shape the
    detector refuses, a ``send_chunk`` that does not fill whole vectors (or whole codewords).
    """

    def __init__(self, modem, channel, detector='kbest', K=16, output_type='hard', stack_size=(1, 3, 5), llr_max=500,
                 ldpc_params=None, ldpc_alg='MSA', ldpc_iters=15, send_chunk=720, seed=1):
        self.modem, self.channel = modem, channel
        self.detector, self.output_type = detector, output_type
        self.K, self.llr_max = int(K), float(llr_max)
        self.seed = int(seed)
        self.ldpc_params, self.ldpc_iters = ldpc_params, int(ldpc_iters)
        self._plan(detector, output_type, stack_size, ldpc_params, ldpc_alg, send_chunk)
        self.tx_batch = max(1, _VECTORS_PER_LAUNCH // self.vectors_per_tx)
        self.keep_rx = False               # tests: keep the last batch's y, H, detector output and messages (self.last_rx)
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
    def _plan(self, detector, output_type, stack_size, ldpc_params, ldpc_alg, send_chunk):
        from commpy_amd.channels import MIMOFlatChannel
        from commpy_amd.modulation import _bf_stacks
        if not isinstance(self.channel, MIMOFlatChannel):
            raise ValueError('DeviceMimoLink needs a MIMOFlatChannel')
        _require_complex(self.channel)
        nr, nt, nb = self.channel.nb_rx, self.channel.nb_tx, self.modem.num_bits_symbol
        m = int(np.size(self.modem.constellation))
        if m != 1 << nb:
            raise ValueError('the modem must have 2^num_bits_symbol points')
        self.coded = ldpc_params is not None
        uncoded_ok = detector == 'ml' and output_type == 'hard' or detector == 'kbest' and output_type == 'hard'
        coded_ok = detector == 'kbest' and output_type == 'soft' or detector == 'best_first'
        if not (coded_ok if self.coded else uncoded_ok):
            raise ValueError("detector %r with output %r %s an LDPC code is not a device MIMO link: uncoded links take 'ml' or "
                             "'kbest' with 'hard' output, coded ones 'kbest' with 'soft' output or 'best_first'"
                             % (detector, output_type, 'and' if self.coded else 'without'))
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
    def _alloc(self, T):
        if self._bufs.get('T') == T:
            return self._bufs
        for b in self._bufs.values():
            if isinstance(b, DeviceBuf):
                b.free()
        V = T * self.vectors_per_tx
        bufs = {'T': T, 'msg': DeviceBuf(T * self.send_chunk), 'y': DeviceBuf(V * self.nr * 16),
                'h': DeviceBuf(V * self.nr * self.nt * 16), 'errs': DeviceBuf(T * 4)}
        if self.coded:
            B = T * self.codewords_per_tx
            bufs.update(code=DeviceBuf(B * self.n), llr=DeviceBuf(B * self.n * 8), dec=DeviceBuf(B * self.n),
                        out=DeviceBuf(B * self.n * 8), blk_errs=DeviceBuf(B * 4))
        else:
            bufs['idx'] = DeviceBuf(V * self.nt * 4)
        self._bufs = bufs
        return bufs

    # -- one batch -------------------------------------------------------------------------------------------------------------
    def run_batch(self, snr_db, T, mark=None):
        """Bit errors per transmission (int32 ``[T]``) of ``T`` transmissions at ``snr_db``; every call draws from fresh
        streams.  ``mark(stage, start)`` (benchmarks) is called around the stages 'source' (bits, encoder), 'channel', 'detector',
        'decoder' (coded links) and 'count'."""
        T = _whole(T)
        if T < 1:
            raise ValueError('T must be at least 1')
        lib, ck, bufs = self.lib, _lib.check, self._alloc(T)
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
        mark('detector', True)
        if self.detector == 'ml':
            ck(lib.cpx_mimo_ml_dev(md, bufs['y'].ptr, bufs['h'].ptr, 1, V, nr, nt, bufs['idx'].ptr, None))
        elif self.detector == 'kbest' and not self.coded:
            ck(lib.cpx_kbest_hard_dev(md, bufs['y'].ptr, bufs['h'].ptr, 1, V, nr, nt, self.K, bufs['idx'].ptr, None))
        elif self.detector == 'kbest':
            ck(lib.cpx_kbest_soft_dev(md, bufs['y'].ptr, bufs['h'].ptr, 1, V, nr, nt, self.K, noise_std ** 2, bufs['llr'].ptr, None))
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

    # -- sweeps ----------------------------------------------------------------------------------------------------------------
    def ber_sweep(self, snrs_db, n_bits, tx_batch=None):
        """BER per SNR over at least ``n_bits`` message bits each (a fixed budget: no early stop)."""
        tx_batch = self.tx_batch if tx_batch is None else max(1, _whole(tx_batch))
        out = []
        for snr in snrs_db:
            done = errs = 0
            while done < n_bits:
                T = int(min(tx_batch, math.ceil((n_bits - done) / self.send_chunk)))
                errs += int(self.run_batch(float(snr), T).sum())
                done += T * self.send_chunk
            out.append(errs / done)
        return np.array(out)

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
