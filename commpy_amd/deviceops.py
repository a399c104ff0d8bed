"""Device memory and the one-shot host conveniences over the link-simulation stages of the C-ABI.

``DeviceBuf`` is a device allocation for callers that keep data in HBM.  The ``*_gpu`` functions and ``LdpcEncoder.encode`` take
host arrays, run ONE stage on the GPU (encoders, puncturing, modulation, binary channels, the MIMO fading channel) and return
host arrays; the device links of ``commpy_amd.devicelink`` chain the same entry points without leaving the device.
"""
import contextlib
import ctypes

import numpy as np

from commpy_amd import _lib
from commpy_amd._results import device_outputs, returned
from commpy_amd.channelcoding.convcode import puncture_keep_mask
from commpy_amd.channelcoding.gfields import whole
from commpy_amd.channelcoding.ldpc import build_matrix

__all__ = ['DeviceBuf', 'conv_encode_gpu', 'modulate_gpu', 'bsc_gpu', 'bec_gpu', 'mimo_channel_gpu', 'puncturing_gpu',
           'depuncturing_gpu', 'puncture_indices', 'depuncture_indices', 'turbo_encode_gpu', 'LdpcEncoder', 'gf2_generator',
           'triang_ldpc_systematic_encode_gpu', 'multipath_dev', 'ofdm_map_dev', 'ofdm_estimate_dev', 'ofdm_estimate_tv_dev', 'sync_estimate_dev', 'sync_align_dev',
           'fading_params_dev', 'fading_gains_dev', 'fading_convolve_dev', 'fading_channel_dev', 'polar_encode_dev', 'polar_decode_dev',
           'bch_encode_dev', 'bch_decode_dev', 'rs_encode_dev', 'rs_decode_dev', 'tailbiting_encode_dev', 'tailbiting_decode_dev',
           'ldpc_layered_decode_dev', 'bch_chase_dev', 'tpc_decode_dev', 'mlse_equalize_dev', 'mmse_equalize_dev', 'adaptive_equalize_dev',
           'timing_recover_dev']


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


class _OneShot(contextlib.ExitStack):
    """The device memory of one host-convenience call: ``with _OneShot() as dev`` uploads inputs, allocates outputs and downloads
    results; everything it allocated is freed when the block ends, also by an exception."""

    lib = property(lambda self: _lib.load())

    def _own(self, buf):
        self.callback(buf.free)
        return buf

    def upload(self, arr):
        """Device pointer of a copy of ``arr``."""
        return self._own(DeviceBuf.from_array(arr)).ptr

    def alloc(self, nbytes):
        return self._own(DeviceBuf(nbytes))

    def download(self, buf, shape, dtype):
        """``buf`` as a host array, once the default stream has finished."""
        _lib.check(self.lib.cpx_stream_sync(None))
        return buf.to_array(shape, dtype)


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
    msgs = np.ascontiguousarray(np.atleast_2d(message_bits), dtype=np.uint8)
    B, nmsg = msgs.shape
    nout = _encoded_length(nmsg, trellis, termination)
    rsc = trellis.code_type == 'rsc'
    # recursive codes clock a tail for 'term' only (convcode.py:538); other codes append zeros for anything but 'cont'
    terminate = (termination == 'term') if rsc else (termination != 'cont')
    with _OneShot() as dev:
        d_out = dev.alloc(B * nout)
        _lib.check(dev.lib.cpx_conv_encode_batch_dev(trellis._device_handle(), dev.upload(msgs), B, nmsg, int(terminate),
                                                     int(rsc), d_out.ptr, nout, None))
        return dev.download(d_out, (B, nout), np.uint8).astype(np.int64)


def modulate_gpu(modem, input_bits):
    """``Modem.modulate`` on the GPU; returns complex128 symbols."""
    bits = np.ascontiguousarray(input_bits, dtype=np.uint8).reshape(-1)
    nsym = bits.size // modem.num_bits_symbol
    with _OneShot() as dev:
        d_sym = dev.alloc(nsym * 16)
        _lib.check(dev.lib.cpx_modulate_dev(modem._device_handle(), dev.upload(bits), nsym, d_sym.ptr, None))
        return dev.download(d_sym, (nsym,), np.complex128)


def puncture_indices(n_positions, punct_vec):
    """Index table of ``puncturing(message, punct_vec)`` (convcode.py:752-774) for messages of ``n_positions`` bits:
    ``punctured[j] = message[idx[j]]`` -- what ``cpx_gather_u8_dev`` is given."""
    return np.flatnonzero(puncture_keep_mask(n_positions, punct_vec)).astype(np.int32)


def depuncture_indices(shouldbe, punct_vec, n_punctured):
    """Index table of ``depuncturing(punctured, punct_vec, shouldbe)`` (convcode.py:777-804): ``out[j] = punctured[idx[j]]`` where
    ``idx[j] >= 0`` and 0.0 where it is -1 -- what ``cpx_gather_f64_dev`` is given.  ``IndexError`` like the reference's
    ``punctured[idx - shift2]`` when ``n_punctured`` values cannot fill the pattern."""
    keep = puncture_keep_mask(shouldbe, punct_vec)
    if keep.sum() > n_punctured:
        raise IndexError('depuncturing: message too short for the puncturing pattern')
    de = -np.ones(int(shouldbe), dtype=np.int32)
    de[keep] = np.arange(keep.sum(), dtype=np.int32)
    return de


def _gather_gpu(entry, rows, idx, dtype):
    """``out[b, j] = rows[b, idx[j]]`` (0 where ``idx[j]`` is -1) through ``cpx_gather_u8_dev`` / ``cpx_gather_f64_dev``."""
    B, n = rows.shape
    with _OneShot() as dev:
        d_out = dev.alloc(B * len(idx) * np.dtype(dtype).itemsize)
        _lib.check(getattr(dev.lib, entry)(dev.upload(rows), B, n, dev.upload(idx), len(idx), d_out.ptr, None))
        return dev.download(d_out, (B, len(idx)), dtype)


def puncturing_gpu(messages, punct_vec):
    """``puncturing`` for a batch ``[B, n]`` of bit rows on the GPU (``cpx_gather_u8_dev``); returns uint8 ``[B, n_kept]``."""
    msgs = np.ascontiguousarray(np.atleast_2d(messages), dtype=np.uint8)
    return _gather_gpu("cpx_gather_u8_dev", msgs, puncture_indices(msgs.shape[1], punct_vec), np.uint8)


def depuncturing_gpu(punctured, punct_vec, shouldbe):
    """``depuncturing`` for a batch ``[B, n_punctured]`` of float rows on the GPU (``cpx_gather_f64_dev``); float64 ``[B, shouldbe]``."""
    rows = np.ascontiguousarray(np.atleast_2d(punctured), dtype=np.float64)
    return _gather_gpu("cpx_gather_f64_dev", rows, depuncture_indices(shouldbe, punct_vec, rows.shape[1]), np.float64)


def _binary_channel_gpu(which, input_bits, p, seed, stream_id):
    bits = np.ascontiguousarray(input_bits, dtype=np.uint8)
    with _OneShot() as dev:
        d_out = dev.alloc(bits.size)
        _lib.check(getattr(dev.lib, which)(dev.upload(bits), bits.size, float(p), int(seed), int(stream_id), d_out.ptr, None, None))
        return dev.download(d_out, bits.shape, np.int8)


def bsc_gpu(input_bits, p_t, seed=0, stream_id=0):
    """``bsc(input_bits, p_t)`` (channels.py:652-673) on the GPU: every bit flipped with probability ``p_t``.  The draws come
    from the Philox stream ``(seed, stream_id)``, not from NumPy's MT19937 generator: an exactly specified function of (seed,
    stream id, position) (include/commpy_amd.h, "Random streams"), tested against the NumPy model tests/rng_model.py."""
    return _binary_channel_gpu("cpx_bsc_dev", input_bits, p_t, seed, stream_id)


def bec_gpu(input_bits, p_e, seed=0, stream_id=0):
    """``bec(input_bits, p_e)`` (channels.py:630-649) on the GPU: every bit erased (-1) with probability ``p_e``."""
    return _binary_channel_gpu("cpx_bec_dev", input_bits, p_e, seed, stream_id)


def turbo_encode_gpu(msg_bits, trellis1, trellis2, interleaver, mode=0):
    """``turbo_encode`` (turbo.py:14-59) for a batch ``[B, N]`` of messages on the GPU.

    Returns ``[sys, p1, p2]`` as int64 arrays ``[B, N]``, ``[B, N]`` and ``[B, 2(N+m2)-m2]``: row ``b`` of each equals
    what the reference returns for ``msg_bits[b]`` (the second parity stream keeps ``conv_encode``'s
    unpunctured length with a zero tail -- use ``p2[:, :N]``).  ``mode``: 0 auto, 1 walk, 2 scan kernel.
    """
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
    with _OneShot() as dev:
        d_sys, d_p1, d_p2 = dev.alloc(B * N), dev.alloc(B * N), dev.alloc(B * np2)
        _lib.check(dev.lib.cpx_turbo_encode_batch_dev(trellis1._device_handle(), trellis2._device_handle(), dev.upload(msgs), B, N,
                                                      dev.upload(perm), d_sys.ptr, d_p1.ptr, d_p2.ptr, np2, int(mode), None))
        return [dev.download(d, (B, cols), np.uint8).astype(np.int64) for d, cols in ((d_sys, N), (d_p1, N), (d_p2, np2))]


def gf2_generator(ldpc_code_params):
    """Systematic generator over GF(2): ``P`` (uint8 ``[m, k]``) with ``H[:, k:] @ P = H[:, :k] (mod 2)``.

    ``build_matrix`` (ldpc.py:44-48) inverts the last ``m`` columns of H over the *reals*, which is only a valid GF(2)
    inverse for (approximately) triangular codes; this is the same construction done in GF(2) arithmetic, so it
    also covers codes like the 802.11n (1944,1296) matrix of BASELINE config 4 whose real inverse is not integral.
    """
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
        self.lib = lib = _lib.load()
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
        self.G2 = G2 = np.ascontiguousarray(G2, dtype=np.uint8)
        self.m, self.k = m, k = G2.shape
        self.n = self.m + self.k

        def create():
            h = ctypes.c_void_p()
            _lib.check(lib.cpx_ldpc_encoder_create(_lib.ptr(G2), m, k, ctypes.byref(h)))
            return h
        self._handles = _lib.DeviceHandles(create, 'cpx_ldpc_encoder_destroy')
        self._handles.get()                 # now, so that a missing device or a refused generator fails the constructor

    @property
    def h(self):
        """Opaque cpx_ldpc_encoder* of the current device (one per device, created on first use there)."""
        return self._handles.get()

    def encode_dev(self, d_msg, B, d_code, stream=None):
        """msg ``[B][k]`` uint8 (device) -> code ``[B][n]`` uint8 (device); asynchronous on ``stream``."""
        _lib.check(self.lib.cpx_ldpc_encode_batch_dev(self.h, d_msg, int(B), d_code, stream))

    def encode(self, msgs):
        """Host convenience: uint8/int ``[B, k]`` -> int8 ``[B, n]``."""
        msgs = np.ascontiguousarray(np.atleast_2d(msgs), dtype=np.uint8)
        B, k = msgs.shape
        if k != self.k:
            raise ValueError('messages must have %d bits' % self.k)
        with _OneShot() as dev:
            d_code = dev.alloc(B * self.n)
            self.encode_dev(dev.upload(msgs), B, d_code.ptr)
            return dev.download(d_code, (B, self.n), np.int8)


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


# ---- the MIMO fading channel --------------------------------------------------------------------------------------------------

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
    come from the Philox streams ``(seed, 2 stream_id)`` and ``(seed, 2 stream_id + 1)`` instead of NumPy's MT19937 generator (an
    exactly specified function of seed, stream id and element index, tested against tests/rng_model.py);
    ``H = sqrtm(Rr) G sqrtm(Rt).T + mean`` and the noise of per-component std ``noise_std / 2`` follow channels.py (quirk B7)."""
    _require_complex(channel)
    if channel.noise_std is None:
        raise AssertionError('Noise standard deviation must be set before propagation.')
    nr, nt, nb = channel.nb_rx, channel.nb_tx, modem.num_bits_symbol
    flat = np.ascontiguousarray(bits, dtype=np.uint8).reshape(-1)
    if flat.size % (nt * nb):
        raise ValueError('%d bits do not fill whole vectors of %d symbols of %d bits' % (flat.size, nt, nb))
    V = flat.size // (nt * nb)
    handles = _channel_handles(channel)
    try:
        with _OneShot() as dev:
            d_y, d_h = dev.alloc(V * nr * 16), dev.alloc(V * nr * nt * 16)
            _lib.check(dev.lib.cpx_mimo_channel_run_dev(handles.get(), modem._device_handle(), dev.upload(flat), V, 0,
                                                        float(channel.noise_std) * 0.5, int(seed), 2 * int(stream_id),
                                                        2 * int(stream_id) + 1, d_y.ptr, d_h.ptr, None))
            return dev.download(d_y, (V, nr), np.complex128), dev.download(d_h, (V, nr, nt), np.complex128)
    finally:
        handles.drop()


# ---- the multipath channel, resource mapping and channel estimation, device resident (csrc/ofdm_chan.hip) -----------------------

def multipath_dev(d_x, d_g, g_batched, B, nt, nr, n, L, stream=None):
    """``cpx_multipath_dev`` over ``DeviceBuf``s: ``d_x [B][nt][n]``, ``d_g [B][nr][nt][L]`` (``g_batched``) or ``[nr][nt][L]`` ->
    a new ``DeviceBuf`` ``[B][nr][n + L - 1]`` (complex128), queued on ``stream`` (None: the library's)."""
    d_y = DeviceBuf(B * nr * (n + L - 1) * 16)
    _lib.check(d_y.lib.cpx_multipath_dev(d_x.ptr, d_g.ptr, int(bool(g_batched)), B, nt, nr, n, L, d_y.ptr, stream))
    return d_y


def ofdm_map_dev(pilots, d_data, B, stream=None):
    """``cpx_pilots_map_dev``: ``d_data [B][ndata][nt]`` -> a new ``DeviceBuf`` ``[B][nt][nsym][nsc]``, ``cpx_ofdm_tx_dev``'s input."""
    d_grid = DeviceBuf(B * pilots.nt * pilots.nsym * pilots.nsc * 16)
    _lib.check(d_grid.lib.cpx_pilots_map_dev(pilots.handle(), d_data.ptr, B, d_grid.ptr, stream))
    return d_grid


def _ofdm_estimate(entry, third, dims, pilots, d_Y, B, nr, want, stream):
    """Both estimators: ``entry`` writes y_data, h_data and its own third output, ``third`` ``[B][*dims][nr][nt]``."""
    from commpy_amd.modulation import ofdm_estimate_shapes
    shapes = ofdm_estimate_shapes(pilots, B, nr, third, dims)
    out, p = device_outputs(_lib.wanted(want, tuple(shapes)), shapes)
    _lib.check(getattr(_lib.load(), entry)(pilots.handle(), d_Y.ptr, B, nr, p(third), p('y'), p('h'), stream))
    return tuple(out.values())


def ofdm_estimate_dev(pilots, d_Y, B, nr, want=('y', 'h'), stream=None):
    """``cpx_pilots_estimate_dev``: ``d_Y [B][nr][nsym][nsc]`` -> a tuple of new ``DeviceBuf``s, the members of ``(y_data
    [B][ndata][nr], h_data [B][ndata][nr][nt], h_sc [B][nsc][nr][nt])`` that ``want`` names ('y', 'h', 'h_sc'), in that order:
    the first two are the ``y`` and ``H`` of the ``cpx_mimo_*_dev`` / ``cpx_kbest_*_dev`` detectors for ``V = B ndata`` vectors."""
    return _ofdm_estimate('cpx_pilots_estimate_dev', 'h_sc', (pilots.nsc,), pilots, d_Y, B, nr, want, stream)


def ofdm_estimate_tv_dev(pilots, d_Y, B, nr, want=('y', 'h'), stream=None):
    """``cpx_pilots_estimate_tv_dev`` (``pilots`` made with ``time_interp``): ``d_Y [B][nr][nsym][nsc]`` -> a tuple of new
    ``DeviceBuf``s, the members of ``(y_data [B][ndata][nr], h_data [B][ndata][nr][nt], h_sym [B][nsym][nsc][nr][nt])`` that ``want``
    names ('y', 'h', 'h_sym'), in that order; the first two feed the detectors as ``ofdm_estimate_dev``'s do."""
    return _ofdm_estimate('cpx_pilots_estimate_tv_dev', 'h_sym', (pilots.nsym, pilots.nsc), pilots, d_Y, B, nr, want, stream)


# ---- timing and frequency-offset synchronisation, device resident (csrc/sync.hip) -------------------------------------------------

def sync_estimate_dev(d_y, B, nr, n, lag, window, search=None, stream=None):
    """``cpx_sync_estimate_dev``: ``d_y [B][nr][n]`` -> new ``DeviceBuf``s ``(d_hat [B] int64, peak [B], step [B])``, queued on ``stream``;
    ``search = (d_lo, d_hi)`` or None for the whole row."""
    lo, hi = (0, (1 << 63) - 1) if search is None else search
    d_hat, peak, step = DeviceBuf(B * 8), DeviceBuf(B * 8), DeviceBuf(B * 8)
    _lib.check(d_hat.lib.cpx_sync_estimate_dev(d_y.ptr, B, nr, n, lag, window, lo, hi, d_hat.ptr, peak.ptr, step.ptr, stream))
    return d_hat, peak, step


def sync_align_dev(d_y, B, nr, n, d_start, d_step, nout, offset=0, stream=None):
    """``cpx_sync_align_dev``: rows ``[B][nr][n]`` cut at ``d_start[b] + offset`` (device int64, e.g. ``sync_estimate_dev``'s d_hat with
    ``offset = -cp_length``) and rotated by ``d_step[b]`` per sample (device float64; None: a pure copy) -> a new ``DeviceBuf``
    ``[B][nr][nout]``."""
    d_out = DeviceBuf(B * nr * nout * 16)
    _lib.check(d_out.lib.cpx_sync_align_dev(d_y.ptr, B, nr, n, d_start.ptr, None if d_step is None else d_step.ptr, offset, nout,
                                            d_out.ptr, stream))
    return d_out


# ---- the Doppler-fading multipath channel, device resident (csrc/fading.hip) -------------------------------------------------------

def _fading_model(B, nr, nt, pdp, fd, hold, t0, n_sin, k_factor, fd_los, seed, stream_id, first_row):
    from commpy_amd.channels import _FadingModel
    return _FadingModel(B, nr, nt, pdp, fd, hold, t0, n_sin, k_factor, fd_los, seed, stream_id, first_row)


def fading_params_dev(B, nr, nt, L, fd, n_sin=16, fd_los=0.0, seed=0, stream_id=0, first_row=0, stream=None):
    """``cpx_fading_params_dev``: a new ``DeviceBuf`` ``[B][nr][nt][L][n_sin + 1][2]`` float64 of every sinusoid's (nu, phi), queued on
    ``stream`` (None: the library's).  The arguments are those of ``channels.fading_params_batch``."""
    from commpy_amd.channels import _whole
    md = _fading_model(B, nr, nt, np.ones(_whole(L, 'L', 1)), fd, 1, 0, n_sin, None, fd_los, seed, stream_id, first_row)
    d_out = DeviceBuf(md.B * md.nr * md.nt * md.L * (md.n_sin + 1) * 16)
    _lib.check(d_out.lib.cpx_fading_params_dev(md.B, md.nr, md.nt, md.L, *md.draw_args(), *md.key_args(), d_out.ptr, stream))
    return d_out


def fading_gains_dev(B, nr, nt, pdp, fd, nblk, hold=1, t0=0, n_sin=16, k_factor=None, fd_los=0.0, seed=0, stream_id=0, first_row=0,
                     stream=None):
    """``cpx_fading_gains_dev``: a new ``DeviceBuf`` ``G [B][nblk][nr][nt][L]`` (complex128), queued on ``stream``.  The arguments are
    those of ``channels.fading_gains_batch``; ``pdp`` and ``k_factor`` are host arrays."""
    md = _fading_model(B, nr, nt, pdp, fd, hold, t0, n_sin, k_factor, fd_los, seed, stream_id, first_row)
    nblk = md.blocks(nblk)
    d_G = DeviceBuf(md.B * nblk * md.nr * md.nt * md.L * 16)
    _lib.check(d_G.lib.cpx_fading_gains_dev(md.B, md.nr, md.nt, md.L, *md.tap_args(), *md.draw_args(), md.hold, md.t0, nblk,
                                            *md.key_args(), d_G.ptr, stream))
    return d_G


def fading_convolve_dev(d_x, d_G, g_batched, B, nt, nr, n, L, hold, stream=None):
    """``cpx_fading_convolve_dev`` over ``DeviceBuf``s: ``d_x [B][nt][n]``, ``d_G [B][nblk][nr][nt][L]`` (``g_batched``) or
    ``[nblk][nr][nt][L]`` with ``nblk = ceil((n + L - 1) / hold)`` -> a new ``DeviceBuf`` ``[B][nr][n + L - 1]``."""
    d_y = DeviceBuf(B * nr * (n + L - 1) * 16)
    _lib.check(d_y.lib.cpx_fading_convolve_dev(d_x.ptr, d_G.ptr, int(bool(g_batched)), B, nt, nr, n, L, hold, d_y.ptr, stream))
    return d_y


def fading_channel_dev(d_x, B, nt, nr, n, pdp, fd, hold=1, t0=0, n_sin=16, k_factor=None, fd_los=0.0, seed=0, stream_id=0, first_row=0,
                       want=('y',), stream=None):
    """``cpx_fading_channel_dev``: ``d_x [B][nt][n]`` through the fading channel -> new ``DeviceBuf``s, the members of ``(y [B][nr][n + L
    - 1], G [B][nblk][nr][nt][L])`` that ``want`` names ('y', 'g'), in that order (a single ``DeviceBuf`` for ``want=('y',)``).  Without
    'g' the gains stay in the engine's scratch arena, at most ``channels.FADING_SCRATCH_BYTES`` of it."""
    want = _lib.wanted(want, ('y', 'g'))
    md = _fading_model(B, nr, nt, pdp, fd, hold, t0, n_sin, k_factor, fd_los, seed, stream_id, first_row)
    if md.B and (isinstance(n, (bool, np.bool_)) or not isinstance(n, (int, np.integer)) or n < 1):
        raise ValueError('n = %r, need an integer >= 1' % (n,))
    lout = n + md.L - 1
    nblk = md.blocks(-(-lout // md.hold)) if md.B else 1
    out, p = device_outputs(want, md.shapes(lout, nblk))
    _lib.check(_lib.load().cpx_fading_channel_dev(d_x.ptr if 'y' in want else None, md.B, md.nt, md.nr, n, md.L, *md.tap_args(),
                                                  *md.draw_args(), md.hold, md.t0, *md.key_args(), p('y'), p('g'), stream))
    return out['y'] if want == ('y',) else tuple(out.values())


# ---- polar codes, device resident (csrc/polar.hip) ----------------------------------------------------------------------------------

def polar_encode_dev(code, d_msg, B, stream=None):
    """``cpx_polar_encode_dev``: ``d_msg [B][A]`` uint8 -> a new ``DeviceBuf`` ``[B][N]`` uint8 of code words, queued on ``stream``
    (None: the library's); ``code`` is a ``channelcoding.PolarCode``."""
    from commpy_amd.channelcoding.polar import _code
    code, B = _code(code), whole(B, 'B', 0)
    d_x = DeviceBuf(B * code.N)
    if B:
        _lib.check(d_x.lib.cpx_polar_encode_dev(code._device_handle(), d_msg.ptr, B, d_x.ptr, stream))
    return d_x


def polar_decode_dev(code, d_llr, B, list_size=1, want=('bits',), stream=None):
    """``cpx_polar_decode_dev``: ``d_llr [B][N]`` float64 -> new ``DeviceBuf``s, the results of ``channelcoding.polar_decode`` that
    ``want`` names, in its order: 'bits' ``[B][A]`` uint8, 'crc' ``[B]`` uint8, 'metric' ``[B]`` float64, 'u_llr' ``[B][N]`` float64
    (``list_size = 1``), 'list' a tuple ``(bits [B][L][K] uint8, metrics [B][L] float64, live [B] int32)``; a single result for one
    name."""
    from commpy_amd.channelcoding.polar import _code, check_want, list_shapes, shapes
    code, B = _code(code), whole(B, 'B', 0)
    L = code.check_list_size(list_size)
    want = check_want(want, L)
    tables = shapes(B, code), list_shapes(B, code, L)
    out, p = device_outputs(want, tables[0])
    lst, q = device_outputs(tables[1] if 'list' in want else (), tables[1])
    if B:
        _lib.check(_lib.load().cpx_polar_decode_dev(code._device_handle(), d_llr.ptr, B, L, *map(p, tables[0]), *map(q, tables[1]), stream))
    if lst:
        out['list'] = tuple(lst.values())                     # 'list' is the last name
    return returned(out)


# ---- BCH codes, device resident (csrc/bch.hip) --------------------------------------------------------------------------------------

def bch_encode_dev(code, d_msg, B, stream=None):
    """``cpx_bch_encode_dev``: ``d_msg [B][k]`` uint8 -> a new ``DeviceBuf`` ``[B][n]`` uint8 of code words, queued on ``stream``
    (None: the library's); ``code`` is a ``channelcoding.BCHCode``."""
    from commpy_amd.channelcoding.bch import _code
    code, B = _code(code), whole(B, 'B', 0)
    d_x = DeviceBuf(B * code.n)
    if B:
        _lib.check(d_x.lib.cpx_bch_encode_dev(code._device_handle(), d_msg.ptr, B, d_x.ptr, stream))
    return d_x


def bch_decode_dev(code, d_bits, B, want=('bits',), stream=None):
    """``cpx_bch_decode_dev``: ``d_bits [B][n]`` uint8 hard decisions (non-zero = 1) -> new ``DeviceBuf``s, the results of
    ``channelcoding.bch_decode`` that ``want`` names, in its order: 'bits' ``[B][k]`` uint8, 'codeword' ``[B][n]`` uint8, 'errors'
    ``[B]`` int32; a single result for one name."""
    from commpy_amd.channelcoding.bch import WANT, _code, check_want, shapes
    code, B = _code(code), whole(B, 'B', 0)
    out, p = device_outputs(check_want(want), shapes(B, code))
    if B:
        _lib.check(_lib.load().cpx_bch_decode_dev(code._device_handle(), d_bits.ptr, B, *map(p, WANT), stream))
    return returned(out)


# ---- Chase-II BCH decoding and turbo product codes, device resident (csrc/bch_chase.hip) -----------------------------------------------

def bch_chase_dev(code, d_llr, B, p, beta, d_prior=None, alpha=1.0, want=('bits',), J=1, strides=None, d_extrinsic=None, stream=None):
    """``cpx_chase_bch_dev``: Chase-II decoding of the ``B * J`` words of ``d_llr`` (float64), queued on ``stream``.  Element ``i`` of
    word ``(b, j)`` is at ``b sb + j sj + i si`` with ``strides = (sb, sj, si)`` in elements (default: the flat batch ``(n, 0, 1)``,
    which needs ``J = 1``); ``d_prior`` (optional) and the 'extrinsic' and 'codeword' results have the same layout, so that the rows
    or the columns of a block decode in place.  Returns new ``DeviceBuf``s, the results of ``channelcoding.chase_decode`` that
    ``want`` names, in its order: 'bits' uint8 (dense, nested as the input: ``[B][J][k]``, or ``[B][k][J]`` where the word axis is the
    inner one), 'codeword' uint8 and 'extrinsic' float64 (each as large as ``sb * B`` elements), 'metric' float64 and 'candidates'
    int32 ``[B][J]``.  ``d_extrinsic``: write the soft output there instead of into a new buffer -- it may be ``d_prior``."""
    from commpy_amd.channelcoding.bch import CHASE_WANT, chase_args, chase_shapes
    code, p, beta, alpha, want = chase_args(code, p, beta, alpha, want)
    B, J = whole(B, 'B', 0), whole(J, 'J', 1)
    if strides is None:
        if J != 1:
            raise ValueError('J = %d needs strides' % J)
        strides = (code.n, 0, 1)
    if len(strides) != 3:
        raise ValueError('strides must be (sb, sj, si)')
    sb, sj, si = (whole(v, 'stride', 0, (1 << 40) - 1) for v in strides)
    span_i, span_j = (code.n - 1) * si, (J - 1) * sj
    if si < 1 or (J > 1 and not (sj > span_i or (sj >= 1 and si > span_j))) or (B > 1 and sb <= span_i + span_j):
        raise ValueError('strides %r: the words overlap' % (tuple(strides),))
    if d_extrinsic is not None and 'extrinsic' not in want:
        raise ValueError("d_extrinsic needs 'extrinsic' in want")
    extent = (B - 1) * sb + span_i + span_j + 1 if B else 0
    out, q = device_outputs(want, chase_shapes((B, J), code.k, (extent,)), {'extrinsic': d_extrinsic})
    if B:
        _lib.check(_lib.load().cpx_chase_bch_dev(code._device_handle(), d_llr.ptr, None if d_prior is None else d_prior.ptr, alpha, beta, p,
                                                 B, J, sb, sj, si, *map(q, CHASE_WANT), stream))
    return returned(out)


def tpc_decode_dev(code, d_llr, B, iters=4, p=4, alpha=None, beta=None, llr_scale=1.0, want=('codeword',), stream=None):
    """Iterative decoding of ``B`` blocks ``d_llr [B][n_c][n_r]`` float64 of a ``channelcoding.ProductCode``, all on the device:
    ``2 * iters`` Chase launches on ``stream``, alternately along the rows and the columns in place, each taking the extrinsic output
    of the one before as its prior (``channelcoding.tpc_decode`` states the schedule).  Returns new ``DeviceBuf``s, what ``want``
    names out of 'codeword' ``[B][n_c][n_r]`` uint8 (the decision of the last half-iteration) and 'extrinsic'
    ``[B][n_c][n_r]`` float64 (its soft output), in this order."""
    from commpy_amd.channelcoding.productcode import TPC_DEV_WANT, shapes, tpc_args
    code, iters, p, alpha, beta = tpc_args(code, iters, p, alpha, beta, llr_scale)
    B = whole(B, 'B', 0)
    want = _lib.wanted(want, TPC_DEV_WANT)
    nr, nc = code.n_r, code.n_c
    d_w = device_outputs(('extrinsic',), shapes(B, code))[0]['extrinsic']     # W, the extrinsic information: zero, then rewritten in place
    if B:
        _lib.check(d_w.lib.cpx_memset(d_w.ptr, 0, d_w.nbytes))
    d_word = None
    for h in range(2 * iters):
        rows = h % 2 == 0
        comp, J, strides = (code.row_code, nc, (nc * nr, nr, 1)) if rows else (code.col_code, nr, (nc * nr, 1, nr))
        last = h == 2 * iters - 1
        names = ('codeword', 'extrinsic') if last and 'codeword' in want else ('extrinsic',)
        res = bch_chase_dev(comp, d_llr, B, min(p, comp.n), beta[h], d_prior=d_w, alpha=alpha[h], want=names, J=J, strides=strides,
                            d_extrinsic=d_w, stream=stream)
        if len(names) == 2:
            d_word = res[0]
    out = {'codeword': d_word, 'extrinsic': d_w}
    return returned({k: out[k] for k in TPC_DEV_WANT if k in want})


# ---- Reed-Solomon codes, device resident (csrc/rs.hip) ------------------------------------------------------------------------------

def rs_encode_dev(code, d_msg, B, stream=None):
    """``cpx_rs_encode_dev``: ``d_msg [B][k]`` uint16 -> a new ``DeviceBuf`` ``[B][n]`` uint16 of code words, queued on ``stream``
    (None: the library's); ``code`` is a ``channelcoding.RSCode``.  Only the low ``m`` bits of a symbol count."""
    from commpy_amd.channelcoding.rs import _code
    code, B = _code(code), whole(B, 'B', 0)
    d_x = DeviceBuf(2 * B * code.n)
    if B:
        _lib.check(d_x.lib.cpx_rs_encode_dev(code._device_handle(), d_msg.ptr, B, d_x.ptr, stream))
    return d_x


def rs_decode_dev(code, d_symbols, B, d_erased=None, want=('symbols',), stream=None):
    """``cpx_rs_decode_dev``: ``d_symbols [B][n]`` uint16 received symbols (the low ``m`` bits count) and ``d_erased [B][n]`` uint8
    flags (non-zero = erased; None: no flags) -> new ``DeviceBuf``s, the results of ``channelcoding.rs_decode`` that ``want`` names,
    in its order: 'symbols' ``[B][k]`` uint16, 'codeword' ``[B][n]`` uint16, 'errors' ``[B]`` int32; a single result for one name."""
    from commpy_amd.channelcoding.rs import WANT, _code, check_want, shapes
    code, B = _code(code), whole(B, 'B', 0)
    out, p = device_outputs(check_want(want), shapes(B, code))
    if B:
        _lib.check(_lib.load().cpx_rs_decode_dev(code._device_handle(), d_symbols.ptr, None if d_erased is None else d_erased.ptr, B,
                                                 *map(p, WANT), stream))
    return returned(out)


# ---- tail-biting convolutional codes, device resident (csrc/tbcc.hip) ---------------------------------------------------------------

def tailbiting_encode_dev(trellis, d_msg, B, T, stream=None):
    """``cpx_tbcc_encode_dev``: ``d_msg [B][T k]`` uint8 (bit 0 of a byte counts) -> two new ``DeviceBuf``s queued on ``stream`` (None:
    the library's): the code words ``[B][T n]`` uint8 and ``closed [B]`` uint8, 1 where the emitting walk ended in the state in which it
    began (``channelcoding.tailbiting_encode`` raises where it is 0).  ``trellis`` is a ``Trellis`` or any duck-typed trellis."""
    from commpy_amd.channelcoding.convcode import device_trellis
    from commpy_amd.channelcoding.tailbiting import check_block, check_trellis
    k, n = check_trellis(trellis)
    B, T = whole(B, 'B', 0), check_block(whole(T, 'T', 1), k)
    d_x, d_closed = DeviceBuf(B * T * n), DeviceBuf(B)
    if B:
        _lib.check(d_x.lib.cpx_tbcc_encode_dev(device_trellis(trellis), d_msg.ptr, B, T, d_x.ptr, d_closed.ptr, stream))
    return d_x, d_closed


def tailbiting_decode_dev(trellis, d_coded, B, T, decoding_type='hard', max_wraps=4, want=('bits',), stream=None):
    """``cpx_tbcc_decode_dev``: ``d_coded [B][T n]`` float64 -> new ``DeviceBuf``s, the results of ``channelcoding.tailbiting_decode``
    that ``want`` names, in its order: 'bits' ``[B][T k]`` uint8, 'wraps' ``[B]`` int32, 'tailbiting' ``[B]`` uint8, 'metric' ``[B]``
    float64; a single result for one name."""
    from commpy_amd.channelcoding.convcode import device_trellis
    from commpy_amd.channelcoding.tailbiting import WANT, check_block, check_max_wraps, check_trellis, check_type, check_want, shapes
    k, n = check_trellis(trellis)
    vtype, max_wraps, want = check_type(decoding_type), check_max_wraps(max_wraps), check_want(want)
    B, T = whole(B, 'B', 0), check_block(whole(T, 'T', 1), k)
    out, p = device_outputs(want, shapes(B, T, k))
    if B:
        _lib.check(_lib.load().cpx_tbcc_decode_dev(device_trellis(trellis), d_coded.ptr, B, T, vtype, max_wraps, *map(p, WANT), stream))
    return returned(out)


# ---- layered min-sum LDPC decoding, device resident (csrc/ldpc_layered.hip) ---------------------------------------------------------

def ldpc_layered_decode_dev(ldpc_code_params, d_llr, B, n_iters, alpha=1.0, beta=0.0, schedule=None, early_stop=True, llr_clip=500.0,
                            want=('bits',), stream=None):
    """``cpx_ldpc_layered_decode_dev``: ``d_llr [B][n_v]`` float64 (left unchanged) -> new ``DeviceBuf``s queued on ``stream`` (None: the
    library's), the results of ``channelcoding.ldpc_layered_decode`` that ``want`` names, in its order: 'bits' ``[B][n_v]`` int8, 'llr'
    ``[B][n_v]`` float64, 'iters' ``[B]`` int32, 'converged' ``[B]`` uint8; a single result for one name.  The same checks, on the host,
    before any device call."""
    from commpy_amd.channelcoding.ldpc_layered import WANT, check_n_iters, check_scaling, check_want, plan, shapes
    n_iters = check_n_iters(n_iters)
    alpha, beta, llr_clip = check_scaling(alpha, beta, llr_clip)
    want = check_want(want)
    p = plan(ldpc_code_params, schedule)
    B = whole(B, 'B', 0)
    out, q = device_outputs(want, shapes(B, p.n_v))
    if B:
        _lib.check(_lib.load().cpx_ldpc_layered_decode_dev(p.handle(), d_llr.ptr, B, n_iters, alpha, beta, 1 if early_stop else 0, llr_clip,
                                                           *map(q, WANT), stream))
    return returned(out)


# ---- trellis equalisation, device resident (csrc/mlse.hip) --------------------------------------------------------------------------

def mlse_equalize_dev(modem, d_y, d_h, h_batched, B, n, L, d_noise_var=None, nv_batched=False, d_prior=None, tail=True,
                      want=('indices',), stream=None):
    """``cpx_mlse_dev``: ``d_y [B][n_y][2]`` float64 (re, im; ``n_y = n + L - 1`` with ``tail``, else ``n``) received through the taps
    ``d_h [L][2]`` or, with ``h_batched``, ``[B][L][2]`` -> new ``DeviceBuf``s queued on ``stream`` (None: the library's), the results of
    ``equalizers.mlse_equalize_batch`` that ``want`` names, in its order: 'indices' ``[B][n]`` int32, 'bits' ``[B][n m]`` uint8,
    'metric' ``[B]`` float64, 'llr' ``[B][n m]`` float64; a single result for one name.  ``d_noise_var``: one float64 or, with
    ``nv_batched``, ``[B]``, required for 'llr' and with ``d_prior [B][n m]``.  The same limits, checked on the host before any device
    call."""
    from commpy_amd.equalizers import WANT, check_sizes, check_want, mlse_shapes
    want = check_want(want)
    B, n, L = whole(B, 'B', 0), whole(n, 'n', 1), whole(L, 'L', 2)
    M, m = check_sizes(modem, L, n)
    if d_noise_var is None and ('llr' in want or d_prior is not None):
        raise ValueError("noise_var is required when 'llr' is wanted or a prior is given")
    out, p = device_outputs(want, mlse_shapes(B, n, m))
    if B:
        _lib.check(_lib.load().cpx_mlse_dev(modem._device_handle(), d_y.ptr, d_h.ptr, int(bool(h_batched)), B, n, L, int(bool(tail)),
                                            None if d_noise_var is None else d_noise_var.ptr, int(bool(nv_batched)),
                                            None if d_prior is None else d_prior.ptr, *map(p, WANT), stream))
    return returned(out)


# ---- MMSE linear and decision-feedback equalisation, device resident (csrc/equalize.hip) --------------------------------------------

def mmse_equalize_dev(modem, d_y, d_h, h_batched, B, n, L, d_noise_var, nv_batched, nf, nb=0, delay=None, tail=True,
                      want=('indices',), stream=None):
    """``cpx_mmse_equalize_dev``: ``d_y [B][n_y][2]`` float64 (re, im; ``n_y = n + L - 1`` with ``tail``, else ``n``) received through
    the taps ``d_h [L][2]`` or, with ``h_batched``, ``[B][L][2]``; ``d_noise_var``: one float64 or, with ``nv_batched``, ``[B]`` -> new
    ``DeviceBuf``s queued on ``stream`` (None: the library's), the results of ``equalizers.mmse_equalize_batch`` that ``want`` names,
    in its order: 'indices' ``[B][n]`` int32, 'bits' ``[B][n m]`` uint8, 'estimate' ``[B][n][2]``, 'llr' ``[B][n m]``, 'noise' ``[B]``,
    'ff' ``[B][nf][2]``, 'fb' ``[B][nb][2]``, 'gain' ``[B]`` float64; a single result for one name.  The same rule and the same limits,
    checked on the host before any device call."""
    from commpy_amd.equalizers import MMSE_WANT, check_mmse_sizes, mmse_shapes
    want = _lib.wanted(want, MMSE_WANT)
    B, n, L, nf, nb = whole(B, 'B', 0), whole(n, 'n', 1), whole(L, 'L', 1), whole(nf, 'nf', 1), whole(nb, 'nb', 0)
    M, m, delay = check_mmse_sizes(modem, L, n, nf, nb, None if delay is None else int(delay), want)
    if d_noise_var is None:
        raise ValueError('noise_var is required')
    out, p = device_outputs(want, mmse_shapes(B, n, m, nf, nb))
    if B:
        _lib.check(_lib.load().cpx_mmse_equalize_dev(modem._device_handle(), float(modem.Es), d_y.ptr, d_h.ptr, int(bool(h_batched)), B, n,
                                                     L, int(bool(tail)), d_noise_var.ptr, int(bool(nv_batched)), nf, nb, delay,
                                                     *map(p, MMSE_WANT), stream))
    return returned(out)


# ---- adaptive LMS / NLMS / RLS equalisation, device resident (csrc/adaptive.hip) -----------------------------------------------------

def adaptive_equalize_dev(modem, d_y, B, n_y, d_training, tr_batched, nt, nf, nb=0, algorithm='lms', d_step=None, step_batched=False,
                          d_forgetting=None, fg_batched=False, d_delta=None, dl_batched=False, eps=1e-6, delay=None, sps=1, n=None,
                          d_ff0=None, ff0_batched=False, d_fb0=None, fb0_batched=False, want=('indices',), stream=None):
    """``cpx_adaptive_equalize_dev``: ``d_y [B][n_y][2]`` float64 (re, im), ``sps`` samples per symbol; ``d_training`` ``[nt]`` int32
    labels or, with ``tr_batched``, ``[B][nt]`` (None with ``nt = 0``); ``d_step`` (for 'lms', 'nlms'), ``d_forgetting`` and ``d_delta``
    (both required for 'rls'): one float64 each or, with their ``_batched`` flag, ``[B]``; ``d_ff0 [nf][2]`` / ``d_fb0 [nb][2]`` or, batched,
    ``[B][..][2]``, None = zeros -> new ``DeviceBuf``s queued on ``stream`` (None: the library's), the results of
    ``equalizers.adaptive_equalize_batch`` that ``want`` names, in its order: 'indices' ``[B][n]`` int32, 'bits' ``[B][n m]`` uint8,
    'estimate' and 'error' ``[B][n][2]``, 'ff' ``[B][nf][2]``, 'fb' ``[B][nb][2]`` float64; a single result for one name.  The same rule
    and the same limits, checked on the host before any device call; the values of step, forgetting and delta are on the device, so
    one outside its range rejects its row."""
    from commpy_amd.equalizers import ADAPT_WANT, adaptive_shapes, check_adaptive_sizes
    want = _lib.wanted(want, ADAPT_WANT)
    B, n_y, nt, nf, nb = whole(B, 'B', 0), whole(n_y, 'n_y', 0), whole(nt, 'nt', 0), whole(nf, 'nf', 1), whole(nb, 'nb', 0)
    sps = int(sps)
    n = n_y // max(sps, 1) if n is None else int(n)
    M, m, delay, code = check_adaptive_sizes(modem, n_y, n, nt, nf, nb, None if delay is None else int(delay), sps, algorithm,
                                             d_step is not None, float(eps), want)
    if algorithm == 'rls' and (d_forgetting is None or d_delta is None):
        raise ValueError("forgetting and delta are required with 'rls'")
    if nt and d_training is None:
        raise ValueError('training is required for nt = %d' % nt)
    opt = lambda buf: None if buf is None else buf.ptr
    out, p = device_outputs(want, adaptive_shapes(B, n, m, nf, nb))
    if B:
        _lib.check(_lib.load().cpx_adaptive_equalize_dev(modem._device_handle(), d_y.ptr, B, n_y, n, sps, opt(d_training),
                                                         int(bool(tr_batched)), nt, nf, nb, delay, code, opt(d_step),
                                                         int(bool(step_batched)), opt(d_forgetting), int(bool(fg_batched)), opt(d_delta),
                                                         int(bool(dl_batched)), float(eps), opt(d_ff0), int(bool(ff0_batched)), opt(d_fb0),
                                                         int(bool(fb0_batched)), *map(p, ADAPT_WANT), stream))
    return returned(out)


# ---- symbol-timing and carrier recovery, device resident (csrc/recovery.hip) ---------------------------------------------------------

def timing_recover_dev(d_y, B, n_y, sps, d_k1, k1_batched, d_k2, k2_batched, d_m0, m0_batched, d_mu0, mu0_batched, d_phase0,
                       phase0_batched, modem=None, ted='gardner', interp='cubic', d_kc1=None, kc1_batched=False, d_kc2=None,
                       kc2_batched=False, d_training=None, tr_batched=False, nt=0, n=None, want=('symbols',), stream=None):
    """``cpx_timing_recover_dev``: ``d_y [B][n_y][2]`` float64 (re, im) at nominally ``sps`` samples per symbol; ``d_k1``, ``d_k2``,
    ``d_mu0``, ``d_phase0`` (float64) and ``d_m0`` (int64): one value each or, with their ``_batched`` flag, ``[B]``; ``d_kc1`` and
    ``d_kc2`` likewise, both given (the carrier loop) or both None; ``d_training`` ``[nt]`` int32 labels or, with ``tr_batched``,
    ``[B][nt]`` (None with ``nt = 0``) -> new ``DeviceBuf``s queued on ``stream`` (None: the library's), the results of
    ``recovery.timing_recover_batch`` that ``want`` names, in its order: 'symbols' ``[B][n][2]`` float64, 'indices' ``[B][n]`` int32,
    'bits' ``[B][n m]`` uint8, 'position', 'error' and 'phase' ``[B][n]`` float64, 'count' ``[B]`` int32; a single result for one name.
    The same rule and the same limits, checked on the host before any device call; the values of the gains and of the loop's start are
    on the device, so one outside its range rejects its row."""
    from commpy_amd.recovery import RECOVERY_WANT, check_recovery_sizes, recovery_shapes, whole_sps
    want = _lib.wanted(want, RECOVERY_WANT)
    B, n_y, nt, sps = whole(B, 'B', 0), whole(n_y, 'n_y', 0), whole(nt, 'nt', 0), whole_sps(sps)
    n = n_y // max(sps, 1) if n is None else int(n)
    if (d_kc1 is None) != (d_kc2 is None):
        raise ValueError('the carrier loop takes both kc1 and kc2')
    M, m, ted_code, interp_code = check_recovery_sizes(modem, n_y, n, nt, sps, ted, interp, d_kc1 is not None, nt > 0, want)
    if d_k1 is None or d_k2 is None:
        raise ValueError('k1 and k2 are required')
    if d_m0 is None or d_mu0 is None or d_phase0 is None:
        raise ValueError('m0, mu0 and phase0 are required')
    if nt and d_training is None:
        raise ValueError('training is required for nt = %d' % nt)
    opt = lambda buf: None if buf is None else buf.ptr
    out, p = device_outputs(want, recovery_shapes(B, n, m))
    if B:
        _lib.check(_lib.load().cpx_timing_recover_dev(None if modem is None else modem._device_handle(), d_y.ptr, B, n_y, n, sps, ted_code,
                                                      interp_code, d_k1.ptr, int(bool(k1_batched)), d_k2.ptr, int(bool(k2_batched)),
                                                      opt(d_kc1), int(bool(kc1_batched)), opt(d_kc2), int(bool(kc2_batched)),
                                                      opt(d_training), int(bool(tr_batched)), nt, d_m0.ptr, int(bool(m0_batched)),
                                                      d_mu0.ptr, int(bool(mu0_batched)), d_phase0.ptr, int(bool(phase0_batched)),
                                                      *map(p, RECOVERY_WANT), stream))
    return returned(out)
