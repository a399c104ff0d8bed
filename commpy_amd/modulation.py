"""PSK / QAM modems with MI355X demodulation.

Same public names, arguments and return conventions as /root/reference/commpy/modulation.py:39-262
(``Modem``, ``PSKModem``, ``QAMModem``).  Construction, Gray re-indexing, ``modulate`` and ``Es`` stay on
the host; ``demodulate`` ('hard' and 'soft') runs on the GPU through ``cpx_demod_hard`` /
``cpx_demod_soft`` (csrc/demod.hip).  The MIMO detectors ``mimo_ml`` and ``kbest`` (modulation.py:299-406) run on the
GPU too (csrc/mimo.hip), with batched forms ``mimo_ml_batch`` / ``kbest_batch`` for throughput; The soft-output
``best_first_detector`` (modulation.py:422-565) runs on the GPU as well, with ``best_first_batch`` as its batched form.
``list_apriori_batch`` is a max-log list detector that takes a-priori LLRs (csrc/mimo_idd.hip), ``apriori_detector`` its form
for ``links.idd_decoder``.  The linear detectors -- zero forcing and MMSE, hard and soft -- are ``zf_detector``, ``mmse_detector``,
``linear_batch`` and ``linear_equalize_batch`` (csrc/mimo_linear.hip; not in the reference).
``max_log_approx`` and ``bit_lvl_repr`` are small host functions.  ``ofdm_tx`` / ``ofdm_rx`` (modulation.py:265-296) run on the
GPU too (csrc/ofdm.hip), float64 only, with the symbol-major batched forms ``ofdm_tx_batch`` / ``ofdm_rx_batch``.
``OfdmPilots`` describes the pilots of an OFDM frame; ``ofdm_map_batch`` puts data and pilots on the resource grid and
``ofdm_estimate_batch`` (``ofdm_estimate_tv_batch`` for a channel that moves inside the frame) estimates the channel from the received
grid and hands ``(y, H)`` to the MIMO detectors in their own layout
(csrc/ofdm_chan.hip; not in the reference).
"""
import ctypes
import numbers
import operator

import numpy as np

from commpy_amd import _lib
from commpy_amd._results import outputs
from commpy_amd.utilities import signal_power

__all__ = ['PSKModem', 'QAMModem', 'Modem', 'mimo_ml', 'kbest', 'max_log_approx', 'bit_lvl_repr', 'mimo_ml_batch',
           'kbest_batch', 'best_first_detector', 'best_first_batch', 'list_apriori_batch', 'apriori_detector', 'zf_detector', 'mmse_detector',
           'linear_batch', 'linear_equalize_batch', 'ofdm_tx', 'ofdm_rx', 'ofdm_tx_batch', 'ofdm_rx_batch', 'OfdmPilots', 'ofdm_map_batch',
           'ofdm_estimate_batch', 'ofdm_estimate_tv_batch', 'ofdm_subcarrier_frequencies']


def _gray_rank(m):
    """Position of each label in the reflected Gray sequence: the reference re-indexes the
    constellation with ``constellation[gray_sequence.argsort()]`` (modulation.py:71-75), where
    ``gray_sequence[i] = i ^ (i >> 1)`` (SymPy's GrayCode order)."""
    idx = np.arange(m)
    return (idx ^ (idx >> 1)).argsort()


class Modem:
    """Custom modem -- modulation.py:39-172.  ``constellation`` must have a power-of-two length."""

    def __init__(self, constellation, reorder_as_gray=True):
        self._cpx_handles = None
        if reorder_as_gray:
            self.constellation = np.array(constellation)[_gray_rank(len(constellation))]
        else:
            self.constellation = constellation

    @property
    def constellation(self):
        return self._constellation

    @constellation.setter
    def constellation(self, value):
        num_bits_symbol = np.log2(len(value))
        if num_bits_symbol != int(num_bits_symbol):
            raise ValueError('Constellation length must be a power of 2.')
        self._constellation = np.array(value)
        self.Es = signal_power(self.constellation)
        self.m = self._constellation.size
        self.num_bits_symbol = int(num_bits_symbol)
        self._drop_handle()

    def modulate(self, input_bits):
        """Bits -> symbols (host): label = MSB-first value of each group of ``num_bits_symbol`` bits
        (modulation.py:79-98)."""
        bits = np.asarray(input_bits).astype(np.int64)
        nb = self.num_bits_symbol
        groups = bits.reshape(-1, nb)
        labels = groups.dot(1 << np.arange(nb - 1, -1, -1))
        return self._constellation[labels]

    def demodulate(self, input_symbols, demod_type, noise_var=0):
        """Symbols -> bits/LLRs on MI355X; same signature/return as modulation.py:100.

        'hard': int8 bits of the nearest point (first minimum), MSB first.
        'soft': float64 LLRs ``log P(1)/P(0)`` with ``noise_var`` used as-is (no factor 2).
        """
        if demod_type not in ('hard', 'soft'):
            raise ValueError('demod_type must be "hard" or "soft"')
        lib = _lib.load()
        y = np.ascontiguousarray(np.atleast_1d(input_symbols), dtype=np.complex128).reshape(-1)
        ns = y.size
        h = self._device_handle()
        if demod_type == 'hard':
            out = np.zeros(ns * self.num_bits_symbol, dtype=np.int8)
            if ns:
                _lib.check(lib.cpx_demod_hard(h, _lib.ptr(y), ns, _lib.ptr(out)))
            return out
        out = np.zeros(ns * self.num_bits_symbol)
        if ns:
            _lib.check(lib.cpx_demod_soft(h, _lib.ptr(y), ns, float(noise_var), _lib.ptr(out)))
        return out

    # -- device handle -----------------------------------------------------------------------
    def _device_handle(self):
        """Opaque cpx_modem* of the current device (created on first use, one per device)."""
        if self._cpx_handles is None:
            def create():
                c = np.ascontiguousarray(self._constellation, dtype=np.complex128)
                h = ctypes.c_void_p()
                _lib.check(_lib.load().cpx_modem_create(_lib.ptr(c), int(self.m), ctypes.byref(h)))
                return h
            self._cpx_handles = _lib.DeviceHandles(create, 'cpx_modem_destroy')
        return self._cpx_handles.get()

    def _drop_handle(self):
        hs = getattr(self, '_cpx_handles', None)
        if hs is not None:
            hs.drop()
        self._cpx_handles = None

    def demodulate_viterbi_hard(self, input_symbols, trellis, tb_depth=None):
        """``viterbi_decode(self.demodulate(y, 'hard'), trellis, tb_depth, 'hard')`` in ONE kernel
        (modulation.py:121-123 feeding convcode.py:578-580, 661-749): the hard decisions are taken inside the
        Viterbi kernel while it prepares the branch metrics, the int8 bits never exist in HBM.  ``input_symbols``:
        1-D (one codeword) or ``[B, nsym]``; returns what the two calls return (int64, tail included).
        Trellises above 64 states take the two calls (the fused kernel keeps one state per lane)."""
        from commpy_amd.channelcoding.convcode import _viterbi_sizes, viterbi_decode
        y = np.ascontiguousarray(input_symbols, dtype=np.complex128)
        single = y.ndim == 1
        y2 = np.atleast_2d(y)
        B, nsym = y2.shape
        length = nsym * self.num_bits_symbol
        if trellis.number_states > 64 or length == 0:
            bits = self.demodulate(y2.reshape(-1), 'hard').reshape(B, length)
            return viterbi_decode(bits[0] if single else bits, trellis, tb_depth, 'hard')
        L, T, tb = _viterbi_sizes(length, trellis, tb_depth)
        out = np.zeros((B, L), dtype=np.uint8)
        if B and L:
            _lib.check(_lib.load().cpx_demod_hard_viterbi_batch(self._device_handle(), trellis._device_handle(),
                                                                _lib.ptr(y2), B, nsym, L, T, tb, _lib.ptr(out)))
        out = out.astype(np.int64)
        return out[0] if single else out


class PSKModem(Modem):
    """m-PSK: ``exp(1j * arange(0, 2*pi, 2*pi/m))`` Gray re-indexed -- modulation.py:175-210."""

    def __init__(self, m):
        num_bits_symbol = np.log2(m)
        if num_bits_symbol != int(num_bits_symbol):
            raise ValueError('Constellation length must be a power of 2.')
        super().__init__(np.exp(1j * np.arange(0, 2 * np.pi, 2 * np.pi / m)))


class QAMModem(Modem):
    """Square m-QAM on the odd-integer grid, snake ordered then Gray re-indexed -- modulation.py:213-262."""

    def __init__(self, m):
        side = np.sqrt(m)
        if side != int(side):
            raise ValueError('m must lead to a square QAM.')
        side = int(side)
        pam = np.arange(-side + 1, side, 2)
        # column c (real part pam[c]) runs upwards for even c, downwards for odd c
        imag = np.tile(np.hstack((pam, pam[::-1])), side // 2)
        real = pam.repeat(side)
        super().__init__(imag * 1j + real)


# ---- MIMO detection (csrc/mimo.hip) ------------------------------------------------------------------------------------------
_const_modems = {}


def _modem_for(constellation):
    """A Modem over ``constellation`` as given (no Gray re-indexing): the device copy the MIMO kernels search over.  Kept per
    constellation so that a link simulation does not re-upload it for every vector.  The engine's modems need a power-of-two
    number of points (ValueError otherwise)."""
    pts = np.ascontiguousarray(constellation, dtype=np.complex128).reshape(-1)
    key = pts.tobytes()
    md = _const_modems.get(key)
    if md is None:
        if len(_const_modems) > 64:
            _const_modems.clear()
        md = _const_modems[key] = Modem(pts, reorder_as_gray=False)
    return md


def _mimo_inputs(y, h):
    """(y [B, nr], h, h_batched, B, nr, nt) as complex128 C arrays; h is [nr, nt] (shared) or [B, nr, nt]."""
    y2 = np.ascontiguousarray(np.atleast_2d(y), dtype=np.complex128)
    hh = np.ascontiguousarray(h, dtype=np.complex128)
    if hh.ndim not in (2, 3):
        raise ValueError('h must be [nr, nt] or [B, nr, nt]')
    B, nr = y2.shape
    if hh.shape[-2] != nr or (hh.ndim == 3 and hh.shape[0] != B):
        raise ValueError('shape mismatch: y %s, h %s' % (y2.shape, hh.shape))
    return y2, hh, int(hh.ndim == 3), B, nr, hh.shape[-1]


def _kbest_checks(nr, nt, output_type):
    if nt > nr:
        raise ValueError('h has more columns than rows')
    if output_type not in ('hard', 'soft'):
        raise ValueError('output_type must be "hard" or "soft"')


def _ml_indices(y, h, modem):
    y2, hh, hb, B, nr, nt = _mimo_inputs(y, h)
    idx = np.zeros((B, nt), dtype=np.int32)
    if B:
        _lib.check(_lib.load().cpx_mimo_ml(modem._device_handle(), _lib.ptr(y2), _lib.ptr(hh), hb, B, nr, nt, _lib.ptr(idx)))
    return idx


def _kbest_list(y, h, modem, K):
    """Final K-best candidates: (indices [B, Ke, nt] with -1 past the count, count [B]); Ke = min(K, m^nt)."""
    y2, hh, hb, B, nr, nt = _mimo_inputs(y, h)
    ke = min(int(K), modem.m ** nt)
    cand = np.zeros((B, ke, nt), dtype=np.int32)
    count = np.zeros(B, dtype=np.int32)
    if B:
        _lib.check(_lib.load().cpx_kbest_list(modem._device_handle(), _lib.ptr(y2), _lib.ptr(hh), hb, B, nr, nt, int(K),
                                              _lib.ptr(cand), _lib.ptr(count)))
    return cand, count


def mimo_ml(y, h, constellation):
    """Exhaustive ML detection of one received vector (modulation.py:299): the hypothesis of ``constellation`` points
    minimising ``|y - h x|``, first minimum in the reference's hypothesis order.  Returns complex [nt]."""
    md = _modem_for(constellation)
    return md.constellation.astype(complex)[_ml_indices(y, h, md)[0]]


def mimo_ml_batch(y, h, constellation):
    """``mimo_ml`` for every row of ``y [B, nr]`` in one launch; ``h`` is [nr, nt] or [B, nr, nt].  Returns complex [B, nt]."""
    md = constellation if isinstance(constellation, Modem) else _modem_for(constellation)
    return md.constellation.astype(complex)[_ml_indices(y, h, md)]


def kbest(y, h, constellation, K, noise_var=0, output_type='hard', demode=None):
    """K-best Schnorr-Euchner detection of one vector (modulation.py:325).  'hard': the best candidate, as the
    constellation's dtype; 'soft': ``max_log_approx`` over the final list with ``demode`` (search on the GPU, the LLRs on the
    host so that any ``demode`` behaves as in the reference).  Ties between equal distances go to the lowest child position."""
    h = np.asarray(h)
    nr, nt = h.shape
    _kbest_checks(nr, nt, output_type)
    pts = np.asarray(constellation)
    kind = complex if isinstance(pts[0], complex) else float
    md = _modem_for(pts)
    if output_type == 'hard':
        y2, hh, hb, B, nr, nt = _mimo_inputs(y, h)
        idx = np.zeros((1, nt), dtype=np.int32)
        _lib.check(_lib.load().cpx_kbest_hard(md._device_handle(), _lib.ptr(y2), _lib.ptr(hh), hb, 1, nr, nt, int(K),
                                              _lib.ptr(idx)))
        return pts[idx[0]].astype(kind)
    cand, count = _kbest_list(y, h, md, K)
    survivors = pts[cand[0, :count[0]]].astype(kind).T            # [nt, n] points column-wise
    return max_log_approx(np.asarray(y), h, noise_var, survivors, demode)


def kbest_batch(y, h, modem, K, noise_var=0, output_type='hard'):
    """``kbest`` for every row of ``y [B, nr]`` in one launch; ``h`` is [nr, nt] or [B, nr, nt].  'hard': symbols
    [B, nt] of ``modem.constellation``; 'soft': LLRs [B, nt * num_bits_symbol] computed on the device with the modem's labels
    (what ``demode = modem.demodulate(., 'hard')`` gives the single-vector form)."""
    y2, hh, hb, B, nr, nt = _mimo_inputs(y, h)
    _kbest_checks(nr, nt, output_type)
    lib, dev = _lib.load(), modem._device_handle()
    if output_type == 'hard':
        idx = np.zeros((B, nt), dtype=np.int32)
        if B:
            _lib.check(lib.cpx_kbest_hard(dev, _lib.ptr(y2), _lib.ptr(hh), hb, B, nr, nt, int(K), _lib.ptr(idx)))
        return modem.constellation[idx]
    llr = np.zeros((B, nt * modem.num_bits_symbol))
    if B:
        _lib.check(lib.cpx_kbest_soft(dev, _lib.ptr(y2), _lib.ptr(hh), hb, B, nr, nt, int(K), float(noise_var), _lib.ptr(llr)))
    return llr


def _bf_stacks(nr, nt, stack_size):
    """The reference's failures as ValueError, then the nr - 1 stack sizes as int32 (entries past them are ignored, sizes
    above 2^31 - 1 clipped: no stack of a tree this engine can search is that deep)."""
    if nr < 2:
        raise ValueError('best_first_detector needs at least 2 receive antennas (h has %d rows)' % nr)
    if nr > nt:
        raise ValueError('h has more rows than columns (%d > %d): the best-first search reaches no leaf' % (nr, nt))
    sizes = [operator.index(s) for s in tuple(stack_size)[:nr - 1]]
    if len(sizes) < nr - 1:
        raise ValueError('stack_size needs %d entries (one per stack but the first), got %d' % (nr - 1, len(sizes)))
    if min(sizes) < 1:
        raise ValueError('every stack size must be at least 1 (got %s): the search would reach no leaf' % (sizes,))
    return np.array([min(s, 2 ** 31 - 1) for s in sizes], dtype=np.int32)


_label_tables = {}


def _demode_labels(demode, constellation, nbits):
    """``demode``'s bits of every constellation point as a [m, nbits] uint8 table, built once per (demode, constellation).
    ValueError unless ``demode`` maps each point on its own (checked on a fixed permutation of the points) to 0 / 1 bits."""
    pts = np.asarray(constellation)
    key = (id(demode), pts.tobytes())
    hit = _label_tables.get(key)
    if hit is not None and hit[0] is demode:
        return hit[1]
    m = pts.size
    table = np.asarray(demode(pts)).reshape(-1)
    if table.size != m * nbits:
        raise ValueError('demode returned %d bits for %d points; %d expected' % (table.size, m, m * nbits))
    if not np.all((table == 0) | (table == 1)):
        raise ValueError('demode must return 0 / 1 bits')
    table = table.reshape(m, nbits)
    perm = np.random.RandomState(m).permutation(m)[::-1]
    again = np.asarray(demode(pts[perm])).reshape(-1)
    if again.size != m * nbits or not np.array_equal(again.reshape(m, nbits), table[perm]):
        raise ValueError('demode is not symbol-wise: the bits of a point depend on the other points given with it')
    labels = np.ascontiguousarray(table, dtype=np.uint8)
    if len(_label_tables) > 64:
        _label_tables.clear()
    _label_tables[key] = (demode, labels)
    return labels


def _best_first(y, h, modem, stack_size, llr_max, labels):
    y2, hh, hb, B, nr, nt = _mimo_inputs(y, h)
    sizes = _bf_stacks(nr, nt, stack_size)
    llr = np.zeros((B, nr * modem.num_bits_symbol))
    if labels is not None:
        labels = np.ascontiguousarray(labels, dtype=np.uint8)
        if labels.shape != (modem.m, modem.num_bits_symbol):
            raise ValueError('labels must be [%d, %d]' % (modem.m, modem.num_bits_symbol))
    if B:
        _lib.check(_lib.load().cpx_best_first(modem._device_handle(), _lib.ptr(y2), _lib.ptr(hh), hb, B, nr, nt, _lib.ptr(sizes),
                                              float(llr_max), None if labels is None else _lib.ptr(labels), _lib.ptr(llr)))
    return llr


def best_first_detector(y, h, constellation, stack_size, noise_var, demode, llr_max):
    """Soft-output best-first detection of one vector (modulation.py:422): LLRs float64 [nr * log2 m], position after
    position, each ``(map metric - counter metric) * (+1 / -1)`` for the MAP's bit as ``demode`` labels it, clipped to
    ``llr_max``.  As in the reference there are nr stacks (``nb_tx, nb_rx = h.shape``), ``stack_size`` needs nr - 1 entries
    (more are ignored) and ``noise_var`` is not used.  ValueError where the reference fails (nr < 2, nr > nt, a short
    stack_size or a size below 1) and for a vector that reaches no leaf (NaN / inf input: the reference raises TypeError);
    also for a ``demode`` that is not symbol-wise or returns other than 0 / 1.  Children of equal metric are taken in
    ascending constellation index."""
    h = np.asarray(h)
    if h.ndim != 2:
        raise ValueError('h must be [nr, nt]')
    nr, nt = h.shape
    _bf_stacks(nr, nt, stack_size)
    md = _modem_for(constellation)
    labels = _demode_labels(demode, np.asarray(constellation), md.num_bits_symbol)
    llr = _best_first(np.asarray(y).reshape(1, -1), h, md, stack_size, llr_max, labels)[0]
    if np.all(np.isnan(llr)):
        raise ValueError('best_first_detector: the search reached no leaf (NaN or inf in y or h?)')
    return llr


def best_first_batch(y, h, modem, stack_size, llr_max, labels=None):
    """``best_first_detector`` for every row of ``y [B, nr]`` in one launch; ``h`` is [nr, nt] or [B, nr, nt].  LLRs
    [B, nr * num_bits_symbol] with the bits of ``labels`` ([m, num_bits_symbol] 0/1, default: the modem's labels, what
    ``demode = modem.demodulate(., 'hard')`` gives); a row of NaN marks a vector that reached no leaf."""
    return _best_first(y, h, modem, stack_size, llr_max, labels)


LIST_MAX_BITS = 64        # bits per vector the list detector carries (one lane each, mimo_idd.hip)
LIST_MAX_KE = 4064        # candidates whose costs and labels fit the kernel's LDS


def _list_checks(modem, K, llr_clip, nr=None, nt=None):
    """The refusals of the list detector that need no device (the engine repeats them): ``(K, llr_clip)`` as int and float."""
    K, clip = operator.index(K), float(llr_clip)
    if K < 1:
        raise ValueError('K must be a positive integer')
    if not clip > 0:
        raise ValueError('llr_clip must be positive (got %r)' % (llr_clip,))
    if modem.m != 1 << modem.num_bits_symbol:
        raise ValueError('the modem must have 2^num_bits_symbol points')
    if nt is not None:
        if nt > nr:
            raise ValueError('h has more columns than rows')
        if nt * modem.num_bits_symbol > LIST_MAX_BITS:
            raise ValueError('%d x %d bits per vector above the list detector\'s %d' % (nt, modem.num_bits_symbol, LIST_MAX_BITS))
        ke = min(K, modem.m ** nt)
        if ke > LIST_MAX_KE:
            raise ValueError('a list of %d candidates exceeds the list detector\'s %d' % (ke, LIST_MAX_KE))
        if ke * modem.m >= 2 ** 31:
            raise ValueError('kbest: K * m above 2^31 children')
    return K, clip


def list_apriori_batch(y, h, modem, K, noise_var, a_priori=None, llr_clip=500.0):
    """Max-log list detection with a-priori LLRs of every row of ``y [B, nr]``; ``h`` is [nr, nt] or [B, nr, nt].  Returns the
    posterior LLRs ``[B, nt * num_bits_symbol]`` (positive: bit 0; the modem's labels, MSB first, antenna after antenna).

    The candidate list is ``kbest``'s final list (K-best search on the channel metric, on the device; the priors do not steer the
    search -- list sphere detection).  With ``La`` = ``a_priori`` clipped to ``[-llr_clip, llr_clip]`` (None: zeros), the cost of a
    candidate is ``|y - h x|^2 / (2 noise_var) + sum of La over its bits 1`` and the LLR of a bit the minimum cost with that bit 1
    minus the minimum with it 0, clipped to ``[-llr_clip, llr_clip]``; a bit value no candidate carries counts as +inf.
    ``K >= m^nt`` keeps every hypothesis: the exhaustive max-log MAP detector.  ``a_priori=None`` and ``llr_clip=inf`` give
    ``kbest_batch(..., 'soft')`` bit for bit.  A NaN in a vector's y, h or prior makes that vector's LLRs NaN."""
    from commpy_amd.deviceops import _OneShot
    y2, hh, hb, B, nr, nt = _mimo_inputs(y, h)
    K, clip = _list_checks(modem, K, llr_clip, nr, nt)
    nbt = nt * modem.num_bits_symbol
    noise_var = float(noise_var)
    if not 0.0 < noise_var < np.inf:
        raise ValueError('noise_var must be positive and finite, got %r' % noise_var)
    prior = None
    if a_priori is not None:
        prior = np.ascontiguousarray(a_priori, dtype=np.float64)
        if prior.shape != (B, nbt):
            raise ValueError('a_priori must be [%d, %d], got %s' % (B, nbt, prior.shape))
    if B == 0:
        return np.zeros((0, nbt))
    ke = min(K, modem.m ** nt)
    md = modem._device_handle()
    with _OneShot() as dev:
        lib, ck = dev.lib, _lib.check
        d_y, d_h = dev.upload(y2), dev.upload(hh)
        d_cand, d_count, d_dist, d_llr = dev.alloc(B * ke * nt * 4), dev.alloc(B * 4), dev.alloc(B * ke * 8), dev.alloc(B * nbt * 8)
        ck(lib.cpx_kbest_list_dev(md, d_y, d_h, hb, B, nr, nt, K, d_cand.ptr, d_count.ptr, None))
        ck(lib.cpx_mimo_list_dist_dev(md, d_y, d_h, hb, B, nr, nt, d_cand.ptr, d_count.ptr, ke, d_dist.ptr, None))
        ck(lib.cpx_mimo_list_llr_dev(md, d_cand.ptr, d_count.ptr, d_dist.ptr, B, nt, ke, None if prior is None else dev.upload(prior),
                                     noise_var, clip, d_llr.ptr, None))
        return dev.download(d_llr, (B, nbt), np.float64)


def apriori_detector(modem, K, llr_clip=500.0):
    """``detector(y, h, constellation, noise_var, a_priori)`` for ``links.idd_decoder``: ``list_apriori_batch`` on one vector.
    The bits are ``modem``'s labels; ``constellation`` is what ``LinkModel`` passes along and is not read."""
    K, llr_clip = _list_checks(modem, K, llr_clip)

    def detector(y, h, constellation, noise_var, a_priori):
        return list_apriori_batch(np.asarray(y).reshape(1, -1), np.asarray(h), modem, K, noise_var,
                                  np.asarray(a_priori, dtype=np.float64).reshape(1, -1), llr_clip)[0]
    return detector


# ---- linear detection: zero forcing and MMSE (csrc/mimo_linear.hip) -----------------------------------------------------------
def _linear_reg(method, noise_var, Es, reg):
    """(reg, noise_var) as floats, checked as the engine checks them; ``reg=None``: 0 for 'zf', ``noise_var / Es`` for 'mmse'."""
    if method not in ('zf', 'mmse'):
        raise ValueError("method must be 'zf' or 'mmse'")
    noise_var = float(noise_var)
    if noise_var != noise_var:
        raise ValueError('noise_var is NaN')
    if reg is None:
        reg = 0.0 if method == 'zf' else noise_var / float(Es)
    reg = float(reg)
    if not reg >= 0:
        raise ValueError('reg must be zero or positive (got %r)' % (reg,))
    return reg, noise_var


def _linear_run(y, h, modem, reg, noise_var, want):
    """One ``cpx_mimo_linear`` call: ``want`` names the outputs ('idx', 'llr', 'xhat', 'nu'); returns them as a dict."""
    y2, hh, hb, B, nr, nt = _mimo_inputs(y, h)
    if modem.m != 1 << modem.num_bits_symbol:
        raise ValueError('the modem must have 2^num_bits_symbol points')
    shapes = {'idx': ((B, nt), np.int32), 'llr': ((B, nt * modem.num_bits_symbol), np.float64), 'xhat': ((B, nt), np.complex128),
              'nu': ((B, nt), np.float64)}
    out = {k: np.zeros(*shapes[k]) for k in want}
    if not out:
        raise ValueError('no output requested')
    if B:
        ptrs = [_lib.ptr(out[k]) if k in out else None for k in ('idx', 'llr', 'xhat', 'nu')]
        _lib.check(_lib.load().cpx_mimo_linear(modem._device_handle(), _lib.ptr(y2), _lib.ptr(hh), hb, B, nr, nt, float(reg),
                                               float(noise_var), *ptrs))
    return out


def linear_batch(y, h, modem, noise_var, method='mmse', output_type='hard', reg=None):
    """Linear detection of every row of ``y [B, nr]`` in one launch; ``h`` is [nr, nt] (shared) or [B, nr, nt]; any nr, nt >= 1.

    ``A = h^H h + reg I``, ``z = A^-1 h^H y``, ``a_i = (A^-1)_ii``; the unbiased estimate is ``xhat_i = z_i / (1 - reg a_i)`` and its
    noise variance ``nu_i = noise_var a_i / (1 - reg a_i)``.  ``reg=None`` means 0 for ``method='zf'`` (``xhat = pinv(h) y``) and
    ``noise_var / modem.Es`` for 'mmse'.  'hard': symbols [B, nt] of ``modem.constellation``, the nearest point per stream (a tie
    to the lowest index); 'soft': LLRs [B, nt * num_bits_symbol], per stream ``(min over the points with bit 1 of |xhat_i - s|^2 -
    min over those with bit 0) / (2 nu_i)`` with the modem's labels, MSB first -- positive: bit 0, the scale of ``kbest_batch``'s
    soft output.  A vector whose ``A`` is not positive definite (singular h under 'zf', nt > nr with reg = 0) or that holds a NaN /
    inf gives NaN LLRs and point 0; it affects no other vector."""
    if output_type not in ('hard', 'soft'):
        raise ValueError('output_type must be "hard" or "soft"')
    reg, noise_var = _linear_reg(method, noise_var, modem.Es, reg)
    if output_type == 'hard':
        return modem.constellation[_linear_run(y, h, modem, reg, noise_var, ('idx',))['idx']]
    return _linear_run(y, h, modem, reg, noise_var, ('llr',))['llr']


def linear_equalize_batch(y, h, noise_var, method, reg=None, Es=1.0):
    """The equaliser of ``linear_batch`` alone: ``(xhat [B, nt] complex, nu [B, nt])``, the unbiased estimates and their noise
    variances.  ``reg=None``: 0 for 'zf', ``noise_var / Es`` for 'mmse'.  Rows of NaN mark a vector that failed."""
    reg, noise_var = _linear_reg(method, noise_var, Es, reg)
    out = _linear_run(y, h, _modem_for(np.array([-1.0, 1.0])), reg, noise_var, ('xhat', 'nu'))
    return out['xhat'], out['nu']


def _linear_detector(method, y, h, constellation, noise_var, output_type, demode):
    h = np.asarray(h)
    if h.ndim != 2:
        raise ValueError('h must be [nr, nt]')
    if output_type not in ('hard', 'soft'):
        raise ValueError('output_type must be "hard" or "soft"')
    pts = np.asarray(constellation)
    kind = complex if isinstance(pts[0], complex) else float
    md = _modem_for(pts)
    reg, noise_var = _linear_reg(method, noise_var, md.Es, None)
    y1 = np.asarray(y).reshape(1, -1)
    if output_type == 'hard':
        return pts[_linear_run(y1, h, md, reg, noise_var, ('idx',))['idx'][0]].astype(kind)
    nb = md.num_bits_symbol
    index_bits = ((np.arange(md.m)[:, None] >> np.arange(nb - 1, -1, -1)) & 1).astype(np.uint8)
    labels = index_bits if demode is None else _demode_labels(demode, pts, nb)
    if np.array_equal(labels, index_bits):
        return _linear_run(y1, h, md, reg, noise_var, ('llr',))['llr'][0]
    out = _linear_run(y1, h, md, reg, noise_var, ('xhat', 'nu'))
    xhat, nu = out['xhat'][0], out['nu'][0]
    diff = xhat[:, None] - pts.astype(complex)[None, :]
    dist = diff.real * diff.real + diff.imag * diff.imag                       # [nt, m]
    llr = np.empty((h.shape[1], nb))
    with np.errstate(all='ignore'):
        for k in range(nb):
            one = labels[:, k] == 1
            mn1 = np.min(np.where(one[None, :], dist, np.inf), axis=1)
            mn0 = np.min(np.where(one[None, :], np.inf, dist), axis=1)
            llr[:, k] = (mn1 - mn0) / (2 * nu)
    llr[np.isnan(nu)] = np.nan
    return llr.reshape(-1)


def zf_detector(y, h, constellation, noise_var, output_type='hard', demode=None):
    """Zero-forcing detection of one vector (``linear_batch`` with ``method='zf'``), the argument order of ``kbest``.  'hard': the
    nearest point of ``xhat = pinv(h) y`` per stream, as the constellation's dtype; 'soft': LLRs [nt * log2 m] with ``demode``'s
    bits (None: the index bits, MSB first).  A ``demode`` equal to the index bits runs on the device; any other is applied on the
    host to the device's ``xhat`` and ``nu``, as ``kbest`` does with its list."""
    return _linear_detector('zf', y, h, constellation, noise_var, output_type, demode)


def mmse_detector(y, h, constellation, noise_var, output_type='hard', demode=None):
    """Unbiased MMSE detection of one vector: ``zf_detector`` with ``reg = noise_var / Es`` (Es: the constellation's mean energy)."""
    return _linear_detector('mmse', y, h, constellation, noise_var, output_type, demode)


def max_log_approx(y, h, noise_var, pts_list, demode):
    """Max-log LLRs of the bits of a candidate list (modulation.py:599): ``pts_list`` [nt, n] holds the candidates
    column-wise, ``demode`` maps their points (candidate after candidate) to bits.  LLR of bit k =
    (min distance with bit 1 - min distance with bit 0) / (2 noise_var), an empty side counting as +inf."""
    n = pts_list.shape[1]
    words = np.asarray(demode(pts_list.reshape(-1, order='F'))).reshape(n, -1)
    dist = np.linalg.norm(y[:, None] - h.dot(pts_list), axis=0) ** 2
    gap = np.empty(words.shape[1])
    for k, column in enumerate(words.T):
        best = [np.min(np.append(dist[column == v], np.inf)) for v in (0, 1)]
        gap[k] = best[0] - best[1]
    return -gap / (2 * noise_var)


def bit_lvl_repr(H, w):
    """Bit-level channel matrix ``H (I_nt kron w)`` (modulation.py:568); ``w`` must have an even length."""
    if len(w) % 2:
        raise ValueError('Beta (length of w) must be even.')
    return np.asarray(H).dot(np.kron(np.identity(np.shape(H)[1]), w))


# ---- OFDM (csrc/ofdm.hip) -----------------------------------------------------------------------------------------------------
OFDM_MAX_NFFT = 65536


def _whole(value, name):
    """``value`` as an int: integers, and floats holding a whole number (the reference casts its sizes to float)."""
    if isinstance(value, (bool, np.bool_)):
        raise ValueError('%s must be a whole number, got %r' % (name, value))
    if isinstance(value, numbers.Integral):
        return int(value)
    if isinstance(value, numbers.Real) and np.isfinite(value) and float(value) == int(value):
        return int(value)
    raise ValueError('%s must be a whole number, got %r' % (name, value))


def _ofdm_sizes(nfft, nsc, cp_length):
    """(nfft, nsc, cp_length) as ints, checked as the engine checks them (ValueError, no device needed)."""
    nfft, nsc, cp_length = _whole(nfft, 'nfft'), _whole(nsc, 'nsc'), _whole(cp_length, 'cp_length')
    if nfft < 2:
        raise ValueError('nfft = %d, need at least 2' % nfft)
    if nfft > OFDM_MAX_NFFT:
        raise ValueError('nfft = %d is above the engine limit of %d' % (nfft, OFDM_MAX_NFFT))
    if nsc < 2 or nsc % 2:
        raise ValueError('nsc = %d, need an even number >= 2' % nsc)
    if nsc // 2 > nfft - 1:
        raise ValueError('nsc / 2 = %d subcarriers per side do not fit nfft = %d (at most nfft - 1)' % (nsc // 2, nfft))
    if cp_length < 0:
        raise ValueError('cp_length = %d is negative' % cp_length)
    return nfft, nsc, cp_length


def ofdm_prefix_length(nfft, cp_length):
    """Samples of prefix in front of each transmitted symbol: ``cp_length`` if 0 < cp_length < nfft, else nfft -- the length of
    the reference's ``t[-cp_length:]``, which takes the whole symbol for cp_length = 0 and for cp_length >= nfft."""
    return cp_length if 0 < cp_length < nfft else nfft


class _OfdmPlan:
    """The engine's plan of one (nfft, nsc, cp_length): twiddles and kernel choice, one handle per device."""

    def __init__(self, nfft, nsc, cp_length):
        self.nfft, self.nsc, self.cp_length = nfft, nsc, cp_length

        def create():
            h = ctypes.c_void_p()
            _lib.check(_lib.load().cpx_ofdm_create(nfft, nsc, cp_length, ctypes.byref(h)))
            return h
        self._handles = _lib.DeviceHandles(create, 'cpx_ofdm_destroy')

    def handle(self):
        return self._handles.get()


_ofdm_plans = {}


def _ofdm_plan(nfft, nsc, cp_length):
    key = (nfft, nsc, cp_length)
    plan = _ofdm_plans.get(key)
    if plan is None:
        if len(_ofdm_plans) > 64:
            _ofdm_plans.clear()
        plan = _ofdm_plans[key] = _OfdmPlan(nfft, nsc, cp_length)
    return plan


def ofdm_tx_batch(symbols, nfft, cp_length):
    """``ofdm_tx`` for B streams at once, symbol-major: ``symbols [B, nsym, nsc]`` (what ``modulate(bits).reshape(B, nsym, nsc)``
    gives) -> complex128 ``[B, nsym * (P + nfft)]``, P = ``ofdm_prefix_length(nfft, cp_length)``."""
    x = np.asarray(symbols)
    if x.ndim != 3:
        raise ValueError('symbols must be [B, nsym, nsc], got %d dimensions' % x.ndim)
    B, nsym, nsc = x.shape
    nfft, nsc, cp_length = _ofdm_sizes(nfft, nsc, cp_length)
    per = ofdm_prefix_length(nfft, cp_length) + nfft
    out = np.zeros((B, nsym * per), dtype=np.complex128)
    if out.size:
        x = np.ascontiguousarray(x, dtype=np.complex128)
        _lib.check(_lib.load().cpx_ofdm_tx(_ofdm_plan(nfft, nsc, cp_length).handle(), _lib.ptr(x), B, nsym, _lib.ptr(out)))
    return out


def ofdm_rx_batch(y, nfft, nsc, cp_length):
    """``ofdm_rx`` for B streams at once: ``y [B, n]`` -> complex128 ``[B, n // (nfft + cp_length), nsc]`` (symbol-major)."""
    y = np.asarray(y)
    if y.ndim != 2:
        raise ValueError('y must be [B, n], got %d dimensions' % y.ndim)
    nfft, nsc, cp_length = _ofdm_sizes(nfft, nsc, cp_length)
    B, n = y.shape
    out = np.zeros((B, n // (nfft + cp_length), nsc), dtype=np.complex128)
    if out.size:
        y = np.ascontiguousarray(y, dtype=np.complex128)
        _lib.check(_lib.load().cpx_ofdm_rx(_ofdm_plan(nfft, nsc, cp_length).handle(), _lib.ptr(y), B, n, _lib.ptr(out)))
    return out


def ofdm_tx(x, nfft, nsc, cp_length):
    """OFDM transmit (modulation.py:265): ``x [nsc, nsym]``, column i = symbol i -> complex128 of length nsym * (P + nfft).
    Per symbol, bins 1..nsc/2 carry ``x[nsc/2:, i]`` and the top nsc/2 bins ``x[:nsc/2, i]`` (the second wins where they
    overlap), every other bin is 0; the block is the last P samples of ``ifft`` of that, then all nfft of them.
    P = cp_length if 0 < cp_length < nfft, else nfft (the reference's ``t[-cp_length:]``)."""
    nfft, nsc, cp_length = _ofdm_sizes(nfft, nsc, cp_length)
    x = np.asarray(x)
    if x.ndim != 2:
        raise ValueError('x must be [nsc, nsym], got %d dimensions' % x.ndim)
    if x.shape[0] != nsc:
        raise ValueError('x has %d rows, nsc = %d' % (x.shape[0], nsc))
    return ofdm_tx_batch(x.T[None], nfft, cp_length)[0]


def ofdm_rx(y, nfft, nsc, cp_length):
    """OFDM receive (modulation.py:286): ``y`` 1-D -> complex128 ``[nsc, len(y) // (nfft + cp_length)]``.  Symbol i is the fft of
    the nfft samples after the first cp_length of its block; column i holds its top nsc/2 bins, then bins 1..nsc/2.  Samples
    past the last whole block are ignored."""
    nfft, nsc, cp_length = _ofdm_sizes(nfft, nsc, cp_length)
    y = np.asarray(y)
    if y.ndim != 1:
        raise ValueError('y must be 1-D, got %d dimensions' % y.ndim)
    return np.ascontiguousarray(ofdm_rx_batch(y[None], nfft, nsc, cp_length)[0].T)


# ---- pilots, resource mapping and channel estimation (csrc/ofdm_chan.hip) ---------------------------------------------------------
OFDM_MAX_ANTENNAS = 1024


def _numeric(a, name, dtype=np.complex128):
    """``a`` as a C array of ``dtype``; anything but numbers is a ValueError."""
    arr = np.asarray(a)
    if arr.dtype.kind not in 'biufc':
        raise ValueError('%s must hold numbers, got dtype %s' % (name, arr.dtype))
    return np.ascontiguousarray(arr, dtype=dtype)


def _indices(a, name, n):
    arr = np.asarray(a)
    if arr.ndim != 1 or arr.shape[0] != n:
        raise ValueError('%s must be 1-D of length %d, got shape %s' % (name, n, arr.shape))
    if arr.dtype.kind not in 'iu':
        raise ValueError('%s must hold integers, got dtype %s' % (name, arr.dtype))
    return arr.astype(np.int64)


def ofdm_subcarrier_frequencies(nsc):
    """Signed frequency (bin) of each of the ``nsc`` used subcarriers in ``ofdm_tx``'s input order: ``k - nsc/2`` for the lower
    half, ``k - nsc/2 + 1`` for the upper one (bin 0, DC, is unused)."""
    k = np.arange(nsc)
    return np.where(k < nsc // 2, k - nsc // 2, k - nsc // 2 + 1)


def _interp_linear(nsc, pk):
    """W [nsc, len(pk)]: linear interpolation in frequency between the neighbouring pilot subcarriers ``pk`` (ascending), the
    nearest pilot held outside their range."""
    f = ofdm_subcarrier_frequencies(nsc).astype(np.float64)
    fp = f[pk]
    W = np.zeros((nsc, len(pk)), dtype=np.complex128)
    j = np.clip(np.searchsorted(fp, f, side='right') - 1, 0, max(len(pk) - 2, 0))
    rows = np.arange(nsc)
    if len(pk) == 1:
        W[:, 0] = 1.0
        return W
    a = np.clip((f - fp[j]) / (fp[j + 1] - fp[j]), 0.0, 1.0)
    W[rows, j] = 1.0 - a
    W[rows, j + 1] += a
    return W


def _interp_taps(nsc, pk, Lmax, nfft):
    """W [nsc, len(pk)] = F_all pinv(F_p): the least-squares fit of ``Lmax`` time-domain taps to the pilots' estimates, evaluated on
    every subcarrier; F[k][l] = exp(-2 pi i f(k) l / nfft)."""
    if Lmax > len(pk):
        raise ValueError("interp ('taps', %d, %d): %d taps cannot be fitted to %d pilot subcarriers" % (Lmax, nfft, Lmax, len(pk)))
    f = ofdm_subcarrier_frequencies(nsc).astype(np.float64)
    F = np.exp(-2j * np.pi * np.outer(f, np.arange(Lmax)) / nfft)
    return np.ascontiguousarray(F.dot(np.linalg.pinv(F[pk])))


def _time_linear(nsym, ps):
    """V [nsym, len(ps)]: linear interpolation in the symbol index between the neighbouring pilot symbols ``ps`` (ascending), the
    nearest one held outside their range -- the time twin of ``_interp_linear``."""
    f, fp = np.arange(nsym, dtype=np.float64), np.asarray(ps, dtype=np.float64)
    V = np.zeros((nsym, len(ps)), dtype=np.complex128)
    if len(ps) == 1:
        V[:, 0] = 1.0
        return V
    i = np.clip(np.searchsorted(fp, f, side='right') - 1, 0, len(ps) - 2)
    rows = np.arange(nsym)
    a = np.clip((f - fp[i]) / (fp[i + 1] - fp[i]), 0.0, 1.0)
    V[rows, i] = 1.0 - a
    V[rows, i + 1] += a
    return V


def _time_hold(nsym, ps):
    """V [nsym, len(ps)]: every symbol takes the estimate of the nearest pilot symbol, the lower one on a tie."""
    ps = np.asarray(ps, dtype=np.int64)
    V = np.zeros((nsym, len(ps)), dtype=np.complex128)
    V[np.arange(nsym), np.argmin(np.abs(np.arange(nsym)[:, None] - ps[None, :]), axis=1)] = 1.0     # argmin: the first = the lower
    return V


def _time_doppler(nsym, ps, fd_sym, nvar):
    """V [nsym, len(ps)] = R_sp (R_pp + nvar I)^-1 with Clarke's autocorrelation R[a][b] = J0(2 pi fd_sym |a - b|): the Wiener filter
    in time for a maximum Doppler shift of ``fd_sym`` cycles per OFDM symbol and a noise variance ``nvar`` of the pilot estimates."""
    from scipy.special import j0
    ps = np.asarray(ps, dtype=np.float64)
    r_sp = j0(2.0 * np.pi * fd_sym * np.abs(np.arange(nsym, dtype=np.float64)[:, None] - ps[None, :]))
    r_pp = j0(2.0 * np.pi * fd_sym * np.abs(ps[:, None] - ps[None, :])) + nvar * np.eye(len(ps))
    try:
        V = np.linalg.solve(r_pp.T, r_sp.T).T
    except np.linalg.LinAlgError:
        raise ValueError("time_interp ('doppler', %g, %g): the pilot symbols' autocorrelation matrix is singular" % (fd_sym, nvar))
    return np.ascontiguousarray(V, dtype=np.complex128)


def _default_pilot_values(n):
    """``n`` unit-modulus QPSK points from the PRBS x^15 + x^14 + 1 (``pnsequence``), two bits per point."""
    from commpy_amd.sequences import pnsequence
    bits = pnsequence(15, '1' * 15, '0' * 13 + '11', 2 * n).astype(np.float64)
    return ((1.0 - 2.0 * bits[0::2]) + 1j * (1.0 - 2.0 * bits[1::2])) * np.sqrt(0.5)


def _antenna_matrices(named, spec, arg, schemes, letter, dims, rows, cols):
    """The interpolation matrices of the len(cols) antennas, each [rows, cols[t]] and finite: ``named``, what the caller made of a
    named scheme, or else argument ``arg`` = ``spec`` itself, a list of that many arrays (``schemes``: the names, for the message)."""
    if named is None:
        if not (isinstance(spec, (list, tuple)) and len(spec) == len(cols) and not isinstance(spec[0], str)):
            raise ValueError("%s must be %s or a list of nt matrices" % (arg, schemes))
        named = [_numeric(m, '%s[%d]' % (arg, t)) for t, m in enumerate(spec)]
    for t, m in enumerate(named):
        if m.shape != (rows, cols[t]):
            raise ValueError('%s[%d] must be [%s] = [%d, %d], got %s' % (letter, t, dims, rows, cols[t], m.shape))
        if not np.all(np.isfinite(m)):
            raise ValueError('%s[%d] holds a value that is not finite' % (letter, t))
    return named


class OfdmPilots:
    """The pilots of a frame of ``nsym`` OFDM symbols x ``nsc`` used subcarriers (``ofdm_tx``'s input order) of ``nt`` transmit
    antennas.  Pilot i puts ``pil_val[i]`` on resource element ``(pil_sym[i], pil_sc[i])`` of antenna ``pil_tx[i]``; the other
    antennas are silent there.  Every other resource element carries data: ``ndata`` of them, numbered symbol-major, then by
    ascending subcarrier (``data_sym``, ``data_sc``).

    ``interp`` gives, per antenna t, the matrix ``W[t] [nsc, np_t]`` that spreads the least-squares estimates at its ``np_t`` distinct
    pilot subcarriers ``pilot_subcarriers[t]`` (ascending) over all subcarriers: 'linear' (in frequency, the nearest pilot held
    outside their range), ``('taps', Lmax, nfft)`` (least-squares fit of Lmax time-domain taps, ``F_all pinv(F_p)``) or a list of
    nt arrays.

    ``time_interp`` (None: the fading is taken as constant over the frame) makes the plan track a channel that moves inside the
    frame: per antenna t a matrix ``V[t] [nsym, ns_t]`` spreads the estimates at its ``ns_t`` distinct pilot symbols
    ``pilot_symbols[t]`` (ascending) over all symbols, for ``ofdm_estimate_tv_batch``.  'linear' (in the symbol index, the nearest
    pilot symbol held outside their range), 'hold' (the nearest pilot symbol, the lower one on a tie), ``('doppler', fd_sym,
    nvar)`` (the Wiener filter ``R_sp (R_pp + nvar I)^-1`` on Clarke's ``J0(2 pi fd_sym |a - b|)``, ``fd_sym`` in cycles per OFDM
    symbol) or a list of nt arrays.  The pattern must then be a rectangle per antenna: the same pilot subcarriers on each of its
    pilot symbols (``comb`` and ``block`` are).  Everything is validated here (ValueError) before a device is touched."""

    def __init__(self, nsc, nsym, nt, pil_sym, pil_sc, pil_tx, pil_val, interp='linear', time_interp=None):
        nsc, nsym, nt = _whole(nsc, 'nsc'), _whole(nsym, 'nsym'), _whole(nt, 'nt')
        if nsc < 2 or nsc % 2:
            raise ValueError('nsc = %d, need an even number >= 2' % nsc)
        if nsym < 1 or nt < 1:
            raise ValueError('nsym = %d, nt = %d, need at least 1 of each' % (nsym, nt))
        if nt > OFDM_MAX_ANTENNAS:
            raise ValueError('nt = %d is above the engine limit of %d' % (nt, OFDM_MAX_ANTENNAS))
        if nsym * nsc >= 2 ** 30:
            raise ValueError('a frame of %d resource elements is above the engine limit' % (nsym * nsc))
        npil = int(np.asarray(pil_sym).shape[0]) if np.asarray(pil_sym).ndim == 1 else -1
        if npil < 1:
            raise ValueError('pil_sym must be 1-D with at least one pilot')
        sym, sc, tx = _indices(pil_sym, 'pil_sym', npil), _indices(pil_sc, 'pil_sc', npil), _indices(pil_tx, 'pil_tx', npil)
        val = _numeric(pil_val, 'pil_val')
        if val.shape != (npil,):
            raise ValueError('pil_val must be 1-D of length %d, got shape %s' % (npil, val.shape))
        for name, a, hi in (('pil_sym', sym, nsym), ('pil_sc', sc, nsc), ('pil_tx', tx, nt)):
            if a.min() < 0 or a.max() >= hi:
                raise ValueError('%s holds an index outside 0 .. %d' % (name, hi - 1))
        re = sym * nsc + sc
        if np.unique(re).size != npil:
            raise ValueError('a resource element appears twice in the pilot list')
        mag2 = val.real * val.real + val.imag * val.imag
        if not (np.all(np.isfinite(val)) and np.all(np.isfinite(mag2)) and np.all(mag2 > 0)):
            raise ValueError('a pilot value is zero or not finite')
        self.pilot_subcarriers = [np.unique(sc[tx == t]) for t in range(nt)]
        for t, pk in enumerate(self.pilot_subcarriers):
            if pk.size == 0:
                raise ValueError('antenna %d has no pilot' % t)
        W = None
        if isinstance(interp, str) and interp == 'linear':
            W = [_interp_linear(nsc, pk) for pk in self.pilot_subcarriers]
        elif isinstance(interp, tuple) and len(interp) == 3 and interp[0] == 'taps':
            Lmax, nfft = _whole(interp[1], 'Lmax'), _whole(interp[2], 'nfft')
            if Lmax < 1 or nfft < 2:
                raise ValueError("interp ('taps', Lmax, nfft) needs Lmax >= 1 and nfft >= 2")
            W = [_interp_taps(nsc, pk, Lmax, nfft) for pk in self.pilot_subcarriers]
        W = _antenna_matrices(W, interp, 'interp', "'linear', ('taps', Lmax, nfft)", 'W', 'nsc, np_t', nsc,
                              [pk.size for pk in self.pilot_subcarriers])
        self.pilot_symbols = [np.unique(sym[tx == t]) for t in range(nt)]
        V = None
        if time_interp is not None:
            for t in range(nt):
                on = np.bincount(sym[tx == t], minlength=nsym)
                bad = np.flatnonzero((on != 0) & (on != self.pilot_subcarriers[t].size))
                if bad.size:
                    raise ValueError('time_interp needs the same pilot subcarriers on every pilot symbol of an antenna: antenna %d has '
                                     '%d of its %d in symbol %d' % (t, on[bad[0]], self.pilot_subcarriers[t].size, bad[0]))
            if isinstance(time_interp, str) and time_interp == 'linear':
                V = [_time_linear(nsym, ps) for ps in self.pilot_symbols]
            elif isinstance(time_interp, str) and time_interp == 'hold':
                V = [_time_hold(nsym, ps) for ps in self.pilot_symbols]
            elif isinstance(time_interp, tuple) and len(time_interp) == 3 and time_interp[0] == 'doppler':
                try:
                    fd_sym, nvar = float(time_interp[1]), float(time_interp[2])
                except (TypeError, ValueError):
                    raise ValueError("time_interp ('doppler', fd_sym, nvar) needs two numbers")
                if not (np.isfinite(fd_sym) and np.isfinite(nvar) and fd_sym >= 0 and nvar >= 0):
                    raise ValueError("time_interp ('doppler', fd_sym, nvar) needs finite fd_sym >= 0 and nvar >= 0")
                V = [_time_doppler(nsym, ps, fd_sym, nvar) for ps in self.pilot_symbols]
            V = _antenna_matrices(V, time_interp, 'time_interp', "None, 'linear', 'hold', ('doppler', fd_sym, nvar)", 'V',
                                  'nsym, ns_t', nsym, [ps.size for ps in self.pilot_symbols])
        self.nsc, self.nsym, self.nt, self.npil = nsc, nsym, nt, npil
        self.pil_sym, self.pil_sc, self.pil_tx, self.pil_val, self.W, self.V = sym, sc, tx, val, W, V
        is_data = np.ones(nsym * nsc, dtype=bool)
        is_data[re] = False
        data_re = np.flatnonzero(is_data)
        self.ndata = int(data_re.size)
        self.data_sym, self.data_sc = data_re // nsc, data_re % nsc
        i32 = [np.ascontiguousarray(a, dtype=np.int32) for a in (sym, sc, tx)]
        wflat = np.ascontiguousarray(np.concatenate([w.reshape(-1) for w in W]))

        vflat = None if V is None else np.ascontiguousarray(np.concatenate([v.reshape(-1) for v in V]))

        def create():
            h = ctypes.c_void_p()
            if vflat is None:
                _lib.check(_lib.load().cpx_pilots_create(nsc, nsym, nt, npil, _lib.ptr(i32[0]), _lib.ptr(i32[1]), _lib.ptr(i32[2]),
                                                              _lib.ptr(val), _lib.ptr(wflat), ctypes.byref(h)))
            else:
                _lib.check(_lib.load().cpx_pilots_create_tv(nsc, nsym, nt, npil, _lib.ptr(i32[0]), _lib.ptr(i32[1]), _lib.ptr(i32[2]),
                                                            _lib.ptr(val), _lib.ptr(wflat), _lib.ptr(vflat), ctypes.byref(h)))
            return h
        self._handles = _lib.DeviceHandles(create, 'cpx_pilots_destroy')

    def handle(self):
        """Opaque cpx_ofdm_pilots* of the current device (created on first use, one per device)."""
        return self._handles.get()

    @classmethod
    def comb(cls, nsc, nsym, nt, spacing, pilot_symbols, interp, values=None, time_interp=None):
        """Comb pilots: on each symbol of ``pilot_symbols`` antenna t takes subcarriers ``t, t + spacing, ...`` (``spacing >= nt``).
        ``values``: one per pilot, pilot symbol after pilot symbol, antenna after antenna (default: PRBS QPSK points)."""
        nsc, nt, spacing = _whole(nsc, 'nsc'), _whole(nt, 'nt'), _whole(spacing, 'spacing')
        if nt < 1 or spacing < nt:
            raise ValueError('comb pilots need spacing >= nt >= 1 (spacing = %d, nt = %d)' % (spacing, nt))
        syms = _indices(pilot_symbols, 'pilot_symbols', len(pilot_symbols))
        sym, sc, tx = [], [], []
        for s in syms:
            for t in range(nt):
                k = np.arange(t, max(nsc, 0), spacing)
                sym.append(np.full(k.size, s)), sc.append(k), tx.append(np.full(k.size, t))
        sym, sc, tx = (np.concatenate(a).astype(np.int64) if a else np.zeros(0, np.int64) for a in (sym, sc, tx))
        return cls(nsc, nsym, nt, sym, sc, tx, _default_pilot_values(sym.size) if values is None else values, interp, time_interp)

    @classmethod
    def block(cls, nsc, nsym, nt, interp='linear', values=None, time_interp=None):
        """Block pilots: symbol t is antenna t's full-band pilot symbol (``nsym >= nt``)."""
        nsc, nsym, nt = _whole(nsc, 'nsc'), _whole(nsym, 'nsym'), _whole(nt, 'nt')
        if nt < 1 or nsym < nt:
            raise ValueError('block pilots need nsym >= nt >= 1 (nsym = %d, nt = %d)' % (nsym, nt))
        tx = np.repeat(np.arange(nt), max(nsc, 0))
        sc = np.tile(np.arange(max(nsc, 0)), nt)
        return cls(nsc, nsym, nt, tx.copy(), sc, tx, _default_pilot_values(tx.size) if values is None else values, interp, time_interp)


def _pilots_arg(pilots):
    if not isinstance(pilots, OfdmPilots):
        raise ValueError('pilots must be an OfdmPilots')
    return pilots


def ofdm_map_batch(data, pilots):
    """Data symbols and pilots on the resource grid: ``data [B, ndata, nt]`` (vector-major, what the MIMO detectors return) ->
    complex128 ``[B, nt, nsym, nsc]``, zeros where an antenna is silent.  ``grid.reshape(B * nt, nsym, nsc)`` is
    ``ofdm_tx_batch``'s input."""
    p = _pilots_arg(pilots)
    x = _numeric(data, 'data')
    if x.ndim != 3 or x.shape[1:] != (p.ndata, p.nt):
        raise ValueError('data must be [B, ndata, nt] = [B, %d, %d], got %s' % (p.ndata, p.nt, x.shape))
    B = x.shape[0]
    grid = np.zeros((B, p.nt, p.nsym, p.nsc), dtype=np.complex128)
    if B:
        _lib.check(_lib.load().cpx_pilots_map(p.handle(), _lib.ptr(x), B, _lib.ptr(grid)))
    return grid


def ofdm_estimate_shapes(p, B, nr, third, dims):
    return {'y': ((B, p.ndata, nr), np.complex128), 'h': ((B, p.ndata, nr, p.nt), np.complex128),
            third: ((B,) + dims + (nr, p.nt), np.complex128)}


def _ofdm_estimate(entry, third, dims, Y, p, want):
    """Both estimators: ``entry`` writes y_data, h_data and its own third output, ``third`` ``[B, *dims, nr, nt]``."""
    want = _lib.wanted(want, ('y', 'h', third))
    y = _numeric(Y, 'Y')
    if y.ndim != 4 or y.shape[1] < 1 or y.shape[2:] != (p.nsym, p.nsc):
        raise ValueError('Y must be [B, nr, nsym, nsc] = [B, nr, %d, %d], got %s' % (p.nsym, p.nsc, y.shape))
    B, nr = y.shape[:2]
    if nr > OFDM_MAX_ANTENNAS:
        raise ValueError('nr = %d is above the engine limit of %d' % (nr, OFDM_MAX_ANTENNAS))
    out, q = outputs(want, ofdm_estimate_shapes(p, B, nr, third, dims))
    if B:
        _lib.check(getattr(_lib.load(), entry)(p.handle(), _lib.ptr(y), B, nr, q(third), q('y'), q('h')))
    return tuple(out.values())


def ofdm_estimate_batch(Y, pilots, want=('y', 'h')):
    """Pilot-aided channel estimation of ``Y [B, nr, nsym, nsc]`` (``ofdm_rx_batch`` of the B nr received streams, reshaped):
    least squares at the pilots, then ``W[t]`` over the subcarriers.  Returns a tuple of the members of ``(y_data, h_data, h_sc)``
    that ``want`` names ('y', 'h', 'h_sc'), in that order: ``y_data [B, ndata, nr]`` the received data elements, ``h_data
    [B, ndata, nr, nt]`` the estimate at each of them -- reshaped to ``[B ndata, nr]`` and ``[B ndata, nr, nt]`` they are the
    ``y`` and ``h`` of ``linear_batch``, ``kbest_batch``, ``mimo_ml_batch`` ... -- and ``h_sc [B, nsc, nr, nt]`` the estimate per
    subcarrier."""
    p = _pilots_arg(pilots)
    return _ofdm_estimate('cpx_pilots_estimate', 'h_sc', (p.nsc,), Y, p, want)


def ofdm_estimate_tv_batch(Y, pilots, want=('y', 'h')):
    """Pilot-aided estimation of a channel that moves inside the frame: ``Y [B, nr, nsym, nsc]`` as for ``ofdm_estimate_batch``,
    ``pilots`` made with ``time_interp``.  Least squares at every pilot, ``W[t]`` over the subcarriers of each pilot symbol, then
    ``V[t]`` over the symbols.  Returns a tuple of the members of ``(y_data, h_data, h_sym)`` that ``want`` names ('y', 'h',
    'h_sym'), in that order: ``y_data [B, ndata, nr]`` and ``h_data [B, ndata, nr, nt]``, the estimate at each data element's own
    symbol and subcarrier, feed the MIMO detectors as ``ofdm_estimate_batch``'s do; ``h_sym [B, nsym, nsc, nr, nt]`` is the estimate
    on the whole grid."""
    p = _pilots_arg(pilots)
    if p.V is None:
        raise ValueError('pilots were made without time_interp')
    return _ofdm_estimate('cpx_pilots_estimate_tv', 'h_sym', (p.nsym, p.nsc), Y, p, want)
