"""Polar codes on MI355X: encoder, successive cancellation (SC) and CRC-aided successive-cancellation list (SCL) decoding.

``x = u F^{(x)n}`` over GF(2) with ``F = [[1, 0], [1, 1]]``, natural order (no bit reversal).  ``K`` positions of ``u`` carry
information, the others are frozen to 0; information bit ``k`` sits at the ``k``-th smallest information position.  With a CRC of
``c`` bits the information bits are ``A = K - c`` message bits followed by the CRC, most significant bit first.  Code construction
(the reliability order, the frozen mask, the CRC table) is host work; the kernels of csrc/polar.hip receive the mask and the table.
The decoders compute in float64 with the min-sum ``f`` and the exact ``g`` and equal the NumPy model tests/polar_model.py bit for
bit.  The precision mode (``set_precision``) has no effect on polar decoding: there is no float32 variant.
"""
import ctypes

import numpy as np

from commpy_amd import _lib
from commpy_amd._results import outputs, returned
from commpy_amd.channelcoding.gfields import whole

__all__ = ['polar_reliability_order', 'PolarCode', 'crc_append', 'crc_check', 'polar_encode', 'polar_decode']

POLAR_MAX_N = 8192          # and list_size * N <= 8192 (csrc/polar.hip)
LIST_SIZES = (1, 2, 4, 8, 16, 32)
WANT = ('bits', 'crc', 'metric', 'u_llr', 'list')


def _block_length(N):
    N = whole(N, 'N', 2)
    if N & (N - 1):
        raise ValueError('N = %d is not a power of two' % N)
    return N


def polar_reliability_order(N):
    """The indices 0 .. N-1 from least to most reliable by the polarization weight ``W(i) = sum_j b_j(i) 2^(j/4)`` (``b_j`` = bit j
    of i, j = 0 the least significant), ties by index: the information set of a (N, K) code is the last K entries."""
    N = _block_length(N)
    idx = np.arange(N)
    w = np.zeros(N)
    for j in range(N.bit_length() - 1):
        w += ((idx >> j) & 1) * 2.0 ** (j / 4.0)
    return np.lexsort((idx, w)).astype(np.int64)


def _crc_poly(crc):
    if isinstance(crc, (bool, np.bool_)) or not isinstance(crc, (int, np.integer)) or crc < 2:
        raise ValueError('crc = %r, need the generator polynomial as an integer with its leading term (e.g. 0xE21)' % (crc,))
    crc = int(crc)
    c = crc.bit_length() - 1
    if c > 32:
        raise ValueError('a CRC of %d bits is above the limit of 32' % c)
    if not crc & 1:
        raise ValueError('crc = 0x%X has no constant term' % crc)
    return crc, c


def _crc_table(crc, K):
    """[K] uint32: entry k = x^(K-1-k) mod g."""
    g, c = _crc_poly(crc)
    tab = np.zeros(K, dtype=np.uint32)
    r = 1
    for k in range(K - 1, -1, -1):
        if r >> c:
            r ^= g
        tab[k] = r
        r <<= 1
    return tab


def _crc_rows(bits, table):
    """XOR of ``table[k]`` over the one bits of every row: [B, len(table)] -> [B] uint32."""
    return np.bitwise_xor.reduce(np.where(bits != 0, table[None, :], np.uint32(0)), axis=1, dtype=np.uint32) if bits.shape[1] else \
        np.zeros(bits.shape[0], dtype=np.uint32)


def _bit_rows(bits, name, width):
    a = np.asarray(bits)
    if a.ndim not in (1, 2):
        raise ValueError('%s must be 1-D or 2-D, got %d dimensions' % (name, a.ndim))
    if a.dtype.kind not in 'biu':
        raise ValueError('%s must hold integers 0 / 1, got dtype %s' % (name, a.dtype))
    if a.shape[-1] != width:
        raise ValueError('%s has %d bits per row, need %d' % (name, a.shape[-1], width))
    rows = np.ascontiguousarray(np.atleast_2d(a), dtype=np.uint8)
    if rows.size and rows.max() > 1:
        raise ValueError('%s must hold 0 / 1' % name)
    return rows, a.ndim == 1


def crc_append(message_bits, crc):
    """``message_bits [B, A]`` (or 1-D) followed by the ``c = deg crc`` remainder bits of ``m(x) x^c mod crc``, most significant
    first; ``crc`` is the generator polynomial as an integer with its leading term (0xE21: the 5G CRC-11).  Host only."""
    g, c = _crc_poly(crc)
    a = np.asarray(message_bits)
    rows, one = _bit_rows(a, 'message_bits', a.shape[-1] if a.ndim else 0)
    A = rows.shape[1]
    rem = _crc_rows(rows, _crc_table(g, A + c)[:A])
    tail = ((rem[:, None] >> np.arange(c - 1, -1, -1, dtype=np.uint32)[None, :]) & 1).astype(np.uint8)
    out = np.concatenate([rows, tail], axis=1)
    return out[0] if one else out


def crc_check(bits, crc):
    """True for every row of ``bits [B, K]`` (or 1-D) -- message followed by its CRC -- that ``crc`` divides.  Host only."""
    g, c = _crc_poly(crc)
    a = np.asarray(bits)
    rows, one = _bit_rows(a, 'bits', a.shape[-1] if a.ndim else 0)
    if rows.shape[1] <= c:
        raise ValueError('%d bits cannot hold a message and a CRC of %d bits' % (rows.shape[1], c))
    ok = _crc_rows(rows, _crc_table(g, rows.shape[1])) == 0
    return bool(ok[0]) if one else ok


class PolarCode:
    """A (N, K) polar code: ``N = 2^n <= 8192``, ``K`` information positions of which the last ``c = deg crc`` carry a CRC
    (``crc``: generator polynomial with its leading term, or None), so ``A = K - c`` message bits.  The information set is the last
    ``K`` entries of ``order`` (default: ``polar_reliability_order(N)``; e.g. the 5G sequence), or the zeros of the mask ``frozen``
    ``[N]`` (1 = frozen).  Attributes: ``N, K, A, info_positions, frozen, crc_table`` (``[K]`` uint32, None without a CRC)."""

    def __init__(self, N, K, crc=None, order=None, frozen=None):
        self.N = N = _block_length(N)
        if N > POLAR_MAX_N:
            raise ValueError('N = %d is above the engine limit of %d' % (N, POLAR_MAX_N))
        self.K = K = whole(K, 'K', 1)
        if K > N:
            raise ValueError('K = %d is above N = %d' % (K, N))
        if order is not None and frozen is not None:
            raise ValueError('give order or frozen, not both')
        if frozen is not None:
            fz = np.asarray(frozen)
            if fz.shape != (N,) or fz.dtype.kind not in 'biu' or (fz.astype(np.int64) & ~1).any():
                raise ValueError('frozen must be %d values 0 / 1' % N)
            fz = fz.astype(np.uint8)
            if int((fz == 0).sum()) != K:
                raise ValueError('frozen leaves %d information positions, K = %d' % (int((fz == 0).sum()), K))
        else:
            od = polar_reliability_order(N) if order is None else np.asarray(order)
            if od.shape != (N,) or od.dtype.kind not in 'iu' or not np.array_equal(np.sort(od), np.arange(N)):
                raise ValueError('order must be a permutation of 0 .. %d' % (N - 1))
            fz = np.ones(N, dtype=np.uint8)
            fz[od[N - K:]] = 0
        self.frozen = fz
        self.info_positions = np.flatnonzero(fz == 0).astype(np.int64)
        self.crc = None
        self.crc_bits = 0
        self.crc_table = None
        if crc is not None:
            self.crc, self.crc_bits = _crc_poly(crc)
            if self.crc_bits >= K:
                raise ValueError('a CRC of %d bits needs K > %d, got K = %d' % (self.crc_bits, self.crc_bits, K))
            self.crc_table = _crc_table(self.crc, K)
        self.A = K - self.crc_bits

        def create():
            h = ctypes.c_void_p()
            tab = None if self.crc_table is None else _lib.ptr(self.crc_table)
            _lib.check(_lib.load().cpx_polar_create(N, _lib.ptr(self.frozen), self.crc_bits, tab, ctypes.byref(h)))
            return h
        self._handles = _lib.DeviceHandles(create, 'cpx_polar_destroy')

    def _device_handle(self):
        return self._handles.get()

    def check_list_size(self, list_size):
        """``list_size`` as an int; ValueError unless it is 1, 2, 4, 8, 16 or 32 with ``list_size * N <= 8192``."""
        L = whole(list_size, 'list_size', 1)
        if L not in LIST_SIZES:
            raise ValueError('list_size = %d, need one of %s' % (L, ', '.join(map(str, LIST_SIZES))))
        if L * self.N > POLAR_MAX_N:
            raise ValueError('list_size * N = %d * %d is above the engine limit of %d' % (L, self.N, POLAR_MAX_N))
        return L


def _code(code):
    if not isinstance(code, PolarCode):
        raise ValueError('code must be a PolarCode')
    return code


def check_want(want, list_size):
    """``want`` as a tuple of names out of 'bits', 'crc', 'metric', 'u_llr', 'list' ('u_llr' with ``list_size = 1`` only)."""
    want = _lib.wanted(want, WANT)
    if 'u_llr' in want and list_size > 1:
        raise ValueError("'u_llr' is defined for list_size = 1 only")
    return want


def shapes(B, code):
    """The results but 'list', which is the three arrays of ``list_shapes``."""
    return {'bits': ((B, code.A), np.uint8), 'crc': ((B,), np.uint8), 'metric': ((B,), np.float64), 'u_llr': ((B, code.N), np.float64)}


def list_shapes(B, code, L):
    return {'bits': ((B, L, code.K), np.uint8), 'metrics': ((B, L), np.float64), 'live': ((B,), np.int32)}


def polar_encode(message_bits, code):
    """``message_bits [B, A]`` (or 1-D ``[A]``) -> code words ``[B, N]`` (``[N]``) uint8: the CRC of ``code`` is appended, the
    information bits are placed and the transform is applied on the GPU."""
    code = _code(code)
    msg, one = _bit_rows(message_bits, 'message_bits', code.A)
    out = np.zeros((msg.shape[0], code.N), dtype=np.uint8)
    if msg.shape[0]:
        _lib.check(_lib.load().cpx_polar_encode(code._device_handle(), _lib.ptr(msg), msg.shape[0], _lib.ptr(out)))
    return out[0] if one else out


def polar_decode(llr, code, list_size=1, want=('bits',)):
    """Decode ``llr [B, N]`` (or 1-D ``[N]``; positive = bit 0, as ``ldpc_bp_decode``) by successive cancellation (``list_size = 1``)
    or list decoding with ``list_size`` in 2, 4, 8, 16, 32 (``list_size * N <= 8192``).  The chosen path is the best-ranked one
    whose information bits pass the code's CRC (rank 0 if none does, or without a CRC).  ``want`` names the results; they are
    returned in the order listed here (a single result for one name):

    ``'bits'`` message bits ``[B, A]`` uint8; ``'crc'`` ``[B]`` bool, the chosen path passed (True without a CRC); ``'metric'``
    ``[B]`` path metric of the chosen path; ``'u_llr'`` ``[B, N]`` decision LLR of every position (``list_size = 1`` only);
    ``'list'`` a tuple ``(bits [B, L, K] uint8, metrics [B, L], live [B] int32)`` of the final list in rank order -- rows past the
    live count hold zeros and metrics of +inf.  The precision mode has no effect."""
    code = _code(code)
    L = code.check_list_size(list_size)
    want = check_want(want, L)
    a = np.asarray(llr)
    if a.ndim not in (1, 2) or a.shape[-1] != code.N or a.dtype.kind not in 'fiu':
        raise ValueError('llr must be real, [B, %d] or [%d]; got shape %s, dtype %s' % (code.N, code.N, a.shape, a.dtype))
    one = a.ndim == 1
    x = np.ascontiguousarray(np.atleast_2d(a), dtype=np.float64)
    B = x.shape[0]
    tables = shapes(B, code), list_shapes(B, code, L)
    res, p = outputs(want, tables[0])
    lst, q = outputs(tables[1] if 'list' in want else (), tables[1])
    if B:
        _lib.check(_lib.load().cpx_polar_decode(code._device_handle(), _lib.ptr(x), B, L, *map(p, tables[0]), *map(q, tables[1])))
    if 'crc' in res:
        res['crc'] = res['crc'].astype(bool)
    if one:
        res, lst = {name: v[0] for name, v in res.items()}, {name: v[0] for name, v in lst.items()}
    if lst:
        res['list'] = tuple(lst.values())                     # 'list' is the last name
    return returned(res)
