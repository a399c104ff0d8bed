"""Turbo product codes (block turbo codes) of two BCH codes on MI355X: encoder and the iterative Chase-Pyndiah decoder.

A code word is a block ``[n_c, n_r]``: every row is a word of ``row_code`` (length ``n_r``), every column a word of ``col_code``
(length ``n_c``); the message ``[k_c, k_r]`` sits in the top-left corner.  The decoder runs csrc/bch_chase.hip alternately along the
rows and the columns of the block, in place on the device, and equals tests/tpc_model.py bit for bit.  Extended BCH components (the
overall parity bit of most deployed product codes) are not provided.
"""
import numpy as np

from commpy_amd import _lib
from commpy_amd._results import outputs, returned
from commpy_amd.channelcoding.bch import BCHCode, bch_encode
from commpy_amd.channelcoding.gfields import whole

__all__ = ['ProductCode', 'tpc_encode', 'tpc_decode']

TPC_WANT = ('bits', 'codeword', 'extrinsic')
TPC_DEV_WANT = ('codeword', 'extrinsic')
ALPHA = (0.0, 0.2, 0.3, 0.5, 0.7, 0.9, 1.0, 1.0)                  # Pyndiah's tables, per half-iteration
BETA = (0.2, 0.4, 0.6, 0.8, 1.0, 1.0, 1.0, 1.0)


def shapes(B, code):
    block = (B, code.n_c, code.n_r)
    return {'bits': ((B, code.k_c, code.k_r), np.uint8), 'codeword': (block, np.uint8), 'extrinsic': (block, np.float64)}


class ProductCode:
    """The product of ``row_code`` and ``col_code`` (``BCHCode``s).  Attributes: ``row_code, col_code, n_r, k_r, n_c, k_c`` and
    ``n = n_c * n_r``, ``k = k_c * k_r``."""

    def __init__(self, row_code, col_code):
        if not isinstance(row_code, BCHCode) or not isinstance(col_code, BCHCode):
            raise ValueError('row_code and col_code must be BCHCodes')
        self.row_code, self.col_code = row_code, col_code
        self.n_r, self.k_r, self.n_c, self.k_c = row_code.n, row_code.k, col_code.n, col_code.k
        self.n, self.k = self.n_c * self.n_r, self.k_c * self.k_r


def _table(values, name, count, default, scale=1.0):
    """``count`` finite floats: ``values`` (a number or a sequence, its last entry repeated) or the default table times ``scale``."""
    if values is None:
        values = [scale * v for v in default]
    elif isinstance(values, (int, float, np.integer, np.floating)) and not isinstance(values, (bool, np.bool_)):
        values = [values]
    try:
        values = [float(v) for v in values]
    except (TypeError, ValueError):
        raise ValueError('%s must be a number or a sequence of numbers' % name)
    if not values or not all(np.isfinite(v) for v in values):
        raise ValueError('%s must hold finite numbers' % name)
    return (values + [values[-1]] * count)[:count]


def tpc_args(code, iters, p, alpha, beta, llr_scale):
    """The arguments of the decoder, checked: ``(code, iters, p, alpha[2 iters], beta[2 iters])``."""
    if not isinstance(code, ProductCode):
        raise ValueError('code must be a ProductCode')
    iters = whole(iters, 'iters', 1, 1000)
    p = whole(p, 'p', 1, 8)
    if isinstance(llr_scale, (bool, np.bool_)) or not isinstance(llr_scale, (int, float, np.integer, np.floating)) or not np.isfinite(llr_scale) \
            or llr_scale <= 0:
        raise ValueError('llr_scale = %r, need a positive finite number' % (llr_scale,))
    alpha = _table(alpha, 'alpha', 2 * iters, ALPHA)
    beta = _table(beta, 'beta', 2 * iters, BETA, float(llr_scale))
    if min(beta) < 0:
        raise ValueError('beta must be >= 0')
    return code, iters, p, alpha, beta


def tpc_encode(message_bits, code):
    """``message_bits [B, k_c, k_r]`` (or ``[k_c, k_r]``) in 0 / 1 -> code words ``[B, n_c, n_r]`` (``[n_c, n_r]``) uint8: the rows are
    encoded with ``row_code``, then all ``n_r`` columns with ``col_code``."""
    if not isinstance(code, ProductCode):
        raise ValueError('code must be a ProductCode')
    a = np.asarray(message_bits)
    if a.ndim not in (2, 3) or a.shape[-2:] != (code.k_c, code.k_r):
        raise ValueError('message_bits has shape %s, need [B, %d, %d]' % (a.shape, code.k_c, code.k_r))
    if a.dtype.kind not in 'biu' or (a.size and (a.min() < 0 or a.max() > 1)):
        raise ValueError('message_bits must hold integers 0 / 1')
    m = a.reshape(-1, code.k_c, code.k_r).astype(np.uint8)
    B = m.shape[0]
    rows = bch_encode(m.reshape(B * code.k_c, code.k_r), code.row_code).reshape(B, code.k_c, code.n_r)
    cols = bch_encode(rows.transpose(0, 2, 1).reshape(B * code.n_r, code.k_c), code.col_code).reshape(B, code.n_r, code.n_c)
    out = np.ascontiguousarray(cols.transpose(0, 2, 1))
    return out[0] if a.ndim == 2 else out


def tpc_decode(llr, code, iters=4, p=4, alpha=None, beta=None, llr_scale=1.0, want=('bits',)):
    """Iterative soft decoding (Pyndiah) of ``llr [B, n_c, n_r]`` (or ``[n_c, n_r]``) float64, positive = bit 0.  With ``R = llr``
    and ``W = 0``: for the half-iterations ``h = 0 .. 2 iters - 1``, ``chase_decode`` runs along the rows (``h`` even) or the columns
    (``h`` odd) with ``llr = R``, ``prior = W``, ``alpha[h]``, ``beta[h]`` and ``min(p, length)`` test positions, and ``W`` becomes
    its extrinsic output.  The decision of the last half-iteration is the result.  There is no early stop, so a block decodes the
    same in every batch.

    ``alpha`` and ``beta`` are numbers or sequences per half-iteration (the last value is repeated); the defaults are Pyndiah's
    tables ``alpha = (0, .2, .3, .5, .7, .9, 1, 1)`` and ``beta = llr_scale * (.2, .4, .6, .8, 1, 1, 1, 1)``.  The tables assume
    soft values of unit mean magnitude: pass the mean ``|LLR|`` as ``llr_scale``, ``2 / sigma^2`` for BPSK over AWGN.

    ``want`` names the results, returned in this order: ``'bits'`` ``[B, k_c, k_r]`` uint8, ``'codeword'`` ``[B, n_c, n_r]`` uint8,
    ``'extrinsic'`` ``[B, n_c, n_r]`` float64 (the last half-iteration's soft output).  One upload, ``2 iters`` kernel launches on
    one stream, one download.  A block with a NaN or an infinity loses only the row and the column through it, in every
    half-iteration (``chase_decode`` rejects those words)."""
    from commpy_amd.deviceops import DeviceBuf, tpc_decode_dev
    code, iters, p, alpha, beta = tpc_args(code, iters, p, alpha, beta, llr_scale)
    want = _lib.wanted(want, TPC_WANT)
    a = np.asarray(llr)
    if a.ndim not in (2, 3) or a.shape[-2:] != (code.n_c, code.n_r):
        raise ValueError('llr has shape %s, need [B, %d, %d]' % (a.shape, code.n_c, code.n_r))
    if a.dtype.kind not in 'iuf':
        raise ValueError('llr must hold real numbers, got dtype %s' % a.dtype)
    x = np.ascontiguousarray(a.reshape(-1, code.n_c, code.n_r), dtype=np.float64)
    B = x.shape[0]
    res, _ = outputs(TPC_DEV_WANT, shapes(B, code))
    if B:
        names = tuple(n for n in ('codeword', 'extrinsic') if n in want or (n == 'codeword' and 'bits' in want))
        d_llr = DeviceBuf.from_array(x)
        got = tpc_decode_dev(code, d_llr, B, iters, p, alpha, beta, 1.0, want=names)
        got = got if isinstance(got, tuple) else (got,)
        _lib.check(_lib.load().cpx_stream_sync(None))
        for n, buf in zip(names, got):
            res[n] = buf.to_array(x.shape, res[n].dtype)
            buf.free()
        d_llr.free()
    res['bits'] = np.ascontiguousarray(res['codeword'][:, :code.k_c, :code.k_r])
    return returned({n: res[n] for n in TPC_WANT if n in want}, a.ndim == 2)
