"""What bch.py and rs.py share on the host: the field degree of a code and the check of a batch of rows."""
import numpy as np

from commpy_amd.channelcoding.gfields import whole

GF_MIN_M, GF_MAX_M = 3, 14                        # csrc/cpx_gf.h


def field_degree(n, m):
    """``m`` of a code of length ``n``, checked; None: the smallest degree with ``2^m - 1 >= n`` (at least 3)."""
    if m is None:
        if n > (1 << GF_MAX_M) - 1:
            raise ValueError('n = %d is above the engine limit of 2^%d - 1' % (n, GF_MAX_M))
        m = max(GF_MIN_M, n.bit_length())
    m = whole(m, 'm', GF_MIN_M, GF_MAX_M)
    if n > (1 << m) - 1:
        raise ValueError('n = %d is above 2^m - 1 = %d' % (n, (1 << m) - 1))
    return m


def rows(a, name, width, dtype, kinds, holds, unit, top=None, need=None):
    """``a`` as a contiguous ``[B, width]`` array of ``dtype`` and whether it was 1-D.  ValueError unless it is 1-D or 2-D, of a dtype
    kind in ``kinds`` ("must hold ``holds``"), ``width`` ``unit`` long and, with ``top``, within ``0 .. top`` ("must hold ``need``")."""
    a = np.asarray(a)
    if a.ndim not in (1, 2):
        raise ValueError('%s must be 1-D or 2-D, got %d dimensions' % (name, a.ndim))
    if a.dtype.kind not in kinds:
        raise ValueError('%s must hold %s, got dtype %s' % (name, holds, a.dtype))
    if a.shape[-1] != width:
        raise ValueError('%s has %d %s per row, need %d' % (name, a.shape[-1], unit, width))
    if top is not None and a.size and (a.min() < 0 or a.max() > top):
        raise ValueError('%s must hold %s' % (name, need))
    return np.ascontiguousarray(np.atleast_2d(a), dtype=dtype), a.ndim == 1

