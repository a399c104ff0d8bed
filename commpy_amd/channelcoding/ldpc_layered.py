"""Layered (row-serial) normalised / offset min-sum LDPC decoding on MI355X (csrc/ldpc_layered.hip).

``ldpc_bp_decode`` is the reference's flooding schedule; this is the schedule decoders are built with: the posterior is refreshed after
every layer, so a layer works from the previous layer's results, and the check node scales (``alpha``) or offsets (``beta``) the minimum.
The kernel equals the NumPy model tests/ldpc_layered_model.py bit for bit, the ``'llr'`` output included.

Limits (csrc/ldpc_layered.hip): every check degree between 2 and 32; a schedule that is a conflict-free partition of the checks;
``n_iters >= 1``; ``alpha > 0``, ``beta >= 0``, ``llr_clip > 0``, all finite; the state of one block in LDS, ``8 n_v + 24 n_c`` bytes, at
most 163 840 (there is no HBM path).
"""
import ctypes
import math

import numpy as np

from commpy_amd import _lib
from commpy_amd._results import outputs, returned
from commpy_amd.channelcoding.ldpc import _edge_list, _edges_from_adjacency

__all__ = ['ldpc_layers', 'ldpc_layered_decode']

LL_MIN_DEG, LL_MAX_DEG, LL_LDS_MAX = 2, 32, 160 * 1024         # csrc/ldpc_layered.hip
WANT = ('bits', 'llr', 'iters', 'converged')


def check_want(want):
    """``want`` as a tuple of names out of 'bits', 'llr', 'iters', 'converged'."""
    return _lib.wanted(want, WANT)


def shapes(B, n_v):
    return {'bits': ((B, n_v), np.int8), 'llr': ((B, n_v), np.float64), 'iters': ((B,), np.int32), 'converged': ((B,), np.uint8)}


def code_edges(ldpc_code_params):
    """``(edge_check, edge_var, row_ptr)`` int32 of the code, the edges sorted by (check, variable): those of
    ``parity_check_matrix`` where the dictionary holds one (what ``ldpc_bp_decode`` decodes), else those of the adjacency lists."""
    if ldpc_code_params.get('parity_check_matrix') is not None:
        ec, ev = _edge_list(ldpc_code_params)
    else:
        ec, ev = _edges_from_adjacency(ldpc_code_params)
    n_c = int(ldpc_code_params['n_cnodes'])
    row_ptr = np.zeros(n_c + 1, dtype=np.int64)
    np.cumsum(np.bincount(ec, minlength=n_c), out=row_ptr[1:])
    return ec, ev, row_ptr


def check_code(ldpc_code_params, row_ptr):
    """The limits of the code itself (ValueError naming the limit; host only)."""
    n_v, n_c = int(ldpc_code_params['n_vnodes']), int(ldpc_code_params['n_cnodes'])
    deg = np.diff(row_ptr)
    if deg.min() < LL_MIN_DEG or deg.max() > LL_MAX_DEG:
        c = int(np.flatnonzero((deg < LL_MIN_DEG) | (deg > LL_MAX_DEG))[0])
        raise ValueError('check %d has degree %d, the limit is %d .. %d' % (c, deg[c], LL_MIN_DEG, LL_MAX_DEG))
    lds = 8 * n_v + 24 * n_c
    if lds > LL_LDS_MAX:
        raise ValueError("the state of one block, 8 n_v + 24 n_c = %d bytes, is above the kernel's LDS budget of %d bytes"
                         % (lds, LL_LDS_MAX))
    return n_v, n_c


def _first_fit(n_v, ev, row_ptr):
    used, layers = [], []
    for c in range(len(row_ptr) - 1):
        vs = ev[row_ptr[c]:row_ptr[c + 1]]
        for l, u in enumerate(used):
            if not u[vs].any():
                break
        else:
            l = len(used)
            used.append(np.zeros(n_v, dtype=bool))
            layers.append([])
        used[l][vs] = True
        layers[l].append(c)
    return [np.array(l, dtype=np.int32) for l in layers]


def ldpc_layers(ldpc_code_params):
    """The default schedule, built first-fit on the host: the checks are taken in index order and each goes into the lowest-numbered layer
    in which it shares no variable with a check already there; a new layer is opened when there is none.  Returns a list of int32
    arrays.  For a quasi-cyclic design this recovers the block rows."""
    _, ev, row_ptr = code_edges(ldpc_code_params)
    return _first_fit(int(ldpc_code_params['n_vnodes']), ev, row_ptr)


def check_schedule(schedule, n_v, ev, row_ptr):
    """``schedule`` as a list of int32 arrays: a conflict-free partition of the checks (ValueError otherwise; host only)."""
    n_c = len(row_ptr) - 1
    try:
        layers = [np.asarray(l).reshape(-1) for l in schedule]
    except (TypeError, ValueError):
        raise ValueError('the schedule is not a list of layers, each a list of checks') from None
    if not layers or any(l.size == 0 or l.dtype.kind not in 'iu' for l in layers):
        raise ValueError('the schedule is not a partition of the checks: it has no layer, or an empty layer, or entries that are not integers')
    flat = np.concatenate(layers).astype(np.int64)
    if flat.size != n_c or flat.min() < 0 or flat.max() >= n_c or np.bincount(flat, minlength=n_c).max() != 1:
        raise ValueError('the schedule is not a partition of the checks: every check 0 .. %d must appear exactly once' % (n_c - 1))
    for i, l in enumerate(layers):
        vs = np.concatenate([ev[row_ptr[c]:row_ptr[c + 1]] for c in l])
        if np.unique(vs).size != vs.size:
            raise ValueError('the schedule is not conflict-free: layer %d holds two checks that share a variable' % i)
    return [l.astype(np.int32) for l in layers]


def check_n_iters(n_iters):
    if isinstance(n_iters, (bool, np.bool_)) or not isinstance(n_iters, (int, np.integer)) or not 1 <= n_iters < 2 ** 31:
        raise ValueError('n_iters = %r: the limit is an integer n_iters >= 1' % (n_iters,))
    return int(n_iters)


def check_scaling(alpha, beta, llr_clip):
    try:
        alpha, beta, llr_clip = float(alpha), float(beta), float(llr_clip)
    except (TypeError, ValueError):
        raise ValueError('alpha, beta and llr_clip must be numbers') from None
    if not (math.isfinite(alpha) and alpha > 0.0):
        raise ValueError('alpha = %r: the limit is alpha > 0 and finite' % alpha)
    if not (math.isfinite(beta) and beta >= 0.0):
        raise ValueError('beta = %r: the limit is beta >= 0 and finite' % beta)
    if not (math.isfinite(llr_clip) and llr_clip > 0.0):
        raise ValueError('llr_clip = %r: the limit is llr_clip > 0 and finite' % llr_clip)
    return alpha, beta, llr_clip


class _Plan:
    """One code with one schedule: the checked host arrays and the device handles made from them (one per device, on first use)."""

    def __init__(self, n_v, n_c, ec, ev, layers):
        self.n_v, self.n_c = n_v, n_c
        start = np.zeros(len(layers) + 1, dtype=np.int32)
        np.cumsum([l.size for l in layers], out=start[1:])
        order = _lib.as_i32(np.concatenate(layers))

        def create():
            h = ctypes.c_void_p()
            _lib.check(_lib.load().cpx_ldpc_layered_create(n_v, n_c, len(ec), _lib.ptr(ec), _lib.ptr(ev), len(layers), _lib.ptr(start),
                                                           _lib.ptr(order), ctypes.byref(h)))
            return h
        self._handles = _lib.DeviceHandles(create, 'cpx_ldpc_layered_destroy')

    def handle(self):
        return self._handles.get()


def plan(ldpc_code_params, schedule=None):
    """The ``_Plan`` of the code and ``schedule`` (None: ``ldpc_layers``), checked on the host and cached in the dictionary per schedule,
    in the way ``triang_ldpc_systematic_encode_gpu`` caches its encoder.  The cache belongs to the matrix it was made from."""
    H = ldpc_code_params.get('parity_check_matrix')
    cache = ldpc_code_params.get('_cpx_ldpc_layered')
    if cache is None or cache['H'] is not H:
        cache = ldpc_code_params['_cpx_ldpc_layered'] = {'H': H, 'plans': {}, 'code': None}
    key = None
    if schedule is not None:
        try:
            key = tuple(np.asarray(l).astype(np.int64).tobytes() for l in schedule)
        except (TypeError, ValueError):
            raise ValueError('the schedule is not a list of layers, each a list of checks') from None
    p = cache['plans'].get(key)
    if p is None:
        if cache['code'] is None:
            ec, ev, row_ptr = code_edges(ldpc_code_params)
            n_v, n_c = check_code(ldpc_code_params, row_ptr)
            cache['code'] = (n_v, n_c, ec, ev, row_ptr)
        n_v, n_c, ec, ev, row_ptr = cache['code']
        layers = _first_fit(n_v, ev, row_ptr) if schedule is None else check_schedule(schedule, n_v, ev, row_ptr)
        p = cache['plans'][key] = _Plan(n_v, n_c, ec, ev, layers)
    return p


def ldpc_layered_decode(llr, ldpc_code_params, n_iters, alpha=1.0, beta=0.0, schedule=None, early_stop=True, llr_clip=500.0,
                        want=('bits',)):
    """Layered min-sum decoding of ``llr [B][n_v]`` (or 1-D ``[n_v]``), block-major: one block per row; positive = bit 0, the convention
    of ``ldpc_bp_decode``.  ``want`` names the results; they are returned in the order listed here (a single result for one name):

    ``'bits'`` int8 ``[B][n_v]``; ``'llr'`` float64 ``[B][n_v]``, the final ``Q``; ``'iters'`` int32 ``[B]``; ``'converged'`` uint8
    ``[B]``.

    The code is the edge list of ``cpx_ldpc_create``, sorted by (check, variable).  A schedule is an ordered list of layers; a layer is a
    list of checks; every check appears exactly once and no two checks of one layer share a variable (None: ``ldpc_layers``).  The rule
    (float64, operations in the order written, no fused multiply-add):

    Start.  ``Q[v] = min(max(llr[v], -llr_clip), llr_clip)`` on a copy (the caller's array is not modified); ``R[e] = +0.0`` for every
    edge.

    Iterations.  ``it = 1 .. n_iters``; within an iteration the layers in order; for every check ``c`` of the layer, its edges ``j`` in
    stored order: ``m_j = Q[v_j] - R_cj``; ``a_j = min over i != j of |m_i|``; ``g_j = max(alpha * a_j - beta, 0.0)`` (two roundings: the
    product, then the difference); ``s_j = XOR over i != j of signbit(m_i)`` (the sign *bit*: -0.0 counts as negative);
    ``R_cj = s_j ? -g_j : g_j``; ``Q[v_j] = m_j + R_cj``.  No variable is touched twice within a layer, so the order of its checks
    cannot matter.

    Decision.  After the last layer of an iteration ``bit[v] = signbit(Q[v])``.  With ``early_stop``: if every check's parity of bits is
    even the block stops with ``iters = it`` and ``converged = 1``; a block that never stops has ``iters = n_iters`` and
    ``converged = 0``.  Without ``early_stop``, ``iters = n_iters`` and ``converged`` is the parity test on the final bits.

    Rejection.  A block with a NaN anywhere in its LLRs is rejected on its own: bits all zero, ``'llr'`` all NaN, ``iters = 0``,
    ``converged = 0``.  +-inf is no reason to reject: the clip maps it to +-``llr_clip``.

    Limits, each refused with a ``ValueError`` that names it before any device call: every check degree between 2 and 32; a schedule
    that is not a conflict-free partition of the checks; ``n_iters >= 1``; ``alpha > 0``, ``beta >= 0``, ``llr_clip > 0``, all finite;
    the state of one block in LDS, ``8 n_v + 24 n_c`` bytes, at most 163 840."""
    n_iters = check_n_iters(n_iters)
    alpha, beta, llr_clip = check_scaling(alpha, beta, llr_clip)
    want = check_want(want)
    p = plan(ldpc_code_params, schedule)
    rows = np.asarray(llr)
    if rows.ndim not in (1, 2):
        raise ValueError('llr must be 1-D or 2-D, got %d dimensions' % rows.ndim)
    one = rows.ndim == 1
    rows = np.atleast_2d(rows)
    if rows.shape[1] != p.n_v:
        raise ValueError('llr has %d values per row, the code has n_v = %d' % (rows.shape[1], p.n_v))
    x = _lib.as_f64(rows)
    B = x.shape[0]
    res, q = outputs(want, shapes(B, p.n_v))
    if B:
        _lib.check(_lib.load().cpx_ldpc_layered_decode(p.handle(), _lib.ptr(x), B, n_iters, alpha, beta, 1 if early_stop else 0, llr_clip,
                                                       *map(q, WANT)))
    return returned(res, one)
