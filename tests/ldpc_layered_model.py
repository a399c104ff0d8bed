"""The layered normalised / offset min-sum LDPC decoder in NumPy, one layer at a time, and the first-fit schedule.

The code is the edge list of ``cpx_ldpc_create``, sorted by (check, variable).  A schedule is an ordered list of layers; a layer is a list
of checks; every check appears exactly once and no two checks of one layer share a variable.  The rule (float64, operations in the order
written, no fused multiply-add -- NumPy has none); LLRs are positive for bit 0:

Start.       ``Q[v] = min(max(llr[v], -llr_clip), llr_clip)`` on a copy; ``R[e] = +0.0`` for every edge.
Iterations.  ``it = 1 .. n_iters``; within an iteration the layers in order; for every check ``c`` of the layer, its edges ``j`` in
             stored order:
                 m_j  = Q[v_j] - R_cj
                 a_j  = min over i != j of |m_i|
                 g_j  = max(alpha * a_j - beta, 0.0)        two roundings: the product, then the difference
                 s_j  = XOR over i != j of signbit(m_i)     the sign BIT: -0.0 counts as negative
                 R_cj = s_j ? -g_j : g_j
                 Q[v_j] = m_j + R_cj
             No variable is touched twice within a layer, so the order of its checks cannot matter.
Decision.    After the last layer of an iteration ``bit[v] = signbit(Q[v])``.  With ``early_stop``: if every check's parity of bits is
             even the block stops with ``iters = it``, ``converged = 1``; a block that never stops has ``iters = n_iters``,
             ``converged = 0``.  Without ``early_stop``, ``iters = n_iters`` and ``converged`` is the parity test on the final bits.
Rejection.   A block with a NaN anywhere in its LLRs is rejected on its own: bits all zero, ``llr`` all NaN, ``iters = 0``,
             ``converged = 0``.  +-inf is no reason to reject: the clip maps it to +-llr_clip.

Ties need no rule: when two magnitudes tie for the minimum every a_j has the same value whichever of them is called first (below: the
two smallest magnitudes of the row; an entry equal to the smallest takes the second smallest, which a tie makes the same number).
"""
import collections

import numpy as np

Code = collections.namedtuple('Code', 'n_v n_c edge_check edge_var row_ptr')


def code_from_rows(n_v, rows):
    """``rows``: for every check the collection of its variables (sorted here, repeats collapse)."""
    rows = [np.unique(np.asarray(r, dtype=np.int64)) for r in rows]
    row_ptr = np.zeros(len(rows) + 1, dtype=np.int64)
    np.cumsum([len(r) for r in rows], out=row_ptr[1:])
    return Code(int(n_v), len(rows), np.repeat(np.arange(len(rows)), np.diff(row_ptr)), np.concatenate(rows), row_ptr)


def code_from_params(p):
    """The code of a parameter dictionary, from its check adjacency lists."""
    adj = np.asarray(p['cnode_adj_list']).reshape(p['n_cnodes'], p['max_cnode_deg'])
    return code_from_rows(p['n_vnodes'], [adj[c, :p['cnode_deg_list'][c]] for c in range(p['n_cnodes'])])


def params_from_code(code):
    """A parameter dictionary (what ``get_ldpc_code_params`` returns, without the maps nobody here reads) of a ``Code``."""
    deg = np.diff(code.row_ptr)
    adj = -np.ones((code.n_c, deg.max()), dtype=np.int32)
    for c in range(code.n_c):
        adj[c, :deg[c]] = code.edge_var[code.row_ptr[c]:code.row_ptr[c + 1]]
    vdeg = np.bincount(code.edge_var, minlength=code.n_v)
    vadj = -np.ones((code.n_v, max(1, vdeg.max())), dtype=np.int32)
    fill = np.zeros(code.n_v, dtype=int)
    for c, v in zip(code.edge_check, code.edge_var):
        vadj[v, fill[v]] = c
        fill[v] += 1
    return {'n_vnodes': code.n_v, 'n_cnodes': code.n_c, 'max_cnode_deg': int(deg.max()), 'max_vnode_deg': int(vadj.shape[1]),
            'cnode_adj_list': adj.flatten(), 'cnode_deg_list': deg.astype(np.int32), 'vnode_adj_list': vadj.flatten(),
            'vnode_deg_list': vdeg.astype(np.int32)}


def first_fit(code):
    """The default schedule: the checks in index order, each into the lowest-numbered layer in which it shares no variable with a check
    already there; a new layer when there is none."""
    taken, layers = [], []
    for c in range(code.n_c):
        vs = set(code.edge_var[code.row_ptr[c]:code.row_ptr[c + 1]].tolist())
        for l in range(len(layers)):
            if not (taken[l] & vs):
                break
        else:
            l = len(layers)
            layers.append([])
            taken.append(set())
        layers[l].append(c)
        taken[l] |= vs
    return [np.array(l, dtype=np.int32) for l in layers]


def is_schedule(code, schedule):
    """True for a conflict-free partition of the checks."""
    flat = np.concatenate([np.asarray(l) for l in schedule])
    if sorted(flat.tolist()) != list(range(code.n_c)) or any(len(l) == 0 for l in schedule):
        return False
    for l in schedule:
        vs = np.concatenate([code.edge_var[code.row_ptr[c]:code.row_ptr[c + 1]] for c in l])
        if len(set(vs.tolist())) != len(vs):
            return False
    return True


def syndrome(code, bits):
    """``[B][n_c]`` parities of ``bits [B][n_v]``."""
    return np.add.reduceat(bits[:, code.edge_var].astype(np.int64), code.row_ptr[:-1], axis=1) & 1


def _layer_tables(code, layer):
    deg = np.diff(code.row_ptr)[layer]
    j = np.arange(deg.max())[None, :]
    mask = j < deg[:, None]
    eid = np.where(mask, code.row_ptr[layer][:, None] + j, 0)
    return mask, eid, code.edge_var[eid]


def decode(llr, code, schedule, n_iters, alpha=1.0, beta=0.0, early_stop=True, llr_clip=500.0):
    """``llr [B][n_v]`` -> ``{'bits' int8 [B][n_v], 'llr' float64 [B][n_v], 'iters' int32 [B], 'converged' uint8 [B]}``."""
    llr = np.atleast_2d(np.asarray(llr, dtype=np.float64))
    B = llr.shape[0]
    alpha, beta, llr_clip = np.float64(alpha), np.float64(beta), np.float64(llr_clip)
    Q = np.minimum(np.maximum(llr, -llr_clip), llr_clip)
    R = np.zeros((B, len(code.edge_var)))
    rejected = np.isnan(llr).any(axis=1)
    iters = np.zeros(B, dtype=np.int32)
    converged = np.zeros(B, dtype=np.uint8)
    tables = [_layer_tables(code, np.asarray(l, dtype=np.int64)) for l in schedule]
    act = np.flatnonzero(~rejected)
    with np.errstate(invalid='ignore'):
        for it in range(1, n_iters + 1):
            if act.size == 0:
                break
            for mask, eid, var in tables:
                m = Q[act[:, None, None], var] - R[act[:, None, None], eid]
                am = np.where(mask, np.abs(m), np.inf)
                two = np.partition(am, 1, axis=2)[:, :, :2]
                a = np.where(am == two[:, :, :1], two[:, :, 1:], two[:, :, :1])          # min over i != j
                g = np.maximum(alpha * a - beta, 0.0)
                sb = np.signbit(m) & mask
                s = np.logical_xor.reduce(sb, axis=2, keepdims=True) ^ sb               # XOR over i != j
                r_new = np.where(s, -g, g)
                R[act[:, None], eid[mask]] = r_new[:, mask]
                Q[act[:, None], var[mask]] = (m + r_new)[:, mask]
            iters[act] = it
            if early_stop or it == n_iters:
                ok = ~syndrome(code, np.signbit(Q[act])).any(axis=1)
                converged[act[ok]] = 1
                if early_stop:
                    act = act[~ok]
    bits = np.signbit(Q).astype(np.int8)
    bits[rejected] = 0
    Q[rejected] = np.nan
    return {'bits': bits, 'llr': Q, 'iters': iters, 'converged': converged}
