"""NumPy model of the pilot-aided OFDM channel estimator that follows a channel moving inside the frame (csrc/ofdm_chan.hip,
cpx_pilots_create_tv / cpx_pilots_estimate_tv): frequency first (W_t over the subcarriers of each pilot symbol), then time (V_t over
the symbols).

Nothing here is taken from the package: the rectangle bookkeeping (which symbols and subcarriers carry an antenna's pilots) and the
three builders of V are written a second time, with plain loops, so that the package's host code is checked as well as its kernels.

The bound (h_tv_bound).  The device forms Hp~_i[k] = chain_j W_t[k][j] LSp_i[j] and the model Hp_i[k] = the same sum in NumPy's order:
two float64 evaluations of np_t products of the same operands, preceded by one rounded product for LSp (count 1, no averaging), differ by
at most e_i[k] = 2 (np_t + 1 + 8) 2^-53 sqrt(2) sum_j |W_t[k][j]| max_j |LSp_i[j]| -- ofdm_chan_model.h_bound of that pilot symbol with
count 1.  Then the device forms H~[s][k] = chain_i V_t[s][i] Hp~_i[k] (ns_t complex multiply-adds from +0) and the model sum_i V_t[s][i]
Hp_i[k].  Each of the two sums of ns_t complex products is within (ns_t + 2) 2^-53 sqrt(2) sum_i |V_t[s][i]| |Hp_i[k]| of the exact
sum of ITS operands (the usual (n + 2) u bound of a complex dot product, sqrt(2) for the complex modulus), and the exact sums differ
by at most sum_i |V_t[s][i]| |Hp~_i[k] - Hp_i[k]| <= sum_i |V_t[s][i]| e_i[k].  Together, to first order in 2^-53:

    |H~[s][k] - H[s][k]| <= sum_i |V_t[s][i]| (e_i[k] + 2 (ns_t + 2) 2^-53 sqrt(2) |Hp_i[k]|)."""
import numpy as np
from scipy.special import j0

U = 2.0 ** -53


def v_linear(nsym, ps):
    """[nsym, len(ps)]: linear in the symbol index between neighbouring pilot symbols, the nearest one held outside them."""
    ps = [int(s) for s in ps]
    V = np.zeros((nsym, len(ps)), complex)
    for s in range(nsym):
        if s <= ps[0]:
            V[s, 0] = 1
        elif s >= ps[-1]:
            V[s, -1] = 1
        else:
            i = max(q for q in range(len(ps)) if ps[q] <= s)
            a = (s - ps[i]) / (ps[i + 1] - ps[i])
            V[s, i] += 1 - a
            V[s, i + 1] += a
    return V


def v_hold(nsym, ps):
    """[nsym, len(ps)]: the nearest pilot symbol, the lower one on a tie."""
    ps = [int(s) for s in ps]
    V = np.zeros((nsym, len(ps)), complex)
    for s in range(nsym):
        best = 0
        for i in range(1, len(ps)):
            if abs(s - ps[i]) < abs(s - ps[best]):
                best = i
        V[s, best] = 1
    return V


def v_doppler(nsym, ps, fd_sym, nvar):
    """[nsym, len(ps)] = R_sp (R_pp + nvar I)^-1, R[a][b] = J0(2 pi fd_sym |a - b|)."""
    ps = [int(s) for s in ps]
    r_sp = np.array([[j0(2 * np.pi * fd_sym * abs(s - q)) for q in ps] for s in range(nsym)])
    r_pp = np.array([[j0(2 * np.pi * fd_sym * abs(a - q)) for q in ps] for a in ps]) + nvar * np.eye(len(ps))
    return (r_sp @ np.linalg.inv(r_pp)).astype(complex)


class Frame:
    """The bookkeeping of one rectangular pilot pattern, from the raw pilot list and the matrices W[t] and V[t].  ValueError (naming
    the antenna and the symbol) unless every antenna has, on each of its pilot symbols, pilots on exactly its pilot subcarriers."""

    def __init__(self, nsc, nsym, nt, pil_sym, pil_sc, pil_tx, pil_val, W, V):
        self.nsc, self.nsym, self.nt = nsc, nsym, nt
        self.pil = {(int(t), int(s), int(k)): complex(v) for s, k, t, v in zip(pil_sym, pil_sc, pil_tx, pil_val)}
        taken = {(s, k) for _, s, k in self.pil}
        self.data = [(s, k) for s in range(nsym) for k in range(nsc) if (s, k) not in taken]
        self.ndata = len(self.data)
        self.pk = [sorted({k for t, _, k in self.pil if t == tx}) for tx in range(nt)]
        self.ps = [sorted({s for t, s, _ in self.pil if t == tx}) for tx in range(nt)]
        for tx in range(nt):
            for s in self.ps[tx]:
                have = sum(1 for k in self.pk[tx] if (tx, s, k) in self.pil)
                if have != len(self.pk[tx]):
                    raise ValueError('antenna %d has pilots on %d of its %d pilot subcarriers in symbol %d' % (tx, have, len(self.pk[tx]), s))
        self.W = [np.asarray(w, complex) for w in W]
        self.V = [np.asarray(v, complex) for v in V]
        # c[t][i][j] = conj(p) / |p|^2 of antenna t's pilot on (s_i, k_j)
        self.coef = [np.array([[np.conj(self.pil[tx, s, k]) / abs(self.pil[tx, s, k]) ** 2 for k in self.pk[tx]] for s in self.ps[tx]])
                     for tx in range(nt)]


def estimate_tv(fr, Y):
    """Y [B, nr, nsym, nsc] -> (y_data [B, ndata, nr], h_data [B, ndata, nr, nt], h_sym [B, nsym, nsc, nr, nt], lsp, hp) with, per
    antenna t, lsp[t] [B, nr, ns_t, np_t] and hp[t] [B, ns_t, nsc, nr]."""
    Y = np.asarray(Y, complex)
    B, nr = Y.shape[:2]
    h_sym = np.zeros((B, fr.nsym, fr.nsc, nr, fr.nt), complex)
    lsp, hp = [], []
    for t in range(fr.nt):
        ls = Y[:, :, fr.ps[t]][:, :, :, fr.pk[t]] * fr.coef[t][None, None]          # [B, nr, ns_t, np_t]
        h = np.einsum('kj,brij->bikr', fr.W[t], ls)                                  # [B, ns_t, nsc, nr]
        h_sym[:, :, :, :, t] = np.einsum('si,bikr->bskr', fr.V[t], h)
        lsp.append(ls)
        hp.append(h)
    if fr.ndata:
        ds, dk = np.array(fr.data).T
        y_data, h_data = np.ascontiguousarray(Y[:, :, ds, dk].transpose(0, 2, 1)), h_sym[:, ds, dk]
    else:
        y_data, h_data = np.zeros((B, 0, nr), complex), np.zeros((B, 0, nr, fr.nt), complex)
    return y_data, h_data, h_sym, lsp, hp


def h_tv_bound(fr, lsp, hp):
    """[B, nsym, nsc, nr, nt]: the bound of the module docstring."""
    B, nr = lsp[0].shape[:2]
    out = np.zeros((B, fr.nsym, fr.nsc, nr, fr.nt))
    for t in range(fr.nt):
        np_t, ns_t = len(fr.pk[t]), len(fr.ps[t])
        wsum = np.sum(np.abs(fr.W[t]), axis=1)                                       # [nsc]
        lmax = np.max(np.abs(lsp[t]), axis=3)                                        # [B, nr, ns_t]
        e = 2 * (np_t + 1 + 8) * U * np.sqrt(2) * wsum[None, None, :, None] * lmax.transpose(0, 2, 1)[:, :, None, :]   # [B, ns_t, nsc, nr]
        per = e + 2 * (ns_t + 2) * U * np.sqrt(2) * np.abs(hp[t])
        out[:, :, :, :, t] = np.einsum('si,bikr->bskr', np.abs(fr.V[t]), per)
    return out
