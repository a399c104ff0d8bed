"""NumPy model of the multipath channel, the resource mapping and the pilot-aided channel estimator (csrc/ofdm_chan.hip).

Nothing here is taken from the package: the frame bookkeeping (which resource elements carry data, which pilots feed which
least-squares item) and the two interpolation-matrix builders are written a second time, with plain loops where that is the clearest
form, so that the package's host code is checked as well as its kernels."""
import numpy as np


def frequencies(nsc):
    """Signed bin of used subcarrier k in ofdm_tx's input order: the lower half sits below DC, the upper half from bin 1 up."""
    h = nsc // 2
    return np.array([k - h if k < h else k - h + 1 for k in range(nsc)])


def w_linear(nsc, pk):
    f = frequencies(nsc)
    fp = [int(f[k]) for k in pk]
    W = np.zeros((nsc, len(pk)), complex)
    for k in range(nsc):
        fk = int(f[k])
        if fk <= fp[0]:
            W[k, 0] = 1
        elif fk >= fp[-1]:
            W[k, -1] = 1
        else:
            j = max(i for i in range(len(fp)) if fp[i] <= fk)
            a = (fk - fp[j]) / (fp[j + 1] - fp[j])
            W[k, j] += 1 - a
            W[k, j + 1] += a
    return W


def w_taps(nsc, pk, Lmax, nfft):
    f = frequencies(nsc)
    F = np.array([[np.exp(-2j * np.pi * int(f[k]) * l / nfft) for l in range(Lmax)] for k in range(nsc)])
    return F @ np.linalg.pinv(F[list(pk)])


def multipath(x, g):
    """x [B, nt, n], g [B, nr, nt, L] or [nr, nt, L] -> [B, nr, n + L - 1]: a sum of numpy.convolve."""
    x, g = np.asarray(x, complex), np.asarray(g, complex)
    B, nt, n = x.shape
    nr, L = g.shape[-3], g.shape[-1]
    y = np.zeros((B, nr, n + L - 1), complex)
    for b in range(B):
        gb = g[b] if g.ndim == 4 else g
        for r in range(nr):
            for t in range(nt):
                y[b, r] += np.convolve(x[b, t], gb[r, t])
    return y


class Frame:
    """The bookkeeping of one pilot pattern, from the raw pilot list and the matrices W[t]."""

    def __init__(self, nsc, nsym, nt, pil_sym, pil_sc, pil_tx, pil_val, W):
        self.nsc, self.nsym, self.nt = nsc, nsym, nt
        self.pil = [(int(s), int(k), int(t), complex(v)) for s, k, t, v in zip(pil_sym, pil_sc, pil_tx, pil_val)]
        taken = {(s, k) for s, k, _, _ in self.pil}
        self.data = [(s, k) for s in range(nsym) for k in range(nsc) if (s, k) not in taken]
        self.ndata = len(self.data)
        self.pk = [sorted({k for _, k, t, _ in self.pil if t == tx}) for tx in range(nt)]
        self.W = [np.asarray(w, complex) for w in W]
        # per antenna and pilot subcarrier: its pilots (symbol, value) in ascending symbol order
        self.items = [[sorted((s, v) for s, k, t, v in self.pil if t == tx and k == kj) for kj in self.pk[tx]] for tx in range(nt)]
        self.max_count = max(len(it) for items in self.items for it in items)


def map_grid(fr, data):
    """data [B, ndata, nt] -> grid [B, nt, nsym, nsc]."""
    data = np.asarray(data, complex)
    B = data.shape[0]
    grid = np.zeros((B, fr.nt, fr.nsym, fr.nsc), complex)
    if fr.ndata:
        ds, dk = np.array(fr.data).T
        for t in range(fr.nt):
            grid[:, t, ds, dk] = data[:, :, t]
    for s, k, t, v in fr.pil:
        grid[:, t, s, k] = v
    return grid


def least_squares(fr, Y):
    """Y [B, nr, nsym, nsc] -> per antenna t the estimates [B, nr, np_t] at its pilot subcarriers."""
    out = []
    for t in range(fr.nt):
        ls = np.zeros(Y.shape[:2] + (len(fr.pk[t]),), complex)
        for j, (kj, item) in enumerate(zip(fr.pk[t], fr.items[t])):
            acc = np.zeros(Y.shape[:2], complex)
            for s, v in item:
                acc = acc + Y[:, :, s, kj] * np.conj(v) / abs(v) ** 2
            ls[:, :, j] = acc / len(item)
        out.append(ls)
    return out


def interpolate(fr, ls):
    """-> h_sc [B, nsc, nr, nt]."""
    B, nr = ls[0].shape[:2]
    h = np.zeros((B, fr.nsc, nr, fr.nt), complex)
    for t in range(fr.nt):
        h[:, :, :, t] = np.einsum('kj,brj->bkr', fr.W[t], ls[t])
    return h


def demap(fr, Y, h_sc):
    """-> y_data [B, ndata, nr], h_data [B, ndata, nr, nt]."""
    B, nr = Y.shape[:2]
    if not fr.ndata:
        return np.zeros((B, 0, nr), complex), np.zeros((B, 0, nr, fr.nt), complex)
    ds, dk = np.array(fr.data).T
    return np.ascontiguousarray(Y[:, :, ds, dk].transpose(0, 2, 1)), h_sc[:, dk]


def estimate(fr, Y):
    """(y_data, h_data, h_sc, ls)."""
    Y = np.asarray(Y, complex)
    ls = least_squares(fr, Y)
    h_sc = interpolate(fr, ls)
    y_data, h_data = demap(fr, Y, h_sc)
    return y_data, h_data, h_sc, ls


def h_bound(fr, ls):
    """[B, nsc, nr, nt]: 2 (np_t + c + 8) 2^-53 sqrt(2) sum_j |W_t[k][j]| max_j |LS_j|, the allowance between two float64
    evaluations of W LS (np_t products summed, c pilot symbols averaged, 8 for the roundings of the division and the mean)."""
    B, nr = ls[0].shape[:2]
    out = np.zeros((B, fr.nsc, nr, fr.nt))
    for t in range(fr.nt):
        wsum = np.sum(np.abs(fr.W[t]), axis=1)                      # [nsc]
        lmax = np.max(np.abs(ls[t]), axis=2)                        # [B, nr]
        out[:, :, :, t] = 2 * (len(fr.pk[t]) + fr.max_count + 8) * 2.0 ** -53 * np.sqrt(2) * wsum[None, :, None] * lmax[:, None, :]
    return out
