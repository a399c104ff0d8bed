"""NumPy model of the timing / frequency-offset synchroniser (csrc/sync.hip).

Nothing here is taken from the package.  The window sums are evaluated literally (every window summed on its own, in extended
precision), so that the model has no running-sum error of its own and energy outside a window cannot reach it; the preamble's bin
rule and ofdm_tx are written a second time."""
import numpy as np

LD = np.longdouble
CLD = np.clongdouble


def q_e(y, D):
    """y [B, nr, n] -> q [B, n - D] (complex), e [B, n - D], in extended precision."""
    y = np.asarray(y, dtype=complex).astype(CLD)
    a, b = y[:, :, :y.shape[2] - D], y[:, :, D:]
    q = np.sum(np.conj(a) * b, axis=1)
    e = np.sum(a.real ** 2 + a.imag ** 2 + b.real ** 2 + b.imag ** 2, axis=1) / 2
    return q, e


def windows(y, D, W):
    """(P [B, nd] clongdouble, E [B, nd] longdouble), nd = n - D - W + 1: every window summed on its own."""
    q, e = q_e(y, D)
    sw = np.lib.stride_tricks.sliding_window_view
    zero = LD(0)                                            # a sum starts from +0: never -0
    return sw(q, W, axis=1).sum(axis=-1) + zero, sw(e, W, axis=1).sum(axis=-1) + zero


def metric_of(P, E):
    """M = |P|^2 / E^2 where E > 0, +0 where E == 0, NaN where E is NaN; in the precision of its arguments."""
    P, E = np.asarray(P), np.asarray(E)
    with np.errstate(divide='ignore', invalid='ignore'):
        m = (P.real ** 2 + P.imag ** 2) / (E * E)
    return np.where(E == 0, 0 * E, m)


def metric(y, D, W):
    """(P complex128, E float64, M float64), each [B, nd], rounded once from the extended-precision values."""
    P, E = windows(y, D, W)
    return P.astype(complex), E.astype(float), metric_of(P, E).astype(float)


def bound(y, D, W):
    """(bound on |P - P_model|, bound on |E - E_model|), each [B, nd]: 2 (W + 2048 + 8) 2^-53 sqrt(2) times the sum over r and
    i in [d - 2048, d + W + 2048) within the row of |y_i| |y_{i+D}| (for E: of e_i)."""
    y = np.asarray(y, dtype=complex)
    n = y.shape[2]
    nq, nd = n - D, n - D - W + 1
    mag = np.abs(y)
    a = np.sum(mag[:, :, :nq] * mag[:, :, D:], axis=1)
    e = np.sum(mag[:, :, :nq] ** 2 + mag[:, :, D:] ** 2, axis=1) / 2
    # every window summed on its own (terms >= 0, no cancellation: a difference of running sums would lose a quiet window behind a
    # loud stretch); 2048 zeros either side stand for the row's ends
    sw = np.lib.stride_tricks.sliding_window_view
    out = []
    for v in (a, e):
        pad = np.zeros((v.shape[0], 2048))
        sums = sw(np.concatenate([pad, v, pad], axis=1), W + 4096, axis=1).sum(axis=-1)
        assert sums.shape[1] == nd
        out.append(2 * (W + 2048 + 8) * 2.0 ** -53 * np.sqrt(2) * sums)
    return out


def first_argmax(M, lo=0, hi=None):
    """Per row the smallest d in [lo, hi) n [0, nd) whose M is the largest of the non-NaN values there; -1 where there is none."""
    M = np.asarray(M)
    lo, hi = max(lo, 0), M.shape[1] if hi is None else min(hi, M.shape[1])
    out = []
    for row in M:
        best, at = None, -1
        for d in range(lo, hi):
            if not np.isnan(row[d]) and (best is None or row[d] > best):
                best, at = row[d], d
        out.append(at)
    return np.array(out, dtype=np.int64)


def align(y, start, step, nout):
    """out[b, r, k] = y[b, r, start[b] + k] exp(1j step[b] k), zeros outside the row; step None: a copy."""
    y = np.asarray(y, dtype=complex)
    B, nr, n = y.shape
    out = np.zeros((B, nr, nout), complex)
    for b in range(B):
        for k in range(nout):
            i = int(start[b]) + k
            if 0 <= i < n:
                out[b, :, k] = y[b, :, i] if step is None else y[b, :, i] * np.exp(1j * step[b] * k)
    return out


def preamble_bins(nfft, nsc):
    """FFT bin of each used subcarrier in ofdm_tx's input order: the lower half below DC (the top bins), the upper from bin 1."""
    h = nsc // 2
    return np.array([nfft - h + k if k < h else k - h + 1 for k in range(nsc)])


def preamble(nfft, nsc, values):
    """values on the used subcarriers whose bin is even, zeros elsewhere, times sqrt(2)."""
    bins = preamble_bins(nfft, nsc)
    return np.array([values[k] * np.sqrt(2.0) if bins[k] % 2 == 0 else 0.0 for k in range(nsc)], dtype=complex)


def ofdm_tx(x, nfft, cp):
    """x [nsym, nsc] -> nsym (cp + nfft) samples: the bins filled by preamble_bins' map, ifft, cyclic prefix (0 < cp < nfft)."""
    x = np.asarray(x, dtype=complex)
    nsym, nsc = x.shape
    F = np.zeros((nsym, nfft), complex)
    F[:, preamble_bins(nfft, nsc)] = x
    t = np.fft.ifft(F, axis=-1)
    return np.concatenate([t[:, nfft - cp:], t], axis=-1).reshape(-1)
