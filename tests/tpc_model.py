"""A NumPy model of turbo product codes of two BCH codes: encoder and the iterative Chase-Pyndiah decoder, on top of chase_model.

A code word is [n_c, n_r]: rows are words of the row code, columns of the column code, the message [k_c, k_r] top-left.  Decoder:
W = 0; for h = 0 .. 2 iters - 1 Chase runs along the rows (h even) or the columns (h odd) with llr = R, prior = W, alpha[h], beta[h] and
min(p, length) test positions; W becomes its extrinsic output; the decision of the last half-iteration is the result.
"""
import numpy as np

import bch_model as M
import chase_model as CM

ALPHA = (0.0, 0.2, 0.3, 0.5, 0.7, 0.9, 1.0, 1.0)
BETA = (0.2, 0.4, 0.6, 0.8, 1.0, 1.0, 1.0, 1.0)


def table(values, count, scale=1.0):
    values = [scale * v for v in values]
    return (values + [values[-1]] * count)[:count]


def encode(msg, row, col):
    """msg [B, k_c, k_r] -> [B, n_c, n_r]."""
    msg = np.asarray(msg, dtype=np.uint8)
    B = msg.shape[0]
    rows = M.encode_batch(msg.reshape(B * col.k, row.k), row).reshape(B, col.k, row.n)
    cols = M.encode_batch(CM.words_of(rows, 1), col)
    return CM.block_of(cols, (B, col.n, row.n), 1)


def decode(llr, row, col, iters=4, p=4, alpha=None, beta=None, llr_scale=1.0):
    """llr [B, n_c, n_r] -> {'bits' [B, k_c, k_r], 'codeword' [B, n_c, n_r] uint8, 'extrinsic' [B, n_c, n_r] float64}."""
    R = np.asarray(llr, dtype=np.float64)
    alpha = table(ALPHA if alpha is None else alpha, 2 * iters)
    beta = table(BETA, 2 * iters, llr_scale) if beta is None else table(beta, 2 * iters)
    W = np.zeros(R.shape)
    word = None
    for h in range(2 * iters):
        axis, code = (2, row) if h % 2 == 0 else (1, col)
        res = CM.decode_batch(CM.words_of(R, axis), code, min(p, code.n), beta[h], CM.words_of(W, axis), alpha[h])
        W = CM.block_of(res["extrinsic"], R.shape, axis)
        word = CM.block_of(res["codeword"], R.shape, axis)
    return {"bits": word[:, :col.k, :row.k].copy(), "codeword": word, "extrinsic": W}
