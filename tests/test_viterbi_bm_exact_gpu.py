"""The fused Viterbi kernel's lean branch-metric arithmetic (csrc/cpx_math.h: exp_pm500, div_unscaled; csrc/viterbi_cw.hip: clip500,
LEAN cw_step, the output flush) is bit-identical to the arithmetic it replaced: (133,171) 'soft' through the forced codeword path, LLRs
in every regime of the rewritten routines, against the C oracle and against the state-per-lane kernels (which keep the library exp,
the IEEE division and the literal clip) on every codeword, at the default depth and at a run-time depth, twice.

Batch: the path switch "cw!" runs the fused kernel at any batch size, so the test uses 2 085 codewords instead of the 29 492 the
default dispatch starts at -- nine workgroups, the last one ragged (37 codewords in its only wave)."""
import numpy as np
import pytest

import oracle
from helpers import make_trellis

pytestmark = pytest.mark.gpu

B, NBITS = 2085, 64
LN2 = float(np.log(2.0))


def _pool():
    tiny = [0.0, 5e-324, 1e-310, 2.2250738585072014e-308, 1e-300]
    sweep = np.linspace(30.0, 40.0, 801)                               # exp(r) + 1 stops changing (r ~ 36.7) / log(1 + e^-r) reaches 0
    k = np.arange(1, 122)
    halves = k * (LN2 / 2)                                             # exp's reduction rounds at odd multiples, steps at even ones
    halves = np.concatenate([halves, np.nextafter(halves, 0.0), np.nextafter(halves, 1e9)])
    roots = np.log(np.sqrt(2.0) * 2.0 ** np.arange(1, 60) - 1.0)       # exp(r) + 1 = 2^k sqrt(2): the logarithm's reduction branch
    roots = np.concatenate([roots, np.nextafter(roots, 0.0), np.nextafter(roots, 1e9)])
    edge = [499.9, np.nextafter(500.0, 0.0), 500.0, np.nextafter(500.0, 1e9), 500.1, 709.0, 710.0, 745.2, 1e308, np.inf]
    pos = np.concatenate([tiny, sweep, halves, roots, edge])
    return np.concatenate([pos, -pos])


@pytest.fixture(scope="module")
def case():
    from commpy_amd.channelcoding import conv_encode_batch
    tr = make_trellis("k7_133_171")
    rs = np.random.RandomState(20261017)
    coded = conv_encode_batch(rs.randint(0, 2, (B, NBITS)), tr).astype(float)
    n = coded.shape[1]
    ebn0 = 10.0 ** 0.3                                                  # 3 dB, rate 1/2, BPSK: LLR = 2 y / sigma^2
    sigma2 = 1.0 / (2.0 * 0.5 * ebn0)
    rx = 2.0 * ((2.0 * coded - 1.0) + rs.randn(B, n) * np.sqrt(sigma2)) / sigma2
    pool = _pool()
    per = 8                                                             # special values per codeword, the rest is the 3 dB channel
    order = np.concatenate([rs.permutation(len(pool)) for _ in range(-(-B * per // len(pool)))])[:B * per].reshape(B, per)
    assert len(np.unique(order)) == len(pool)                           # every value of the pool is used
    for b in range(B):
        rx[b, rs.choice(n, per, replace=False)] = pool[order[b]]
    for b, vals in ((3, pool[:n]), (700, pool[n:2 * n]), (B - 2, np.resize(pool[2 * n:], n))):   # whole codewords of pool values
        rx[b] = vals
    rx[5] = np.where(rs.rand(n) < 0.5, 500.1, -1e308)                   # every value clipped
    for b, t in ((0, 0), (64, n - 1), (1000, 17), (1001, 18), (B - 1, 40)):   # NaN: the redo launch (first / last group, neighbours)
        rx[b, t] = np.nan
    rx[1500, 7] = -np.nan
    return tr, rx


@pytest.mark.parametrize("tb", [None, 15])
def test_lean_branch_metrics_decode_identically(gpu, case, tb):
    from commpy_amd import _lib
    from test_viterbi_cw_gpu import _decode
    tr, rx = case
    got = _decode(rx, tr, tb, "soft", "cw!")
    note = _lib.last_kernel()
    assert "viterbi_cw_fused_kernel<6," in note and ("runtime hops" in note) == (tb is not None), note
    want = oracle.viterbi_decode_mt(rx, tr, tb, "soft")
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, ("oracle", tb, bad[:10], int((got != want).sum()))
    wave = _decode(rx, tr, tb, "soft", "wave")
    assert "viterbi_wave_kernel" in _lib.last_kernel(), _lib.last_kernel()
    bad = np.flatnonzero((got != wave).any(axis=1))
    assert bad.size == 0, ("state-per-lane kernels", tb, bad[:10])
    assert np.array_equal(_decode(rx, tr, tb, "soft", "cw!"), got)      # a second launch
