"""The fused Viterbi kernel reads the first-argmin state of a 'soft' step off the minima of an 8 x 8 grid of the 64 high dwords: state
s = 8 j + i sits in row j and column i, a step computes the eight row minima and the eight column minima, and "exactly one row and
exactly one column equal the overall minimum" holds exactly when one state does -- state 8 j* + i*.  Any other lane sends its wave to the
float64 minimum tree and first-equal scan, as before (csrc/viterbi_cw.hip, cw_step, "first-argmin on the high dwords").

What the block can get wrong is an operand: state s sits in register rotl(s, R + 1) with R = step mod 6, so each of the 6 x 64 (rotation,
state) pairs is one operand slot of the row part and one of the column part; and the tie test has three geometries -- two hits in one
row, in one column, in neither.  `test_inputs_reach_every_operand_and_tie_geometry` checks on the CPU, with a NumPy float64
add-compare-select, that the inputs of tests/test_viterbi_argmin32_gpu.py exercise all of them and that the identity itself holds on their
metrics; the GPU tests then ask for bit equality with the C oracle and the state-per-lane kernels in every flavour that shares the step."""
import ctypes

import numpy as np
import pytest

import oracle
from test_viterbi_argmin32_gpu import B, case  # noqa: F401  (the fixture: 2085 codewords of 64 bits, 33 waves, the last one ragged)

ROWS, COLS = 8, 8                                                      # the kernel's split of the six state bits: s = COLS * j + i


def _hit_masks(tr, rx):
    """NumPy float64 add-compare-select, the rule of test_viterbi_argmin32_gpu._host_acs: per step and codeword the high dwords of
    the 64 path metrics, (T, B, 64) uint32."""
    nxt, out = np.asarray(tr.next_state_table), np.asarray(tr.output_table)
    S, Bn, L = 64, rx.shape[0], rx.shape[1] // 2
    T = L + 6 - 1
    ps, pc, cnt = np.zeros((S, 2), np.int64), np.zeros((S, 2), np.int64), np.zeros(S, np.int64)
    for p in range(S):
        for i in range(2):
            s = nxt[p, i]
            ps[s, cnt[s]], pc[s, cnt[s]] = p, out[p, i]
            cnt[s] += 1
    x = np.clip(rx, -500, 500)
    pm = np.full((Bn, S), np.inf)
    pm[:, 0] = 0.0
    hi = np.zeros((T, Bn, S), np.uint32)
    with np.errstate(over="ignore", invalid="ignore"):
        for t in range(1, T + 1):
            r = x[:, 2 * (t - 1):2 * t] if t <= L else np.zeros((Bn, 2))
            nll0 = np.log(np.exp(r) + 1)
            nll1 = nll0 - r
            bm = np.stack([(0.0 + (nll1 if c >> 1 else nll0)[:, 0]) + (nll1 if c & 1 else nll0)[:, 1] for c in range(4)], axis=1)
            cand = pm[:, ps] + bm[:, pc.reshape(-1)].reshape(Bn, S, 2)
            pm = np.take_along_axis(cand, np.argmin(cand, axis=2)[:, :, None], axis=2)[:, :, 0]
            hi[t - 1] = (pm.view(np.uint64) >> np.uint64(32)).astype(np.uint32)
    return hi


def _popcount(w):
    return sum((w >> k) & 1 for k in range(16))


def _lowest_bit(w):
    """Index of the lowest set bit of a non-zero word (v_ffbl_b32)."""
    return np.log2((w & -w).astype(np.float64)).astype(np.int64)


def test_inputs_reach_every_operand_and_tie_geometry(case):  # noqa: F811
    tr, rx, _, nan_rows = case
    hi = _hit_masks(tr, np.delete(rx, nan_rows, axis=0))               # (a row with a NaN is decoded again by the redo launch)
    T = hi.shape[0]
    m = hi.min(axis=2, keepdims=True)
    hit = hi == m
    nhit = hit.sum(axis=2)
    first = hit.argmax(axis=2)
    # the identity, on the block's own terms: row and column minima, one 16-bit word with the column hits in bits 15:8 and the row hits
    # in bits 7:0, tie <=> popcount != 2, index = 8 * (lowest row bit) + (lowest column bit)
    grid = hi.reshape(T, -1, ROWS, COLS)
    rmin, qmin = grid.min(axis=3), grid.min(axis=2)
    assert np.array_equal(qmin.min(axis=2, keepdims=True), m) and np.array_equal(rmin.min(axis=2, keepdims=True), m)
    word = np.zeros(nhit.shape, np.int64)
    for i in range(COLS):
        word |= (qmin[:, :, i] == m[:, :, 0]).astype(np.int64) << (8 + i)
    for j in range(ROWS):
        word |= (rmin[:, :, j] == m[:, :, 0]).astype(np.int64) << j
    assert ((word & 0xFF) != 0).all() and ((word >> 8) != 0).all()      # at least one row and one column hit in every lane
    tie = _popcount(word) != 2
    assert np.array_equal(tie, nhit >= 2)
    index = COLS * _lowest_bit(word & 0xFF) + _lowest_bit(word >> 8)
    assert np.array_equal(index[~tie], first[~tie])
    # every (first-argmin state, step mod 6) pair among the steps with one hit: 64 states x 6 rotations of the register map
    step = np.broadcast_to(np.arange(T)[:, None], nhit.shape)
    one = nhit == 1
    pairs = np.bincount(first[one] * 6 + step[one] % 6, minlength=384)
    print("(state, step mod 6) pairs among one-hit steps: %d of 384, the rarest %d times" % (np.count_nonzero(pairs), pairs.min()))
    assert pairs.min() >= 1
    # two hits: same row, same column, neither
    two = nhit == 2
    a = first[two]
    b = 63 - hit[two][:, ::-1].argmax(axis=1)                           # the other hit
    same_row, same_col = a // COLS == b // COLS, a % COLS == b % COLS
    geo = {"same row": int(same_row.sum()), "same column": int(same_col.sum()), "neither": int((~same_row & ~same_col).sum())}
    print("two-hit steps by geometry:", geo)
    assert (a != b).all() and min(geo.values()) >= 50, geo


@pytest.fixture(scope="module")
def want(case):  # noqa: F811
    tr, rx, _, _ = case
    memo = {}

    def get(tb):
        if tb not in memo:
            memo[tb] = oracle.viterbi_decode_mt(rx, tr, tb, "soft")
        return memo[tb]
    return get


@pytest.mark.gpu
@pytest.mark.parametrize("tb", [None, 15, 40])
def test_row_column_argmin_decodes_identically(gpu, case, want, tb):  # noqa: F811
    """Mirrored32 (default depth), run-time hops (tb 15) and Deep64 (tb 40)."""
    from commpy_amd import _lib
    from test_viterbi_cw_gpu import _decode
    tr, rx, _, _ = case
    got = _decode(rx, tr, tb, "soft", "cw!")
    note = _lib.last_kernel()
    assert "viterbi_cw_fused_kernel<6," in note and ("runtime hops" in note) == (tb is not None), note
    assert ("64-slot ring" in note) == (tb == 40), note
    bad = np.flatnonzero((got != want(tb)).any(axis=1))
    assert bad.size == 0, ("oracle", tb, bad[:10], int((got != want(tb)).sum()))
    wave = _decode(rx, tr, tb, "soft", "wave")
    assert "viterbi_wave_kernel" in _lib.last_kernel(), _lib.last_kernel()
    bad = np.flatnonzero((got != wave).any(axis=1))
    assert bad.size == 0, ("state-per-lane kernels", tb, bad[:10])
    assert np.array_equal(_decode(rx, tr, tb, "soft", "cw!"), got)      # a second launch


@pytest.mark.gpu
def test_row_column_argmin_in_the_lean_ring(gpu, case, want):  # noqa: F811
    """Lean32, the ring stored once: what a whole round takes when a remainder runs beside it (one round of 256 codewords per compute
    unit plus 64).  The batch is the case's rows over and over -- 2085 = 37 mod 64, so every repeat puts them on other lanes -- and
    every codeword is compared with the oracle's row it repeats."""
    from commpy_amd import _lib
    from test_viterbi_cw_gpu import _decode
    tr, rx, _, _ = case
    cus = ctypes.c_int(0)
    _lib.check(_lib.load().cpx_device_info(None, 0, ctypes.byref(cus), None))
    nb = 256 * cus.value + 64
    src = np.arange(nb) % B
    got = _decode(rx[src], tr, None, "soft", "auto")
    note = _lib.last_kernel()
    assert "ring stored once" in note and "beside the round" in note, note
    ref = want(None)[src]
    bad = np.flatnonzero((got != ref).any(axis=1))
    assert bad.size == 0, ("oracle", bad[:10], int((got != ref).sum()))
