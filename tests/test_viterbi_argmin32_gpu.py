"""The fused Viterbi kernel finds the first-argmin state of a 'soft' step on the HIGH DWORDS of the 64 path metrics and falls back to
the float64 minimum tree + first-equal scan for a whole wave when any lane has two or more states whose high dword equals the minimum
one (csrc/viterbi_cw.hip, cw_step, "first-argmin on the high dwords").  (133,171) 'soft' through the forced codeword path against the C
oracle and the state-per-lane kernels on every codeword, at the default depth, a run-time depth and a deep ring, twice.

The rows that can make it fail -- near ties (metrics equal in the high dword, different in the low one), exact ties, large LLRs
(metrics crossing powers of two), a NaN per regime -- fill whole waves of 64 consecutive codewords and also sit alone among ordinary
3 dB codewords; `test_inputs_do_what_they_are_for` checks with a NumPy float64 add-compare-select, on the CPU, that they do so.

The m - 1 = 5 zero-padded steps that end every codeword (steps L + 1 .. T) tie EXACTLY in every codeword -- all branch metrics of such a
step are equal, so states j and j + 32 leave it with equal metrics -- and every wave takes the fallback there.  "A wave that never
ties" can therefore only be asked of the L steps that carry received values; the two wave conditions below are stated over those."""
import numpy as np
import pytest

import oracle
from helpers import make_trellis

B, NBITS = 2085, 64                                                    # 33 waves, the last one ragged (37 codewords)
NEAR_WAVE, TIE_WAVE, LARGE_WAVE, ONE_WAVE, ONE_LANE = 2, 5, 8, 12, 17   # whole waves of one regime; the wave with a single special lane


def _near(rs, n):
    return rs.choice([-1.0, 1.0], n) * 10.0 ** rs.uniform(-9.0, -6.0, n)


def _tie(rs, n, kind):
    if kind == 0:
        return np.zeros(n)
    if kind == 1:
        return rs.choice([-500.0, 500.0], n)
    return rs.choice([-1e308, -501.0, 500.5, 1e300, np.inf, -np.inf], n)   # every value clipped


def _large(rs, coded_row, kind):
    n = coded_row.size
    sign = 2.0 * coded_row - 1.0
    flip = np.where(rs.rand(n) < 0.15, -1.0, 1.0)                      # the survivor's own metric grows too
    if kind == 0:
        mag = rs.uniform(20.0, 499.0, n)
    elif kind == 1:                                                    # runs: large, then ordinary, then large
        mag = np.where((np.arange(n) // 14) % 2 == 0, rs.uniform(100.0, 500.0, n), rs.uniform(0.5, 8.0, n))
    else:                                                              # powers of two and their neighbours
        p = 2.0 ** rs.randint(3, 9, n)
        mag = np.minimum(np.nextafter(p, rs.choice([0.0, 1e9], n)), 500.0)
    return sign * flip * mag


def _encode(tr, msgs):
    """Terminated encoding through the trellis tables, on the host (the input check below runs without a GPU)."""
    nxt, out = np.asarray(tr.next_state_table), np.asarray(tr.output_table)
    bits = np.concatenate([msgs, np.zeros((msgs.shape[0], 6), msgs.dtype)], axis=1)
    st = np.zeros(msgs.shape[0], np.int64)
    coded = np.zeros((msgs.shape[0], bits.shape[1], 2))
    for t in range(bits.shape[1]):
        o = out[st, bits[:, t]]
        coded[:, t, 0], coded[:, t, 1] = o >> 1, o & 1
        st = nxt[st, bits[:, t]]
    return coded.reshape(msgs.shape[0], -1)


@pytest.fixture(scope="module")
def case():
    tr = make_trellis("k7_133_171")
    rs = np.random.RandomState(20261018)
    coded = _encode(tr, rs.randint(0, 2, (B, NBITS)))
    n = coded.shape[1]
    sigma2 = 1.0 / (2.0 * 0.5 * 10.0 ** 0.3)                            # 3 dB, rate 1/2, BPSK: LLR = 2 y / sigma^2
    rx = 2.0 * ((2.0 * coded - 1.0) + rs.randn(B, n) * np.sqrt(sigma2)) / sigma2
    regime = np.zeros(B, int)                                           # 0 ordinary, 1 near ties, 2 exact ties, 3 large
    rows = {1: list(range(64 * NEAR_WAVE, 64 * NEAR_WAVE + 64)) + [64 * ONE_WAVE + ONE_LANE] + list(range(3, B, 97)),
            2: list(range(64 * TIE_WAVE, 64 * TIE_WAVE + 64)) + list(range(40, B, 131)),
            3: list(range(64 * LARGE_WAVE, 64 * LARGE_WAVE + 64)) + list(range(59, B, 113))}
    for reg in (1, 2, 3):
        for i, b in enumerate(rows[reg]):
            if 64 * ONE_WAVE <= b < 64 * ONE_WAVE + 64 and b != 64 * ONE_WAVE + ONE_LANE:
                continue                                                # that wave keeps 63 ordinary codewords
            regime[b] = reg
            rx[b] = _near(rs, n) if reg == 1 else _tie(rs, n, i % 3) if reg == 2 else _large(rs, coded[b], i % 3)
    # half a codeword of near ties / exact ties, then the channel: the tie has to resolve as the reference resolves it
    for b in (200, 201, 1300, B - 5):
        rx[b, :n // 2] = _near(rs, n // 2) if b % 2 == 0 else 0.0
        regime[b] = 1 if b % 2 == 0 else 2
    nan_rows = {0: (0, 1), 64 * NEAR_WAVE + 9: (n - 1, 1), 64 * TIE_WAVE + 63: (17, 1), 64 * LARGE_WAVE: (40, 1), 1000: (18, -1),
                B - 1: (5, 1)}                                          # one NaN per regime: the redo launch (first / last group too)
    for b, (t, sgn) in nan_rows.items():
        rx[b, t] = sgn * np.nan
    return tr, rx, regime, np.array(sorted(nan_rows))


def _host_acs(tr, rx):
    """Per codeword and step of the NumPy float64 add-compare-select (the rule of oracle/np_viterbi.py): number of states whose high
    dword equals the minimum high dword, number of states equal to the minimum, first such state of either kind."""
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
    nhit, neq, first_hit, first_min = (np.zeros((T, Bn), np.int64) for _ in range(4))
    with np.errstate(over="ignore", invalid="ignore"):
        for t in range(1, T + 1):
            r = x[:, 2 * (t - 1):2 * t] if t <= L else np.zeros((Bn, 2))
            nll0 = np.log(np.exp(r) + 1)
            nll1 = nll0 - r
            bm = np.stack([(0.0 + (nll1 if c >> 1 else nll0)[:, 0]) + (nll1 if c & 1 else nll0)[:, 1] for c in range(4)], axis=1)
            cand = pm[:, ps] + bm[:, pc.reshape(-1)].reshape(Bn, S, 2)
            pm = np.take_along_axis(cand, np.argmin(cand, axis=2)[:, :, None], axis=2)[:, :, 0]
            hi = pm.view(np.uint64) >> np.uint64(32)
            hit = hi == hi.min(axis=1, keepdims=True)
            eq = pm == pm.min(axis=1, keepdims=True)
            nhit[t - 1], neq[t - 1] = hit.sum(axis=1), eq.sum(axis=1)
            first_hit[t - 1], first_min[t - 1] = hit.argmax(axis=1), np.argmin(pm, axis=1)
    return L, nhit, neq, first_hit, first_min


def test_inputs_do_what_they_are_for(case):
    tr, rx, regime, nan_rows = case
    clean = np.ones(B, bool)
    clean[nan_rows] = False
    L, nhit, neq, first_hit, first_min = _host_acs(tr, np.where(np.isnan(rx), -500.0, rx))   # (what the kernel's first pass decodes)
    nhit, neq, first_hit, first_min = nhit[:, clean], neq[:, clean], first_hit[:, clean], first_min[:, clean]
    wrong_first = int(((nhit >= 2) & (first_hit != first_min)).sum())
    exact = int((neq[:L] >= 2).sum())                                  # (the padded tail ties in every codeword: not counted)
    print("codeword-steps: >= 2 hits and the first hit is not the first-argmin: %d; exact float64 tie of the minimum in a data step: %d"
          % (wrong_first, exact))
    assert wrong_first >= 100
    assert exact >= 100
    assert (neq[L:] >= 2).all()                                        # (the module docstring's claim about the padded steps)
    # waves of 64 consecutive codewords, over the L steps that carry received values; waves with a NaN row are left out
    tie = np.zeros((L, B), bool)
    tie[:, clean] = nhit[:L] >= 2
    lanes = np.array([np.count_nonzero(tie[:, 64 * w:64 * w + 64].any(axis=0)) for w in range(B // 64)])
    whole = np.array([clean[64 * w:64 * w + 64].all() for w in range(B // 64)])
    print("tying lanes per whole wave:", lanes.tolist())
    assert np.any(whole & (lanes == 0)), "no wave that never ties"
    assert whole[ONE_WAVE] and lanes[ONE_WAVE] == 1 and tie[:, 64 * ONE_WAVE + ONE_LANE].any(), "no wave with exactly one tying lane"
    assert lanes[NEAR_WAVE] >= 63 and lanes[TIE_WAVE] >= 63             # whole waves of them (one lane each holds a NaN)
    assert set(regime[nan_rows]) == {0, 1, 2, 3}                        # a NaN in every regime
    # large LLRs: the minimum crosses powers of two along the codeword
    assert all(np.unique(np.floor(np.log2(np.maximum(np.where(np.isnan(rx[b]), 0, np.abs(np.clip(rx[b], -500, 500))).cumsum(), 1)))).size >= 4
               for b in range(64 * LARGE_WAVE, 64 * LARGE_WAVE + 64))


@pytest.mark.gpu
@pytest.mark.parametrize("tb", [None, 15, 40])
def test_argmin_on_high_dwords_decodes_identically(gpu, case, tb):
    from commpy_amd import _lib
    from test_viterbi_cw_gpu import _decode
    tr, rx, _, _ = case
    got = _decode(rx, tr, tb, "soft", "cw!")
    note = _lib.last_kernel()
    assert "viterbi_cw_fused_kernel<6," in note and ("runtime hops" in note) == (tb is not None), note
    assert ("64-slot ring" in note) == (tb == 40), note
    want = oracle.viterbi_decode_mt(rx, tr, tb, "soft")
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, ("oracle", tb, bad[:10], int((got != want).sum()))
    wave = _decode(rx, tr, tb, "soft", "wave")
    assert "viterbi_wave_kernel" in _lib.last_kernel(), _lib.last_kernel()
    bad = np.flatnonzero((got != wave).any(axis=1))
    assert bad.size == 0, ("state-per-lane kernels", tb, bad[:10])
    assert np.array_equal(_decode(rx, tr, tb, "soft", "cw!"), got)      # a second launch
