"""The traceback walk of the fused Viterbi kernel (csrc/viterbi_cw.hip, tb_hop / WalkHook) never masks its state: a hop is
st' = (st << 1) | bit, in unmasked 32-bit arithmetic, where `bit` is bit 63 - (st mod S) of the step's 64-bit decision word.  After n hops
bit k of the state is therefore the bit shifted in at hop n - k (k < n), or bit k - n of the start state (k >= n).  The output of a walk of
H hops is bit LGS - 1 of its final state; with

    he = max(H - (LGS - 1), 0)         hops to execute
    sh = LGS - 1 - min(H, LGS - 1)     bit to take after them

that is bit sh of the state after he hops: the last LGS - 1 hops of a walk (and the ring words they read) cannot change its output.  The
run-time-hop flavours of the kernel stop there.  NumPy model, no GPU: random decision words and start states, LGS in {2, 4, 6}, H = 0 .. 48
(H < LGS - 1, H = LGS - 1 and H = LGS among them)."""
import numpy as np
import pytest

N = 4096
HMAX = 48


def tb_hop(lgs, w, st):
    """One hop as the kernel computes it: hi = high dword of (w << (st mod S)), st' = alignbit(st, hi, 31) = (st << 1) | (hi >> 31)."""
    sh = (st & np.uint32((1 << lgs) - 1)).astype(np.uint64)
    hi = ((w << sh) >> np.uint64(32)).astype(np.uint32)
    return (st << np.uint32(1)) | (hi >> np.uint32(31))                   # uint32: the bits shifted out at the top are dropped


def walk(lgs, words, st, hops):
    for h in range(hops):
        st = tb_hop(lgs, words[h], st)
    return st


def _inputs(lgs):
    rs = np.random.RandomState(100 + lgs)
    words = rs.randint(0, 1 << 32, (HMAX, N)).astype(np.uint64) << np.uint64(32) | rs.randint(0, 1 << 32, (HMAX, N)).astype(np.uint64)
    # start states: a first-argmin state (< S) for half of the walks, any 32-bit pattern for the rest (the identity does not need st < S)
    st = rs.randint(0, 1 << lgs, N).astype(np.uint32)
    st[N // 2:] = rs.randint(0, 1 << 32, N - N // 2).astype(np.uint32)
    return words, st


def test_hop_model_reads_the_state_s_own_bit():
    """bit 63 - s of the word is the decision of state s (cw_step packs state s there)."""
    for lgs in (2, 4, 6):
        for s in range(1 << lgs):
            w = np.array([1 << (63 - s)], np.uint64)
            assert tb_hop(lgs, w, np.array([s], np.uint32))[0] == ((s << 1) | 1)
            assert tb_hop(lgs, ~w, np.array([s], np.uint32))[0] == (s << 1)


@pytest.mark.parametrize("lgs", [2, 4, 6])
def test_output_bit_is_fixed_lgs_minus_one_hops_early(lgs):
    words, st0 = _inputs(lgs)
    for H in range(HMAX + 1):
        he = max(H - (lgs - 1), 0)
        sh = lgs - 1 - min(H, lgs - 1)
        assert 0 <= sh <= lgs - 1 and he + (lgs - 1 - sh) == H
        full = (walk(lgs, words, st0, H) >> np.uint32(lgs - 1)) & np.uint32(1)
        early = (walk(lgs, words, st0, he) >> np.uint32(sh)) & np.uint32(1)
        assert np.array_equal(full, early), (lgs, H, he, sh, int((full != early).sum()))
    # the test would see a wrong identity: one hop fewer gives other bits
    H = 2 * lgs + 3
    full = (walk(lgs, words, st0, H) >> np.uint32(lgs - 1)) & np.uint32(1)
    short = (walk(lgs, words, st0, H - lgs) >> np.uint32(0)) & np.uint32(1)
    assert not np.array_equal(full, short)


@pytest.mark.parametrize("lgs", [2, 4, 6])
def test_hops_beyond_the_run_time_count_leave_the_state_alone(lgs):
    """The kernel's run-time form: every compiled hop slot h runs, a select keeps the state where h >= he; slots are compiled for the
    deepest window only up to HT - (LGS - 1)."""
    words, st0 = _inputs(lgs)
    HT = 5 * lgs - 2
    slots = HT - (lgs - 1)
    for H in range(HT + 1):
        he = max(H - (lgs - 1), 0)
        sh = lgs - 1 - min(H, lgs - 1)
        assert he <= slots
        st = st0.copy()
        for h in range(slots):
            nx = tb_hop(lgs, words[h], st)
            st = nx if h < he else st
        full = (walk(lgs, words, st0, H) >> np.uint32(lgs - 1)) & np.uint32(1)
        assert np.array_equal((st >> np.uint32(sh)) & np.uint32(1), full), (lgs, H)
