"""NumPy model of where the fused Viterbi kernel's ring write stands after it was moved into the first-argmin block of its own step
(csrc/viterbi_cw.hip, cw_step "FILLERS").  In the last step of a group, step t + 5, the write of that step's decision word now comes
BEFORE WalkBurst::finish() and behind the four read batches of the group's walks; in Lean32, the other flavour that takes the pinned
form (ring stored once, walk per step), it comes before WalkHook::finish() and behind the reads of the walk of the step before.  LDS executes a wave's accesses in order, so the reads see the
ring as it was; what the model checks is the stronger statement that the order does not matter at all: the slots the step writes
(ring slot t & 31 and its mirror 32 slots above) are never among the slots those reads name, for every step over two wraps of the
ring, for four waves of a workgroup; and that no wave's slots, dummy slots or tile reach into a neighbour's part of the workgroup's LDS.
The present address formula -- slot (t & 31) * 64 + lane words from the wave's base -- is the one the kernel keeps.  The ring sizes, the
tile row and the waves per workgroup are read from the kernel's source, and the two layout formulas are asserted to stand there as
modelled; the schedule itself (which step writes, which words a walk names) is a model of the source's comments and code, not parsed."""
import os
import re

import numpy as np

SRC = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "commpy_amd", "csrc", "viterbi_cw.hip")).read()


def _const(name):
    m = re.search(r"\b%s\s*=\s*(\d+)\b" % name, SRC)
    assert m, name
    return int(m.group(1))


# the layout as csrc/viterbi_cw.hip states it: a changed constant or formula there changes (or fails) the model
RING, RING_DEEP, CHUNK, OBPAD, WAVES = _const("FR_RING"), _const("FR_RING_DEEP"), _const("FR_CHUNK"), _const("FR_OBPAD"), _const("ACS_WAVES")
assert "return MIR ? 2 * RING + 2 : RING + 1;" in SRC                                     # fused_slots
assert "return (size_t)fused_slots<RING, MIR>() * 64 * 8 + (size_t)64 * FR_OBPAD;" in SRC   # fused_wave_lds
assert "smem + (size_t)wv * fused_wave_lds<RING, MIR, GEN>()" in SRC and "ring + fused_slots<RING, MIR>() * 64" in SRC
assert "return 5 * LGS; }" in SRC and "return 8 * LGS; }" in SRC                          # fused_tb, fused_tb_deep
LGS = 6
HOPS = 5 * LGS - 2                            # Mirrored32 / Lean32: the default depth
NHE = HOPS - (LGS - 1)                        # hops a walk's output can see
NW = NHE + LGS - 1                            # distinct words of a group's six walks
SLOTS = 2 * RING + 2                          # mirrored ring + two dummy slots
WAVE_BYTES = SLOTS * 64 * 8 + 64 * OBPAD


def _slot_byte(wave, slot, lane):
    return wave * WAVE_BYTES + (slot * 64 + lane) * 8


def test_a_wave_stays_inside_its_part_of_the_workgroup():
    lanes = np.arange(64)
    assert RING == 32 and CHUNK + 1 <= OBPAD and WAVES * WAVE_BYTES == 160768 <= 160 * 1024   # 157 KB of the CU's 160: unchanged
    for w in range(WAVES):
        lo, hi = w * WAVE_BYTES, (w + 1) * WAVE_BYTES
        ring = np.array([_slot_byte(w, s, lanes) for s in range(SLOTS)])
        assert ring.min() == lo and ring.max() + 8 == lo + SLOTS * 512             # ring, mirror, dummies: contiguous from the base
        tile = lo + SLOTS * 512 + lanes * OBPAD
        assert tile.min() == ring.max() + 8 and tile.max() + OBPAD == hi           # the tile behind them, up to the next wave's base
        assert len(np.unique(ring)) == ring.size


def test_the_step_write_is_not_among_the_words_the_burst_reads():
    lanes = np.arange(64)
    for t in range(1, 2 * RING + 2 * LGS, LGS):                                    # groups over more than two wraps
        tt = t + LGS - 1                                                           # the burst's step
        pb = (tt - 1) & (RING - 1)                                                 # slot of step t + LGS - 2, lower copy
        reads = {pb + RING - d for d in range(NW)}                                 # pb[(RING - d) * 64]
        q = tt & (RING - 1)
        writes = {q, q + RING}
        assert not (reads & writes), (t, sorted(reads), writes)
        assert max(reads) < 2 * RING and min(reads) >= 0
        for w in range(WAVES):                                                     # the same in bytes, against the present formula
            want = w * WAVE_BYTES + ((tt & (RING - 1)) * 64 + lanes) * 8
            assert np.array_equal(_slot_byte(w, q, lanes), want)
        # the words of the reads are those of steps t + LGS - 2 - d, each still in the ring when the step's write has happened
        for d in range(NW):
            step = t + LGS - 2 - d
            if step >= 1:
                assert (step & (RING - 1)) in {(pb + RING - d) % RING} and tt - step < RING


def test_the_step_write_is_not_among_the_words_a_per_step_walk_reads():
    # Lean32 (the flavour this is about); the same holds on a mirrored ring walked per step and on the deep ring (8 LGS - 2 hops)
    for ring, mirrored, hops in ((RING, False, HOPS), (RING, True, HOPS), (RING_DEEP, False, 8 * LGS - 2)):
        for tt in range(1, 3 * ring):
            q = tt & (ring - 1)
            writes = {q, q + ring} if mirrored else {q}
            prev = (tt - 1) & (ring - 1)
            reads = {prev + ring - h for h in range(hops)} if mirrored else {(prev - h) & (ring - 1) for h in range(hops)}
            assert not (reads & writes), (ring, mirrored, tt)
