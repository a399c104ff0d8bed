"""The burst form of the fused Viterbi kernel's traceback (csrc/viterbi_cw.hip, WalkBurst): in a group of LGS = 6 steps starting at step t,
steps t .. t + 4 run no walk and step t + 5 carries the walks of steps t - 1 .. t + 4, which read their NHE + 5 distinct ring words once,
at constant offsets from the ring slot of step t + 4: the word of step t + 4 - d at slot base + RING - d of the mirrored ring, before step
t + 5 writes its own word.  NumPy model of that schedule, no GPU: the ring as the kernel writes it (slot tt mod RING and its copy RING slots
above, the two dummy slots for steps > T, chunks of 96 steps), every read of every walk checked against what its slot holds at that moment.

Which walks count: the flushes write the output of the walk of step s where 1 <= s - H <= min(T - H, L) (H = NHE + 5 hops of the whole
walk), so every word of a walk with H + 1 <= s <= T must be the right one; earlier walks read unwritten slots and later ones stale ones,
to valid addresses, and their bytes are never written out.

The limit.  The ring holds the words of steps t + 4 .. t + 4 - (RING - 1) when the burst reads, so the schedule fits while the oldest
distance NHE - 1 + 5 is at most RING - 1: up to 27 hops on 32 slots, and 28 hops + 5 is the first depth the model rejects (the word at
distance 32 is the lower copy of step t + 4 itself).  The kernel asserts NHE + LGS <= RING, one slot inside that.  The issue that asked
for this model names "24 hops + 5" as a depth that fails on 32 slots; by its own ring arithmetic (oldest distance against RING) that depth
fits -- 29 words at distances 0 .. 28 -- and the model finds every one of them, so 24 .. 27 are asserted to FIT below and the rejection
is asserted at the true limit, for three ring sizes, together with the kernel's rule."""
import numpy as np
import pytest

from test_viterbi_walk_stop import tb_hop

LGS, CHUNK = 6, 96
LENGTHS = (12, 16, 17, 18, 23, 24, 25, 26, 27, 28, 29, 30, 96, 97, 98, 99, 100, 101, 102, 103, 206, 300)


def burst_schedule(T, nhe, ring, check=None):
    """Runs the kernel's step / write / burst order for a codeword of T steps.  Returns (violations, walks): violations = the reads of
    walks that count (see above) whose slot offset is negative or whose slot does not hold the word of step s - h, as tuples
    (t, s, h, offset, step found); walks = {s: tile entry} of every walk a burst ran, tile entry relative to its chunk.
    `check(s, words)`, if given, gets the steps whose words the walk of step s read, in hop order."""
    H = nhe + LGS - 1
    slots = np.full(2 * ring + 2, -10 ** 6)                            # the step whose word a slot holds (nothing yet)
    bad, walks = [], {}
    for tc0 in range(1, T + 1, CHUNK):
        ngroups = min((T - tc0) // LGS + 1, CHUNK // LGS)
        for g in range(ngroups):
            t = tc0 + LGS * g
            for R in range(LGS):
                tt = t + R
                if R == LGS - 1:                                       # the burst: before this step's own ring write
                    base = (t + LGS - 2) & (ring - 1)
                    for k in range(LGS):
                        s = t - 1 + k
                        assert s not in walks
                        walks[s] = t - tc0 + k                         # entry li holds the walk of step tc0 + li - 1
                        read = []
                        for h in range(nhe):
                            off = ring - (t + LGS - 2 - s + h)
                            found = slots[base + off] if 0 <= base + off < len(slots) else None
                            read.append(found)
                            if H + 1 <= s <= T and (off < 0 or found != s - h):
                                bad.append((t, s, h, off, found))
                        if check is not None and H + 1 <= s <= T:
                            check(s, read)
                q = tt & (ring - 1)
                if tt <= T:
                    slots[q] = slots[q + ring] = tt
                else:
                    slots[2 * ring] = slots[2 * ring + 1] = tt         # the dummy slots
    return bad, walks


@pytest.mark.parametrize("T", LENGTHS)
def test_every_burst_read_finds_its_word(T):
    """RING = 32, 23 hops: group starts t = 1, 7, ... across the ring wrap (t + 4 >= 32), the 96-step flush and the groups that run past T."""
    bad, walks = burst_schedule(T, 23, 32)
    assert bad == []
    last = ((T - 1) // LGS + 1) * LGS                                  # the last step any group runs
    assert sorted(walks) == list(range(0, last))                       # every walk once; the one of step `last` stays pending
    for s, li in walks.items():
        tc0 = 1 + s // CHUNK * CHUNK                                   # the chunk of step s + 1, whose group runs the walk of step s
        assert li == s - tc0 + 1 and 0 <= li < CHUNK


def test_offsets_and_pairs():
    """The 28 words of a group sit at offsets RING - d, d = 0 .. 27, from the slot of step t + 4: all >= 0, adjacent, an even count."""
    seen = set()
    for k in range(LGS):
        for h in range(23):
            seen.add(32 - (LGS - 1 - k + h))
    assert sorted(seen) == list(range(5, 33)) and len(seen) % 2 == 0


def test_burst_walks_equal_the_walks_taken_one_by_one():
    """Random decision words: the burst's walks, fed with the words its reads find in the ring, give the bits of walks taken step by step."""
    T, nhe, n = 206, 23, 64
    rs = np.random.RandomState(7)
    words = rs.randint(0, 1 << 32, (T + 1, n)).astype(np.uint64) << np.uint64(32) | rs.randint(0, 1 << 32, (T + 1, n)).astype(np.uint64)
    best = rs.randint(0, 64, (T + 1, n)).astype(np.uint32)
    got = {}

    def check(s, read):
        st = best[s]
        for step in read:
            st = tb_hop(LGS, words[step], st)
        got[s] = st & np.uint32(1)
    bad, _ = burst_schedule(T, nhe, 32, check)
    assert bad == [] and sorted(got) == list(range(nhe + LGS, T + 1))
    for s in got:
        st = best[s]
        for h in range(nhe + LGS - 1):                                 # the whole walk of H hops, output = bit LGS - 1
            st = tb_hop(LGS, words[s - h], st)
        assert np.array_equal(got[s], (st >> np.uint32(LGS - 1)) & np.uint32(1)), s


@pytest.mark.parametrize("nhe", [24, 25, 26, 27])
def test_depths_up_to_the_ring_s_31_older_words_fit(nhe):
    assert burst_schedule(206, nhe, 32)[0] == []


@pytest.mark.parametrize("nhe,ring", [(28, 32), (29, 32), (46, 32), (12, 16), (60, 64)])
def test_model_rejects_a_depth_that_does_not_fit(nhe, ring):
    """hops + 5 > RING - 1: the oldest words have been overwritten (or, at distance RING, are the newest word's lower copy)."""
    bad, _ = burst_schedule(206, nhe, ring)
    assert bad and all(off <= 0 for _, _, _, off, _ in bad)


def test_the_limit_is_where_the_arithmetic_puts_it():
    """The first hop count the model rejects is RING - 4: one below it every read finds its word, at it the pending walk's last hop
    reads distance RING.  The kernel's static_assert (hops + LGS <= RING) refuses every depth the model rejects, and one more."""
    for ring in (16, 32, 64):
        assert burst_schedule(206, ring - LGS + 1, ring)[0] == []
        bad, _ = burst_schedule(206, ring - LGS + 2, ring)
        assert bad and {(s - t, h) for t, s, h, _, _ in bad} == {(-1, ring - LGS + 1)}   # only the pending walk's last hop
        for nhe in range(1, ring + 8):
            if burst_schedule(206, nhe, ring)[0]:
                assert not nhe + LGS <= ring, (nhe, ring)
