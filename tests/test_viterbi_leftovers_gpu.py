"""Fused Viterbi kernel (csrc/viterbi_cw.hip): the step's own work besides its arithmetic -- the ring slot's address, the NaN test of the
step's two values, the ring write of the decision word and the OR into the NaN mask -- now stands between the asm statements of the 32-bit
first-argmin (cw_step, "FILLERS"), the NaN test writes a scalar pair of its own, the tie mask is computed ahead of the index, and the two
selects of a butterfly are one statement.  None of that may change a bit: (133,171) 'soft' through the forced fused path "cw!", bit for
bit against `oracle.viterbi_decode_mt` and against the state-per-lane path "wave".

B = 130 codewords (two full waves and a ragged one of two lanes), every lane with LLRs of its own (4 x standard normal: a value taken
from another step, group or lane changes bits).  T trellis steps = L + 5 for L pairs of LLRs:
  * T = 6, 11, 12, 17, 18, 23, 105: no fast group, the first lengths with one, the fast -> general hand-over, more than one 96-step chunk;
    at the default depth (min(30, L)) and at a run-time depth of 15 wherever the reference traces back at all (tb_depth - 1 <= T) and the
    fused kernel applies (tb_depth >= 2).  T = 6 has neither (default depth 1, 14 > 6); it runs the deepest window the reference has, 7.
  * ring: T = 105 wraps the 32-slot ring at steps 32, 64 and 96; depths 2, 7, 29, 30 with B = 256, all four waves of a workgroup
    populated, so that a ring write landing in a neighbour's ring or tile shows.
  * NaN mask: a quiet NaN and a negative-sign NaN at the first and the last step of a group, in the last group that carries received
    values, at step 1 of the ragged wave; lanes 0 and 63.  Flagged codewords equal the oracle, their neighbours the clean decode.
  * tie branch: all-zero LLRs for a whole wave (every step ties in every lane) and one all-zero codeword among noisy ones (one lane
    takes the wave into the float64 fallback).
Only the compile-time-hop kernels (depth 30 here; Lean32) take the new form of the step; the run-time depths run kernels that keep the
former step and share the file, the dispatch and the ring with them.  Expected outputs are computed once per case; `test_oracle_decodes_every_case` produces them without a GPU."""
import functools

import numpy as np
import pytest

import oracle
from helpers import make_trellis

B = 130
STEPS = (6, 11, 12, 17, 18, 23, 105)
RING_DEPTHS = (2, 7, 29, 30)
NAN_AT = ((0, 7, 0, False), (63, 12, 1, True), (64, 100, 1, False), (127, 97, 0, True), (129, 1, 0, False))   # codeword, step, value, negative


@functools.lru_cache(maxsize=None)
def _trellis():
    return make_trellis("k7_133_171")


def _depths(T):
    L = T - 5
    out = [tb for tb in (None, 15) if (min(30, L) if tb is None else tb) >= 2 and (tb is None or tb - 1 <= T)]
    return tuple(out) or (T + 1,)


@functools.lru_cache(maxsize=None)
def _rx(T, variant="plain", b=B):
    rs = np.random.RandomState(7000 + T + 13 * b)
    rx = 4.0 * rs.standard_normal((b, 2 * (T - 5)))
    if variant == "nan":
        for cw, step, val, neg in NAN_AT:
            rx[cw, 2 * (step - 1) + val] = np.copysign(np.nan, -1.0 if neg else 1.0)
    elif variant == "zero_wave":
        rx[:64] = 0.0
    elif variant == "zero_lane":
        rx[70] = 0.0
    rx.setflags(write=False)
    return rx


@functools.lru_cache(maxsize=None)
def _want(T, tb, variant="plain", b=B):
    got = oracle.viterbi_decode_mt(_rx(T, variant, b), _trellis(), tb, "soft")
    got.setflags(write=False)
    return got


def _cases():
    for T in STEPS:
        for tb in _depths(T):
            yield T, tb, "plain", B
    for tb in RING_DEPTHS:
        yield 105, tb, "plain", 256
    for tb in (None, 15):
        yield 105, tb, "nan", B
        yield 105, tb, "plain", B
        for variant in ("zero_wave", "zero_lane"):
            yield 105, tb, variant, B
            yield 23, tb, variant, B


def test_oracle_decodes_every_case():
    assert _depths(6) == (7,) and _depths(11) == (None,) and _depths(12) == (None,) and all(_depths(T) == (None, 15) for T in STEPS[3:])
    assert len({r.tobytes() for r in _rx(105)}) == B                                # every lane has values of its own
    rx = _rx(105, "nan")
    assert np.isnan(rx).sum() == len(NAN_AT) and np.signbit(rx[63, 23]) and np.signbit(rx[127, 192]) and not np.signbit(rx[0, 12])
    assert {(s - 1) % 6 for _, s, _, _ in NAN_AT} == {0, 5, 3} and max(s for _, s, _, _ in NAN_AT) == 100   # first / last step of a group; the last received step
    for T, tb, variant, b in _cases():
        want = _want(T, tb, variant, b)
        assert want.shape == (b, T - 5) and set(np.unique(want)) <= {0, 1}, (T, tb, variant, b)


def _both(T, tb, variant="plain", b=B):
    from commpy_amd import _lib
    from commpy_amd.channelcoding import viterbi_decode
    with _lib.forced_path("viterbi", "cw!"):
        got = viterbi_decode(_rx(T, variant, b), _trellis(), tb, "soft")
        note = _lib.last_kernel()
    with _lib.forced_path("viterbi", "wave"):
        wave = viterbi_decode(_rx(T, variant, b), _trellis(), tb, "soft")
        wnote = _lib.last_kernel()
    assert "viterbi_cw_fused_kernel<6," in note and ",soft," in note and "viterbi_cw_fused_kernel" not in wnote, (note, wnote)
    want = _want(T, tb, variant, b)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, (T, tb, variant, b, note, bad[:10], int((got != want).sum()))
    assert np.array_equal(got, wave), (T, tb, variant, b, note, wnote)
    return got, note


@pytest.mark.gpu
@pytest.mark.parametrize("T", STEPS)
def test_lengths_around_the_first_fast_group_and_the_second_chunk(gpu, T):
    for tb in _depths(T):
        _, note = _both(T, tb)
        eff = min(30, T - 5) if tb is None else tb
        assert ("runtime hops" in note) == (eff != 30), (note, T, tb)


@pytest.mark.gpu
@pytest.mark.parametrize("tb", RING_DEPTHS)
def test_ring_wraps_with_four_waves_in_the_workgroup(gpu, tb):
    _, note = _both(105, tb, "plain", 256)
    assert ("runtime hops" in note) == (tb != 30), note


@pytest.mark.gpu
@pytest.mark.parametrize("tb", [None, 15])
def test_nan_of_either_sign_at_group_edges_in_lanes_0_and_63(gpu, tb):
    got, _ = _both(105, tb, "nan")
    clean = np.setdiff1d(np.arange(B), [cw for cw, _, _, _ in NAN_AT])
    assert np.array_equal(got[clean], _want(105, tb)[clean])                        # neighbours of the flagged codewords: untouched


@pytest.mark.gpu
@pytest.mark.parametrize("T", [23, 105])
@pytest.mark.parametrize("variant", ["zero_wave", "zero_lane"])
def test_ties_in_every_step_of_a_wave_and_of_a_single_lane(gpu, variant, T):
    for tb in (None, 15):
        _both(T, tb, variant)
