"""Fused Viterbi kernel (csrc/viterbi_cw.hip, WalkBurst): on the mirrored 32-slot ring the 'soft' float64 flavours with compiled-in
generators walk the six tracebacks of a group in one burst in the group's last step (the model: tests/test_viterbi_walk_burst.py).  Bit for
bit against the C oracle through the forced codeword path, as tests/test_viterbi_walk_stop_gpu.py: 130 codewords of (133,171) (two full
waves and one of two lanes), encoded, BPSK over AWGN at Eb/N0 = 3 dB, LLRs.

Message lengths (T = length + 11 trellis steps): 1 and 5 (T = 12, 16: no fast group), 6 and 7 (T = 17, 18: exactly one fast group, then
general ones), 12 .. 17 (every T mod 6), 85 .. 91 (T = 96 .. 102: the walk pending across the 96-step flush, the first group of a second
chunk), 200.  Depths: the default (None: min(30, L), i.e. 30 -- the compile-time hop count -- from length 24 on), 29, 9, 8, 7, 3, 2 on the
burst flavours and 31, 48 on the 64-slot ring, which keeps the walk per step; a depth is compared where the reference traces back at all,
tb_depth - 1 <= T.  Every expected output is computed once and `test_oracle_decodes_every_listed_case` produces them without a GPU."""
import functools

import numpy as np
import pytest

import oracle
from test_viterbi_walk_stop_gpu import B, _decode, _eff, _exists, _rx, _trellis, _want

K7 = "k7_133_171"
MSG = (1, 5, 6, 7, 12, 13, 14, 15, 16, 17, 85, 86, 87, 88, 89, 90, 91, 200)
DEPTHS = (None, 29, 9, 8, 7, 3, 2, 31, 48)


def _cases():
    for nmsg in MSG:
        for tb in DEPTHS:
            if _exists(K7, nmsg, tb):
                yield nmsg, tb


@functools.lru_cache(maxsize=None)
def _tail_rx(nmsg):
    """The last 12 steps all zero: every state ties in the high dwords there, in burst steps and in the steps without a walk."""
    rx = _rx(K7, "soft", nmsg).copy()
    rx[:, -24:] = 0.0
    rx.setflags(write=False)
    return rx


@functools.lru_cache(maxsize=None)
def _tail_want(nmsg, tb):
    return oracle.viterbi_decode(_tail_rx(nmsg), _trellis(K7), tb, "soft")


def test_oracle_decodes_every_listed_case():
    cases = list(_cases())
    assert {n for n, _ in cases} == set(MSG) and {(200, tb) for tb in DEPTHS} <= set(cases)
    assert {(n + 11) % 6 for n in (12, 13, 14, 15, 16, 17)} == set(range(6))
    assert _eff(K7, 1, None) == 7 and _eff(K7, 17, None) == 23 and all(_eff(K7, n, None) == 30 for n in MSG if n >= 85)
    for nmsg, tb in cases:
        want = _want(K7, "soft", nmsg, tb)
        assert want.shape == (B, nmsg + 6) and set(np.unique(want)) <= {0, 1}, (nmsg, tb)
    for nmsg in (16, 91, 200):
        for tb in (None, 9):
            assert _tail_want(nmsg, tb).shape == (B, nmsg + 6)
    assert _want(K7, "soft", 200, None, "nan").shape == (B, 206) and _want(K7, "hard", 200, None).shape == (B, 206)
    assert _want("k7_135_147", "soft", 200, None).shape == (B, 206)


def _note_ok(note, eff):
    assert "viterbi_cw_fused_kernel<6," in note and ",soft," in note, note
    assert ("64-slot ring" in note) == (eff > 30) and ("runtime hops" in note) == (eff != 30), (note, eff)
    assert (",46" in note) == (eff > 30) and (",28" in note) == (eff <= 30), (note, eff)


@pytest.mark.gpu
@pytest.mark.parametrize("nmsg", MSG)
def test_every_depth_at_every_length(gpu, nmsg):
    ran = set()
    for tb in DEPTHS:
        if not _exists(K7, nmsg, tb):
            continue
        got, note = _decode(_rx(K7, "soft", nmsg), _trellis(K7), tb, "soft")
        want = _want(K7, "soft", nmsg, tb)
        bad = np.flatnonzero((got != want).any(axis=1))
        assert bad.size == 0, (nmsg, tb, note, bad[:10], int((got != want).sum()))
        _note_ok(note, _eff(K7, nmsg, tb))
        ran.add(tb)
    assert ran >= {None, 9, 8, 7, 3, 2} and (nmsg < 85 or ran == set(DEPTHS))


@pytest.mark.gpu
@pytest.mark.parametrize("nmsg", [16, 91, 200])
@pytest.mark.parametrize("tb", [None, 9])
def test_zero_tail_takes_the_float64_argmin_in_steps_of_either_kind(gpu, nmsg, tb):
    got, note = _decode(_tail_rx(nmsg), _trellis(K7), tb, "soft")
    assert np.array_equal(got, _tail_want(nmsg, tb)), (nmsg, tb, note)
    _note_ok(note, _eff(K7, nmsg, tb))


@pytest.mark.gpu
@pytest.mark.parametrize("tb", [None, 9])
def test_nan_codewords_in_a_full_a_second_and_the_ragged_wave(gpu, tb):
    got, note = _decode(_rx(K7, "soft", 200, "nan"), _trellis(K7), tb, "soft")
    assert np.array_equal(got, _want(K7, "soft", 200, tb, "nan")), (tb, note)
    clean = np.setdiff1d(np.arange(B), [3, 70, 73, 129])
    assert np.array_equal(got[clean], _want(K7, "soft", 200, tb)[clean])
    assert "viterbi_cw_fused_kernel<6," in note and ("runtime hops" in note) == (tb is not None), note


@pytest.mark.gpu
def test_decoded_twice_into_different_buffers(gpu):
    first, note = _decode(_rx(K7, "soft", 200), _trellis(K7), None, "soft")
    again, note2 = _decode(_rx(K7, "soft", 200).copy(), _trellis(K7), None, "soft")
    assert first is not again and np.array_equal(first, again) and np.array_equal(first, _want(K7, "soft", 200, None))
    _note_ok(note, 30)
    assert note2 == note


@pytest.mark.gpu
def test_untouched_flavours_still_decode(gpu):
    got, note = _decode(_rx(K7, "hard", 200), _trellis(K7), None, "hard")
    assert np.array_equal(got, _want(K7, "hard", 200, None)), note
    assert "viterbi_cw_fused_kernel<6," in note and ",hard," in note and "runtime hops" not in note, note
    got, note = _decode(_rx("k7_135_147", "soft", 200), _trellis("k7_135_147"), None, "soft")
    assert np.array_equal(got, _want("k7_135_147", "soft", 200, None)), note
    assert "table-driven" in note and "runtime hops" not in note, note
