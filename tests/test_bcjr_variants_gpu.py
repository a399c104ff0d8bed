"""Every row of the BCJR kernel-variant table (csrc/bcjr.hip with_variant) and the path above 16 states (csrc/bcjr_exact.hip), each
through map_decode and turbo_decode, against the CPU oracle: 2 states, 4 states on the shift-register fast path and off it, 8, 16
and 32 states.  B = 3 codewords of N = 9 steps: one full 8-step chunk plus a one-step tail, idle codeword slots.  Two inputs per
trellis: moderate noise, which raises no "detect and redo" flag, and the same data with one received value of 40.0 in codeword 1,
which raises flag (A) for that codeword alone (its literal decode is NaN throughout: every branch probability of that step
underflows).  cpx_last_kernel() must name the row that was meant and the number of codewords that were decoded again."""
import functools

import numpy as np
import pytest

import oracle
from helpers import Perm, make_trellis

pytestmark = pytest.mark.gpu
TOL = 1e-5
B, N, NV, ITERS, SEED = 3, 9, 0.81, 2, 5

# trellis -> (log2 of the state count, shift-register fast path) of the wave-pair kernel that serves it; None: bcjr_exact.hip
ROWS = {"two_state": (1, False), "rsc_legacy_4": (2, True), "rsc_legacy_4_relabelled": (2, False), "rsc_legacy_8": (3, False),
        "k5_23_35": (4, False), "k6_53_75": None}
CASES = [(name, outlier) for name in ROWS for outlier in (False, True)]
IDS = ["%s-%s" % (name, "outlier" if outlier else "moderate") for name, outlier in CASES]


@functools.lru_cache(maxsize=None)
def trellis(name):
    from commpy_amd.channelcoding import Trellis
    if name == "two_state":
        return Trellis(np.array([1]), np.array([[1, 3]]))
    if name == "k6_53_75":
        return Trellis(np.array([5]), np.array([[0o53, 0o75]]))
    if name == "rsc_legacy_4_relabelled":
        # the same code with states 1 and 2 exchanged: the successors of a state are no longer s >> 1 and 2 | (s >> 1)
        tr, pi = make_trellis("rsc_legacy_4"), np.array([0, 2, 1, 3])
        return Trellis.from_tables(tr.k, tr.n, tr.total_memory, pi[tr.next_state_table][pi], tr.output_table[pi])
    return make_trellis(name)


@functools.lru_cache(maxsize=None)
def inputs(outlier):
    rs = np.random.RandomState(SEED)
    sy, p1, p2 = (np.sign(rs.randn(B, N)) + 0.9 * rs.randn(B, N) for _ in range(3))
    li, perm = rs.randn(B, N), rs.permutation(N)
    if outlier:
        sy[1, 4] = 40.0
    for a in (sy, p1, p2, li, perm):
        a.setflags(write=False)
    return sy, p1, p2, li, perm


@functools.lru_cache(maxsize=None)
def reference(name, outlier):
    """The oracle's (L [B][N], bits [B][N]) of map_decode and the bits [B][N] of turbo_decode, computed once per case."""
    sy, p1, p2, li, perm = inputs(outlier)
    tr = trellis(name)
    maps = [oracle.map_decode(sy[b], p1[b], tr, NV, li[b], "decode") for b in range(B)]
    L, bits = np.array([m[0] for m in maps]), np.array([m[1] for m in maps])
    dec = np.array([oracle.turbo_decode(sy[b], p1[b], p2[b], tr, NV, ITERS, Perm(perm), li[b]) for b in range(B)])
    for a in (L, bits, dec):
        a.setflags(write=False)
    return L, bits, dec


def check_note(note, name, outlier, fast_kernel, exact_kernel):
    row = ROWS[name]
    if row is None:
        assert exact_kernel in note, note
    else:
        assert "%s<%d,%s" % (fast_kernel, row[0], "true" if row[1] else "false") in note, note
        assert "redo: %d of %d" % (1 if outlier else 0, B) in note, note


@pytest.mark.parametrize("name,outlier", CASES, ids=IDS)
def test_map_decode_every_variant(gpu, name, outlier):
    from commpy_amd import _lib
    from commpy_amd.channelcoding import map_decode
    sy, p1, _, li, _ = inputs(outlier)
    want, want_bits, _ = reference(name, outlier)
    L, bits = map_decode(sy, p1, trellis(name), NV, li, "decode")
    check_note(_lib.last_kernel(), name, outlier, "map_decode_kernel", "map_exact_kernel")
    assert ("map_literal_kernel" in _lib.last_kernel()) == (ROWS[name] is not None)
    fin = np.isfinite(want)
    assert fin[0].all() and fin[2].all() and fin[1].all() != outlier      # the outlier, and only it, leaves the reference's range
    for pattern in (np.isnan, np.isposinf, np.isneginf):
        assert np.array_equal(pattern(L), pattern(want)), (name, pattern.__name__)
    err = np.max(np.abs(L[fin] - want[fin]))
    print("map_decode %s outlier=%s: max |L - oracle| = %.3e" % (name, outlier, err))
    assert err <= TOL, err
    undecided = fin & (np.abs(want) <= TOL)
    assert undecided.sum() == 0                                          # the seed leaves no decision to rounding: every bit is compared
    assert np.array_equal(bits, want_bits), name


@pytest.mark.parametrize("name,outlier", CASES, ids=IDS)
def test_turbo_decode_every_variant(gpu, name, outlier):
    from commpy_amd import _lib
    from commpy_amd.channelcoding import turbo_decode
    sy, p1, p2, li, perm = inputs(outlier)
    dec = turbo_decode(sy, p1, p2, trellis(name), NV, ITERS, Perm(perm), li)
    check_note(_lib.last_kernel(), name, outlier, "turbo_pass_kernel", "turbo_exact_kernel")
    assert np.array_equal(dec, reference(name, outlier)[2]), name


def test_turbo_decode_float32_slab(gpu):
    """The float32-slab instantiation of the pass (the `fp32-fast` precision mode) on the 4-state row, with the contract of
    tests/test_fp32_fast_gpu.py test_turbo_fast_mode_float32_slab: the note says so and fewer than 1e-4 of the bits differ from the
    float64 decode -- of these 27, none."""
    import commpy_amd
    from commpy_amd import _lib
    from commpy_amd.channelcoding import turbo_decode
    sy, p1, p2, li, perm = inputs(False)
    tr = trellis("rsc_legacy_4")
    ref = turbo_decode(sy, p1, p2, tr, NV, ITERS, Perm(perm), li)
    assert "f32" not in _lib.last_kernel(), _lib.last_kernel()
    commpy_amd.set_precision("fp32-fast")
    try:
        fast = turbo_decode(sy, p1, p2, tr, NV, ITERS, Perm(perm), li)
        note = _lib.last_kernel()
    finally:
        commpy_amd.set_precision("fp64-parity")
    assert "f32 slab" in note and "turbo_pass_kernel<2,true,f32 slab>" in note, note
    assert float(np.mean(fast != ref)) < 1e-4
