"""The fused Viterbi kernel runs a group of log2(S) steps through one of two bodies (csrc/viterbi_cw.hip, `group`): the FAST one when
the group's own steps and the steps it prefetches all carry received values and lie inside [1, T] (t + 2 lg - 1 <= tmax), today's
general one otherwise.  Bit-exact against the C oracle through the forced codeword path, on 131 codewords (two full waves and one of
3 lanes), at step counts T on every boundary of that split.

What the step counts can be.  The oracle, like the reference, derives everything from the row length: L = len / 2 decoded bits,
T = L + m - 1 steps (m = memory), tmax = L, default depth min(5 m, L).  So for the K = 7 code T >= 6 and tmax = T - 5:
  * T = 6 .. 16 has no fast group (the first one needs 12 <= tmax), T = 17 has exactly one;
  * T = 1 does not exist for any code the kernel serves (m >= 2), and T = 5 only for the smaller codes ((23,35): L = 2, (5,7): L = 4):
    those two K = 7 rows are run through the device entry point, which takes L and the step count separately, against the
    state-per-lane kernels instead of the oracle (`test_step_counts_the_oracle_cannot_express`);
  * the last group of the first 96-step chunk (t = 91) is fast and the first group of the second (t = 97) is general for
    102 <= tmax <= 107, i.e. T = 107 .. 112.
A traceback depth is compared with the oracle where the reference traces back at all (tb - 1 <= T) and the engine accepts it
(tb >= 2); a length at which none of the three depths of a case qualifies runs at tb = 2 instead, so that no length is left out.
`test_oracle_decodes_every_listed_shape` runs without a GPU and produces every expected output the GPU tests use."""
import ctypes
import functools

import numpy as np
import pytest

import oracle
from helpers import make_trellis

B = 131
# K = 7: no fast group | the first fast group (16 | 17) | T mod 6 in {0, 1, 5} around one and two chunks | fast last group of chunk 1 + general first of chunk 2
K7_T = (6, 7, 11, 12, 13, 16, 17, 18, 95, 96, 97, 101, 102, 107, 108, 112, 191, 192, 193)
DEPTHS = (None, 15, 40)
SMALL_T = (5, 6, 7, 11, 12, 13, 17, 18, 95, 96, 97, 101, 102, 191, 192, 193)


@functools.lru_cache(maxsize=None)
def _trellis(name):
    if name == "k7_135_147":                                           # a 64-state pair without compiled-in kernels: table-driven
        from commpy_amd.channelcoding import Trellis
        return Trellis(np.array([6]), np.array([[0o135, 0o147]]))
    return make_trellis(name)


@functools.lru_cache(maxsize=None)
def _rx(name, dtype, T, batch=B):
    m = _trellis(name).total_memory
    L = T - m + 1
    rs = np.random.RandomState(7 * T + {"hard": 0, "soft": 1, "unquantized": 2}[dtype] + 1000 * m)
    bits = rs.randint(0, 2, (batch, 2 * L)).astype(np.float64)
    if dtype == "hard":
        rx = bits
    elif dtype == "unquantized":
        rx = 2.0 * bits - 1 + rs.randn(batch, 2 * L) * 0.8
    else:
        rx = 4.0 * bits - 2 + rs.randn(batch, 2 * L) * 2.0
        rx[rs.rand(*rx.shape) < 0.01] = np.inf
        rx[rs.rand(*rx.shape) < 0.01] = -np.inf
        rx[rs.rand(*rx.shape) < 0.01] = 0.0
    rx.setflags(write=False)
    return rx


def _depths(name, T, wanted):
    """The depths of `wanted` that exist at this length (module docstring); tb = 2 where none does."""
    m = _trellis(name).total_memory
    L = T - m + 1
    ok = [tb for tb in wanted if (min(5 * m, L) >= 2 if tb is None else tb - 1 <= T)]
    return ok or [2]


@functools.lru_cache(maxsize=None)
def _want(name, dtype, T, tb):
    got = oracle.viterbi_decode(_rx(name, dtype, T), _trellis(name), tb, dtype)
    got.setflags(write=False)
    return got


def _cases():
    for dtype in ("hard", "soft", "unquantized"):
        for T in K7_T:
            for tb in _depths("k7_133_171", T, DEPTHS):
                yield "k7_133_171", dtype, T, tb
    for name in ("t57", "k5_23_35", "k7_135_147"):
        for dtype in ("hard", "soft", "unquantized"):
            for T in (K7_T if name == "k7_135_147" else SMALL_T):
                for tb in _depths(name, T, (None,)):
                    yield name, dtype, T, tb


def test_oracle_decodes_every_listed_shape():
    n = 0
    for name, dtype, T, tb in _cases():
        m = _trellis(name).total_memory
        want = _want(name, dtype, T, tb)
        assert want.shape == (B, T - m + 1) and set(np.unique(want)) <= {0, 1}, (name, dtype, T, tb)
        n += 1
    seen = {(name, T) for name, _, T, _ in _cases()}
    assert {("k7_133_171", T) for T in K7_T} <= seen and {("k7_135_147", T) for T in K7_T} <= seen
    assert {(nm, T) for nm in ("t57", "k5_23_35") for T in SMALL_T} <= seen
    assert n >= 3 * (len(K7_T) + 2 * len(SMALL_T) + len(K7_T))
    for name, T, c in NAN_CASES:                                        # the NaN rows sit where their names say
        t_fast, t_gen, tmax = _nan_steps(T)
        assert t_fast + 1 == t_gen and (t_gen - c - 1) % 6 == 0 and t_gen - 6 + 11 <= tmax < t_gen + 11 and tmax == T - 5


def _decode(x, tr, tb, dtype, path):
    from commpy_amd import _lib
    from commpy_amd.channelcoding import viterbi_decode
    with _lib.forced_path("viterbi", path):
        return viterbi_decode(x, tr, tb, dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["hard", "soft", "unquantized"])
@pytest.mark.parametrize("tb", DEPTHS)
def test_k7_every_boundary_of_the_split(gpu, dtype, tb):
    from commpy_amd import _lib
    tr = _trellis("k7_133_171")
    for T in K7_T:
        for d in _depths("k7_133_171", T, (tb,)):
            if d == 2 and tb is not DEPTHS[0]:
                continue                                               # (the tb = 2 stand-in runs once, with the default depth)
            got = _decode(_rx("k7_133_171", dtype, T), tr, d, dtype, "cw!")
            note = _lib.last_kernel()
            eff = min(30, T - 5) if d is None else d
            assert "viterbi_cw_fused_kernel<6," in note and ("64-slot ring" in note) == (eff > 30), (note, T, d)
            assert ("runtime hops" in note) == (eff != 30), (note, T, d)
            want = _want("k7_133_171", dtype, T, d)
            bad = np.flatnonzero((got != want).any(axis=1))
            assert bad.size == 0, (dtype, T, d, bad[:10], int((got != want).sum()))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["hard", "soft", "unquantized"])
@pytest.mark.parametrize("name", ["t57", "k5_23_35", "k7_135_147"])
def test_small_and_table_driven_flavours(gpu, name, dtype):
    from commpy_amd import _lib
    tr = _trellis(name)
    for T in (K7_T if name == "k7_135_147" else SMALL_T):
        for d in _depths(name, T, (None,)):
            got = _decode(_rx(name, dtype, T), tr, d, dtype, "cw!")
            note = _lib.last_kernel()
            assert ("table-driven" if name == "k7_135_147" else "small ring") in note, (note, T)
            want = _want(name, dtype, T, d)
            bad = np.flatnonzero((got != want).any(axis=1))
            assert bad.size == 0, (name, dtype, T, d, bad[:10], int((got != want).sum()))


def _nan_steps(T):
    """K = 7, tmax = T - 5: (last step of the last fast group, first step of the first general group, tmax)."""
    tmax = T - 5
    c = 96 * ((tmax - 1) // 96)                                         # steps before the chunk that holds the boundary
    t_gen = next(t for t in range(c + 1, T + 1, 6) if t + 11 > tmax)
    return t_gen - 1, t_gen, tmax


NAN_CASES = (("one chunk", 101, 0), ("two chunks", 193, 96))


@pytest.mark.gpu
@pytest.mark.parametrize("label,T,c", NAN_CASES)
def test_soft_nan_at_the_seam(gpu, label, T, c):
    """A NaN in the last step of the last fast group, in the first step of the first general group and in step tmax, the neighbour of
    the zero-padded tail -- each in a full wave, in the ragged wave, first and second received value: the flagged codewords come back
    NaN-exact from the redo launch and every other codeword is what it is without them."""
    from commpy_amd import _lib
    tr = _trellis("k7_133_171")
    rx = _rx("k7_133_171", "soft", T).copy()
    rows = {}
    for i, t in enumerate(_nan_steps(T)):
        for b, second in ((5 + i, 0), (64 + 17 + i, 1), (128 + i, i & 1)):
            rx[b, 2 * (t - 1) + second] = np.nan
            rows[b] = t
    got = _decode(rx, tr, None, "soft", "cw!")
    assert "viterbi_cw_fused_kernel<6," in _lib.last_kernel(), _lib.last_kernel()
    want = oracle.viterbi_decode(rx, tr, None, "soft")
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, (label, bad[:10], rows)
    clean = np.setdiff1d(np.arange(B), sorted(rows))
    assert np.array_equal(got[clean], _want("k7_133_171", "soft", T, None)[clean])   # untouched by their neighbours' NaNs


def _dev_decode(tr, rx, L, T, tb, vtype, path, rows_alloc=None, guard=0):
    """cpx_viterbi_decode_batch_dev on a byte buffer of `rows_alloc` rows with `guard` bytes on either side, pre-filled with 0xA5."""
    from commpy_amd import _lib
    from commpy_amd.deviceops import DeviceBuf
    lib = _lib.load()
    nb = rx.shape[0]
    rows_alloc = rows_alloc or nb
    fill = np.full(2 * guard + rows_alloc * L, 0xA5, np.uint8)
    d_in, d_out = DeviceBuf.from_array(rx), DeviceBuf.from_array(fill)
    try:
        with _lib.forced_path("viterbi", path):
            _lib.check(lib.cpx_viterbi_decode_batch_dev(tr._device_handle(), d_in.ptr, nb, rx.shape[1], L, T, tb, vtype,
                                                        ctypes.c_void_p(d_out.ptr.value + guard), None))
            note = _lib.last_kernel()
        return d_out.to_array(fill.shape, np.uint8), note
    finally:
        d_in.free()
        d_out.free()


@pytest.mark.gpu
@pytest.mark.parametrize("L", [96, 97, 98, 99, 191])
def test_flush_writes_its_rows_and_nothing_else(gpu, L):
    """Row lengths with L mod 4 = 0, 1, 2, 3 (and two chunks): 64 guard bytes on either side of the output and the rows beyond the
    batch keep their fill; the rows of the batch are the oracle's."""
    tr = _trellis("k7_133_171")
    T = L + 5
    raw, note = _dev_decode(tr, _rx("k7_133_171", "soft", T), L, T, 30, 1, "cw!", rows_alloc=B + 3, guard=64)
    assert "viterbi_cw_fused_kernel<6," in note, note
    assert (raw[:64] == 0xA5).all() and (raw[-64:] == 0xA5).all(), "guard bytes written"
    body = raw[64:-64].reshape(B + 3, L)
    assert (body[B:] == 0xA5).all(), "rows beyond the batch written"
    assert np.array_equal(body[:B], _want("k7_133_171", "soft", T, None))


@pytest.mark.gpu
@pytest.mark.parametrize("T", [1, 5])
def test_step_counts_the_oracle_cannot_express(gpu, T):
    """K = 7 with 1 and 5 steps (L = T received pairs, no tail): only the device entry point can ask for them; the fused kernel (general
    groups only) against the state-per-lane kernels, all three decoding types, guards intact."""
    tr = _trellis("k7_133_171")
    for vtype, dtype in enumerate(("hard", "soft", "unquantized")):
        rx = np.ascontiguousarray(_rx("k7_133_171", dtype, 17)[:, :2 * T])
        raw, note = _dev_decode(tr, rx, T, T, 2, vtype, "cw!", rows_alloc=B + 1, guard=64)
        assert "viterbi_cw_fused_kernel<6," in note, note
        ref, note = _dev_decode(tr, rx, T, T, 2, vtype, "wave", rows_alloc=B + 1, guard=64)
        assert "viterbi_wave_kernel" in note, note
        assert np.array_equal(raw, ref), (T, dtype)
        assert (raw[:64] == 0xA5).all() and (raw[-64:] == 0xA5).all() and (raw[64 + B * T:] == 0xA5).all()


@pytest.mark.gpu
def test_lean_ring_round_beside_a_remainder(gpu):
    """The ring stored once (Lean32) is what a whole round takes when a remainder runs beside it.  The dispatcher (viterbi.hip,
    viterbi_plan; cpx_internal.h, viterbi_round / viterbi_round_pays) cuts a batch into rounds of 256 codewords per compute unit and
    sends a remainder to the state-per-lane kernels when 20 * remainder < 9 * round: the smallest such batch is one round + 1."""
    from commpy_amd import _lib
    lib = _lib.load()
    cus = ctypes.c_int(0)
    _lib.check(lib.cpx_device_info(None, 0, ctypes.byref(cus), None))
    nb = 256 * cus.value + 1
    assert 20 * nb >= 9 * 256 * cus.value and 20 * 1 < 9 * 256 * cus.value
    tr = _trellis("k7_133_171")
    T = 101                                                             # fast groups, a general tail, a padded tail
    rs = np.random.RandomState(5)
    rx = 4.0 * rs.randint(0, 2, (nb, 2 * (T - 5))) - 2 + rs.standard_normal((nb, 2 * (T - 5))) * 1.6
    got = _decode(rx, tr, None, "soft", "auto")
    note = _lib.last_kernel()
    assert "ring stored once" in note and "beside the round" in note, note
    wave = _decode(rx, tr, None, "soft", "wave")
    assert "viterbi_wave_kernel" in _lib.last_kernel(), _lib.last_kernel()
    bad = np.flatnonzero((got != wave).any(axis=1))
    assert bad.size == 0, (bad[:10], int((got != wave).sum()))
