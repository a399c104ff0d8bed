"""Fused Viterbi kernel (csrc/viterbi_cw.hip): where the step has the 32-bit first-argmin ('soft', 64 states, float64, compiled-in
generators) the traceback walk runs all of its hops behind one wait for the LDS counter, elsewhere in four batches; the
run-time-hop flavours of either kind stop a walk LGS - 1 hops early and take a lower bit of the state (the identity: tests/test_viterbi_walk_stop.py).
Bit for bit against the C oracle through the forced codeword path, 130 codewords (two full waves and one of two lanes), messages of 13
and 200 bits, encoded, BPSK over AWGN at Eb/N0 = 3 dB ('soft': LLRs, 'unquantized': the received values, 'hard': their signs).

Depths: the issue's list, tb_depth 2 / 3 (fewer hops than LGS - 1), 6 / 7 / 8 / 9 (H = LGS - 2 .. LGS + 1 for 64 states), 29 / 30 / 31 (the
default depth and its neighbours on either ring), 36 / 37 / 48 (64-slot ring).  A depth is compared where the reference traces back at
all, tb_depth - 1 <= T (beyond that it returns its uninitialised buffer and the oracle has nothing to say): the 13-bit message, T = 24 for
K = 7, takes the depths up to 9 and its default, min(5 m, L) = 19; the 200-bit one takes them all.  The `cpx_last_kernel()` note of every
decode shows which flavour ran.  Every expected output is computed once (`_want`) and `test_oracle_decodes_every_listed_case` produces
them without a GPU.  Not run here: the ring stored once (Lean32), which only a whole round beside a remainder takes --
tests/test_viterbi_tailpeel_gpu.py::test_lean_ring_round_beside_a_remainder decodes through it."""
import functools

import numpy as np
import pytest

import oracle
from helpers import make_trellis

B = 130
MSG = (13, 200)
K7_DEPTHS = (2, 3, 6, 7, 8, 9, 29, 30, 31, 36, 37, 48, None)
SMALL = {"t57": (2, 3, 4, None), "k5_23_35": (2, 5, 6, None)}
TABLE_DEPTHS = (None, 12)                                             # (0o135, 0o147): its default depth and one below it
TYPES = ("hard", "soft", "unquantized")


@functools.lru_cache(maxsize=None)
def _trellis(name):
    if name == "k7_135_147":                                          # a 64-state pair without compiled-in kernels: table-driven
        from commpy_amd.channelcoding import Trellis
        return Trellis(np.array([6]), np.array([[0o135, 0o147]]))
    return make_trellis(name)


@functools.lru_cache(maxsize=None)
def _rx(name, dtype, nmsg, variant="plain"):
    """Encoded random messages, BPSK (bit b -> 2 b - 1), AWGN at Eb/N0 = 3 dB for rate 1/2: sigma^2 = 1 / (2 R Eb/N0) = 10^-0.3."""
    from commpy_amd.channelcoding.convcode import conv_encode_batch
    tr = _trellis(name)
    rs = np.random.RandomState(1000 * tr.total_memory + nmsg + {"hard": 0, "soft": 1, "unquantized": 2}[dtype])
    coded = conv_encode_batch(rs.randint(0, 2, (B, nmsg)), tr, "term").astype(np.float64)
    sigma2 = 10.0 ** -0.3
    y = 2.0 * coded - 1.0 + rs.standard_normal(coded.shape) * np.sqrt(sigma2)
    if dtype == "hard":
        rx = (y > 0).astype(np.float64)
    elif dtype == "unquantized":
        rx = y
    else:
        rx = 2.0 * y / sigma2                                         # LLR log P1 / P0
    if variant == "zero_tail":                                        # the last 12 steps carry no information: every state ties there
        rx = rx.copy()
        rx[:, -24:] = 0.0
    elif variant == "nan":                                            # a full wave, the second wave, the ragged one; first / second value
        rx = rx.copy()
        for b, pos in ((3, 0), (64 + 9, 41), (129, rx.shape[1] - 1), (70, rx.shape[1] // 2)):
            rx[b, pos] = np.nan
    rx.setflags(write=False)
    return rx


def _steps(name, nmsg):
    m = _trellis(name).total_memory
    L = nmsg + m
    return L, L + m - 1                                               # decoded bits, trellis steps


def _exists(name, nmsg, tb):
    L, T = _steps(name, nmsg)
    return True if tb is None else tb - 1 <= T


def _eff(name, nmsg, tb):
    L, _ = _steps(name, nmsg)
    return min(5 * _trellis(name).total_memory, L) if tb is None else tb


@functools.lru_cache(maxsize=None)
def _want(name, dtype, nmsg, tb, variant="plain"):
    got = oracle.viterbi_decode(_rx(name, dtype, nmsg, variant), _trellis(name), tb, dtype)
    got.setflags(write=False)
    return got


def _cases():
    for dtype in TYPES:
        for nmsg in MSG:
            for tb in K7_DEPTHS:
                if _exists("k7_133_171", nmsg, tb):
                    yield "k7_133_171", dtype, nmsg, tb
            for name, depths in SMALL.items():
                for tb in depths:
                    if _exists(name, nmsg, tb):
                        yield name, dtype, nmsg, tb
        for tb in TABLE_DEPTHS:
            yield "k7_135_147", dtype, 200, tb


def test_oracle_decodes_every_listed_case():
    cases = list(_cases())
    for name, dtype, nmsg, tb in cases:
        want = _want(name, dtype, nmsg, tb)
        assert want.shape == (B, _steps(name, nmsg)[0]) and set(np.unique(want)) <= {0, 1}, (name, dtype, nmsg, tb)
    k7 = {(nmsg, tb) for name, _, nmsg, tb in cases if name == "k7_133_171"}
    assert {(200, tb) for tb in K7_DEPTHS} <= k7                      # the long message runs every depth of the list
    assert {(13, tb) for tb in (2, 3, 6, 7, 8, 9, None)} <= k7 and _eff("k7_133_171", 13, None) == 19
    for name, depths in SMALL.items():                                # the small codes run all of theirs at either length
        assert {(nmsg, tb) for nmsg in MSG for tb in depths} <= {(n, t) for nm, _, n, t in cases if nm == name}
    for variant in ("zero_tail", "nan"):
        assert _want("k7_133_171", "soft", 200, None, variant).shape == (B, 206)
    assert np.isnan(_rx("k7_133_171", "soft", 200, "nan")).sum() == 4


def _decode(x, tr, tb, dtype):
    from commpy_amd import _lib
    from commpy_amd.channelcoding import viterbi_decode
    with _lib.forced_path("viterbi", "cw!"):
        got = viterbi_decode(x, tr, tb, dtype)
        return got, _lib.last_kernel()


def _check(name, dtype, nmsg, tb, variant="plain"):
    got, note = _decode(_rx(name, dtype, nmsg, variant), _trellis(name), tb, dtype)
    want = _want(name, dtype, nmsg, tb, variant)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, (name, dtype, nmsg, tb, variant, note, bad[:10], int((got != want).sum()))
    return got, note


@pytest.mark.gpu
@pytest.mark.parametrize("nmsg", MSG)
@pytest.mark.parametrize("dtype", TYPES)
def test_k7_depths_on_every_flavour(gpu, dtype, nmsg):
    ran = set()
    for tb in K7_DEPTHS:
        if not _exists("k7_133_171", nmsg, tb):
            continue
        _, note = _check("k7_133_171", dtype, nmsg, tb)
        eff = _eff("k7_133_171", nmsg, tb)
        assert "viterbi_cw_fused_kernel<6," in note and ",%s," % dtype in note, (note, tb)
        assert ("64-slot ring" in note) == (eff > 30), (note, tb)     # Deep64: always run-time hops
        assert ("runtime hops" in note) == (eff != 30), (note, tb)
        assert (",46" in note) == (eff > 30) and (",28" in note) == (eff <= 30), (note, tb)
        ran.add(eff)
    assert ran >= ({2, 3, 6, 7, 8, 9, 19} if nmsg == 13 else {2, 3, 6, 7, 8, 9, 29, 30, 31, 36, 37, 48})


@pytest.mark.gpu
@pytest.mark.parametrize("nmsg", MSG)
@pytest.mark.parametrize("dtype", TYPES)
@pytest.mark.parametrize("name", sorted(SMALL))
def test_small_ring_depths(gpu, name, dtype, nmsg):
    m = _trellis(name).total_memory
    for tb in SMALL[name]:
        _, note = _check(name, dtype, nmsg, tb)
        assert "viterbi_cw_fused_kernel<%d," % m in note and "small ring" in note, (note, tb)
        assert ("runtime hops" in note) == (_eff(name, nmsg, tb) != 5 * m), (note, tb)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", TYPES)
def test_table_driven_depths(gpu, dtype):
    for tb in TABLE_DEPTHS:
        _, note = _check("k7_135_147", dtype, 200, tb)
        assert "table-driven" in note and ("runtime hops" in note) == (tb is not None), (note, tb)


@pytest.mark.gpu
@pytest.mark.parametrize("tb", [None, 9, 37])
def test_soft_zero_tail_takes_the_float64_argmin(gpu, tb):
    """Twelve all-zero steps at the end (and the zero padding behind them): every state ties in the high dwords, the wave leaves the hot
    path for the float64 first-argmin and comes back to the join the walk's wait sits behind."""
    _, note = _check("k7_133_171", "soft", 200, tb, "zero_tail")
    assert ("runtime hops" in note) == (tb is not None) and ("64-slot ring" in note) == (tb == 37), note


@pytest.mark.gpu
@pytest.mark.parametrize("tb", [None, 9, 37])
def test_soft_nan_codewords_are_decoded_again(gpu, tb):
    got, _ = _check("k7_133_171", "soft", 200, tb, "nan")
    clean = np.setdiff1d(np.arange(B), [3, 70, 73, 129])
    assert np.array_equal(got[clean], _want("k7_133_171", "soft", 200, tb)[clean])   # untouched by their neighbours' NaNs


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", TYPES)
def test_repeated_decodes_agree(gpu, dtype):
    """Four decodes of one input at the default depth: a hop that overtook its ring word, or a ring write that overtook a read, would
    not come out the same four times."""
    first, note = _check("k7_133_171", dtype, 200, None)
    assert "runtime hops" not in note and "viterbi_cw_fused_kernel<6," in note, note
    for _ in range(3):
        again, _ = _decode(_rx("k7_133_171", dtype, 200), _trellis("k7_133_171"), None, dtype)
        assert np.array_equal(first, again)


@pytest.mark.gpu
def test_float32_flavour_hard_is_exact(gpu):
    """The float32 flavour ('fp32-fast') shares the walk.  'hard' metrics of 0 / 1 inputs are Hamming distances, exact in float32: the
    oracle's bits, at the default depth (compile-time hops) and below it (run-time hops, early stop)."""
    import commpy_amd
    for tb in (None, 9):
        with commpy_amd.precision("fp32-fast"):
            got, note = _decode(_rx("k7_133_171", "hard", 200), _trellis("k7_133_171"), tb, "hard")
        assert ",f32" in note and ("runtime hops" in note) == (tb is not None), note
        assert np.array_equal(got, _want("k7_133_171", "hard", 200, tb)), (tb, note)

