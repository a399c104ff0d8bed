"""The tail-biting codec on the GPU against tests/tbcc_model.py: every comparison is exact (``array_equal``; ``'metric'`` bit for bit),
for the encoder and the decoder, at 2 .. 64 states, n = 2 and 3, k = 2, a table-driven trellis, block lengths on both sides of a chunk
of S steps, batches on both sides of a wave's 64 / S code words and above the resident grid, the three decoding types and
max_wraps 1, 4 and 8."""
import ctypes
import itertools
import re

import numpy as np
import pytest

import tbcc_model as M
from commpy_amd import _lib, deviceops
from commpy_amd.channelcoding import Trellis, tailbiting_decode, tailbiting_encode
from commpy_amd.deviceops import DeviceBuf
from test_tbcc_host import bpsk_llr, code57, lte_code, outcome_classes

pytestmark = pytest.mark.gpu
EVERYTHING = ("bits", "wraps", "tailbiting", "metric")
COMPUTE_UNITS = 256                                               # of an MI355X: the grids below are sized from it
LENGTHS = (1, 2, 63, 64, 65, 130)
# three (decoding type, max_wraps) pairs per block length: every pair of the 3 x 3 occurs for every trellis
MODES = {1: (('hard', 1), ('soft', 4), ('unquantized', 8)), 2: (('hard', 4), ('soft', 8), ('unquantized', 1)),
         63: (('hard', 8), ('soft', 1), ('unquantized', 4)), 64: (('soft', 4), ('hard', 1), ('unquantized', 8)),
         65: (('soft', 8), ('unquantized', 1), ('hard', 4)), 130: (('unquantized', 4), ('soft', 1), ('hard', 8))}


def permuted57():
    """(5, 7) with its state labels permuted: no shift register any more, so the table-driven traceback decodes it."""
    base, p = code57(), np.array([2, 0, 3, 1])
    nxt, out = np.zeros((4, 2), int), np.zeros((4, 2), int)
    for s in range(4):
        nxt[p[s]], out[p[s]] = p[base.next_state_table[s]], base.output_table[s]
    return Trellis.from_tables(1, 2, 2, nxt, out)


TRELLISES = {
    "s2": lambda: Trellis(np.array([1]), np.array([[1, 3]])),
    "s4": code57,
    "s4_n3": lambda: Trellis(np.array([2]), np.array([[5, 7, 7]])),
    "s8": lambda: Trellis(np.array([3]), np.array([[0o13, 0o17]])),
    "s16": lambda: Trellis(np.array([4]), np.array([[0o25, 0o37]])),
    "s32": lambda: Trellis(np.array([5]), np.array([[0o65, 0o57]])),
    "s64": lambda: Trellis(np.array([6]), np.array([[0o133, 0o171]])),
    "s64_n3": lte_code,
    "s4_k2": lambda: Trellis(np.array([1, 1]), np.array([[3, 1, 2], [1, 3, 3]])),
    "s16_k2": lambda: Trellis(np.array([2, 2]), np.array([[7, 1, 4], [2, 5, 7]])),
    "s4_tables": permuted57,
}


def received(tr, T, B, dtype, seed, ebn0_db=1.0):
    """Noisy tail-biting words (rows that do not close for a short T are just as good an input), the second half pure noise."""
    rs = np.random.RandomState(seed)
    sent, _ = M.encode_batch(rs.randint(0, 2, (B, T * tr.k)), tr)
    sent[B // 2:] = rs.randint(0, 2, sent[B // 2:].shape)
    if dtype == 'hard':
        return (sent ^ (rs.rand(*sent.shape) < 0.08)).astype(float)
    if dtype == 'soft':
        return bpsk_llr(sent, ebn0_db, tr.k / tr.n, rs)
    return (2.0 * sent - 1.0) + 0.8 * rs.randn(*sent.shape)


def same(got, ref, what=None):
    """Every output against the model's, the metric by its bit pattern."""
    bits, wraps, tb, metric = got
    assert bits.dtype == np.uint8 and wraps.dtype == np.int32 and tb.dtype == np.uint8 and metric.dtype == np.float64
    assert np.array_equal(wraps, ref['wraps']), what
    assert np.array_equal(tb, ref['tailbiting']), what
    assert np.array_equal(bits, ref['bits']), what
    assert np.array_equal(np.isnan(metric), np.isnan(ref['metric'])), what
    ok = ~np.isnan(metric)
    assert np.array_equal(metric[ok].view(np.int64), ref['metric'][ok].view(np.int64)), what
    return ref


def check(rx, tr, dtype, max_wraps, what=None):
    return same(tailbiting_decode(rx, tr, dtype, max_wraps, want=EVERYTHING), M.decode_batch(rx, tr, dtype, max_wraps), what)


def resident_rows(tr):
    """Rows that the decoder's grid takes in one pass, from what the launcher reports: waves per workgroup, its LDS, and the
    workgroups it counts per compute unit (what LDS and 32 waves allow)."""
    waves, lds, per_cu = (int(v) for v in re.search(r"waves=(\d+) lds=(\d+) per_cu=(\d+)", _lib.last_kernel()).groups())
    assert per_cu == min(160 * 1024 // lds, 32 // waves)
    return 16 * COMPUTE_UNITS * per_cu * waves * (64 // tr.number_states)      # the grid is sixteen times what is resident


# ---- every trellis class, block length, batch size, decoding type and trip limit ----------------------------------------------------
@pytest.mark.parametrize("name", sorted(TRELLISES))
def test_decoder_equals_the_model(gpu, name):
    tr = TRELLISES[name]()
    S, G = tr.number_states, 64 // tr.number_states
    lg = S.bit_length() - 1
    sr = 1 if tr.k == 1 and name != "s4_tables" else 0            # a shift register: the kernel is compiled for its n = 2 or 3
    want_kernel = "tbcc_decode_kernel<%d,%d,%d,%d>" % (lg, 1 << tr.k, sr, tr.n if sr else 0)
    seen = set()
    for T in LENGTHS:
        for dtype, max_wraps in MODES[T]:
            rx = received(tr, T, G + 1 + 4, dtype, 1000 * T + max_wraps)
            ref = check(rx, tr, dtype, max_wraps, (name, T, dtype, max_wraps))
            assert _lib.last_kernel().startswith(want_kernel), _lib.last_kernel()
            for B in (1, G - 1, G + 1):                                # one row, a wave short of one row, a wave and one row
                got = tailbiting_decode(rx[:B], tr, dtype, max_wraps, want=EVERYTHING)
                assert got[0].shape == (B, T * tr.k) and got[3].shape == (B,)
                same(got, {key: v[:B] for key, v in ref.items()}, (name, T, dtype, max_wraps, B))
            seen.add((dtype, max_wraps))
    assert len(seen) == 9


@pytest.mark.parametrize("name", ["s4", "s64", "s16_k2"])
def test_batch_above_the_resident_grid(gpu, name):
    tr = TRELLISES[name]()
    T = 2
    base = received(tr, T, 96, 'soft', 5)
    ref = check(base, tr, 'soft', 4)
    B = resident_rows(tr) + 1
    assert B > 8192
    rx = np.resize(base, (B, base.shape[1]))
    got = tailbiting_decode(rx, tr, 'soft', 4, want=EVERYTHING)
    for g, key in zip(got, EVERYTHING):
        assert np.array_equal(g.view(np.int64) if key == 'metric' else g,
                              np.resize(ref[key], g.shape).view(np.int64) if key == 'metric' else np.resize(ref[key], g.shape)), key


# ---- 0 dB: every way to finish, side by side in one wave ----------------------------------------------------------------------------
@pytest.mark.parametrize("name, T, seed", [("s4", 10, 6), ("s64_n3", 40, 4)])
def test_every_outcome_at_0_db(gpu, name, T, seed):
    tr = TRELLISES[name]()
    rs = np.random.RandomState(seed)
    sent, closed = M.encode_batch(rs.randint(0, 2, (512, T)), tr)
    assert closed.all()
    rx = bpsk_llr(sent, 0.0, 1.0 / tr.n, rs)
    ref = check(rx, tr, 'soft', 4)
    assert all(outcome_classes(ref, 4).values()), outcome_classes(ref, 4)
    if name == "s4":                                                   # 16 rows share a wave: some wave holds all four classes
        waves = [{k2: v[i:i + 16] for k2, v in ref.items()} for i in range(0, 512, 16)]
        assert any(all(outcome_classes(w, 4).values()) for w in waves)
    same(tailbiting_decode(rx, tr, 'soft', 8, want=EVERYTHING), M.decode_batch(rx, tr, 'soft', 8))


# ---- exact ties ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["s2", "s4", "s64", "s64_n3", "s4_k2", "s4_tables"])
def test_exact_ties(gpu, name):
    tr = TRELLISES[name]()
    for T in (7, 64):
        for dtype in ('hard', 'soft', 'unquantized'):
            ref = check(np.zeros((3, T * tr.n)), tr, dtype, 4, (name, T, dtype))       # every candidate of every step ties
            assert (ref['wraps'] >= 1).all()
        rs = np.random.RandomState(T)
        sent, _ = M.encode_batch(rs.randint(0, 2, (70, T * tr.k)), tr)
        for p in (0.05, 0.25, 0.5):                                    # integer metrics: ties at every turn
            check((sent ^ (rs.rand(*sent.shape) < p)).astype(float), tr, 'hard', 4, (name, T, p))
        check(np.ones((2, T * tr.n)), tr, 'hard', 8)
        check(rs.randint(-2, 4, (20, T * tr.n)).astype(float) + 0.5 * rs.randint(0, 2, (20, T * tr.n)), tr, 'hard', 4)   # non-binary values


# ---- rejected rows ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["s4", "s64_n3"])
def test_rejected_rows_between_good_ones(gpu, name):
    tr = TRELLISES[name]()
    T = 24
    for dtype in ('hard', 'soft', 'unquantized'):
        rx = received(tr, T, 40, dtype, 9)
        clean = tailbiting_decode(rx, tr, dtype, 4, want=EVERYTHING)
        bad = rx.copy()
        bad[0, 0], bad[7, T * tr.n - 1], bad[17, 5], bad[18, 6], bad[39, 11] = np.nan, np.nan, np.inf, -np.inf, -np.nan
        ref = check(bad, tr, dtype, 4, (name, dtype))
        gone = [0, 7, 39] if dtype == 'soft' else [0, 7, 17, 18, 39]
        assert (ref['wraps'][gone] == 0).all() and (ref['tailbiting'][gone] == 0).all() and np.isnan(ref['metric'][gone]).all()
        assert not ref['bits'][gone].any()
        keep = np.setdiff1d(np.arange(40), [0, 7, 17, 18, 39])
        for c, r in zip(clean, EVERYTHING):                            # no other row's result changes
            assert np.array_equal(c[keep].view(np.int64) if r == 'metric' else c[keep],
                                  ref[r][keep].view(np.int64) if r == 'metric' else ref[r][keep]), (name, dtype, r)
        if dtype == 'soft':
            assert (ref['wraps'][[17, 18]] >= 1).all()                 # an infinite LLR is clipped to +-500


# ---- encoder ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(TRELLISES))
def test_encoder(gpu, name):
    tr = TRELLISES[name]()
    rs = np.random.RandomState(len(name))
    memory = max(1, int(tr.number_states).bit_length() - 1)
    for T in LENGTHS:
        for B in (1, 63, 65, 300):
            msg = rs.randint(0, 2, (B, T * tr.k)).astype(np.uint8)
            word, closed = M.encode_batch(msg, tr)
            d_x, d_closed = deviceops.tailbiting_encode_dev(tr, DeviceBuf.from_array(msg | (rs.randint(0, 128, msg.shape) << 1).astype(np.uint8)), B, T)
            _lib.check(_lib.load().cpx_stream_sync(None))
            assert _lib.last_kernel() == "tbcc_encode_kernel"
            assert np.array_equal(d_x.to_array((B, T * tr.n), np.uint8), word), (name, T, B)               # bit 0 of a byte counts
            assert np.array_equal(d_closed.to_array((B,), np.uint8), closed.astype(np.uint8)), (name, T, B)
            if closed.all():
                x = tailbiting_encode(msg, tr)
                assert x.dtype == np.uint8 and np.array_equal(x, word)
            else:
                assert T < memory
                with pytest.raises(ValueError, match="row %d does not tail-bite" % int(np.argmin(closed))):
                    tailbiting_encode(msg, tr)
        if T >= 63:
            assert np.array_equal(tailbiting_encode(msg[-1], tr), word[-1])                                 # the 1-D form
            bits, wraps, tb, metric = tailbiting_decode(2.0 * word - 1.0, tr, 'unquantized', want=EVERYTHING)   # and back
            assert np.array_equal(bits, msg) and (wraps == 1).all() and tb.all() and not metric.any()
            one = tailbiting_decode(word[-1].astype(float), tr, 'hard', want=EVERYTHING)
            assert np.array_equal(one[0], msg[-1]) and one[1] == 1 and one[2] == 1 and one[3] == 0.0


def test_encoder_refuses_a_recursive_trellis_and_wraps_the_grid(gpu):
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        rsc = Trellis(np.array([2]), np.array([[1, 7]]), 5, "rsc")
    msg = np.random.RandomState(0).randint(0, 2, (64, 12))
    assert not M.encode_batch(msg, rsc)[1].all()
    with pytest.raises(ValueError, match="does not tail-bite"):
        tailbiting_encode(msg, rsc)
    # a workgroup encodes 256 words, the grid holds at most 8 workgroups per compute unit: one word more than that
    tr = code57()
    every = np.array(list(itertools.product([0, 1], repeat=3)), dtype=np.uint8)
    B = 256 * 8 * COMPUTE_UNITS + 1
    assert np.array_equal(tailbiting_encode(np.resize(every, (B, 3)), tr), np.resize(M.encode_batch(every, tr)[0], (B, 6)))
    assert tailbiting_encode(np.zeros((0, 10), int), tr).shape == (0, 20)
    empty = tailbiting_decode(np.zeros((0, 20)), tr, want=EVERYTHING)
    assert [e.shape for e in empty] == [(0, 10), (0,), (0,), (0,)]


# ---- layout independence ------------------------------------------------------------------------------------------------------------
def equal(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int64) if a.dtype == np.float64 else a, b.view(np.int64) if b.dtype == np.float64 else b)


@pytest.mark.parametrize("name, T", [("s4", 33), ("s64_n3", 40), ("s4_k2", 20)])
def test_batch_size_position_and_requested_outputs_do_not_matter(gpu, name, T):
    tr = TRELLISES[name]()
    rx = received(tr, T, 259, 'soft', 3, ebn0_db=0.0)
    rx[100, 3] = np.nan
    full = tailbiting_decode(rx, tr, 'soft', 4, want=EVERYTHING)
    assert (full[1] == 1).any() and (full[1] == 4).any() and (full[1] == 0).sum() == 1
    for B in (1, 5, 64):
        part = tailbiting_decode(rx[:B], tr, 'soft', 4, want=EVERYTHING)
        assert all(equal(p, f[:B]) for p, f in zip(part, full))
    for i in (0, 100, 130, 258):
        alone = tailbiting_decode(rx[i], tr, 'soft', 4, want=EVERYTHING)
        assert np.array_equal(alone[0], full[0][i]) and alone[1] == full[1][i] and alone[2] == full[2][i]
        assert np.array([alone[3]]).view(np.int64) == full[3][i:i + 1].view(np.int64)
    moved = tailbiting_decode(rx[::-1], tr, 'soft', 4, want=EVERYTHING)
    assert all(equal(mv[::-1], f) for mv, f in zip(moved, full))
    for r in (1, 2, 3, 4):
        for want in itertools.combinations(EVERYTHING, r):
            for order in (want, want[::-1]):
                got = tailbiting_decode(rx, tr, 'soft', 4, want=order)
                got = (got,) if r == 1 else got
                assert len(got) == r
                for key, g in zip(want, got):
                    assert equal(g, full[EVERYTHING.index(key)]), order
    assert equal(tailbiting_decode(rx, tr, 'soft', 4, want="metric"), full[3])
    assert equal(tailbiting_decode(rx, tr, 'soft'), full[0])


def test_streams_and_device_buffers(gpu):
    tr = lte_code()
    lib = _lib.load()
    T, B = 40, 37
    rx = received(tr, T, B, 'soft', 4, ebn0_db=0.0)
    msg = np.random.RandomState(4).randint(0, 2, (B, T)).astype(np.uint8)
    host = tailbiting_decode(rx, tr, 'soft', 4, want=EVERYTHING)
    words = tailbiting_encode(msg, tr)
    shapes = ((B, T), np.uint8), ((B,), np.int32), ((B,), np.uint8), ((B,), np.float64)
    streams = [ctypes.c_void_p() for _ in range(2)]
    for s in streams:
        _lib.check(lib.cpx_stream_create(ctypes.byref(s)))
    try:
        d_msg, d_rx = DeviceBuf.from_array(msg), DeviceBuf.from_array(rx)
        outs = [(deviceops.tailbiting_encode_dev(tr, d_msg, B, T, stream=s),
                 deviceops.tailbiting_decode_dev(tr, d_rx, B, T, 'soft', 4, want=EVERYTHING, stream=s)) for s in streams + [None]]
        assert _lib.last_kernel().startswith("tbcc_decode_kernel<6,2,1,3>")
        for s in streams + [None]:
            _lib.check(lib.cpx_stream_sync(s))
        for (d_x, d_closed), decoded in outs:
            assert np.array_equal(d_x.to_array((B, T * 3), np.uint8), words) and d_closed.to_array((B,), np.uint8).all()
            for d, (shape, dtype), want in zip(decoded, shapes, host):
                assert equal(d.to_array(shape, dtype), want)
        d_m = deviceops.tailbiting_decode_dev(tr, d_rx, B, T, 'soft', 4, want="metric")
        d_w, d_b = deviceops.tailbiting_decode_dev(tr, d_rx, B, T, 'soft', 4, want=("wraps", "bits"))[::-1]
        _lib.check(lib.cpx_stream_sync(None))
        assert equal(d_m.to_array((B,), np.float64), host[3]) and equal(d_b.to_array((B, T), np.uint8), host[0])
        assert equal(d_w.to_array((B,), np.int32), host[1])
    finally:
        for s in streams:
            lib.cpx_stream_destroy(s)


@pytest.mark.parametrize("name, T", [("s64", 8192), ("s16_k2", 4096)])
def test_the_longest_block(gpu, name, T):
    """T k = 8192: 64 KiB of decision words, one wave per workgroup above the default LDS limit; one step more is refused."""
    tr = TRELLISES[name]()
    rx = received(tr, T, 2, 'hard', 8)
    check(rx, tr, 'hard', 2, name)
    assert "waves=1 " in _lib.last_kernel()
    with pytest.raises(ValueError, match="8192"):
        tailbiting_decode(np.zeros((1, (T + 1) * tr.n)), tr)
