"""The BCH codec on the GPU against tests/bch_model.py: every comparison is exact (``array_equal``), for the encoder and the decoder, at
the sizes where the kernels change their path -- fewer positions than lanes, one chunk and one position more, remainders of one to three
64-bit words, shortened codes, every table size class (4, 8 and 16 waves per workgroup), batches above the resident grid."""
import ctypes
import itertools

import numpy as np
import pytest

import bch_model as M
from commpy_amd import _lib, deviceops
from commpy_amd.channelcoding import BCHCode, bch_decode, bch_encode
from commpy_amd.deviceops import DeviceBuf
from test_bch_host import BEYOND_T, DVB_PRIM_POLY, SHORTENED, SHORTENED_SEED, noisy_words, shortened_region_failures

pytestmark = pytest.mark.gpu
EVERYTHING = ("bits", "codeword", "errors")
# (n, t, m, prim_poly)
SHAPES = [(7, 1, 3, None), (15, 2, 4, None), (63, 2, 6, None), (127, 2, 7, None), (255, 18, 8, None), (1023, 10, 10, None), (64, 2, 7, None),
          (65, 2, 7, None), (100, 2, 7, None), (300, 12, 14, DVB_PRIM_POLY), (16383, 12, 14, None)]
COMPUTE_UNITS = 256                                               # of an MI355X: the grids below are sized from it


def both(n, t, m, prim_poly=None):
    return BCHCode(n, t, m=m, prim_poly=prim_poly), M.Code(n, t, m, prim_poly)


def check_decode(code, model, rx):
    """Every output of the engine against the model, word by word; returns the model's results."""
    bits, word, errors = bch_decode(rx, code, want=EVERYTHING)
    ref = M.decode_batch(rx, model)
    what = (code.n, code.k, code.t)
    assert bits.dtype == np.uint8 and word.dtype == np.uint8 and errors.dtype == np.int32
    assert np.array_equal(errors, ref["errors"]), what
    assert np.array_equal(word, ref["codeword"]), what
    assert np.array_equal(bits, ref["bits"]), what
    assert _lib.last_kernel() == "bch_decode_kernel"
    return ref


# ---- every word of two small codes -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", [2, 3])
def test_every_received_word(gpu, t):
    code, model = both(15, t, 4)
    words = ((np.arange(2 ** 15)[:, None] >> np.arange(14, -1, -1)) & 1).astype(np.uint8)
    ref = check_decode(code, model, words)
    assert (ref["errors"] == -1).any() and all((ref["errors"] == e).any() for e in range(t + 1))


# ---- encoder ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, t, m, prim_poly", SHAPES)
def test_encoder(gpu, n, t, m, prim_poly):
    code, model = both(n, t, m, prim_poly)
    assert (code.k, code.genpoly) == (model.k, model.g)
    rs = np.random.RandomState(n)
    for B in ((2,) if n == 16383 else (1, 3, 67)):
        msg = rs.randint(0, 2, (B, code.k)).astype(np.uint8)
        msg[0] = 1 if B > 1 else msg[0]                            # the all-ones message
        x = bch_encode(msg, code)
        assert x.dtype == np.uint8 and x.shape == (B, n)
        assert np.array_equal(x, M.encode_batch(msg, model)), (n, t, B)
    assert _lib.last_kernel() == "bch_encode_kernel<%d>" % ((n - code.k + 63) // 64)
    assert np.array_equal(bch_encode(msg[-1], code), x[-1])       # the 1-D form
    assert not bch_encode(np.zeros(code.k, np.uint8), code).any()


def test_encoder_batch_larger_than_the_grid(gpu):
    """A wave encodes 64 words, a workgroup 256, the grid holds 8 workgroups per compute unit: one word more than that."""
    code, model = both(7, 1, 3)
    every = np.array(list(itertools.product([0, 1], repeat=4)), dtype=np.uint8)
    B = 256 * 8 * COMPUTE_UNITS + 1
    msg = np.resize(every, (B, 4))
    assert np.array_equal(bch_encode(msg, code), np.resize(M.encode_batch(every, model), (B, 7)))


# ---- decoder: up to t errors --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, t, m, prim_poly", SHAPES)
def test_decoder_corrects_up_to_t_errors(gpu, n, t, m, prim_poly):
    code, model = both(n, t, m, prim_poly)
    B = 4 if n == 16383 else 16
    for e in sorted({0, 1, t - 1, t}):
        _, sent, rx, pos = noisy_words(n, t, m, e, 100 * n + e, B, prim_poly)
        if e:                                                     # the cases every set holds
            assert 0 in pos[0] and n - 1 in pos[1] and all(len(p) == e for p in pos)
            assert min(pos[2]) >= code.k or n - code.k < e
            assert max(pos[3]) < code.k or code.k < e
        ref = check_decode(code, model, rx)
        assert np.array_equal(ref["errors"], np.full(B, e)) and np.array_equal(ref["codeword"], sent), (n, t, e)
        assert np.array_equal(bch_decode(rx, code), sent[:, :code.k])


# ---- decoder: beyond t --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, t, m", sorted(BEYOND_T))
def test_failures_and_miscorrections(gpu, n, t, m):
    code, model = both(n, t, m)
    for e in (t + 1, 2 * t):
        _, sent, rx, _ = noisy_words(n, t, m, e, BEYOND_T[(n, t, m)])
        ref = check_decode(code, model, rx)
        failed = ref["errors"] == -1
        wrong = ~failed & (ref["codeword"] != sent).any(axis=1)
        assert failed.sum() >= 10 and wrong.sum() >= 10, (e, failed.sum(), wrong.sum())


def test_root_in_the_shortened_region_is_a_failure(gpu):
    code, model = both(*SHORTENED)
    for e in (3, 4):
        _, _, rx, _ = noisy_words(*SHORTENED, e, SHORTENED_SEED)
        ref = check_decode(code, model, rx)
        if e == 3:
            lost = shortened_region_failures(model, rx)
            assert lost.sum() >= 1 and (ref["errors"][lost] == -1).all()


@pytest.mark.parametrize("n, t, m, prim_poly", [(31, 2, 5, None), (1023, 10, 10, None), (3240, 12, 14, DVB_PRIM_POLY)])
def test_clean_correctable_and_failing_words_share_a_workgroup(gpu, n, t, m, prim_poly):
    """Rows 0, 3, 6, ... are code words, rows 1, 4, ... hold up to t errors, rows 2, 5, ... 2t + 1: waves of one workgroup leave at
    different points."""
    code, model = both(n, t, m, prim_poly)
    B = 48 if n < 2000 else 18
    rs = np.random.RandomState(n)
    sent = M.encode_batch(rs.randint(0, 2, (B, model.k)), model)
    pos = [[] if b % 3 == 0 else sorted(rs.choice(n, 1 + b % t if b % 3 == 1 else 2 * t + 1, replace=False)) for b in range(B)]
    rx = M.with_errors(sent, pos)
    ref = check_decode(code, model, rx)
    # about half of the words of (31, 21) lie within distance t of a code word, so about half of the rows with 2t + 1 errors are
    # miscorrected instead of failing; two failures are enough for the mix this test is about
    assert (ref["errors"][0::3] == 0).all() and (ref["errors"][1::3] > 0).all() and (ref["errors"][2::3] == -1).sum() >= 2


def test_batch_larger_than_the_resident_grid(gpu):
    """(15, 7): 4 words per workgroup, 8 workgroups per compute unit: one word more than the grid decodes in one pass."""
    code, model = both(15, 2, 4)
    _, _, rx, _ = noisy_words(15, 2, 4, 3, 5, 63)
    rx[::7] = M.encode_batch(np.random.RandomState(1).randint(0, 2, (9, 7)), model)
    ref = M.decode_batch(rx, model)
    B = 4 * 8 * COMPUTE_UNITS + 1
    bits, word, errors = bch_decode(np.resize(rx, (B, 15)), code, want=EVERYTHING)
    assert np.array_equal(errors, np.resize(ref["errors"], B)) and np.array_equal(word, np.resize(ref["codeword"], (B, 15)))
    assert np.array_equal(bits, np.resize(ref["bits"], (B, 7)))


# ---- layout independence --------------------------------------------------------------------------------------------------------------
def mixed_words(n, t, m, B, seed):
    """B received words with 0 .. 2t errors."""
    model = M.Code(n, t, m)
    rs = np.random.RandomState(seed)
    sent = M.encode_batch(rs.randint(0, 2, (B, model.k)), model)
    return M.with_errors(sent, [sorted(rs.choice(n, b % (2 * t + 1), replace=False)) for b in range(B)])


def test_batch_size_position_and_requested_outputs_do_not_matter(gpu):
    code, _ = both(127, 4, 7)
    rx = mixed_words(127, 4, 7, 257, 3)
    full = bch_decode(rx, code, want=EVERYTHING)
    assert (full[2] == -1).any() and (full[2] == 4).any() and (full[2] == 0).any()
    for B in (1, 5):
        part = bch_decode(rx[:B], code, want=EVERYTHING)
        assert all(np.array_equal(p, f[:B]) for p, f in zip(part, full))
    for i in (0, 130, 256):
        alone = bch_decode(rx[i], code, want=EVERYTHING)
        assert np.array_equal(alone[0], full[0][i]) and np.array_equal(alone[1], full[1][i]) and alone[2] == full[2][i]
    moved = bch_decode(rx[::-1], code, want=EVERYTHING)
    assert all(np.array_equal(mv[::-1], f) for mv, f in zip(moved, full))
    for r in (1, 2, 3):
        for want in itertools.permutations(EVERYTHING, r):
            got = bch_decode(rx, code, want=want)
            got = (got,) if r == 1 else got
            assert len(got) == r
            for name, g in zip([w for w in EVERYTHING if w in want], got):
                assert np.array_equal(g, full[EVERYTHING.index(name)]), want
    assert np.array_equal(bch_decode(rx, code, want="errors"), full[2])


def test_streams_device_buffers_and_nonzero_bytes(gpu):
    code, _ = both(255, 4, 8)
    lib = _lib.load()
    rx = mixed_words(255, 4, 8, 37, 4)
    msg = np.random.RandomState(4).randint(0, 2, (37, code.k)).astype(np.uint8)
    host = bch_decode(rx, code, want=EVERYTHING)
    words = bch_encode(msg, code)
    loud = (rx * np.random.RandomState(5).randint(1, 256, rx.shape)).astype(np.uint8)        # any non-zero byte is a one
    assert loud.max() > 1 and np.array_equal(loud != 0, rx != 0)
    streams = [ctypes.c_void_p() for _ in range(2)]
    for s in streams:
        _lib.check(lib.cpx_stream_create(ctypes.byref(s)))
    try:
        d_msg, d_rx, d_loud = DeviceBuf.from_array(msg), DeviceBuf.from_array(rx), DeviceBuf.from_array(loud)
        outs = [(deviceops.bch_encode_dev(code, d_msg, 37, stream=s), deviceops.bch_decode_dev(code, d_rx, 37, want=EVERYTHING, stream=s),
                 deviceops.bch_decode_dev(code, d_loud, 37, want=EVERYTHING, stream=s)) for s in streams + [None]]
        assert _lib.last_kernel() == "bch_decode_kernel"
        for s in streams + [None]:
            _lib.check(lib.cpx_stream_sync(s))
        for d_x, plain, noisy in outs:
            assert np.array_equal(d_x.to_array((37, 255), np.uint8), words)
            for d_bits, d_word, d_err in (plain, noisy):
                assert np.array_equal(d_bits.to_array((37, code.k), np.uint8), host[0])
                assert np.array_equal(d_word.to_array((37, 255), np.uint8), host[1])
                assert np.array_equal(d_err.to_array((37,), np.int32), host[2])
        d_e = deviceops.bch_decode_dev(code, d_loud, 37, want="errors")
        d_w, d_b = deviceops.bch_decode_dev(code, d_rx, 37, want=("codeword", "bits"))[::-1]
        _lib.check(lib.cpx_stream_sync(None))
        assert np.array_equal(d_e.to_array((37,), np.int32), host[2]) and np.array_equal(d_b.to_array((37, code.k), np.uint8), host[0])
        assert np.array_equal(d_w.to_array((37, 255), np.uint8), host[1])
    finally:
        for s in streams:
            lib.cpx_stream_destroy(s)


def test_encode_then_decode_round_trip(gpu):
    code, _ = both(3240, 12, 14, DVB_PRIM_POLY)
    rs = np.random.RandomState(6)
    msg = rs.randint(0, 2, (5, code.k)).astype(np.uint8)
    x = bch_encode(msg, code)
    for b in range(5):
        x[b, rs.choice(3240, 3 * b, replace=False)] ^= 1
    bits, errors = bch_decode(x, code, want=("bits", "errors"))
    assert np.array_equal(bits, msg) and errors.tolist() == [0, 3, 6, 9, 12]
