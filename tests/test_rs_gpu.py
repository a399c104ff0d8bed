"""The Reed-Solomon codec on the GPU against tests/rs_model.py: every comparison is exact (``array_equal``), for the encoder and the
decoder, at the sizes where the kernels change their path -- fewer positions than lanes, one chunk and one position more, 8 / 16 / 32 /
64 remainder registers, r = 1 and r = 63, shortened codes, every table size class (4, 8 and 16 waves per workgroup), batches above the
resident grid."""
import ctypes
import itertools

import numpy as np
import pytest

import rs_model as M
from commpy_amd import _lib, deviceops
from commpy_amd.channelcoding import RSCode, rs_decode, rs_encode
from commpy_amd.deviceops import DeviceBuf
from test_rs_host import (BEYOND, SHORTENED, SHORTENED_SEED, beyond_pairs, boundary_pairs, noisy_words, shortened_region_failures)

pytestmark = pytest.mark.gpu
EVERYTHING = ("symbols", "codeword", "errors")
# (n, k, m, fcr)
SHAPES = [(7, 3, 3, 1), (15, 11, 4, 1), (63, 1, 6, 1), (64, 1, 7, 1), (65, 33, 7, 1), (100, 90, 7, 1), (255, 223, 8, 1), (204, 188, 8, 0),
          (255, 254, 8, 1), (544, 514, 10, 1), (300, 280, 14, 1)]
COMPUTE_UNITS = 256                                               # of an MI355X: the grids below are sized from it


def resident_words(m, n):
    """Words that rs_decode_kernel's grid decodes in one pass, as its launcher sizes it: 4 / 8 / 16 waves per workgroup by m, as many
    workgroups per compute unit as 160 KiB of LDS (tables 4 * 2^m bytes, 16 * ceil(n / 64) + 512 bytes per wave) and 32 waves allow."""
    waves = 4 if m <= 8 else 8 if m <= 11 else 16
    lds = (4 << m) + waves * (16 * ((n + 63) // 64) + 512)
    return waves, min(160 * 1024 // lds, 32 // waves) * COMPUTE_UNITS * waves


def regs(r):
    return 8 if r <= 8 else 16 if r <= 16 else 32 if r <= 32 else 64


def both(n, k, m, fcr=1, prim_poly=None):
    return RSCode(n, k, m=m, prim_poly=prim_poly, fcr=fcr), M.Code(n, k, m, prim_poly, fcr)


def check_decode(code, model, rx, flags=None):
    """Every output of the engine against the model, word by word; returns the model's results."""
    sym, word, errors = rs_decode(rx, code, erasures=flags, want=EVERYTHING)
    ref = M.decode_batch(rx, model, flags)
    what = (code.n, code.k, code.fcr)
    assert sym.dtype == np.uint16 and word.dtype == np.uint16 and errors.dtype == np.int32
    assert np.array_equal(errors, ref["errors"]), what
    assert np.array_equal(word, ref["codeword"]), what
    assert np.array_equal(sym, ref["symbols"]), what
    assert _lib.last_kernel() == "rs_decode_kernel<%d>" % regs(code.n - code.k)
    return ref


# ---- every word of a small code -----------------------------------------------------------------------------------------------------
def test_every_received_word_under_every_erasure_mask(gpu):
    """All 8^4 words of the (4, 2) code over GF(8) under each of the 16 masks; f = 3, 4 are the f > r failures."""
    code, model = both(4, 2, 3)
    words = np.array(list(itertools.product(range(8), repeat=4)), dtype=np.uint16)
    masks = np.array(list(itertools.product([0, 1], repeat=4)), dtype=bool)
    rx, flags = np.tile(words, (16, 1)), np.repeat(masks, len(words), axis=0)
    assert rx.shape == (65536, 4)
    ref = check_decode(code, model, rx, flags)
    f = flags.sum(axis=1)
    assert (ref["errors"][f > 2] == -1).all() and (ref["errors"][f <= 2] == -1).any()
    assert (ref["errors"] == 0).any() and (ref["errors"] == 1).any()
    # zero-valued erasure fills: decoded with S != 0, and a flagged position that kept its value
    dirty = M.syndromes(rx, model).any(axis=1)
    assert ((ref["errors"] >= 0) & dirty & (flags & (ref["codeword"] == rx)).any(axis=1)).any()


# ---- encoder ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, k, m, fcr", SHAPES)
def test_encoder(gpu, n, k, m, fcr):
    code, model = both(n, k, m, fcr)
    assert code.genpoly.tolist() == model.g
    rs = np.random.RandomState(n)
    for B in (1, 3, 67):
        msg = rs.randint(0, 1 << m, (B, k)).astype(np.uint16)
        msg[0] = (1 << m) - 1 if B > 1 else msg[0]                # the all-ones symbols
        x = rs_encode(msg, code)
        assert x.dtype == np.uint16 and x.shape == (B, n)
        assert np.array_equal(x, M.encode_batch(msg, model)), (n, k, B)
    assert _lib.last_kernel() == "rs_encode_kernel<%d>" % regs(n - k)
    assert np.array_equal(rs_encode(msg[-1], code), x[-1])        # the 1-D form
    assert not rs_encode(np.zeros(k, np.uint16), code).any()
    sym, errors = rs_decode(x, code, want=("symbols", "errors"))  # and back
    assert np.array_equal(sym, msg) and not errors.any()


def test_encoder_batch_larger_than_the_grid(gpu):
    """A wave encodes 64 words, a workgroup 256, the grid holds at most 8 workgroups per compute unit: one word more than that."""
    code, model = both(7, 3, 3)
    every = np.array(list(itertools.product(range(8), repeat=3)), dtype=np.uint16)
    B = 256 * 8 * COMPUTE_UNITS + 1
    msg = np.resize(every, (B, 3))
    assert np.array_equal(rs_encode(msg, code), np.resize(M.encode_batch(every, model), (B, 7)))


# ---- decoder: up to the budget ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, k, m, fcr", SHAPES)
def test_decoder_corrects_up_to_the_budget(gpu, n, k, m, fcr):
    """Every (e, f) with 2e + f in {r - 1, r}, and the clean word, mixed in one batch; the errors lie on unflagged positions."""
    pairs = boundary_pairs(n - k)
    code, model = both(n, k, m, fcr)
    _, sent, rx, flags, e = noisy_words(n, k, m, pairs, 100 * n + k, per=2, fcr=fcr)
    assert (0, 0) in pairs and (0, n - k) in pairs and ((n - k) // 2, (n - k) % 2) in pairs
    ref = check_decode(code, model, rx, flags)
    assert np.array_equal(ref["codeword"], sent) and np.array_equal(ref["errors"], e), (n, k)
    assert np.array_equal(rs_decode(rx, code, erasures=flags.astype(np.uint8)), sent[:, :k])


# ---- decoder: beyond the budget -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, k, m", sorted(BEYOND))
def test_failures_and_miscorrections(gpu, n, k, m):
    code, model = both(n, k, m)
    _, sent, rx, flags, _ = noisy_words(n, k, m, beyond_pairs(n - k), BEYOND[(n, k, m)], per=40)
    ref = check_decode(code, model, rx, flags)
    failed = ref["errors"] == -1
    wrong = ~failed & (ref["codeword"] != sent).any(axis=1)
    assert failed.sum() >= 10 and wrong.sum() >= 10, (failed.sum(), wrong.sum())


def test_root_in_the_shortened_region_is_a_failure(gpu):
    code, model = both(*SHORTENED)
    _, _, rx, flags, _ = noisy_words(*SHORTENED, [(3, 0), (2, 1)], SHORTENED_SEED, per=100)
    ref = check_decode(code, model, rx, flags)
    lost = shortened_region_failures(model, rx, flags)
    assert lost.sum() >= 1 and (ref["errors"][lost] == -1).all()


@pytest.mark.parametrize("n, k, m", [(15, 11, 4), (255, 223, 8), (300, 280, 14)])
def test_erasures_only_with_garbage_and_one_flag_too_many(gpu, n, k, m):
    """f = r: every flagged symbol is replaced by garbage and comes back; f = r + 1 fails whatever the word."""
    code, model = both(n, k, m)
    r = n - k
    rs = np.random.RandomState(n)
    sent = M.encode_batch(rs.randint(0, 1 << m, (24, k)), model)
    flags = M.flag_sets(rs, 24, n, [r] * 12 + [r + 1] * 12)
    flags[0, :r], flags[0, r:] = True, False                      # a burst at the head, one at the tail
    flags[1, -r:], flags[1, :-r] = True, False
    rx = np.where(flags, rs.randint(0, 1 << m, sent.shape), sent).astype(np.uint16)
    rx[12] = sent[12]                                             # a code word with r + 1 flags fails as well
    ref = check_decode(code, model, rx, flags)
    assert np.array_equal(ref["codeword"][:12], sent[:12]) and not ref["errors"][:12].any()
    assert (ref["errors"][12:] == -1).all() and np.array_equal(ref["codeword"][12:], rx[12:])


def test_bursts_at_every_bit_offset(gpu):
    """(255, 223): 8 (t - 1) + 1 consecutive flipped bits touch at most t symbols wherever they start."""
    code, model = both(255, 223, 8)
    rs = np.random.RandomState(7)
    sent = M.encode_batch(rs.randint(0, 256, (16, 223)), model)
    bits = np.unpackbits(sent.astype(np.uint8), axis=1)
    for b in range(16):
        start = 8 * int(rs.randint(0, 255 - 16)) + b % 8
        bits[b, start:start + 8 * 15 + 1] ^= 1
    rx = np.packbits(bits, axis=1).astype(np.uint16)
    ref = check_decode(code, model, rx)
    assert np.array_equal(ref["codeword"], sent) and (ref["errors"] == 16).all()


# ---- waves of one workgroup, the grid stride ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, k, m, waves, per_cu", [(31, 25, 5, 4, 8), (1023, 1003, 10, 8, 4), (300, 280, 14, 16, 2)])
def test_mixed_words_share_a_workgroup_and_the_grid_wraps(gpu, n, k, m, waves, per_cu):
    """Rows 0, 4, ... are code words, rows 1, 5, ... hold up to t errors, rows 2, 6, ... r erasures, rows 3, 7, ... t + 1 errors: the
    waves of one workgroup leave at different points.  The batch is one word more than waves x resident workgroups."""
    code, model = both(n, k, m)
    r, t = n - k, (n - k) // 2
    pairs = [(0, 0), (t, 0), (0, r), (t + 1, 0)] * 12 + [(0, 0), (1, r - 2), (0, r), (t + 1, 1)] * 12
    _, sent, rx, flags, _ = noisy_words(n, k, m, pairs, n)
    ref = M.decode_batch(rx, model, flags)
    assert (ref["errors"][0::4] == 0).all() and (ref["errors"][1::4] > 0).all() and (ref["errors"][2::4] == 0).all()
    assert (ref["errors"][3::4] == -1).sum() >= 12
    assert resident_words(m, n) == (waves, waves * per_cu * COMPUTE_UNITS)      # every size class of the launcher, and its grid
    B = waves * per_cu * COMPUTE_UNITS + 1
    sym, word, errors = rs_decode(np.resize(rx, (B, n)), code, erasures=np.resize(flags, (B, n)), want=EVERYTHING)
    assert np.array_equal(errors, np.resize(ref["errors"], B)) and np.array_equal(word, np.resize(ref["codeword"], (B, n)))
    assert np.array_equal(sym, np.resize(ref["symbols"], (B, k)))


# ---- layout independence --------------------------------------------------------------------------------------------------------------
def mixed_words(n, k, m, B, seed):
    """B received words and flags with 2e + f from 0 to r + 2."""
    r = n - k
    every = [(e, f) for f in range(r + 1) for e in range(r) if 2 * e + f <= r + 2]
    rs = np.random.RandomState(seed)
    pairs = [every[i] for i in rs.randint(0, len(every), B)]
    _, _, rx, flags, _ = noisy_words(n, k, m, pairs, seed)
    return rx, flags


def test_batch_size_position_and_requested_outputs_do_not_matter(gpu):
    code, _ = both(127, 119, 7)
    rx, flags = mixed_words(127, 119, 7, 257, 3)
    full = rs_decode(rx, code, erasures=flags, want=EVERYTHING)
    assert (full[2] == -1).any() and (full[2] == 4).any() and (full[2] == 0).any()
    for B in (1, 5):
        part = rs_decode(rx[:B], code, erasures=flags[:B], want=EVERYTHING)
        assert all(np.array_equal(p, f[:B]) for p, f in zip(part, full))
    for i in (0, 130, 256):
        alone = rs_decode(rx[i], code, erasures=flags[i], want=EVERYTHING)
        assert np.array_equal(alone[0], full[0][i]) and np.array_equal(alone[1], full[1][i]) and alone[2] == full[2][i]
    moved = rs_decode(rx[::-1], code, erasures=flags[::-1], want=EVERYTHING)
    assert all(np.array_equal(mv[::-1], f) for mv, f in zip(moved, full))
    for r in (1, 2, 3):
        for want in itertools.permutations(EVERYTHING, r):
            got = rs_decode(rx, code, erasures=flags, want=want)
            got = (got,) if r == 1 else got
            assert len(got) == r
            for name, g in zip([w for w in EVERYTHING if w in want], got):
                assert np.array_equal(g, full[EVERYTHING.index(name)]), want
    assert np.array_equal(rs_decode(rx, code, erasures=flags, want="errors"), full[2])
    # no flag array and an all-zero one
    none = rs_decode(rx, code, want=EVERYTHING)
    zero = rs_decode(rx, code, erasures=np.zeros(rx.shape, np.int64), want=EVERYTHING)
    assert all(np.array_equal(a, b) for a, b in zip(none, zero)) and (none[2] > 0).any()


def test_streams_and_device_buffers(gpu):
    code, _ = both(255, 247, 8)
    lib = _lib.load()
    rx, flags = mixed_words(255, 247, 8, 37, 4)
    flags8 = flags.astype(np.uint8) * 7                           # any non-zero byte is a flag
    msg = np.random.RandomState(4).randint(0, 256, (37, code.k)).astype(np.uint16)
    host = rs_decode(rx, code, erasures=flags, want=EVERYTHING)
    bare = rs_decode(rx, code, want=EVERYTHING)
    words = rs_encode(msg, code)
    streams = [ctypes.c_void_p() for _ in range(2)]
    for s in streams:
        _lib.check(lib.cpx_stream_create(ctypes.byref(s)))
    try:
        d_msg, d_rx, d_fl = DeviceBuf.from_array(msg), DeviceBuf.from_array(rx), DeviceBuf.from_array(flags8)
        outs = [(deviceops.rs_encode_dev(code, d_msg, 37, stream=s), deviceops.rs_decode_dev(code, d_rx, 37, d_fl, want=EVERYTHING, stream=s),
                 deviceops.rs_decode_dev(code, d_rx, 37, want=EVERYTHING, stream=s)) for s in streams + [None]]
        assert _lib.last_kernel() == "rs_decode_kernel<8>"
        for s in streams + [None]:
            _lib.check(lib.cpx_stream_sync(s))
        for d_x, flagged, plain in outs:
            assert np.array_equal(d_x.to_array((37, 255), np.uint16), words)
            for (d_sym, d_word, d_err), want in ((flagged, host), (plain, bare)):
                assert np.array_equal(d_sym.to_array((37, code.k), np.uint16), want[0])
                assert np.array_equal(d_word.to_array((37, 255), np.uint16), want[1])
                assert np.array_equal(d_err.to_array((37,), np.int32), want[2])
        d_e = deviceops.rs_decode_dev(code, d_rx, 37, d_fl, want="errors")
        d_w, d_s = deviceops.rs_decode_dev(code, d_rx, 37, d_fl, want=("codeword", "symbols"))[::-1]
        _lib.check(lib.cpx_stream_sync(None))
        assert np.array_equal(d_e.to_array((37,), np.int32), host[2]) and np.array_equal(d_s.to_array((37, code.k), np.uint16), host[0])
        assert np.array_equal(d_w.to_array((37, 255), np.uint16), host[1])
    finally:
        for s in streams:
            lib.cpx_stream_destroy(s)


@pytest.mark.parametrize("n, k, m", [(7, 3, 3), (544, 514, 10)])
def test_bits_above_the_symbol_width_do_not_count(gpu, n, k, m):
    """A device buffer with random bits set above bit m - 1 encodes and decodes exactly like the masked buffer.  This is the result
    of masking: rs_decode_kernel ANDs every symbol with 2^m - 1 as it arrives from global memory, in the syndrome pass and again in
    the output pass, and rs_encode_kernel does so before a message symbol goes to the output and to the LDS tile; no symbol reaches
    a table index (gf.lg[...]) unmasked."""
    code, _ = both(n, k, m)
    rx, flags = mixed_words(n, k, m, 40, n)
    rs = np.random.RandomState(m)
    msg = rs.randint(0, 1 << m, (40, k)).astype(np.uint16)
    high = lambda a: (a | (rs.randint(0, 1 << (16 - m), a.shape) << m)).astype(np.uint16)
    loud_rx, loud_msg = high(rx), high(msg)
    assert loud_rx.max() >= 1 << m and np.array_equal(loud_rx & ((1 << m) - 1), rx) and (loud_msg != msg).any()
    host = rs_decode(rx, code, erasures=flags, want=EVERYTHING)
    assert (host[2] > 0).any() and (host[2] == -1).any()
    d_fl = DeviceBuf.from_array(flags.astype(np.uint8))
    d_sym, d_word, d_err = deviceops.rs_decode_dev(code, DeviceBuf.from_array(loud_rx), 40, d_fl, want=EVERYTHING)
    d_x = deviceops.rs_encode_dev(code, DeviceBuf.from_array(loud_msg), 40)
    _lib.check(_lib.load().cpx_stream_sync(None))
    assert np.array_equal(d_sym.to_array((40, k), np.uint16), host[0]) and np.array_equal(d_word.to_array((40, n), np.uint16), host[1])
    assert np.array_equal(d_err.to_array((40,), np.int32), host[2])
    assert np.array_equal(d_x.to_array((40, n), np.uint16), rs_encode(msg, code))
