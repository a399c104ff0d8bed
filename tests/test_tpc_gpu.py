"""Turbo product codes on the GPU against tests/tpc_model.py: the encoder, the iterative decoder bit for bit (floats by bit pattern), a
block with a NaN, noise-free blocks, and one seeded check that iterating gains over hard-decision decoding."""
import numpy as np
import pytest

import bch_model as M
import chase_model as CM
import tpc_model as TM
from commpy_amd import _lib, deviceops
from commpy_amd.channelcoding import BCHCode, ProductCode, bch_decode, chase_decode, tpc_decode, tpc_encode
from commpy_amd.deviceops import DeviceBuf

pytestmark = pytest.mark.gpu
EVERYTHING = ("bits", "codeword", "extrinsic")
# the behavioural check: (31, 26) x (31, 26) over BPSK and AWGN
EBN0_DB, BLOCKS, SEED = 3.0, 24, 2024


def same(got, ref):
    got, ref = np.asarray(got), np.asarray(ref)
    if got.dtype != ref.dtype or got.shape != ref.shape:
        return False
    return np.array_equal(got.view(np.int64), ref.view(np.int64)) if got.dtype == np.float64 else np.array_equal(got, ref)


def product(row, col):
    """((n, t, m) of the row code, of the column code) -> the engine's code and the two models."""
    return ProductCode(BCHCode(row[0], row[1], m=row[2]), BCHCode(col[0], col[1], m=col[2])), M.Code(*row), M.Code(*col)


def channel(code, B, ebn0_db, seed):
    """(messages, code words, LLRs 2 y / sigma^2, sigma) of B seeded blocks over BPSK and AWGN."""
    rs = np.random.RandomState(seed)
    msg = rs.randint(0, 2, (B, code.k_c, code.k_r)).astype(np.uint8)
    x = tpc_encode(msg, code)
    sigma = np.sqrt(1.0 / (2.0 * (code.k / code.n) * 10.0 ** (ebn0_db / 10.0)))
    return msg, x, 2.0 * (1.0 - 2.0 * x + sigma * rs.randn(*x.shape)) / sigma ** 2, sigma


def test_encoder(gpu):
    code, row, col = product((15, 1, 4), (7, 1, 3))
    msg = np.random.RandomState(1).randint(0, 2, (5, 4, 11)).astype(np.uint8)
    x = tpc_encode(msg, code)
    assert x.dtype == np.uint8 and same(x, TM.encode(msg, row, col)) and same(x[:, :4, :11], msg)
    assert not M.syndromes(CM.words_of(x, 2), row).any() and not M.syndromes(CM.words_of(x, 1), col).any()
    assert same(tpc_encode(msg[2], code), x[2])


@pytest.mark.parametrize("row, col, iters, p, B", [((15, 1, 4), (7, 1, 3), 2, 4, 5), ((31, 2, 5), (31, 1, 5), 2, 3, 2)])
def test_decoder_equals_the_model(gpu, row, col, iters, p, B):
    """[n_c, n_r] = [7, 15] of (7, 4) columns and (15, 11) rows; [31, 31] of (31, 26) columns and (31, 21, t = 2) rows."""
    code, rm, cm = product(row, col)
    _, _, llr, sigma = channel(code, B, 2.5, 7)
    scale = 2.0 / sigma ** 2
    ref = TM.decode(llr, rm, cm, iters, p, llr_scale=scale)
    got = tpc_decode(llr, code, iters, p, llr_scale=scale, want=EVERYTHING)
    assert _lib.last_kernel() == "bch_chase_kernel"
    assert all(same(g, ref[name]) for name, g in zip(EVERYTHING, got))
    assert ref["extrinsic"].any() and same(got[0], got[1][:, :code.k_c, :code.k_r])
    # one block alone, a single result, explicit tables, and the device form
    assert same(tpc_decode(llr[B - 1], code, iters, p, llr_scale=scale), ref["bits"][B - 1])
    tables = TM.decode(llr, rm, cm, iters, p, alpha=[0.5], beta=[0.3, 0.6])
    assert same(tpc_decode(llr, code, iters, p, alpha=0.5, beta=[0.3, 0.6], want="extrinsic"), tables["extrinsic"])
    d_word, d_ext = deviceops.tpc_decode_dev(code, DeviceBuf.from_array(llr), B, iters, p, llr_scale=scale, want=("extrinsic", "codeword"))
    _lib.check(_lib.load().cpx_stream_sync(None))
    assert same(d_word.to_array(llr.shape, np.uint8), ref["codeword"]) and same(d_ext.to_array(llr.shape, np.float64), ref["extrinsic"])
    # one name alone: a bare buffer, equal to the host flavour's result
    for name, dtype in (("codeword", np.uint8), ("extrinsic", np.float64)):
        d_one = deviceops.tpc_decode_dev(code, DeviceBuf.from_array(llr), B, iters, p, llr_scale=scale, want=name)
        _lib.check(_lib.load().cpx_stream_sync(None))
        assert isinstance(d_one, DeviceBuf) and same(d_one.to_array(llr.shape, dtype), got[EVERYTHING.index(name)])


def test_a_nan_costs_its_row_and_its_column_only(gpu):
    code, rm, cm = product((15, 1, 4), (7, 1, 3))
    msg, x, llr, _ = channel(code, 3, 6.0, 11)
    llr[1, 2, 5] = np.nan
    ref = TM.decode(llr, rm, cm, 2, 3)
    got = tpc_decode(llr, code, 2, 3, want=EVERYTHING)
    assert all(same(g, ref[name]) for name, g in zip(EVERYTHING, got))
    # the last half-iteration runs along the columns: column 5 of block 1 is rejected (extrinsic 0, NaN as bit 0), the rest decodes
    assert not got[2][1, :, 5].any() and got[1][1, 2, 5] == 0 and got[2][1, :, 4].all()
    keep = np.ones(x.shape, bool)
    keep[1, :, 5] = False
    assert same(got[1][keep], x[keep])


def test_noise_free_blocks_return_the_message(gpu):
    for row, col in (((15, 1, 4), (7, 1, 3)), ((63, 2, 6), (31, 1, 5))):
        code, _, _ = product(row, col)
        msg = np.random.RandomState(3).randint(0, 2, (4, code.k_c, code.k_r)).astype(np.uint8)
        x = tpc_encode(msg, code)
        bits, word = tpc_decode(4.0 * (1.0 - 2.0 * x), code, iters=1, want=("bits", "codeword"))
        assert same(bits, msg) and same(word, x)


def test_iterating_beats_hard_decisions(gpu):
    """(31, 26) x (31, 26) at Eb/N0 = 3 dB, 24 seeded blocks.  Message-bit errors after four iterations against one pass of bch_decode
    over the rows of the same hard decisions, and word errors of chase_decode (p = 4) against bch_decode on the rows as flat words.
    Only the comparisons are asserted; the counts are in DESIGN.md (section 4.22)."""
    code, rm, _ = product((31, 1, 5), (31, 1, 5))
    msg, x, llr, sigma = channel(code, BLOCKS, EBN0_DB, SEED)
    rows, sent = llr.reshape(-1, 31), x.reshape(-1, 31)
    hard_words = bch_decode((rows < 0).astype(np.uint8), code.row_code, want="codeword")
    hard_bits = int((hard_words.reshape(x.shape)[:, :26, :26] != msg).sum())
    soft_bits = int((tpc_decode(llr, code, 4, 4, llr_scale=2.0 / sigma ** 2) != msg).sum())
    chase_words = chase_decode(rows, code.row_code, 4, 0.5, want="codeword")
    hard_word_errors, chase_word_errors = int((hard_words != sent).any(axis=1).sum()), int((chase_words != sent).any(axis=1).sum())
    print("tpc (31,26)^2 at %.1f dB, %d blocks: bit errors hard %d, iterated %d; row word errors hard %d, chase %d"
          % (EBN0_DB, BLOCKS, hard_bits, soft_bits, hard_word_errors, chase_word_errors))
    assert hard_bits > 0 and soft_bits < hard_bits
    assert chase_word_errors <= hard_word_errors
