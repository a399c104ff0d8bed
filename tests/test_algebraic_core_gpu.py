"""bch_decode_kernel, rs_decode_kernel and bch_chase_kernel run one Berlekamp-Massey and one Chien search (csrc/cpx_gf.h): the three
decoders must agree wherever the codes do.

A binary word is also a word over GF(2^m), and the narrow-sense BCH code (n, t) is the subfield subcode of the Reed-Solomon code
(n, n - 2t), fcr = 1, over the same primitive polynomial: both decoders see the syndromes S_1 .. S_2t of the word, run Berlekamp-Massey
from f = 0 and search the same positions for roots, so they fail on the same words and find the same locator.  Forney's values are 1:
from S_2j = S_j^2 and L <= t the error values satisfy Y^2 = Y and Y != 0.  Hence rs_decode returns bch_decode's `errors` and `codeword`,
failures (-1, the word unchanged) and miscorrections included.  tests/bch_model.py and tests/rs_model.py agree on every word at these
shapes, so the premise holds without the kernels."""
import numpy as np
import pytest

import bch_model as BM
import rs_model as RM
from commpy_amd import _lib
from commpy_amd.channelcoding import BCHCode, RSCode, bch_decode, rs_decode
from test_chase_gpu import both, check

pytestmark = pytest.mark.gpu


def received(model, t, B, seed):
    """B code words of the BCH model with 0, 1, t - 1, t, t + 1 and t + 3 flipped bits, cycling over the words."""
    rs = np.random.RandomState(seed)
    words = BM.encode_batch(rs.randint(0, 2, (B, model.k)), model)
    for b, flips in zip(range(B), np.resize([0, 1, t - 1, t, t + 1, t + 3], B)):
        words[b, rs.choice(model.n, min(flips, model.n), replace=False)] ^= 1
    return words


# (7, 1, 3): least m, one chunk; (100, 5, 7): shortened, two chunks of a four-chunk group; (300, 4, 9): five chunks, a second group with
# one live chunk; t = 31: r = 62, rs_decode_kernel<64>, locators of up to 31 coefficients, primitive and shortened
@pytest.mark.parametrize("n, t, m, B", [(7, 1, 3, 300), (63, 3, 6, 300), (100, 5, 7, 300), (300, 4, 9, 300), (1023, 31, 10, 48), (700, 31, 10, 48)])
def test_rs_decode_equals_bch_decode_on_binary_words(gpu, n, t, m, B):
    bch, bch_model = both(n, t, m)
    rs, rs_model = RSCode(n, n - 2 * t, m=m, fcr=1), RM.Code(n, n - 2 * t, m, fcr=1)
    assert rs.prim_poly == bch.prim_poly
    words = received(bch_model, t, B, n + t)
    b_word, b_err = bch_decode(words, bch, want=("codeword", "errors"))
    assert _lib.last_kernel() == "bch_decode_kernel"
    r_word, r_err = rs_decode(words.astype(np.uint16), rs, want=("codeword", "errors"))
    assert _lib.last_kernel() == "rs_decode_kernel<%d>" % (8 if t <= 4 else 16 if t <= 8 else 64)
    assert np.array_equal(b_err, r_err) and np.array_equal(b_word, r_word)
    b_ref, r_ref = BM.decode_batch(words, bch_model), RM.decode_batch(words.astype(np.uint16), rs_model)
    assert np.array_equal(b_err, b_ref["errors"]) and np.array_equal(b_word, b_ref["codeword"])
    assert np.array_equal(r_err, r_ref["errors"]) and np.array_equal(r_word, r_ref["codeword"])
    assert (b_ref["errors"] == t).any()
    assert (b_ref["errors"] == -1).any() or (n, t) == (7, 1)      # the (7, 4) Hamming code is perfect: every word decodes


def test_chase_decision_equals_bch_decode_at_unit_reliabilities(gpu):
    """LLRs of magnitude 1 with the signs of the received bits make a candidate's metric its Hamming distance from the word.  Where
    bch_decode finds a code word it lies within t of the word, every other code word at t + 1 or more (d >= 2t + 1): it is the zero
    pattern's candidate and the decision, with no tie."""
    n, t, m, p = 63, 3, 6, 4
    code, model = both(n, t, m)
    words = received(model, t, 120, 5)
    b_word, b_err = bch_decode(words, code, want=("codeword", "errors"))
    ref = check(code, model, 1.0 - 2.0 * words, p)                # every output of bch_chase_kernel against tests/chase_model.py
    found = b_err >= 0
    assert found.any() and (~found).any() and np.array_equal(b_err, BM.decode_batch(words, model)["errors"])
    assert (ref["candidates"][found] >= 1).all() and np.array_equal(ref["codeword"][found], b_word[found])
