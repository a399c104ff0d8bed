"""Host side of the Chase-II / turbo-product-code work: the NumPy models (tests/chase_model.py, tests/tpc_model.py) against brute force
and a deliberately naive second implementation; the C-ABI's names; every refusal (ValueError before the library is touched) and the
loud failure without a device."""
import itertools
import os
import re

import numpy as np
import pytest

import bch_model as M
import chase_model as CM
import tpc_model as TM
from commpy_amd import _lib, channelcoding, deviceops
from commpy_amd.channelcoding import BCHCode, ProductCode, chase_decode, tpc_decode, tpc_encode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["cpx_chase_bch", "cpx_chase_bch_dev"]
SMALL = [(7, 1, 3), (15, 2, 4), (15, 3, 4)]


def bits_equal(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.int64), np.asarray(b, dtype=np.float64).view(np.int64))


def soft_words(n, B, seed, kind):
    """B words of n LLRs: 'random' floats, or 'integer' values in -3 .. 3 (exact ties in reliabilities and in metrics)."""
    rs = np.random.RandomState(seed)
    if kind == "integer":
        return rs.randint(-3, 4, (B, n)).astype(np.float64)
    return 2.0 * rs.randn(B, n)


def all_codewords(code):
    return M.encode_batch(np.array(list(itertools.product([0, 1], repeat=code.k)), dtype=np.uint8), code)


def naive_word(x, cws, t, p, beta):
    """The rule in plain Python loops, with the candidates from an exhaustive search of the code words within distance t."""
    n = len(x)
    h = [1 if v < 0 else 0 for v in x]
    r = [abs(float(v)) for v in x]
    lrp = [i for _, i in sorted((r[i], i) for i in range(n))[:p]]
    cands = []
    for tau in range(1 << p):
        word = list(h)
        for j, pos in enumerate(lrp):
            if (tau >> j) & 1:
                word[pos] ^= 1
        near = [c for c in cws if sum(int(a) != b for a, b in zip(c, word)) <= t]
        assert len(near) <= 1
        if near:
            metric = 0.0
            for i in range(n):
                if int(near[0][i]) != h[i]:
                    metric = metric + r[i]
            cands.append((tau, [int(b) for b in near[0]], metric))
    if not cands:
        return h, [0.0] * n, float("inf"), 0, cands
    best = min(cands, key=lambda c: (c[2], c[0]))
    ext = []
    for i in range(n):
        s = 1.0 if best[1][i] == 0 else -1.0
        rivals = [c[2] for c in cands if c[1][i] != best[1][i]]
        ext.append(s * (min(rivals) - best[2]) - float(x[i]) if rivals else s * beta)
    return best[1], ext, best[2], len(cands), cands


# ---- the model ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["random", "integer"])
@pytest.mark.parametrize("n, t, m", SMALL)
def test_model_against_brute_force(n, t, m, kind):
    code = M.Code(n, t, m)
    cws = all_codewords(code)
    some_failed = False
    for p in (1, 2, 4, 5):
        x = soft_words(n, 12, 10 * n + p, kind)
        got = CM.decode_batch(x, code, p, 0.5)
        for b in range(len(x)):
            word, ext, metric, count, cands = naive_word(x[b], cws, t, p, 0.5)
            _, model_cands = CM.candidates(x[b], code, p)
            assert [(c[0], c[1].tolist()) for c in model_cands] == [(c[0], c[1]) for c in cands], (p, b)
            assert bits_equal([c[2] for c in model_cands], [c[2] for c in cands])
            assert got["candidates"][b] == count and got["codeword"][b].tolist() == word, (p, b)
            assert bits_equal(got["metric"][b], metric) and bits_equal(got["extrinsic"][b], ext), (p, b)
            some_failed |= count < (1 << p)
        assert np.array_equal(got["bits"], got["codeword"][:, :code.k])
    assert some_failed or (n, t) == (7, 1)                        # a perfect code decodes every test word


def test_integer_llrs_hold_ties():
    """The integer sets are there for ties: equal reliabilities at the selection boundary, and equal metrics of different code words."""
    code = M.Code(15, 2, 4)
    x = soft_words(15, 12, 154, "integer")
    boundary = metric_ties = 0
    for row in x:
        r = np.sort(np.abs(row))
        boundary += r[3] == r[4]
        _, cands = CM.candidates(row, code, 4)
        by_word = {tuple(c[1]): c[2] for c in cands}
        metric_ties += len(set(by_word.values())) < len(by_word)
    assert boundary >= 3 and metric_ties >= 3


def test_perfect_code_with_every_position_is_max_log_map():
    """(7, 4), p = 7: the test words are all 128 words, each decodes, the decision is the code word of least cost over all 16 and
    x + extrinsic is the exact max-log LLR."""
    code = M.Code(7, 1, 3)
    cws = all_codewords(code).astype(np.int64)
    for kind in ("integer", "random"):
        x = soft_words(7, 20, 77, kind)
        got = CM.decode_batch(x, code, 7, 0.25)
        assert (got["candidates"] == 128).all()
        for b, row in enumerate(x):
            h, r = (row < 0).astype(np.int64), np.abs(row)
            cost = np.array([CM.serial_sum(r[np.flatnonzero(c != h)]) for c in cws])
            assert got["metric"][b] == cost.min() and cost[(cws == got["codeword"][b]).all(axis=1)][0] == cost.min()
            llr = np.array([cost[cws[:, i] == 1].min() - cost[cws[:, i] == 0].min() for i in range(7)])
            s = np.where(got["codeword"][b] == 0, 1.0, -1.0)
            assert bits_equal(got["extrinsic"][b], s * np.abs(llr) - row)    # every position has a competitor: beta is never used
            if kind == "integer":
                assert np.array_equal(row + got["extrinsic"][b], llr)        # exact in integers
            else:
                assert np.allclose(row + got["extrinsic"][b], llr, rtol=0, atol=1e-12)


def test_more_test_positions_never_raise_the_metric():
    for n, t, m in SMALL + [(31, 2, 5)]:
        code = M.Code(n, t, m)
        x = soft_words(n, 10, n, "random")
        last = None
        for p in range(1, 7):
            got = CM.decode_batch(x, code, p, 0.5)
            if last is not None:
                both = (got["candidates"] > 0) & (last["candidates"] > 0)
                assert (got["metric"][both] <= last["metric"][both]).all() and (got["candidates"] >= last["candidates"]).all()
            last = got


def test_model_rejects_a_word_on_its_own_and_applies_the_prior():
    code = M.Code(15, 2, 4)
    x = soft_words(15, 5, 3, "random")
    ref = CM.decode_batch(x, code, 3, 0.5)
    bad = x.copy()
    bad[1, 4], bad[3, 0], bad[3, 1] = np.nan, -np.inf, np.inf
    got = CM.decode_batch(bad, code, 3, 0.5)
    assert got["candidates"].tolist() == [ref["candidates"][0], -1, ref["candidates"][2], -1, ref["candidates"][4]]
    assert np.isinf(got["metric"][[1, 3]]).all() and not got["extrinsic"][[1, 3]].any()
    assert got["codeword"][1, 4] == 0 and got["codeword"][3, :2].tolist() == [1, 0]
    assert np.array_equal(got["codeword"][1], np.where(np.isnan(bad[1]), 0, bad[1] < 0))
    for b in (0, 2, 4):
        assert bits_equal(got["extrinsic"][b], ref["extrinsic"][b])
    prior = soft_words(15, 5, 4, "random")
    with_prior = CM.decode_batch(x, code, 3, 0.5, prior, 0.3)
    direct = CM.decode_batch(x + np.float64(0.3) * prior, code, 3, 0.5)
    assert all(bits_equal(with_prior[k], direct[k]) for k in ("extrinsic", "metric")) and np.array_equal(with_prior["codeword"], direct["codeword"])


def test_tpc_model_encoder_and_layout_helpers():
    row, col = M.Code(15, 1, 4), M.Code(7, 1, 3)
    assert (row.k, col.k) == (11, 4)
    msg = np.random.RandomState(1).randint(0, 2, (3, 4, 11)).astype(np.uint8)
    x = TM.encode(msg, row, col)
    assert x.shape == (3, 7, 15) and np.array_equal(x[:, :4, :11], msg)
    assert not M.syndromes(CM.words_of(x, 2), row).any() and not M.syndromes(CM.words_of(x, 1), col).any()
    for axis in (1, 2):
        assert np.array_equal(CM.block_of(CM.words_of(x, axis), x.shape, axis), x)
    assert np.array_equal(CM.words_of(x, 1)[15 + 2], x[1, :, 2])
    clean = TM.decode(4.0 * (1.0 - 2.0 * x), row, col, iters=1, p=2)
    assert np.array_equal(clean["bits"], msg) and np.array_equal(clean["codeword"], x)


# ---- names --------------------------------------------------------------------------------------------------------------------------
def test_abi_names():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "commpy_amd.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(cpx_chase_[a-z0-9_]+)\s*\(", text))
    assert declared == set(NAMES) == {s for s in _lib.SYMBOLS if s.startswith("cpx_chase_")}
    lib = _lib.load()
    assert all(hasattr(lib, s) for s in NAMES)
    names = {"chase_decode", "ProductCode", "tpc_encode", "tpc_decode"}
    assert names <= set(channelcoding.__all__) and all(callable(getattr(channelcoding, n)) for n in names)
    assert {"bch_chase_dev", "tpc_decode_dev"} <= set(deviceops.__all__)
    from commpy_amd import build
    assert "bch_chase.hip" in build.SOURCES and any(h.endswith("bch_dev.h") for h in build.HEADERS)
    read = lambda name: open(os.path.join(build.CSRC, name)).read()
    for source, header in (("bch.hip", "bch_dev.h"), ("bch_chase.hip", "bch_dev.h"), ("rs.hip", "cpx_gf.h")):
        text = read(source)                                       # one copy of the algebraic decoder's stages, called by all three
        assert '#include "%s"' % header in text and "struct Gf" not in text and "berlekamp_massey(" in text and "chien_search<" in text
        assert not re.search(r"\b(?:void|unsigned)\s+wave_(?:sync|xor)\s*\(", text) and not re.search(r"\bbool\s+berlekamp_massey\s*\(", text)
    assert '#include "cpx_gf.h"' in read("bch_dev.h") and "struct Gf" in read("cpx_gf.h") and "struct Gf" not in read("bch_dev.h")
    assert sum(read(name).count("hipFuncSetAttribute") for name in ("bch.hip", "bch_chase.hip", "rs.hip", "bch_dev.h", "cpx_gf.h")) == 1


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def no_device(monkeypatch):
    """Any attempt to load the engine fails the test: the refusals below must come from the host-side checks."""
    def boom(*a, **k):
        raise AssertionError("the engine was touched")
    monkeypatch.setattr(_lib, "load", boom)


def test_python_refusals(no_device):
    code = BCHCode(15, 2)
    tpc = ProductCode(BCHCode(15, 1), BCHCode(7, 1))
    assert (tpc.n_r, tpc.k_r, tpc.n_c, tpc.k_c, tpc.n, tpc.k) == (15, 11, 7, 4, 105, 44)
    x, blk = np.zeros((2, 15)), np.zeros((2, 7, 15))
    for bad in (lambda: chase_decode(x, None, 2, 0.5), lambda: chase_decode(x, code, 0, 0.5), lambda: chase_decode(x, code, 9, 0.5),
                lambda: chase_decode(x, code, 2.0, 0.5), lambda: chase_decode(x, code, True, 0.5), lambda: chase_decode(np.zeros((2, 7)), BCHCode(7, 1), 8, 0.5),
                lambda: chase_decode(x, code, 2, -0.1), lambda: chase_decode(x, code, 2, np.nan), lambda: chase_decode(x, code, 2, np.inf),
                lambda: chase_decode(x, code, 2, "1"), lambda: chase_decode(x, code, 2, 0.5, alpha=np.inf), lambda: chase_decode(x, code, 2, 0.5, alpha=None),
                lambda: chase_decode(np.zeros((2, 14)), code, 2, 0.5), lambda: chase_decode(np.zeros((2, 2, 15)), code, 2, 0.5),
                lambda: chase_decode(np.zeros(()), code, 2, 0.5), lambda: chase_decode(x.astype(complex), code, 2, 0.5),
                lambda: chase_decode(x, code, 2, 0.5, prior=np.zeros((3, 15))), lambda: chase_decode(x, code, 2, 0.5, prior=np.zeros(15)),
                lambda: chase_decode(x, code, 2, 0.5, prior=np.zeros((2, 14))), lambda: chase_decode(x, code, 2, 0.5, want=()),
                lambda: chase_decode(x, code, 2, 0.5, want=("bits", "errors")), lambda: chase_decode(x, code, 2, 0.5, want="llr"),
                lambda: ProductCode(code, None), lambda: ProductCode(15, 7),
                lambda: tpc_encode(np.zeros((2, 4, 10), np.uint8), tpc), lambda: tpc_encode(np.zeros((4,), np.uint8), tpc),
                lambda: tpc_encode(np.full((2, 4, 11), 2), tpc), lambda: tpc_encode(np.zeros((2, 4, 11)), tpc),
                lambda: tpc_encode(np.zeros((2, 4, 11), np.uint8), code),
                lambda: tpc_decode(blk, code), lambda: tpc_decode(np.zeros((2, 15, 7)), tpc), lambda: tpc_decode(np.zeros(105), tpc),
                lambda: tpc_decode(blk, tpc, iters=0), lambda: tpc_decode(blk, tpc, iters=1.0), lambda: tpc_decode(blk, tpc, p=0),
                lambda: tpc_decode(blk, tpc, p=9), lambda: tpc_decode(blk, tpc, alpha=[np.nan]), lambda: tpc_decode(blk, tpc, alpha=[]),
                lambda: tpc_decode(blk, tpc, alpha="x"), lambda: tpc_decode(blk, tpc, beta=[0.5, -1.0]), lambda: tpc_decode(blk, tpc, llr_scale=0.0),
                lambda: tpc_decode(blk, tpc, llr_scale=np.inf), lambda: tpc_decode(blk, tpc, want=("bits", "metric")),
                lambda: tpc_decode(blk.astype(complex), tpc),
                lambda: deviceops.bch_chase_dev(code, None, -1, 2, 0.5), lambda: deviceops.bch_chase_dev(None, None, 2, 2, 0.5),
                lambda: deviceops.bch_chase_dev(code, None, 2, 9, 0.5), lambda: deviceops.bch_chase_dev(code, None, 2, 2, 0.5, J=2),
                lambda: deviceops.bch_chase_dev(code, None, 2, 2, 0.5, J=0, strides=(15, 0, 1)),
                lambda: deviceops.bch_chase_dev(code, None, 2, 2, 0.5, J=4, strides=(60, 14, 1)),       # rows overlap
                lambda: deviceops.bch_chase_dev(code, None, 2, 2, 0.5, J=4, strides=(60, 1, 3)),        # columns overlap
                lambda: deviceops.bch_chase_dev(code, None, 2, 2, 0.5, J=4, strides=(59, 15, 1)),       # blocks overlap
                lambda: deviceops.bch_chase_dev(code, None, 2, 2, 0.5, strides=(15, 0, 0)), lambda: deviceops.bch_chase_dev(code, None, 2, 2, 0.5, strides=(15, 0, -1)),
                lambda: deviceops.bch_chase_dev(code, None, 2, 2, 0.5, strides=(15, 1)), lambda: deviceops.bch_chase_dev(code, None, 2, 2, 0.5, strides=(1 << 40, 0, 1)),
                lambda: deviceops.bch_chase_dev(code, None, 2, 2, 0.5, want="errors"),
                lambda: deviceops.bch_chase_dev(code, None, 2, 2, 0.5, want="bits", d_extrinsic=object()),
                lambda: deviceops.tpc_decode_dev(code, None, 2), lambda: deviceops.tpc_decode_dev(tpc, None, -1),
                lambda: deviceops.tpc_decode_dev(tpc, None, 2, want="bits"), lambda: deviceops.tpc_decode_dev(tpc, None, 2, iters=0)):
        with pytest.raises(ValueError):
            bad()
    # empty batches need no device
    assert chase_decode(np.zeros((0, 15)), code, 2, 0.5).shape == (0, 7)
    got = chase_decode(np.zeros((0, 15)), code, 2, 0.5, want=("candidates", "metric", "extrinsic", "codeword", "bits"))
    assert [g.shape for g in got] == [(0, 7), (0, 15), (0, 15), (0,), (0,)]
    assert [g.dtype for g in got] == [np.uint8, np.uint8, np.float64, np.float64, np.int32]
    assert tpc_decode(np.zeros((0, 7, 15)), tpc).shape == (0, 4, 11)


def test_engine_checks_without_device():
    lib = _lib.load()
    buf = np.zeros(64)
    P = _lib.ptr
    for rc in (lib.cpx_chase_bch(None, P(buf), None, 1.0, 0.5, 2, 1, P(buf), None, None, None, None),
               lib.cpx_chase_bch_dev(None, P(buf), None, 1.0, 0.5, 2, 0, 1, 15, 0, 1, P(buf), None, None, None, None, None)):
        assert rc == _lib.CPX_EINVAL and "null handle" in _lib.last_error()


def test_entry_points_fail_loudly_without_device():
    if _lib.device_count() > 0:
        return
    code = BCHCode(15, 2)
    tpc = ProductCode(BCHCode(15, 1), BCHCode(7, 1))
    for call in (lambda: chase_decode(np.ones((2, 15)), code, 2, 0.5), lambda: chase_decode(np.ones(15), code, 2, 0.5, want=("bits", "metric")),
                 lambda: tpc_decode(np.ones((2, 7, 15)), tpc), lambda: tpc_encode(np.zeros((2, 4, 11), np.uint8), tpc),
                 lambda: deviceops.bch_chase_dev(code, None, 2, 2, 0.5)):
        with pytest.raises(_lib.EngineError):
            call()
