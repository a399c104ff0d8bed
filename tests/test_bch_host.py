"""Host side of the Galois-field, cyclic-code and BCH work: the NumPy model (tests/bch_model.py) against brute-force bounded-distance
decoding; gfields / algcode against the live reference's fixture, the reference test suite's recorded values and their own properties;
the conditions the GPU tests' input sets must meet; the C-ABI's names; every refusal (ValueError / CPX_EINVAL / CPX_ELIMIT before any
device is touched) and the loud failure without a device."""
import ctypes
import itertools
import json
import os
import re

import numpy as np
import pytest

import bch_model as M
from commpy_amd import _lib, channelcoding, deviceops
from commpy_amd.channelcoding import (GF, BCHCode, bch_decode, bch_encode, bch_genpoly, cyclic_code_genpoly, poly_to_string, polydivide,
                                      polymultiply)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["cpx_bch_create", "cpx_bch_destroy", "cpx_bch_encode", "cpx_bch_encode_dev", "cpx_bch_decode", "cpx_bch_decode_dev"]
DVB_PRIM_POLY = 16427
# (n, t, m): the sets of 200 words with t + 1 errors each, and the shortened (100, 86) set with 3 errors; tests/test_bch_gpu.py decodes
# the same words on the device
BEYOND_T = {(15, 2, 4): 11, (31, 2, 5): 12}
SHORTENED, SHORTENED_SEED = (100, 2, 7), 13


def noisy_words(n, t, m, errors, seed, B=200, prim_poly=None):
    """(code, sent [B, n], received [B, n], positions): B seeded code words with exactly ``errors`` flipped bits each."""
    code = M.Code(n, t, m, prim_poly)
    rs = np.random.RandomState(seed)
    sent = M.encode_batch(rs.randint(0, 2, (B, code.k)), code)
    pos = M.error_sets(rs, B, n, code.k, errors) if errors else [[] for _ in range(B)]
    return code, sent, M.with_errors(sent, pos), pos


# ---- the model ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, t, m", [(7, 1, 3), (15, 2, 4), (15, 3, 4)])
def test_model_is_bounded_distance_decoding(n, t, m):
    """Every one of the 2^n words: the unique code word within distance t where there is one, else a failure and the word unchanged."""
    code = M.Code(n, t, m)
    assert (code.n, code.k) in ((7, 4), (15, 7), (15, 5))
    words = ((np.arange(2 ** n)[:, None] >> np.arange(n - 1, -1, -1)) & 1).astype(np.uint8)
    cws = M.encode_batch(np.array(list(itertools.product([0, 1], repeat=code.k)), dtype=np.uint8), code)
    dist = (words[:, None, :] ^ cws[None, :, :]).sum(axis=2)
    near, best = dist.argmin(axis=1), dist.min(axis=1)
    assert ((dist <= t).sum(axis=1) <= 1).all()                   # the spheres of radius t do not meet
    got = M.decode_batch(words, code)
    inside = best <= t
    assert np.array_equal(got["errors"][inside], best[inside]) and (got["errors"][~inside] == -1).all()
    assert np.array_equal(got["codeword"][inside], cws[near[inside]]) and np.array_equal(got["codeword"][~inside], words[~inside])
    assert np.array_equal(got["bits"], got["codeword"][:, :code.k])
    if (n, t) != (7, 1):
        assert 0 < inside.sum() < len(words)                      # a perfect code has no failures


def test_model_encoder_is_systematic_and_cyclic():
    for n, t, m in ((15, 2, 4), (63, 2, 6), (100, 2, 7), (255, 18, 8)):
        code = M.Code(n, t, m)
        rs = np.random.RandomState(n)
        for msg in rs.randint(0, 2, (4, code.k)):
            cw = M.encode(msg, code)
            assert np.array_equal(cw[:code.k], msg)
            assert polydivide(int("".join(map(str, cw)), 2), code.g) == 0
            assert not M.syndromes(cw, code).any()


# ---- generator values ---------------------------------------------------------------------------------------------------------------
def test_bch_generators():
    for (m, t), g in {(4, 1): 19, (4, 2): 465, (4, 3): 1335, (5, 2): 1897, (6, 2): 5433, (7, 2): 17271, (8, 2): 94051}.items():
        assert bch_genpoly(m, t) == g == M.genpoly(m, t) and isinstance(bch_genpoly(m, t), int)
    assert bch_genpoly(8, 18).bit_length() - 1 == 124 and bch_genpoly(8, 18) == M.genpoly(8, 18)
    assert bch_genpoly(14, 12).bit_length() - 1 == 168
    dvb = bch_genpoly(14, 12, DVB_PRIM_POLY)
    assert dvb.bit_length() - 1 == 168 and dvb != bch_genpoly(14, 12) and dvb == M.genpoly(14, 12, DVB_PRIM_POLY)
    for args, nk in (((15, 2), (15, 7)), ((15, 3), (15, 5)), ((31, 2), (31, 21)), ((63, 2), (63, 51)), ((127, 2), (127, 113)),
                     ((255, 2), (255, 239)), ((255, 18), (255, 131)), ((100, 2), (100, 86)), ((1023, 10), (1023, 923))):
        code = BCHCode(*args)
        assert (code.n, code.k) == nk and code.t == args[1] and code.m == max(3, args[0].bit_length())
        assert code.genpoly == bch_genpoly(code.m, code.t) and code.prim_poly == M.DEFAULT_PRIM_POLY[code.m]
    code = BCHCode(3240, 12, m=14, prim_poly=DVB_PRIM_POLY)       # the DVB-S2 short-frame code
    assert (code.n, code.k, code.m, code.prim_poly, code.genpoly) == (3240, 3072, 14, DVB_PRIM_POLY, dvb)
    assert BCHCode(64, 2, m=7).k == 50 and BCHCode(7, 1).m == 3 and BCHCode(7, 1).k == 4


# ---- gfields ------------------------------------------------------------------------------------------------------------------------
def test_gf_equals_the_live_reference():
    with open(os.path.join(ROOT, "tests", "golden", "gfields.json")) as f:
        golden = json.load(f)
    assert sorted(map(int, golden)) == [2, 3, 4, 5, 6, 8]
    for m, case in golden.items():
        m = int(m)
        assert GF(1, m).prim_poly == case["prim_poly"] and GF(1, m).m == m
        for s in case["sets"]:
            g = GF(np.array(s["elements"]), m)
            assert g.elements.tolist() == s["elements"]
            assert g.tuple_to_power().elements.tolist() == s["tuple_to_power"]
            assert g.order().tolist() == s["order"] and g.order().dtype == np.float64
            assert [c.elements.tolist() for c in g.cosets()] == s["cosets"]
            if "minpolys" in s:
                assert g.minpolys().tolist() == s["minpolys"]
        assert GF(np.array(case["exponents"]), m).power_to_tuple().elements.tolist() == case["power_to_tuple"]
        a, b = GF(np.array(case["a"]), m), GF(np.array(case["b"]), m)
        assert (a + b).elements.tolist() == case["sum"]
        if "product" in case:
            assert (a * b).elements.tolist() == case["product"]
    assert "minpolys" in golden["4"]["sets"][0] and "product" in golden["4"]


def test_gf_values_of_the_reference_test_suite():
    ar = np.arange
    assert (GF(ar(8), 3) + GF(np.array([6, 4, 3, 1, 2, 0, 5, 7]), 3)).elements.tolist() == [6, 5, 1, 2, 6, 5, 3, 0]
    assert (GF(np.array([7, 6, 5, 4, 3, 2, 1, 0]), 3) * GF(np.array([6, 4, 3, 1, 2, 0, 5, 7]), 3)).elements.tolist() == [4, 5, 4, 4, 6, 0, 5, 0]
    assert GF(ar(0, 7), 3).power_to_tuple().elements.tolist() == [1, 2, 4, 3, 6, 7, 5]
    assert GF(ar(1, 8), 3).tuple_to_power().elements.tolist() == [0, 1, 3, 2, 6, 4, 5]
    assert GF(ar(1, 16), 4).tuple_to_power().elements.tolist() == [0, 1, 4, 2, 8, 5, 10, 3, 14, 9, 7, 6, 13, 11, 12]
    assert GF(ar(1, 16), 4).order().tolist() == [1, 15, 15, 15, 15, 3, 3, 5, 15, 5, 15, 5, 15, 15, 5]
    assert GF(ar(16), 4).minpolys().tolist() == [2, 3, 19, 19, 19, 19, 7, 7, 31, 25, 31, 25, 31, 25, 25, 31]
    assert [c.elements.tolist() for c in GF(ar(16), 4).cosets()] == [[0], [1], [2, 3, 4, 5], [6, 7], [8, 10, 12, 15], [9, 11, 13, 14]]
    assert GF(np.array([2, 8, 32, 6, 24, 35, 10, 40, 59, 41, 14, 37]), 6).minpolys().tolist() == [67, 87, 103, 73, 13, 109, 91, 117, 7, 115, 11,
                                                                                                 97]
    for m in range(1, 9):                                         # closure, as the reference's test_closure
        q = 2 ** m
        a, b = np.repeat(ar(q), q), np.tile(ar(q), q)
        assert (GF(a, m) + GF(b, m)).elements.max() < q and (GF(a, m) * GF(b, m)).elements.max() < q


def test_gf_field_axioms_and_helpers():
    defaults = [3, 7, 11, 19, 37, 67, 137, 285, 529, 1033, 2053, 4179, 8219, 17475, 32771, 69643]
    assert [GF(1, m).prim_poly for m in range(1, 17)] == defaults
    for m, p in ((4, None), (8, None), (10, None), (14, DVB_PRIM_POLY)):
        rs = np.random.RandomState(m)
        q = 2 ** m
        kw = {} if p is None else {"prim_poly": p}
        a, b, c = (GF(rs.randint(0, q, 300), m, **kw) for _ in range(3))
        assert np.array_equal((a * b).elements, (b * a).elements)
        assert np.array_equal(((a * b) * c).elements, (a * (b * c)).elements)
        assert np.array_equal((a * (b + c)).elements, ((a * b) + (a * c)).elements)
        pp = a.prim_poly
        assert (a * b).elements.tolist() == [polymultiply(int(x), int(y), m, pp) for x, y in zip(a.elements, b.elements)]
        nz = GF(a.elements[a.elements > 0], m, **kw)
        assert np.array_equal(nz.tuple_to_power().power_to_tuple().elements, nz.elements)
        # a minimal polynomial vanishes at its element and is irreducible of the coset's degree
        x = int(nz.elements[0])
        mp = int(nz.minpolys()[0])
        acc = 0
        for i in range(mp.bit_length() - 1, -1, -1):
            acc = polymultiply(acc, x, m, pp) ^ ((mp >> i) & 1)
        assert acc == 0
    assert GF(1, 14, prim_poly=DVB_PRIM_POLY).prim_poly == DVB_PRIM_POLY
    assert polydivide(0b1000, 0b1011) == 0b011 and polydivide(5, 19) == 5 and polydivide(19, 19) == 0
    assert polymultiply(7, 6, 3, 11) == 4
    assert poly_to_string(19) == "x^0 + x^1 + x^4 " and poly_to_string(0) == "" and poly_to_string(1) == "x^0 "


# ---- cyclic codes -------------------------------------------------------------------------------------------------------------------
def test_cyclic_code_genpoly_recorded_lists():
    assert cyclic_code_genpoly(15, 4).tolist() == [2479, 3171, 3929]
    assert cyclic_code_genpoly(31, 21).tolist() == [1653, 1667, 1503, 1207, 1787, 1561, 1903, 1219, 1137, 2013, 1453, 1897, 1975, 1395, 1547]
    assert cyclic_code_genpoly(23, 12).tolist() == [2787, 3189]


@pytest.mark.parametrize("n, k, count", [(7, 4, 2), (15, 7, 3), (21, 12, 7), (23, 12, 2), (63, 51, 63)])
def test_cyclic_code_genpoly_properties(n, k, count):
    polys = [int(p) for p in cyclic_code_genpoly(n, k)]
    assert len(polys) == count == len(set(polys))
    for p in polys:
        assert p.bit_length() - 1 == n - k and polydivide((1 << n) | 1, p) == 0
    if (n, k) == (15, 7):
        assert bch_genpoly(4, 2) in polys


# ---- the input sets of the GPU tests ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, t, m", sorted(BEYOND_T))
def test_sets_beyond_t_hold_failures_and_miscorrections(n, t, m):
    code, sent, rx, _ = noisy_words(n, t, m, t + 1, BEYOND_T[(n, t, m)])
    got = M.decode_batch(rx, code)
    failures = int((got["errors"] == -1).sum())
    wrong = int(((got["errors"] >= 0) & (got["codeword"] != sent).any(axis=1)).sum())
    assert failures >= 10 and wrong >= 10 and failures + wrong == 200, (failures, wrong)
    assert np.array_equal(got["codeword"][got["errors"] == -1], rx[got["errors"] == -1])


def shortened_region_failures(code, rx):
    """Rows that fail in the shortened code although the mother code of length 2^m - 1 finds sigma's roots: one of them lies in the
    shortened-away positions."""
    mother = M.Code(code.field.N, code.t, code.m)
    padded = np.concatenate([np.zeros((len(rx), mother.n - code.n), np.uint8), rx], axis=1)
    return (M.decode_batch(rx, code)["errors"] == -1) & (M.decode_batch(padded, mother)["errors"] >= 0)


def test_shortened_set_holds_a_root_in_the_shortened_region():
    code, _, rx, _ = noisy_words(*SHORTENED, 3, SHORTENED_SEED)
    assert (code.n, code.k) == (100, 86)
    assert shortened_region_failures(code, rx).sum() >= 1


# ---- names --------------------------------------------------------------------------------------------------------------------------
def test_abi_names():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "commpy_amd.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(cpx_bch_[a-z0-9_]+)\s*\(", text))
    assert declared == set(NAMES) == {s for s in _lib.SYMBOLS if s.startswith("cpx_bch_")}
    lib = _lib.load()
    assert all(hasattr(lib, s) for s in NAMES)
    names = {"GF", "polydivide", "polymultiply", "poly_to_string", "cyclic_code_genpoly", "bch_genpoly", "BCHCode", "bch_encode", "bch_decode"}
    assert names <= set(channelcoding.__all__) and all(callable(getattr(channelcoding, n)) for n in names)
    assert {"bch_encode_dev", "bch_decode_dev"} <= set(deviceops.__all__)
    from commpy_amd import build
    assert "bch.hip" in build.SOURCES


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def no_device(monkeypatch):
    """Any attempt to load the engine fails the test: the refusals below must come from the host-side checks."""
    def boom(*a, **k):
        raise AssertionError("the engine was touched")
    monkeypatch.setattr(_lib, "load", boom)


def test_python_refusals(no_device):
    code = BCHCode(15, 2)
    assert BCHCode(3240, 12, m=14, prim_poly=DVB_PRIM_POLY).k == 3072         # accepted
    rx = np.zeros((2, 15), np.uint8)
    for bad in (lambda: BCHCode(1, 1), lambda: BCHCode(0, 1), lambda: BCHCode(15.0, 2), lambda: BCHCode(True, 1), lambda: BCHCode(15, 0),
                lambda: BCHCode(15, 33), lambda: BCHCode(15, 2.0), lambda: BCHCode(15, 8), lambda: BCHCode(3, 1, m=2), lambda: BCHCode(15, 2, m=15),
                lambda: BCHCode(16, 2, m=4), lambda: BCHCode(16384, 2), lambda: BCHCode(40000, 2, m=14), lambda: BCHCode(10, 3, m=4),
                lambda: BCHCode(8, 2, m=4), lambda: BCHCode(15, 2, prim_poly=31), lambda: BCHCode(15, 2, prim_poly=37),
                lambda: BCHCode(15, 2, prim_poly=16), lambda: BCHCode(15, 2, prim_poly=19.0), lambda: BCHCode(3240, 12, m=14, prim_poly=16385),
                lambda: bch_encode(np.zeros((2, 6), np.uint8), code), lambda: bch_encode(np.zeros((2, 2, 7), np.uint8), code),
                lambda: bch_encode(np.full((2, 7), 2), code), lambda: bch_encode(np.full((2, 7), -1), code), lambda: bch_encode(np.zeros((2, 7)), code),
                lambda: bch_encode(np.zeros((2, 7), np.uint8), None), lambda: bch_encode(np.zeros((), np.uint8), code),
                lambda: bch_decode(np.zeros((2, 14), np.uint8), code), lambda: bch_decode(np.zeros((2, 2, 15), np.uint8), code),
                lambda: bch_decode(np.full((2, 15), 3), code), lambda: bch_decode(np.zeros((2, 15)), code), lambda: bch_decode(rx, None),
                lambda: bch_decode(rx, code, want=()), lambda: bch_decode(rx, code, want=("bits", "word")), lambda: bch_decode(rx, code, want="nothing"),
                lambda: deviceops.bch_encode_dev(code, None, -1), lambda: deviceops.bch_encode_dev(None, None, 2),
                lambda: deviceops.bch_decode_dev(code, None, 2, want="llr"), lambda: deviceops.bch_decode_dev(code, None, 2.0),
                lambda: deviceops.bch_decode_dev(None, None, 2),
                lambda: GF(1, 0), lambda: GF(1, 17), lambda: GF(16, 4), lambda: GF(np.arange(4), 4, prim_poly=31), lambda: GF(np.arange(4), 4, prim_poly=37),
                lambda: GF(np.arange(4), 4) + GF(np.arange(5), 4), lambda: GF(np.arange(4), 4) * GF(np.arange(5), 4),
                lambda: GF(np.arange(4), 4) * GF(np.arange(4), 5), lambda: GF(np.array([16]), 4).tuple_to_power(), lambda: GF(np.zeros((2, 2)), 4),
                lambda: cyclic_code_genpoly(16, 4), lambda: cyclic_code_genpoly(15, 15), lambda: cyclic_code_genpoly(15, 0),
                lambda: bch_genpoly(4, 8), lambda: bch_genpoly(4, 0), lambda: bch_genpoly(17, 1), lambda: bch_genpoly(4, 2, prim_poly=31),
                lambda: polydivide(5, 0)):
        with pytest.raises(ValueError):
            bad()
    # empty batches need no device
    assert bch_encode(np.zeros((0, 7), np.uint8), code).shape == (0, 15)
    assert bch_decode(np.zeros((0, 15), np.uint8), code).shape == (0, 7)
    bits, word, errors = bch_decode(np.zeros((0, 15), np.uint8), code, want=("errors", "codeword", "bits"))
    assert bits.shape == (0, 7) and word.shape == (0, 15) and errors.shape == (0,) and errors.dtype == np.int32 and bits.dtype == np.uint8


def genpoly_bytes(g):
    return np.array([(g >> i) & 1 for i in range(g.bit_length())], dtype=np.uint8)


def test_engine_checks_without_device():
    """The C entry points: argument errors are reported before the device is looked for; a valid call fails loudly without one."""
    lib = _lib.load()
    P, E, Lm = _lib.ptr, _lib.CPX_EINVAL, _lib.CPX_ELIMIT
    h = ctypes.c_void_p()
    g465 = genpoly_bytes(465)

    def create(m=4, prim=19, n=15, t=2, g=g465, deg=None, out=ctypes.byref(h)):
        return lib.cpx_bch_create(m, prim, n, t, None if g is None else P(g), len(g465) - 1 if deg is None else deg, out)

    def message(rc, code=E):
        assert rc == code, (rc, _lib.last_error())
        return _lib.last_error()

    assert "null pointer" in message(create(out=None)) and "null pointer" in message(create(g=None))
    assert "m = 2" in message(create(m=2, prim=7, n=3, t=1), Lm) and "m = 15" in message(create(m=15, prim=32771), Lm)
    assert "t = 0" in message(create(t=0), Lm) and "t = 33" in message(create(t=33), Lm)
    assert "n = 16" in message(create(n=16), Lm) and "n = 1 " in message(create(n=1), Lm)
    assert "2 t <" in message(create(m=3, prim=11, n=7, t=4), Lm)
    assert "has not degree" in message(create(prim=37)) and "has not degree" in message(create(prim=11))
    assert "not primitive" in message(create(prim=31)) and "order 5" in _lib.last_error()
    assert "not primitive" in message(create(prim=16))
    assert "degree 8 is outside" in message(create(n=8)) and "degree 0 is outside" in message(create(deg=0))
    big = genpoly_bytes(1 << 449 | 1)
    assert "above the engine's limit of 448" in message(create(m=9, prim=529, n=511, t=2, g=big, deg=449), Lm)
    two = g465.copy()
    two[3] = 2
    assert "genpoly_bits[3] = 2" in message(create(g=two))
    assert "coefficient of x^5 is zero" in message(create(g=g465, deg=5))
    assert "no constant term" in message(create(g=genpoly_bytes(465 << 1), deg=9))
    assert "does not vanish at alpha^3" in message(create(g=genpoly_bytes(19), deg=4))
    assert "does not vanish at alpha^1" in message(create(g=genpoly_bytes(0b100101), deg=5))
    assert h.value is None
    buf = np.zeros(1 << 10, np.uint8)
    for rc in (lib.cpx_bch_encode(None, P(buf), 1, P(buf)), lib.cpx_bch_encode_dev(None, P(buf), 0, P(buf), None),
               lib.cpx_bch_decode(None, P(buf), 1, P(buf), None, None), lib.cpx_bch_decode_dev(None, P(buf), 0, P(buf), None, None, None)):
        assert "null handle" in message(rc)
    assert lib.cpx_bch_destroy(None) == _lib.CPX_OK
    if _lib.device_count() > 0:
        return
    assert create() == _lib.CPX_ENODEV and _lib.last_error().startswith("no HIP device available") and h.value is None
    dvb = genpoly_bytes(bch_genpoly(14, 12, DVB_PRIM_POLY))
    assert create(m=14, prim=DVB_PRIM_POLY, n=3240, t=12, g=dvb, deg=168) == _lib.CPX_ENODEV
    assert "does not vanish" in message(create(m=14, prim=17475, n=3240, t=12, g=dvb, deg=168))


def test_entry_points_fail_loudly_without_device():
    if _lib.device_count() > 0:
        pytest.skip("a HIP device is present")
    code = BCHCode(15, 2)
    for call in (lambda: bch_encode(np.zeros((2, 7), np.uint8), code), lambda: bch_encode(np.zeros(7, np.uint8), code),
                 lambda: bch_decode(np.zeros((2, 15), np.uint8), code), lambda: bch_decode(np.zeros(15, np.uint8), code, want=("bits", "errors")),
                 lambda: deviceops.bch_decode_dev(code, None, 2)):
        with pytest.raises(_lib.EngineError):
            call()
