"""Host side of the Reed-Solomon work: the NumPy model (tests/rs_model.py) against brute-force bounded-distance errors-and-erasures
decoding; the encoder's and the generator's properties; the conditions the GPU tests' input sets must meet; the C-ABI's names; every
refusal (ValueError / CPX_EINVAL / CPX_ELIMIT before any device is touched) and the loud failure without a device."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest

import rs_model as M
from commpy_amd import _lib, channelcoding, deviceops
from commpy_amd.channelcoding import RSCode, rs_decode, rs_encode, rs_genpoly

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["cpx_rs_create", "cpx_rs_destroy", "cpx_rs_encode", "cpx_rs_encode_dev", "cpx_rs_decode", "cpx_rs_decode_dev"]
# (n, k, m, fcr)
BRUTE = [(7, 3, 3, 0), (7, 3, 3, 1), (7, 4, 3, 1), (6, 2, 3, 1), (5, 2, 3, 3), (7, 5, 3, 1), (9, 3, 4, 1)]
ENCODER = BRUTE + [(255, 223, 8, 1), (204, 188, 8, 0), (544, 514, 10, 1), (300, 280, 14, 1)]
# the sets tests/test_rs_gpu.py decodes on the device as well: (n, k, m) -> seed
BEYOND = {(15, 11, 4): 21, (31, 25, 5): 22}
SHORTENED, SHORTENED_SEED = (20, 16, 5), 23


def noisy_words(n, k, m, pairs, seed, per=1, fcr=1, prim_poly=None):
    """(code, sent, received, flags, e): ``per`` seeded code words for every (e, f) of ``pairs``, with f flagged positions (holding
    their sent value or, every other one, garbage) and e changed symbols at unflagged positions."""
    code = M.Code(n, k, m, prim_poly, fcr)
    rs = np.random.RandomState(seed)
    e = np.repeat([p[0] for p in pairs], per)
    f = np.repeat([p[1] for p in pairs], per)
    sent = M.encode_batch(rs.randint(0, 1 << m, (len(e), k)), code)
    flags = M.flag_sets(rs, len(e), n, f)
    rx, _ = M.with_errors(rs, sent, flags, e, 1 << m)
    garbage = rs.randint(0, 1 << m, rx.shape).astype(np.uint16)
    rx[1::2] = np.where(flags[1::2], garbage[1::2], rx[1::2])
    return code, sent, rx, flags, e


def boundary_pairs(r):
    """Every (e, f) with 2e + f in {r - 1, r}, and the clean word."""
    return [(0, 0)] + [(e, f) for f in range(r + 1) for e in range(r + 1) if 2 * e + f in (r - 1, r) and (e, f) != (0, 0)]


def beyond_pairs(r):
    return [(e, f) for f in range(r + 1) for e in range(1, r + 2) if 2 * e + f in (r + 1, r + 2)]


# ---- the model ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, k, m, fcr", BRUTE)
def test_model_is_bounded_distance_decoding(n, k, m, fcr):
    """Sampled words and flag sets: the unique code word c with 2 #{i unflagged: c_i != r_i} + f <= r where there is one, else a
    failure and the word unchanged; no unflagged root ever receives Y = 0."""
    code = M.Code(n, k, m, fcr=fcr)
    r, q, B = n - k, 1 << m, 640
    cws = M.encode_batch(np.array(list(itertools.product(range(q), repeat=k))), code)
    rs = np.random.RandomState(1000 * n + 10 * k + fcr)
    f = np.arange(B) % (r + 2)                                    # 0 .. r + 1 flags
    flags = M.flag_sets(rs, B, n, f)
    words = rs.randint(0, q, (B, n)).astype(np.uint16)
    e = np.minimum((np.arange(B) // (r + 2)) % (r + 2), n - f)    # 0 .. r + 1 errors
    words[B // 2:], _ = M.with_errors(rs, cws[rs.randint(0, len(cws), B - B // 2)], flags[B // 2:], e[B // 2:], q)
    idx, diff = M.brute_force(words, flags, cws, r)
    got = M.decode_batch(words, code, flags, detail=True)
    found = idx >= 0
    assert np.array_equal(got["errors"] >= 0, found)
    assert np.array_equal(got["errors"][found], diff[found]) and (got["errors"][~found] == -1).all()
    assert np.array_equal(got["codeword"][found], cws[idx[found]]) and np.array_equal(got["codeword"][~found], words[~found])
    assert np.array_equal(got["symbols"], got["codeword"][:, :k])
    assert not got["zero_at_unflagged"].any()
    counts = (int((~found).sum()), int((got["errors"] > 0).sum()), int((found & (f == r)).sum()))
    assert min(counts) >= 10, counts


@pytest.mark.parametrize("n, k, m, fcr", ENCODER)
def test_model_encoder_is_systematic_and_vanishes_at_the_roots(n, k, m, fcr):
    code = M.Code(n, k, m, fcr=fcr)
    rs = np.random.RandomState(n)
    msg = rs.randint(0, 1 << m, (4, k))
    cw = M.encode_batch(msg, code)
    assert cw.dtype == np.uint16 and np.array_equal(cw[:, :k], msg) and cw[:, k:].any()
    assert not M.syndromes(cw, code).any()
    f = code.field
    for j in range(n - k):                                        # Horner, symbol by symbol: independent of syndromes()
        x = f.exp[(fcr + j) % f.N]
        assert M.poly_eval(f, [int(c) for c in cw[0][::-1]], x) == 0
    assert not M.encode_batch(np.zeros((1, k), int), code).any()


# ---- the generator and the code object ----------------------------------------------------------------------------------------------
def test_rs_generators_and_code_attributes():
    for n, k, m, fcr in ENCODER:
        g = rs_genpoly(m, n - k, fcr)
        f = M.Field(m)
        assert g.dtype == np.int64 and g.shape == (n - k + 1,) and g[-1] == 1 and g.max() < 1 << m
        assert g.tolist() == M.genpoly(f, n - k, fcr)
        for j in range(n - k):
            assert M.poly_eval(f, g.tolist(), f.exp[(fcr + j) % f.N]) == 0
        assert M.poly_eval(f, g.tolist(), f.exp[(fcr + n - k) % f.N]) != 0
        code = RSCode(n, k, m=m, fcr=fcr)
        assert (code.n, code.k, code.m, code.nroots, code.t, code.fcr) == (n, k, m, n - k, (n - k) // 2, fcr)
        assert code.prim_poly == f.prim_poly and np.array_equal(code.genpoly, g)
    assert rs_genpoly(3, 2).tolist() == [3, 6, 1]                 # (x - a)(x - a^2) = x^2 + a^4 x + a^3 over GF(8), 1011
    assert rs_genpoly(4, 1, fcr=0).tolist() == [1, 1]
    assert [RSCode(n, n - 2).m for n in (4, 7, 8, 15, 16, 255, 256, 544, 16383)] == [3, 3, 4, 4, 5, 8, 9, 10, 14]
    assert RSCode(255, 223).fcr == 1 and RSCode(204, 188, fcr=0).m == 8
    dvb = RSCode(300, 280, m=14, prim_poly=16427)
    assert dvb.prim_poly == 16427 and not np.array_equal(dvb.genpoly, rs_genpoly(14, 20))
    assert np.array_equal(dvb.genpoly, M.genpoly(M.Field(14, 16427), 20))


# ---- the input sets of the GPU tests ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, k, m", sorted(BEYOND))
def test_sets_beyond_the_budget_hold_failures_and_miscorrections(n, k, m):
    code, sent, rx, flags, _ = noisy_words(n, k, m, beyond_pairs(n - k), BEYOND[(n, k, m)], per=40)
    got = M.decode_batch(rx, code, flags)
    failures = int((got["errors"] == -1).sum())
    wrong = int(((got["errors"] >= 0) & (got["codeword"] != sent).any(axis=1)).sum())
    assert failures >= 10 and wrong >= 10 and failures + wrong == len(rx), (failures, wrong)
    assert np.array_equal(got["codeword"][got["errors"] == -1], rx[got["errors"] == -1])


def shortened_region_failures(code, rx, flags):
    """Rows that fail in the shortened code although the mother code of length 2^m - 1 finds Lambda's roots: one of them lies in the
    shortened-away positions."""
    mother = M.Code(code.field.N, code.field.N - code.r, code.m, fcr=code.fcr)
    pad = np.zeros((len(rx), mother.n - code.n), np.uint16)
    return ((M.decode_batch(rx, code, flags)["errors"] == -1) &
            (M.decode_batch(np.concatenate([pad, rx], axis=1), mother, np.concatenate([pad, flags], axis=1))["errors"] >= 0))


def test_shortened_set_holds_a_root_in_the_shortened_region():
    code, _, rx, flags, _ = noisy_words(*SHORTENED, [(3, 0), (2, 1)], SHORTENED_SEED, per=100)
    assert (code.n, code.k, code.r) == (20, 16, 4)
    assert shortened_region_failures(code, rx, flags).sum() >= 1


# ---- names --------------------------------------------------------------------------------------------------------------------------
def test_abi_names():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "commpy_amd.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(cpx_rs_[a-z0-9_]+)\s*\(", text))
    assert declared == set(NAMES) == {s for s in _lib.SYMBOLS if s.startswith("cpx_rs_")}
    lib = _lib.load()
    assert all(hasattr(lib, s) for s in NAMES)
    names = {"rs_genpoly", "RSCode", "rs_encode", "rs_decode"}
    assert names <= set(channelcoding.__all__) and all(callable(getattr(channelcoding, n)) for n in names)
    assert {"rs_encode_dev", "rs_decode_dev"} <= set(deviceops.__all__)
    from commpy_amd import build
    assert "rs.hip" in build.SOURCES


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def no_device(monkeypatch):
    """Any attempt to load the engine fails the test: the refusals below must come from the host-side checks."""
    def boom(*a, **k):
        raise AssertionError("the engine was touched")
    monkeypatch.setattr(_lib, "load", boom)


def test_python_refusals(no_device):
    code = RSCode(15, 11)
    assert RSCode(16383, 16320, m=14).nroots == 63 and RSCode(2, 1).m == 3 and RSCode(15, 11, fcr=14).fcr == 14        # accepted
    rx, z = np.zeros((2, 15), np.uint16), np.zeros
    for bad in (lambda: RSCode(1, 1), lambda: RSCode(15.0, 11), lambda: RSCode(True, 1), lambda: RSCode(15, 0), lambda: RSCode(15, 11.0),
                lambda: RSCode(15, 15), lambda: RSCode(15, 16), lambda: RSCode(255, 191), lambda: RSCode(3, 1, m=2), lambda: RSCode(15, 11, m=15),
                lambda: RSCode(16, 12, m=4), lambda: RSCode(16384, 16380), lambda: RSCode(40000, 39990, m=14), lambda: RSCode(15, 11, fcr=-1),
                lambda: RSCode(15, 11, fcr=15), lambda: RSCode(15, 11, fcr=1.0), lambda: RSCode(15, 11, prim_poly=31),
                lambda: RSCode(15, 11, prim_poly=37), lambda: RSCode(15, 11, prim_poly=19.0), lambda: RSCode(15, 11, m=4.0),
                lambda: rs_genpoly(4, 0), lambda: rs_genpoly(4, 15), lambda: rs_genpoly(4, 2, fcr=15), lambda: rs_genpoly(17, 2),
                lambda: rs_genpoly(4, 2, prim_poly=31),
                lambda: rs_encode(z((2, 10), np.uint16), code), lambda: rs_encode(z((2, 2, 11), np.uint16), code),
                lambda: rs_encode(np.full((2, 11), 16), code), lambda: rs_encode(np.full((2, 11), -1), code), lambda: rs_encode(z((2, 11)), code),
                lambda: rs_encode(z((2, 11), np.uint16), None), lambda: rs_encode(z((), np.uint16), code),
                lambda: rs_decode(z((2, 14), np.uint16), code), lambda: rs_decode(z((2, 2, 15), np.uint16), code),
                lambda: rs_decode(np.full((2, 15), 16), code), lambda: rs_decode(np.full((2, 15), -1), code), lambda: rs_decode(z((2, 15)), code),
                lambda: rs_decode(rx, None), lambda: rs_decode(rx, code, want=()), lambda: rs_decode(rx, code, want=("symbols", "word")),
                lambda: rs_decode(rx, code, want="bits"), lambda: rs_decode(rx, code, erasures=z((2, 14), bool)),
                lambda: rs_decode(rx, code, erasures=z(15, bool)), lambda: rs_decode(rx[0], code, erasures=z((1, 15), bool)),
                lambda: rs_decode(rx, code, erasures=z((2, 15))), lambda: rs_decode(z((0, 15), np.uint16), code, erasures=z((1, 15), bool)),
                lambda: deviceops.rs_encode_dev(code, None, -1), lambda: deviceops.rs_encode_dev(None, None, 2),
                lambda: deviceops.rs_decode_dev(code, None, 2, want="llr"), lambda: deviceops.rs_decode_dev(code, None, 2.0),
                lambda: deviceops.rs_decode_dev(None, None, 2)):
        with pytest.raises(ValueError):
            bad()
    # empty batches need no device
    assert rs_encode(z((0, 11), np.uint16), code).shape == (0, 15)
    assert rs_decode(z((0, 15), np.uint16), code).shape == (0, 11)
    sym, word, errors = rs_decode(z((0, 15), np.uint16), code, erasures=z((0, 15), bool), want=("errors", "codeword", "symbols"))
    assert sym.shape == (0, 11) and word.shape == (0, 15) and errors.shape == (0,)
    assert errors.dtype == np.int32 and sym.dtype == np.uint16 and word.dtype == np.uint16


def test_engine_checks_without_device():
    """The C entry points: argument errors are reported before the device is looked for; a valid call fails loudly without one."""
    lib = _lib.load()
    P, E, Lm = _lib.ptr, _lib.CPX_EINVAL, _lib.CPX_ELIMIT
    h = ctypes.c_void_p()
    g15 = rs_genpoly(4, 4).astype(np.uint16)

    def create(m=4, prim=19, n=15, k=11, fcr=1, g=g15, out=ctypes.byref(h)):
        return lib.cpx_rs_create(m, prim, n, k, fcr, None if g is None else P(g), out)

    def message(rc, code=E):
        assert rc == code, (rc, _lib.last_error())
        return _lib.last_error()

    assert "null pointer" in message(create(out=None)) and "null pointer" in message(create(g=None))
    assert "m = 2" in message(create(m=2, prim=7, n=3, k=1), Lm) and "m = 15" in message(create(m=15, prim=32771), Lm)
    assert "n = 16" in message(create(n=16, k=12), Lm) and "n = 1 " in message(create(n=1, k=1), Lm)
    assert "k = 0" in message(create(k=0)) and "k = 15" in message(create(k=15)) and "k = -1" in message(create(k=-1))
    big = rs_genpoly(8, 64).astype(np.uint16)
    assert "n - k = 64 is above the engine's limit of 63" in message(create(m=8, prim=285, n=255, k=191, g=big), Lm)
    assert "fcr = -1" in message(create(fcr=-1)) and "fcr = 15" in message(create(fcr=15))
    assert "has not degree" in message(create(prim=37)) and "has not degree" in message(create(prim=11))
    assert "not primitive" in message(create(prim=31)) and "order 5" in _lib.last_error()
    assert "not primitive" in message(create(prim=16))
    wide = g15.copy()
    wide[2] = 16
    assert "genpoly[2] = 16" in message(create(g=wide))
    for lead in (0, 2):                                           # not monic; a generator of another degree has another x^4 term
        bad = g15.copy()
        bad[4] = lead
        assert "coefficient of x^4 is %d" % lead in message(create(g=bad))
    low = np.concatenate([rs_genpoly(4, 3), [0]]).astype(np.uint16)
    assert "coefficient of x^4 is 0" in message(create(g=low))
    assert "does not vanish at alpha^0" in message(create(fcr=0))
    assert "does not vanish at alpha^5" in message(create(fcr=2))
    assert "does not vanish" in message(create(g=np.array([1, 0, 0, 0, 1], np.uint16)))
    assert h.value is None
    buf = np.zeros(1 << 10, np.uint16)
    for rc in (lib.cpx_rs_encode(None, P(buf), 1, P(buf)), lib.cpx_rs_encode_dev(None, P(buf), 0, P(buf), None),
               lib.cpx_rs_decode(None, P(buf), None, 1, P(buf), None, None),
               lib.cpx_rs_decode_dev(None, P(buf), None, 0, P(buf), None, None, None)):
        assert "null handle" in message(rc)
    assert lib.cpx_rs_destroy(None) == _lib.CPX_OK
    if _lib.device_count() > 0:
        return
    assert create() == _lib.CPX_ENODEV and _lib.last_error().startswith("no HIP device available") and h.value is None
    g10 = rs_genpoly(10, 30).astype(np.uint16)
    assert create(m=10, prim=1033, n=544, k=514, g=g10) == _lib.CPX_ENODEV
    assert create(m=4, fcr=0, g=rs_genpoly(4, 4, fcr=0).astype(np.uint16)) == _lib.CPX_ENODEV


def test_entry_points_fail_loudly_without_device():
    if _lib.device_count() > 0:
        pytest.skip("a HIP device is present")
    code = RSCode(15, 11)
    for call in (lambda: rs_encode(np.zeros((2, 11), np.uint16), code), lambda: rs_encode(np.zeros(11, np.uint16), code),
                 lambda: rs_decode(np.zeros((2, 15), np.uint16), code),
                 lambda: rs_decode(np.zeros(15, np.uint16), code, erasures=np.zeros(15, bool), want=("symbols", "errors")),
                 lambda: deviceops.rs_decode_dev(code, None, 2)):
        with pytest.raises(_lib.EngineError):
            call()
