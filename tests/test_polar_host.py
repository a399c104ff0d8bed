"""Host side of the polar codec: the NumPy model (tests/polar_model.py) against the Kronecker matrix, bitwise long division and its own
invariants; code construction and the CRC helpers of commpy_amd.channelcoding.polar; the C-ABI's names; every refusal (ValueError /
CPX_EINVAL before any device is touched) and the loud failure without a device."""
import ctypes
import os
import re

import numpy as np
import pytest

import polar_model as M
from commpy_amd import _lib, channelcoding, deviceops
from commpy_amd.channelcoding import (PolarCode, crc_append, crc_check, polar_decode, polar_encode, polar_reliability_order)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["cpx_polar_create", "cpx_polar_destroy", "cpx_polar_encode", "cpx_polar_encode_dev", "cpx_polar_decode", "cpx_polar_decode_dev"]
CRCS = {6: 0x61, 11: 0xE21, 16: 0x11021, 24: 0x1B2B117}
# block errors of the model on the seeded (128, 64 + CRC-11) set, 150 words at Eb/N0 = 3 dB (M.awgn_llrs(SET_SEED, ...)): SC, SCL-8 judged
# on all 64 information bits; CRC-aided SCL-8 judged on the 53 message bits.  tests/test_polar_gpu.py holds the engine to the same counts.
SET_SEED, SET_WORDS, SET_EBN0 = 1, 150, 3.0
MODEL_BLOCK_ERRORS = {"sc": 17, "scl8": 3, "ca_scl8": 1}


def block_errors(decode):
    """``decode(llr, L, with_crc) -> bits`` on the seeded set: the three counts of MODEL_BLOCK_ERRORS."""
    fz, g = M.frozen_mask(128, 64), CRCS[11]
    msg, llr = M.awgn_llrs(SET_SEED, fz, g, SET_WORDS, SET_EBN0)
    full = np.stack([M.info_bits(m, 64, g) for m in msg])
    return {"sc": int((decode(llr, 1, False) != full).any(axis=1).sum()), "scl8": int((decode(llr, 8, False) != full).any(axis=1).sum()),
            "ca_scl8": int((decode(llr, 8, True) != msg).any(axis=1).sum())}


# ---- the model ----------------------------------------------------------------------------------------------------------------------
def test_model_encoder_is_the_kronecker_product():
    rs = np.random.RandomState(0)
    for N in (2, 4, 8, 64, 256):
        u = rs.randint(0, 2, (6, N)).astype(np.uint8)
        assert np.array_equal(M.transform(u), u.astype(np.int64) @ M.kron_matrix(N) % 2)
    fz = M.frozen_mask(8, 4)
    assert list(np.flatnonzero(fz == 0)) == [3, 5, 6, 7]
    assert np.array_equal(M.encode([1, 0, 1, 1], fz), np.array([0, 0, 0, 1, 0, 0, 1, 1]) @ M.kron_matrix(8) % 2)


@pytest.mark.parametrize("c", sorted(CRCS))
def test_crc_against_long_division(c):
    g = CRCS[c]
    rs = np.random.RandomState(c)
    for A in (1, 7, 53, 200):
        m = rs.randint(0, 2, (5, A)).astype(np.uint8)
        out = crc_append(m, g)
        assert out.shape == (5, A + c) and out.dtype == np.uint8 and np.array_equal(out[:, :A], m)
        for i in range(5):
            assert np.array_equal(out[i, A:], M.crc_long_division(m[i], g))
            assert np.array_equal(out[i], M.info_bits(m[i], A + c, g))
            assert np.array_equal(crc_append(m[i], g), out[i]) and crc_check(out[i], g) is True
        assert crc_check(out, g).all()
        for i in range(5):
            bad = out.copy()
            bad[i, rs.randint(A + c)] ^= 1
            ok = crc_check(bad, g)
            assert not ok[i] and ok.sum() == 4
        assert np.array_equal(PolarCode(512, A + c, crc=g).crc_table, M.crc_table(g, A + c))
    assert crc_append(np.zeros((0, 9), np.uint8), g).shape == (0, 9 + c)


def test_reliability_order():
    assert list(polar_reliability_order(8)) == [0, 1, 2, 4, 3, 5, 6, 7]
    N = 2
    while N <= 8192:
        od = polar_reliability_order(N)
        assert od.shape == (N,) and np.array_equal(np.sort(od), np.arange(N)) and od[0] == 0 and od[-1] == N - 1
        if N <= 1024:
            assert np.array_equal(od, M.reliability_order(N))
        N *= 2
    code = PolarCode(8, 4)
    assert (code.N, code.K, code.A) == (8, 4, 4) and list(code.info_positions) == [3, 5, 6, 7] and list(code.frozen) == [1, 1, 1, 0, 1, 0, 0, 0]
    assert code.crc_table is None
    code = PolarCode(32, 20, crc=CRCS[6])
    assert code.A == 14 and code.crc_table.dtype == np.uint32 and code.crc_table.shape == (20,)
    assert np.array_equal(PolarCode(8, 3, order=[7, 6, 5, 4, 3, 2, 1, 0]).info_positions, [0, 1, 2])
    assert np.array_equal(PolarCode(8, 2, frozen=[0, 1, 1, 1, 1, 1, 1, 0]).info_positions, [0, 7])


@pytest.mark.parametrize("N, K", [(8, 4), (32, 16), (128, 64), (128, 100)])
def test_model_decodes_noise_free_words(N, K):
    rs = np.random.RandomState(N + K)
    fz = M.frozen_mask(N, K)
    for L in (1, 2, 4, 8, 16, 32):
        m = rs.randint(0, 2, K).astype(np.uint8)
        r = M.decode(4.0 * (1.0 - 2.0 * M.encode(m, fz)), fz, L)
        assert np.array_equal(r["bits"], m) and r["crc_ok"] == 1 and r["metric"] == 0.0 and r["live"] == min(L, 2 ** K)
        assert np.array_equal(r["list_bits"][0], m)


def test_model_lists_are_sorted_and_hold_ties():
    fz = M.frozen_mask(128, 64)
    ties = 0
    for llr in M.sign_llrs(5, 6, 128):
        r = M.decode(llr, fz, 8)
        assert r["live"] == 8 and np.all(np.diff(r["list_metric"]) >= 0)
        assert len({row.tobytes() for row in r["list_bits"]}) == 8
        ties += int((np.diff(r["list_metric"]) == 0).sum())
    assert ties >= 6, ties                                   # the GPU test that reuses this input tests the tie rule
    r = M.decode(np.random.RandomState(0).randn(16), M.frozen_mask(16, 2), 8, None)
    assert r["live"] == 4 and np.all(r["list_metric"][4:] == np.inf) and not r["list_bits"][4:].any()
    assert np.all(np.diff(r["list_metric"][:4]) >= 0)
    # SC is the list decoder of size 1: u = (lambda < 0) at the information positions, 0 elsewhere
    llr = np.random.RandomState(1).randn(64) + 0.5
    fz = M.frozen_mask(64, 30)
    a = M.decode(llr, fz, 1)
    assert a["u_llr"].shape == (64,) and M.decode(llr, fz, 2)["u_llr"] is None
    pm = 0.0
    for v in a["u_llr"][(fz == 1) & (a["u_llr"] < 0)]:
        pm = pm + abs(v)
    assert np.array_equal(a["bits"], (a["u_llr"] < 0)[fz == 0]) and a["metric"] == pm


def test_model_block_errors_on_the_seeded_set():
    def model(llr, L, with_crc):
        return M.decode_batch(llr, M.frozen_mask(128, 64), L, CRCS[11] if with_crc else None)["bits"]
    got = block_errors(model)
    assert got == MODEL_BLOCK_ERRORS, got
    assert got["ca_scl8"] < got["sc"]


# ---- names --------------------------------------------------------------------------------------------------------------------------
def test_abi_names():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "commpy_amd.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(cpx_polar_[a-z0-9_]+)\s*\(", text))
    assert declared == set(NAMES) == {s for s in _lib.SYMBOLS if s.startswith("cpx_polar_")}
    lib = _lib.load()
    assert all(hasattr(lib, s) for s in NAMES)
    names = {"polar_reliability_order", "PolarCode", "crc_append", "crc_check", "polar_encode", "polar_decode"}
    assert names <= set(channelcoding.__all__) and all(callable(getattr(channelcoding, n)) for n in names)
    assert {"polar_encode_dev", "polar_decode_dev"} <= set(deviceops.__all__)
    from commpy_amd import build
    assert "polar.hip" in build.SOURCES


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def no_device(monkeypatch):
    """Any attempt to load the engine fails the test: the refusals below must come from the host-side checks."""
    def boom(*a, **k):
        raise AssertionError("the engine was touched")
    monkeypatch.setattr(_lib, "load", boom)


def test_python_refusals(no_device):
    code, crc_code = PolarCode(64, 32), PolarCode(64, 32, crc=CRCS[11])
    big = PolarCode(1024, 512)
    llr = np.zeros((2, 64))
    for bad in (lambda: PolarCode(48, 8), lambda: PolarCode(1, 1), lambda: PolarCode(0, 0), lambda: PolarCode(64.0, 8), lambda: PolarCode(True, 1),
                lambda: PolarCode(16384, 8), lambda: PolarCode(64, 0), lambda: PolarCode(64, 65), lambda: PolarCode(64, 8.0),
                lambda: PolarCode(64, 11, crc=CRCS[11]), lambda: PolarCode(64, 6, crc=CRCS[6]), lambda: PolarCode(64, 40, crc=1 << 33 | 1),
                lambda: PolarCode(64, 40, crc=1), lambda: PolarCode(64, 40, crc=0x60), lambda: PolarCode(64, 40, crc=-5), lambda: PolarCode(64, 40, crc=2.5),
                lambda: PolarCode(8, 4, order=[0, 1, 2, 3]), lambda: PolarCode(8, 4, order=[0, 1, 2, 3, 4, 5, 6, 6]), lambda: PolarCode(8, 4, order=np.arange(8.0)),
                lambda: PolarCode(8, 4, frozen=[1, 1, 1, 0, 1, 0, 0]), lambda: PolarCode(8, 4, frozen=[1, 1, 1, 1, 1, 0, 0, 0]),
                lambda: PolarCode(8, 4, frozen=[2, 1, 1, 0, 1, 0, 0, 0]), lambda: PolarCode(8, 4, order=np.arange(8), frozen=[1, 1, 1, 0, 1, 0, 0, 0]),
                lambda: polar_reliability_order(12), lambda: polar_reliability_order(0),
                lambda: polar_encode(np.zeros((2, 31), np.uint8), code), lambda: polar_encode(np.zeros((2, 32), np.uint8), crc_code),
                lambda: polar_encode(np.zeros((2, 2, 32), np.uint8), code), lambda: polar_encode(np.full((2, 32), 2), code),
                lambda: polar_encode(np.zeros((2, 32)), code), lambda: polar_encode(np.zeros((2, 32), np.uint8), None),
                lambda: polar_decode(np.zeros((2, 63)), code), lambda: polar_decode(np.zeros((2, 2, 64)), code), lambda: polar_decode(np.zeros(()), code),
                lambda: polar_decode(np.zeros((2, 64), complex), code), lambda: polar_decode(llr, None),
                lambda: polar_decode(llr, code, list_size=3), lambda: polar_decode(llr, code, list_size=0), lambda: polar_decode(llr, code, list_size=64),
                lambda: polar_decode(llr, code, list_size=2.0), lambda: polar_decode(np.zeros((1, 1024)), big, list_size=16),
                lambda: polar_decode(llr, code, list_size=2, want=("bits", "u_llr")), lambda: polar_decode(llr, code, want=()),
                lambda: polar_decode(llr, code, want=("bits", "llr")), lambda: polar_decode(llr, code, want="nothing"),
                lambda: crc_append(np.zeros((2, 2, 4), np.uint8), CRCS[6]), lambda: crc_append(np.zeros(4), CRCS[6]), lambda: crc_append([0, 3], CRCS[6]),
                lambda: crc_append([0, 1], 0), lambda: crc_check(np.zeros(6, np.uint8), CRCS[6]), lambda: crc_check(np.zeros(9, np.uint8), None),
                lambda: deviceops.polar_encode_dev(code, None, -1), lambda: deviceops.polar_decode_dev(code, None, 2, list_size=5),
                lambda: deviceops.polar_decode_dev(code, None, 2, list_size=2, want="u_llr"), lambda: deviceops.polar_decode_dev(None, None, 2)):
        with pytest.raises(ValueError):
            bad()
    # empty batches need no device
    assert polar_encode(np.zeros((0, 32), np.uint8), code).shape == (0, 64)
    assert polar_decode(np.zeros((0, 64)), crc_code, 4).shape == (0, 21)
    bits, (lb, lm, live) = polar_decode(np.zeros((0, 64)), code, 4, want=("list", "bits"))
    assert bits.shape == (0, 32) and lb.shape == (0, 4, 32) and lm.shape == (0, 4) and live.shape == (0,)


def test_engine_checks_without_device():
    """The C entry points: argument errors are reported before the device is looked for; a valid call fails loudly without one."""
    lib = _lib.load()
    P, E, Lm = _lib.ptr, _lib.CPX_EINVAL, _lib.CPX_ELIMIT
    h = ctypes.c_void_p()
    fz = M.frozen_mask(64, 32)
    tab = M.crc_table(CRCS[11], 32)

    def create(N=64, mask=fz, c=11, table=tab, out=ctypes.byref(h)):
        return lib.cpx_polar_create(N, None if mask is None else P(mask), c, None if table is None else P(table), out)

    def message(rc):
        assert rc == E, rc
        return _lib.last_error()

    assert "null pointer" in message(create(out=None)) and "null pointer" in message(create(mask=None))
    assert "power of two" in message(create(N=48)) and "power of two" in message(create(N=1)) and "power of two" in message(create(N=0))
    assert create(N=16384) == Lm
    two = fz.copy()
    two[5] = 2
    assert "frozen[5] = 2" in message(create(mask=two))
    assert "every position is frozen" in message(create(mask=np.ones(64, np.uint8)))
    assert "crc_bits = 33" in message(create(c=33)) and "crc_bits = -1" in message(create(c=-1))
    assert "fewer than the K = 32" in message(create(c=32, table=M.crc_table(1 << 32 | 0x04C11DB7, 32)))
    assert "CRC table" in message(create(c=0)) and "CRC table" in message(create(table=None))
    bad = tab.copy()
    bad[3] = 0
    assert "crc_table[3]" in message(create(table=bad))
    bad = tab.copy()
    bad[3] |= 1 << 11
    assert "crc_table[3]" in message(create(table=bad))
    bad = tab.copy()
    bad[30] = 5
    assert "crc_table[30]" in message(create(table=bad)) and "x^1" in _lib.last_error()
    assert h.value is None
    buf = np.zeros(1 << 12)
    # null handle; empty batches succeed without a device, in both forms
    for rc in (lib.cpx_polar_encode(None, P(buf), 1, P(buf)), lib.cpx_polar_encode_dev(None, P(buf), 0, P(buf), None),
               lib.cpx_polar_decode(None, P(buf), 1, 1, P(buf), None, None, None, None, None, None),
               lib.cpx_polar_decode_dev(None, P(buf), 0, 1, P(buf), None, None, None, None, None, None, None)):
        assert "null handle" in message(rc)
    assert lib.cpx_polar_destroy(None) == _lib.CPX_OK
    if _lib.device_count() > 0:
        return
    assert create() == _lib.CPX_ENODEV and _lib.last_error().startswith("no HIP device available") and h.value is None
    assert create(c=0, table=None) == _lib.CPX_ENODEV


def test_entry_points_fail_loudly_without_device():
    if _lib.device_count() > 0:
        pytest.skip("a HIP device is present")
    code = PolarCode(64, 32, crc=CRCS[11])
    for call in (lambda: polar_encode(np.zeros((2, 21), np.uint8), code), lambda: polar_encode(np.zeros(21, np.uint8), code),
                 lambda: polar_decode(np.zeros((2, 64)), code), lambda: polar_decode(np.zeros(64), code, 8, want=("bits", "list")),
                 lambda: deviceops.polar_decode_dev(code, None, 2)):
        with pytest.raises(_lib.EngineError):
            call()
