"""Which kernel serves which Viterbi request: the exact ``cpx_last_kernel()`` note of every request below, as recorded from the
library BEFORE the host dispatch of csrc/viterbi.hip / csrc/viterbi_cw.hip was reorganised (tests/golden/viterbi_dispatch_names.json,
written by ``gen_viterbi_dispatch_names`` of tests/golden/make_golden.py, which calls ``record()`` below), and bit equality with the
CPU oracle.  A request that raised when the fixture was recorded must raise the same error.

Every request but one (DEEP_RING_TB) decodes B = 70 codewords of 40 message bits: ragged (more than one wave, no multiple of 64), shorter than one flush
chunk of 96 steps.  'soft' inputs carry one NaN codeword, so that the redo launch runs (cpx_last_kernel() does not name it)."""
import ctypes
import hashlib
import json
import os
import shutil

import numpy as np
import pytest

import oracle
from helpers import GOLDEN, make_trellis

B, NBITS = 70, 40
TYPES = ("hard", "soft", "unquantized")
NAMES_JSON = os.path.join(GOLDEN, "viterbi_dispatch_names.json")

# (memory, generators, polynomial format) of the trellises that helpers.TRELLIS_SPECS does not have
EXTRA = {
    "k7_171_133": (6, [0o171, 0o133], "MSB"), "k7_133_171_lsb": (6, [0o133, 0o171], "LSB"), "k7_171_133_lsb": (6, [0o171, 0o133], "LSB"),
    # both generators tap the input and the oldest register bit, not built in: the table-driven kernel, or the pair's code object
    "p3_15_17": (3, [0o15, 0o17], "MSB"), "p4_25_37": (4, [0o25, 0o37], "MSB"), "p5_53_75": (5, [0o53, 0o75], "MSB"),
    "p6_135_147": (6, [0o135, 0o147], "MSB"),
    # the first generator lacks the oldest-bit tap / the input tap (tests/test_viterbi_cw_gpu.py::test_table_driven_codes: bit 0 is
    # the oldest register bit, bit `memory` the input)
    "p6_136_147_no_oldest": (6, [0o136, 0o147], "MSB"), "p6_035_147_no_input": (6, [0o035, 0o147], "MSB"),
    "k9_561_753": (8, [0o561, 0o753], "MSB"), "k10_1167_1545": (9, [0o1167, 0o1545], "MSB"),
}
BUILTIN_64 = ("k7_133_171", "k7_171_133", "k7_133_171_lsb", "k7_171_133_lsb", "wifi_decimal_133_171")
BUILTIN_SMALL = ("t57", "k5_23_35")
END_TAP = ("p3_15_17", "p4_25_37", "p5_53_75", "p6_135_147")
NO_END_TAP = ("p6_136_147_no_oldest", "p6_035_147_no_input")
# rate 1/3 (n = 3 wave template); k = 2 (I = 4); recursive (table traceback); 128 and 256 states (wide kernel); 512 states (general)
OTHER = ("r13_k4", "k2_default", "rsc_legacy_4", "k8_247_371", "k9_561_753", "k10_1167_1545")
# 64 states: a traceback ring of 8192 slots, 9 B each, exceeds 64 KiB of LDS -> general kernel.  This one request decodes 4200 message
# bits: with 40, the depth lies beyond the block's end, where the engine documents that it does not follow the reference (one
# full-length traceback, convcode.viterbi_decode) and so differs from the oracle
DEEP_RING_TB, DEEP_RING_NBITS = 4100, 4200

_trellis_cache, _input_cache = {}, {}


def trellis(name, specialised=False):
    key = (name, specialised)
    if key not in _trellis_cache:
        if name in EXTRA:
            from commpy_amd.channelcoding import Trellis
            mem, g, fmt = EXTRA[name]
            _trellis_cache[key] = Trellis(np.array([mem]), np.array([g]), polynomial_format=fmt)
        else:
            _trellis_cache[key] = make_trellis(name)
    return _trellis_cache[key]


def depth(name, label):
    if label == "default":
        return None
    d = 5 * trellis(name).total_memory
    return {"default-1": d - 1, "default+1": d + 1}.get(label) or int(label)


def requests(name):
    """(path, decoding type, depth label, flag) of every request on trellis `name`; flag: '' | 'f32' (fp32-fast) | 'spec' (after
    Trellis.specialize())."""
    out = []
    if name in BUILTIN_64 or name in BUILTIN_SMALL:
        depths = ["default", "2", "default-1", "default+1"] + (["48", "49"] if name in BUILTIN_64 else [])
        out += [(p, t, d, "") for p in ("cw!", "cw2!", "wave", "general") for t in TYPES for d in depths]
    if name == "k7_133_171":
        out += [(p, t, "default", "f32") for p in ("cw!", "auto") for t in TYPES]
        out += [("auto", t, str(DEEP_RING_TB), "") for t in TYPES]
    if name in END_TAP:
        out += [("cw!", t, d, f) for f in ("", "spec") for t in TYPES for d in ("default", "default-1")]
    if name == "p6_135_147":
        out += [(p, t, "default", "f32") for p in ("cw!", "cw", "auto") for t in TYPES]
    if name in NO_END_TAP:
        out += [(p, t, "default", "") for p in ("cw!", "cw", "auto") for t in TYPES]
    if name in OTHER:
        out += [("auto", t, "default", "") for t in TYPES]
    return out


ALL = BUILTIN_64 + BUILTIN_SMALL + END_TAP + NO_END_TAP + OTHER


def key_of(name, req):
    return "|".join((name,) + req)


def inputs(name, dtype, tb):
    """(received values, the oracle's bits) -- computed once per trellis, type and depth, shared by every path."""
    k = (name, dtype, tb)
    if k not in _input_cache:
        from commpy_amd.channelcoding import conv_encode_batch
        tr = trellis(name)
        rs = np.random.RandomState(len(name) * 7 + TYPES.index(dtype))
        coded = conv_encode_batch(rs.randint(0, 2, (B, DEEP_RING_NBITS if tb == DEEP_RING_TB else NBITS)), tr).astype(float)
        if dtype == "hard":
            rx = np.where(rs.rand(*coded.shape) < 0.08, 1 - coded, coded)
        elif dtype == "soft":
            rx = 4.0 * coded - 2 + rs.randn(*coded.shape) * 2.0
            rx[B // 2, 7] = np.nan
        else:
            rx = 2.0 * coded - 1 + rs.randn(*coded.shape) * 0.8
        rx.setflags(write=False)
        _input_cache[k] = (rx, oracle.viterbi_decode(rx, tr, tb, dtype))
    return _input_cache[k]


def observe(name, req):
    """What the library does with one request: {'note': cpx_last_kernel(), 'oracle': bits equal the oracle's, 'sha1': of the bits}
    or {'raises': 'Type: message'}."""
    import commpy_amd
    from commpy_amd import _lib
    from commpy_amd.channelcoding import viterbi_decode
    path, dtype, dlabel, flag = req
    tb = depth(name, dlabel)
    tr = trellis(name, flag == "spec")
    rx, want = inputs(name, dtype, tb)
    try:
        with commpy_amd.precision("fp32-fast" if flag == "f32" else "fp64-parity"), \
                _lib.forced_path("viterbi", None if path == "auto" else path):
            got = viterbi_decode(rx, tr, tb, dtype)
            note = _lib.last_kernel()
    except (ValueError, _lib.EngineError) as exc:
        return {"raises": "%s: %s" % (type(exc).__name__, exc)}
    return {"note": note, "oracle": bool(np.array_equal(got, want)), "sha1": hashlib.sha1(np.ascontiguousarray(got).tobytes()).hexdigest()}


def spec_query(name):
    from commpy_amd import _lib
    lg, g0, g1 = ctypes.c_int(-1), ctypes.c_uint(0), ctypes.c_uint(0)
    _lib.check(_lib.load().cpx_trellis_viterbi_spec_query(trellis(name)._device_handle(), ctypes.byref(lg), ctypes.byref(g0), ctypes.byref(g1)))
    return [lg.value, g0.value, g1.value]


def demod_hard(name):
    """The fused hard-demodulation entry point, cpx_demod_hard_viterbi_batch, called directly (16-QAM)."""
    from commpy_amd import _lib
    from commpy_amd.channelcoding import conv_encode_batch
    from commpy_amd.channelcoding.convcode import _viterbi_sizes
    from commpy_amd.modulation import QAMModem
    tr, md = trellis(name), QAMModem(16)
    rs = np.random.RandomState(len(name))
    coded = conv_encode_batch(rs.randint(0, 2, (B, NBITS)), tr)
    coded = coded[:, :coded.shape[1] // 4 * 4]
    y = md.modulate(coded.reshape(-1)).reshape(B, -1)
    y = np.ascontiguousarray(y + 0.35 * (rs.randn(*y.shape) + 1j * rs.randn(*y.shape)))
    length = y.shape[1] * 4
    L, T, tb = _viterbi_sizes(length, tr, None)
    out = np.zeros((B, L), dtype=np.uint8)
    try:
        _lib.check(_lib.load().cpx_demod_hard_viterbi_batch(md._device_handle(), tr._device_handle(), _lib.ptr(y), B, y.shape[1], L, T, tb,
                                                            _lib.ptr(out)))
        note = _lib.last_kernel()
    except (ValueError, _lib.EngineError) as exc:
        return {"raises": "%s: %s" % (type(exc).__name__, exc)}
    bits = md.demodulate(y.reshape(-1), "hard").reshape(B, length)
    return {"note": note, "oracle": bool(np.array_equal(out, oracle.viterbi_decode(bits, tr, None, "hard"))),
            "sha1": hashlib.sha1(out.tobytes()).hexdigest()}


def specialise(name):
    """True when the 'spec' requests of `name` can run: the trellis carries its pair's code object."""
    return bool(trellis(name, True).specialize())


def record():
    """The fixture's content, from the library that is loaded (needs the GPU)."""
    names = {}
    for name in ALL:
        can_spec = name in END_TAP and specialise(name)
        for req in requests(name):
            if req[3] != "spec" or can_spec:
                names[key_of(name, req)] = observe(name, req)
    return {"what": "cpx_last_kernel() per request of tests/test_viterbi_dispatch_gpu.py, recorded before the dispatch refactor",
            "names": names, "spec_query": {name: spec_query(name) for name in ALL},
            "demod_hard": {name: demod_hard(name) for name in ("k7_133_171", "k8_247_371")}}


def fixture():
    with open(NAMES_JSON) as f:
        return json.load(f)


def test_fixture_holds_every_request():
    """Every listed request either decoded (a non-empty note, the oracle's bits unless fp32-fast) or raised when it was recorded."""
    fx = fixture()
    for name in ALL:
        for req in requests(name):
            rec = fx["names"][key_of(name, req)]
            assert rec.get("note") or rec.get("raises"), (name, req)
            assert "raises" in rec or rec["oracle"] or req[3] == "f32", (name, req)
        assert len(fx["spec_query"][name]) == 3
    for rec in fx["demod_hard"].values():
        assert rec.get("note") or rec.get("raises")


def _check(name, flags):
    fx = fixture()["names"]
    bad = []
    for req in requests(name):
        if req[3] in flags:
            got, want = observe(name, req), fx[key_of(name, req)]
            print(key_of(name, req), got)
            if got != want:
                bad.append((key_of(name, req), got, want))
    assert not bad, bad[:5]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ALL)
def test_request_takes_the_recorded_kernel(gpu, name):
    _check(name, ("", "f32"))


@pytest.mark.gpu
@pytest.mark.parametrize("name", END_TAP)
def test_specialised_pair_takes_its_code_object(gpu, name):
    if not specialise(name):
        from commpy_amd import build, jit
        if shutil.which(build._hipcc()) is None:
            pytest.skip("no hipcc here")
        pytest.fail("no code object: %s" % jit.viterbi_code_object.last_error)
    _check(name, ("spec",))
    for req in requests(name):
        if req[3] == "spec":
            assert "code object of this pair" in fixture()["names"][key_of(name, req)]["note"]


@pytest.mark.gpu
def test_spec_query_is_unchanged(gpu):
    assert {name: spec_query(name) for name in ALL} == fixture()["spec_query"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["k7_133_171", "k8_247_371"])
def test_fused_hard_demodulation(gpu, name):
    got, want = demod_hard(name), fixture()["demod_hard"][name]
    print(name, got)
    assert got == want
    assert ("raises" in got) == (name == "k8_247_371")
