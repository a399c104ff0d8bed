"""Which kernel serves which demodulator request, and what it computes: the exact ``cpx_last_kernel()`` note and the SHA-1 of the
output bytes of every request below, as recorded from the library BEFORE the host dispatch of csrc/demod.hip was reorganised
(tests/golden/demod_dispatch_names.json, written by ``gen_demod_dispatch_names`` of tests/golden/make_golden.py, which calls
``record()`` below).  A request that raised when the fixture was recorded must raise the same error.  Bit equality is the right bar:
the reorganisation leaves every kernel as it was.

Soft requests go to ``cpx_demod_soft_scaled_dev`` on NS = 325 symbols (two blocks, six waves, the last one ragged, an odd count: the
scalar tail store of the transposed kernels runs) or on one symbol.  The symbols are constellation points plus noise; symbol NAN_AT
has a NaN component and symbol FAR_AT lies 1e3 away from every point, so the point-by-point redo runs in every kernel family.  The
output buffer is one element longer than the result and pre-filled; all of it is hashed, so a store past the end shows too."""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest

from helpers import GOLDEN

NAMES_JSON = os.path.join(GOLDEN, "demod_dispatch_names.json")
NS, NAN_AT, FAR_AT = 325, 37, 300
MODES = ("auto", "plain", "libm")
PRECISIONS = ("fp64-parity", "fp32-fast")
NOISE_VARS = ("0.1", "1e-300", "1e300", "1e-31", "1e31", "-0.1")   # rcp off: 1e-300, 1e300; outside the fp32 window: 1e-31, 1e31
ALIGN = ("aligned", "offset")                                      # output pointer 16-byte aligned / 8 bytes (hard: 1 byte) past that
QAMS = ("qam4", "qam16", "qam64", "qam256")
MODEMS = ("psk2", "psk4", "psk8", "psk16") + QAMS + ("custom32", "grid16_unequal", "grid16_repeated", "table512", "grid64_unequal")
SENTINEL = -7.25

_modem_cache, _input_cache = {}, {}


def _grid(xs, ys):
    """label (a << nh) | b -> xs[a] + 1j ys[b]: what the library recognises as axis-separable."""
    return (np.asarray(xs, dtype=float)[:, None] + 1j * np.asarray(ys, dtype=float)[None, :]).reshape(-1)


def modem(name):
    if name not in _modem_cache:
        from commpy_amd.modulation import Modem, PSKModem, QAMModem
        if name.startswith("psk"):
            md = PSKModem(int(name[3:]))
        elif name.startswith("qam"):
            md = QAMModem(int(name[3:]))
        else:
            pts = {
                # two rings of 16: five bits per symbol, an odd NB
                "custom32": lambda: np.concatenate([r * np.exp(2j * np.pi * (np.arange(16) + 0.25 * r) / 16) for r in (1.0, 2.0)]),
                "grid16_unequal": lambda: _grid([-3.0, -1.0, 1.5, 4.0], [-2.5, -1.0, 1.0, 3.5]),      # separable, no progression
                "grid16_repeated": lambda: _grid([-3.0, -1.0, -1.0, 3.0], [-3.0, -1.0, 1.0, 3.0]),    # a repeated level: generic
                "table512": lambda: _grid(np.arange(16) - 7.5, np.arange(32) - 15.5),                  # above the LDS kernels' 256
                # eight levels per axis in Gray order, unequal steps: separable where QAM-64 takes the progression
                "grid64_unequal": lambda: _grid(np.array([-7, -5, -3, -1, 1, 3, 5, 7.5])[_gray(8)], np.array([-7, -5, -3, -1, 1, 3, 5, 7.5])[_gray(8)]),
            }[name]()
            md = Modem(pts, reorder_as_gray=False)
        _modem_cache[name] = md
    return _modem_cache[name]


def _gray(r):
    """position -> index such that level j carries label j ^ (j >> 1)"""
    j = np.arange(r)
    return (j ^ (j >> 1)).argsort()


def symbols(name):
    """The NS received symbols of modem `name` (read-only, shared by every request on it)."""
    if name not in _input_cache:
        c = modem(name).constellation
        rs = np.random.RandomState(100 + MODEMS.index(name))
        y = c[rs.randint(0, len(c), NS)] + 0.3 * (rs.randn(NS) + 1j * rs.randn(NS))
        y[NAN_AT] = complex(np.nan, y[NAN_AT].imag)
        y[FAR_AT] = y[FAR_AT] + 1e3 * (1 + 1j)
        y.setflags(write=False)
        _input_cache[name] = y
    return _input_cache[name]


def soft_requests(name):
    """(mode, precision, noise_var, scale, alignment, Ns) of every soft request on modem `name`: the product of the factors, without
    the combinations in which a factor cannot matter -- `scale` is a kernel argument and takes part in the choice only through
    isfinite() under fp32-fast, so -1.0 and inf go with noise_var 0.1 alone; the one-symbol requests go with noise_var 0.1 and scale
    1.0; a table of more than 256 points has one kernel, whatever the mode."""
    out = []
    for mode in (MODES if name != "table512" else ("auto",)):
        for prec in PRECISIONS:
            for al in ALIGN:
                out += [(mode, prec, nv, "1.0", al, str(NS)) for nv in NOISE_VARS]
                out += [(mode, prec, "0.1", sc, al, str(NS)) for sc in (("-1.0", "inf") if prec == "fp32-fast" else ("-1.0",))]
                out.append((mode, prec, "0.1", "1.0", al, "1"))
    return out


def hard_requests(name):
    return [(al, ns) for al in ALIGN for ns in (str(NS), "1")]


# the fused front end: mode, precision, noise_var -- the default and the three calls it refuses
FRONT_REQUESTS = (("auto", "fp64-parity", "0.1"), ("plain", "fp64-parity", "0.1"), ("auto", "fp32-fast", "0.1"), ("auto", "fp64-parity", "1e-300"))
FRONT_T, FRONT_NBITS = 5, 24


def key_of(name, req):
    return "|".join((name,) + tuple(req))


def _run(fn, mode, prec):
    """fn() under a demodulator mode and a precision -> its record, or the error it raised."""
    import commpy_amd
    from commpy_amd import _lib
    try:
        with commpy_amd.precision(prec), _lib.forced_path("demod", None if mode == "auto" else mode):
            return fn()
    except (ValueError, _lib.EngineError) as exc:
        return {"raises": "%s: %s" % (type(exc).__name__, exc)}


def _sha1(arr):
    return hashlib.sha1(np.ascontiguousarray(arr).tobytes()).hexdigest()


def observe_soft(name, req):
    from commpy_amd import _lib
    from commpy_amd.deviceops import DeviceBuf
    mode, prec, nv, sc, al, ns = req
    ns = int(ns)
    md = modem(name)
    n_out = ns * md.num_bits_symbol + 1                           # one spare element: room for the 8-byte offset
    d_y = DeviceBuf.from_array(symbols(name)[:ns])
    d_out = DeviceBuf.from_array(np.full(n_out, SENTINEL))
    out_ptr = ctypes.c_void_p(d_out.ptr.value + (8 if al == "offset" else 0))

    def call():
        lib = _lib.load()
        _lib.check(lib.cpx_demod_soft_scaled_dev(md._device_handle(), d_y.ptr, ns, float(nv), float(sc), out_ptr, None))
        note = _lib.last_kernel()
        _lib.check(lib.cpx_stream_sync(None))
        return {"note": note, "sha1": _sha1(d_out.to_array((n_out,), np.float64))}
    try:
        return _run(call, mode, prec)
    finally:
        d_y.free()
        d_out.free()


def observe_hard(name, req):
    from commpy_amd import _lib
    from commpy_amd.deviceops import DeviceBuf
    al, ns = req
    ns = int(ns)
    md = modem(name)
    n_out = ns * md.num_bits_symbol + 1
    d_y = DeviceBuf.from_array(symbols(name)[:ns])
    d_out = DeviceBuf.from_array(np.full(n_out, 0x55, dtype=np.int8))
    out_ptr = ctypes.c_void_p(d_out.ptr.value + (1 if al == "offset" else 0))

    def call():
        lib = _lib.load()
        _lib.check(lib.cpx_demod_hard_dev(md._device_handle(), d_y.ptr, ns, out_ptr, None))
        note = _lib.last_kernel()
        _lib.check(lib.cpx_stream_sync(None))
        return {"note": note, "sha1": _sha1(d_out.to_array((n_out,), np.int8))}
    try:
        return _run(call, "auto", "fp64-parity")
    finally:
        d_y.free()
        d_out.free()


def _front_trellis():
    if "front" not in _modem_cache:
        from commpy_amd.channelcoding import Trellis
        _modem_cache["front"] = Trellis(np.array([2]), np.array([[0o5, 0o7]]))    # K = 3, feed-forward
    return _modem_cache["front"]


def _front_create(name):
    """cpx_link_front* for FRONT_NBITS message bits per transmission through modem `name`, rate 1/2, no puncturing."""
    from commpy_amd import _lib
    h = ctypes.c_void_p()
    ntx = 2 * FRONT_NBITS
    _lib.check(_lib.load().cpx_link_front_create(_front_trellis()._device_handle(), modem(name)._device_handle(), FRONT_NBITS, None, ntx,
                                                 None, ntx, ctypes.byref(h)))
    return h


def observe_front(name, req):
    """One fused front-end launch: note, SHA-1 of the message bits and of the LLRs."""
    from commpy_amd import _lib
    from commpy_amd.deviceops import DeviceBuf
    mode, prec, nv = req
    nv = float(nv)
    nde = 2 * FRONT_NBITS
    lib = _lib.load()
    d_msg = DeviceBuf.from_array(np.full(FRONT_T * FRONT_NBITS, 0x55, dtype=np.uint8))
    d_llr = DeviceBuf.from_array(np.full(FRONT_T * nde, SENTINEL))
    handle = []

    def call():
        handle.append(_front_create(name))
        std = np.sqrt(abs(nv))
        _lib.check(lib.cpx_link_front_run_dev(handle[0], FRONT_T, nv, std * 0.5, std * 0.5, 1.0, 11, 2, 3, d_msg.ptr, d_llr.ptr, None, None))
        note = _lib.last_kernel()
        _lib.check(lib.cpx_stream_sync(None))
        return {"note": note, "msg_sha1": _sha1(d_msg.to_array((FRONT_T * FRONT_NBITS,), np.uint8)),
                "llr_sha1": _sha1(d_llr.to_array((FRONT_T * nde,), np.float64))}
    try:
        return _run(call, mode, prec)
    finally:
        for h in handle:
            lib.cpx_link_front_destroy(h)
        d_msg.free()
        d_llr.free()


def record():
    """The fixture's content, from the library that is loaded (needs the GPU)."""
    return {"what": "cpx_last_kernel() and SHA-1 of the output per request of tests/test_demod_dispatch_gpu.py, recorded before the dispatch refactor",
            "soft": {key_of(n, r): observe_soft(n, r) for n in MODEMS for r in soft_requests(n)},
            "hard": {key_of(n, r): observe_hard(n, r) for n in MODEMS for r in hard_requests(n)},
            "front": {key_of(n, r): observe_front(n, r) for n in QAMS + ("grid64_unequal",) for r in FRONT_REQUESTS}}


def fixture():
    with open(NAMES_JSON) as f:
        return json.load(f)


def test_fixture_holds_every_request():
    """Every listed request either ran (a non-empty note and a digest) or raised when it was recorded."""
    fx = fixture()
    for name in MODEMS:
        for kind, reqs in (("soft", soft_requests(name)), ("hard", hard_requests(name))):
            for req in reqs:
                rec = fx[kind][key_of(name, req)]
                assert (rec.get("note") and len(rec["sha1"]) == 40) or rec.get("raises"), (kind, name, req)
    for name in QAMS + ("grid64_unequal",):
        for req in FRONT_REQUESTS:
            rec = fx["front"][key_of(name, req)]
            assert (rec.get("note") and len(rec["msg_sha1"]) == 40 and len(rec["llr_sha1"]) == 40) or rec.get("raises"), (name, req)
    # what the requests are there for: every kernel family is among the notes, and the refusals were refusals
    notes = " ".join(rec.get("note", "") for rec in fx["soft"].values())
    for family in ("demod_soft_any_kernel<9>", "demod_soft_sep_f32_kernel<", "demod_soft_f32_kernel<5>", "demod_soft_sep_kernel<3,rcp,gp,tab>",
                   "demod_soft_sep_kernel<3,div,gp>", "demod_soft_sep_kernel<3,rcp>", "demod_soft_gen_kernel<5,rcp>", "demod_soft_kernel<5,div>"):
        assert family in notes, family
    for name in QAMS:
        assert "note" in fx["front"][key_of(name, FRONT_REQUESTS[0])]
        for req in FRONT_REQUESTS[1:]:
            assert "only the default float64 demodulator path is fused" in fx["front"][key_of(name, req)]["raises"]
    assert "not equally spaced Gray levels" in fx["front"][key_of("grid64_unequal", FRONT_REQUESTS[0])]["raises"]


def _check(kind, name, reqs, observe):
    fx = fixture()[kind]
    bad = []
    for req in reqs:
        got, want = observe(name, req), fx[key_of(name, req)]
        print(key_of(name, req), got)
        if got != want:
            bad.append((key_of(name, req), got, want))
    assert not bad, (len(bad), bad[:5])


@pytest.mark.gpu
@pytest.mark.parametrize("name", MODEMS)
def test_soft_request_takes_the_recorded_kernel_and_gives_the_recorded_bits(gpu, name):
    _check("soft", name, soft_requests(name), observe_soft)


@pytest.mark.gpu
@pytest.mark.parametrize("name", MODEMS)
def test_hard_request_takes_the_recorded_kernel_and_gives_the_recorded_bits(gpu, name):
    _check("hard", name, hard_requests(name), observe_hard)


@pytest.mark.gpu
@pytest.mark.parametrize("name", QAMS + ("grid64_unequal",))
def test_fused_front_end_follows_the_soft_dispatch(gpu, name):
    _check("front", name, FRONT_REQUESTS, observe_front)
