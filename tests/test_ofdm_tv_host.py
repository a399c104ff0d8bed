"""Host side of the time-tracking pilot-aided estimator (cpx_pilots_create_tv / cpx_pilots_estimate_tv): the three builders of V
against the NumPy model and a direct scipy evaluation, every refusal (ValueError before any device is touched), the C entry points'
argument checks without a device, and the header against the library's exports."""
import ctypes
import os
import re
import struct

import numpy as np
import pytest
from scipy.special import j0

import ofdm_tv_model as T
from commpy_amd import _lib
from commpy_amd.modulation import OfdmPilots, ofdm_estimate_tv_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOL_SETS = [(14, [0, 4, 9, 13]), (14, [3]), (7, [2, 3]), (6, [0, 1, 2, 3, 4, 5]), (9, [1, 6]), (1, [0]), (12, [5, 6, 11])]


def single(nsym, ps, time_interp):
    """One antenna with one pilot subcarrier on the symbols ``ps``."""
    n = len(ps)
    return OfdmPilots(4, nsym, 1, np.array(ps), np.full(n, 2), np.zeros(n, int), np.ones(n), 'linear', time_interp)


@pytest.mark.parametrize("nsym, ps", SYMBOL_SETS)
def test_linear_rows(nsym, ps):
    p = single(nsym, ps, 'linear')
    V = p.V[0]
    assert list(p.pilot_symbols[0]) == ps and len(p.V) == 1
    assert V.shape == (nsym, len(ps)) and V.dtype == np.complex128 and np.all(V.imag == 0)
    assert np.all(np.count_nonzero(V, axis=1) <= 2) and np.all(V.real >= 0)
    assert np.allclose(V.sum(axis=1), 1.0, rtol=0, atol=1e-15)
    assert np.allclose(V, T.v_linear(nsym, ps), rtol=0, atol=1e-15)
    assert np.array_equal(V[ps], np.eye(len(ps)))                                  # a pilot symbol keeps its own estimate
    line = 3.0 * np.arange(nsym) - 2
    assert np.allclose(V @ line[ps], np.clip(line, line[ps[0]], line[ps[-1]]), rtol=0, atol=1e-13)   # exact on a line, held outside


@pytest.mark.parametrize("nsym, ps", SYMBOL_SETS)
def test_hold_rows(nsym, ps):
    V = single(nsym, ps, 'hold').V[0]
    assert np.array_equal(V, T.v_hold(nsym, ps))
    assert np.all(np.count_nonzero(V, axis=1) == 1) and np.all(V.sum(axis=1) == 1)
    for s in range(nsym):
        i = int(np.flatnonzero(V[s])[0])
        d = [abs(s - q) for q in ps]
        assert d[i] == min(d) and i == d.index(min(d))                             # the nearest, the lower one on a tie
    if ps == [0, 4, 9, 13]:
        assert list(np.argmax(V.real, axis=1)) == [0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 2, 3, 3]     # symbol 2 is a tie: the lower


@pytest.mark.parametrize("fd_sym, nvar", [(0.02, 1e-8), (0.005, 0.0), (0.1, 0.01), (0.0, 0.5)])
@pytest.mark.parametrize("nsym, ps", SYMBOL_SETS)
def test_doppler_rows(nsym, ps, fd_sym, nvar):
    V = single(nsym, ps, ('doppler', fd_sym, nvar)).V[0]
    s, q = np.arange(nsym)[:, None], np.array(ps)[None, :]
    r_sp = j0(2 * np.pi * fd_sym * np.abs(s - q))
    r_pp = j0(2 * np.pi * fd_sym * np.abs(q.T - q)) + nvar * np.eye(len(ps))
    direct = r_sp @ np.linalg.inv(r_pp)
    scale = np.linalg.cond(r_pp) * 1e-15 * max(1.0, np.max(np.abs(direct)))
    assert V.shape == (nsym, len(ps)) and np.all(V.imag == 0)
    assert np.max(np.abs(V - direct)) <= 10 * scale
    assert np.max(np.abs(V - T.v_doppler(nsym, ps, fd_sym, nvar))) <= 10 * scale
    if nvar == 0.0:
        assert np.allclose(V[ps], np.eye(len(ps)), rtol=0, atol=10 * scale)        # no noise: a pilot symbol keeps its own estimate


def test_attributes_of_comb_and_block():
    p = OfdmPilots.comb(52, 14, 2, 4, [0, 4, 9, 13], 'linear', time_interp='linear')
    assert [list(s) for s in p.pilot_symbols] == [[0, 4, 9, 13]] * 2 and [v.shape for v in p.V] == [(14, 4)] * 2
    assert OfdmPilots.comb(52, 14, 2, 4, [0, 4, 9, 13], 'linear').V is None
    p = OfdmPilots.block(8, 5, 3, time_interp='hold')
    assert [list(s) for s in p.pilot_symbols] == [[0], [1], [2]] and all(np.array_equal(v, np.ones((5, 1))) for v in p.V)
    given = [np.arange(10).reshape(5, 2) * (1 - 2j), np.ones((5, 1)), -np.ones((5, 1))]
    p = OfdmPilots(8, 5, 3, [0, 3, 1, 2], [0, 0, 1, 2], [0, 0, 1, 2], [1, 1, 1, 1], 'linear', given)
    assert all(np.array_equal(a, b) for a, b in zip(p.V, given)) and p.V[1].dtype == np.complex128
    fr = T.Frame(p.nsc, p.nsym, p.nt, p.pil_sym, p.pil_sc, p.pil_tx, p.pil_val, p.W, p.V)
    assert fr.ps == [[0, 3], [1], [2]] and fr.pk == [[0], [1], [2]] and fr.ndata == p.ndata


@pytest.fixture
def no_device(monkeypatch):
    """Any attempt to load the engine fails the test: the refusals below must come from the host-side checks."""
    def boom(*a, **k):
        raise AssertionError("the engine was touched")
    monkeypatch.setattr(_lib, "load", boom)


# antenna 0: subcarriers {0, 4} on symbols {0, 2}; antenna 1: subcarrier 1 on symbol 0
GOOD = dict(nsc=8, nsym=3, nt=2, pil_sym=[0, 0, 2, 2, 0], pil_sc=[0, 4, 0, 4, 1], pil_tx=[0, 0, 0, 0, 1], pil_val=[1, 1j, -1, 1, 1],
            interp='linear', time_interp='linear')


@pytest.mark.parametrize("change", [
    dict(time_interp='cubic'), dict(time_interp=('doppler', 0.01)), dict(time_interp=('doppler', -0.01, 0.0)),
    dict(time_interp=('doppler', 0.01, -1e-3)), dict(time_interp=('doppler', np.nan, 0.0)), dict(time_interp=('doppler', 0.01, np.inf)),
    dict(time_interp=('doppler', 'a', 0.0)), dict(time_interp=('wiener', 0.01, 0.0)),
    dict(time_interp=('doppler', 0.0, 0.0)),                                        # R_pp of two pilot symbols is singular
    dict(time_interp=[np.ones((3, 2))]),                                            # one matrix for two antennas
    dict(time_interp=[np.ones((3, 2)), np.ones((3, 2))]), dict(time_interp=[np.ones((2, 2)), np.ones((3, 1))]),
    dict(time_interp=[np.ones((3, 2)), np.full((3, 1), np.nan)]), dict(time_interp=[np.ones((3, 2)), np.full((3, 1), np.inf)]),
    dict(time_interp=[np.ones((3, 2)), np.array([['x']] * 3)]), dict(time_interp=[np.ones(6), np.ones(3)]),
    dict(pil_sym=[0, 0, 2, 1, 0]),                                                  # staggered: antenna 0 has one of its two in symbols 1, 2
    dict(pil_sym=[0, 0, 2, 2, 0, 1], pil_sc=[0, 4, 0, 4, 1, 5], pil_tx=[0, 0, 0, 0, 1, 1], pil_val=[1] * 6),   # antenna 1 staggered
])
def test_time_interp_refused(no_device, change):
    with pytest.raises(ValueError):
        OfdmPilots(**dict(GOOD, **change))


def test_refusal_names_antenna_and_symbol(no_device):
    with pytest.raises(ValueError, match="antenna 0 has 1 of its 2 in symbol 1"):
        OfdmPilots(**dict(GOOD, pil_sym=[0, 0, 2, 1, 0]))
    OfdmPilots(**dict(GOOD, pil_sym=[0, 0, 2, 1, 0], time_interp=None))            # a staggered pattern is fine without time tracking
    with pytest.raises(ValueError, match="antenna 0 has pilots on 1 of its 2 pilot subcarriers in symbol 1"):
        T.Frame(8, 3, 2, [0, 0, 2, 1, 0], [0, 4, 0, 4, 1], [0, 0, 0, 0, 1], [1] * 5, [np.ones((8, 2)), np.ones((8, 1))], [None, None])


def test_calls_refused(no_device):
    p = OfdmPilots(**GOOD)
    assert [list(s) for s in p.pilot_symbols] == [[0, 2], [0]] and [v.shape for v in p.V] == [(3, 2), (3, 1)]
    for ok in ('hold', ('doppler', 0.02, 1e-8), ('doppler', 0.0, 1.0), [np.ones((3, 2)) * 1j, np.zeros((3, 1))]):
        OfdmPilots(**dict(GOOD, time_interp=ok))
    plain = OfdmPilots(**dict(GOOD, time_interp=None))
    assert plain.V is None and [list(s) for s in plain.pilot_symbols] == [[0, 2], [0]]
    Y = np.zeros((1, 2, 3, 8))
    for bad in (lambda: ofdm_estimate_tv_batch(Y, plain), lambda: ofdm_estimate_tv_batch(Y, None),
                lambda: ofdm_estimate_tv_batch(np.zeros((1, 2, 3, 7)), p), lambda: ofdm_estimate_tv_batch(np.zeros((2, 3, 8)), p),
                lambda: ofdm_estimate_tv_batch(np.zeros((1, 0, 3, 8)), p), lambda: ofdm_estimate_tv_batch(Y, p, want=()),
                lambda: ofdm_estimate_tv_batch(Y, p, want=('y', 'h_sc')), lambda: ofdm_estimate_tv_batch(np.zeros((1, 2, 3, 8), dtype=object), p),
                lambda: OfdmPilots.comb(52, 4, 2, 4, [0, 2], 'linear', time_interp='nearest'),
                lambda: OfdmPilots.block(52, 3, 2, time_interp=('doppler', -1, 0))):
        with pytest.raises(ValueError):
            bad()
    # an empty batch needs no device
    assert [a.shape for a in ofdm_estimate_tv_batch(np.zeros((0, 3, 3, 8)), p, want=('h_sym', 'y', 'h'))] == [(0, 19, 3), (0, 19, 3, 2), (0, 3, 8, 3, 2)]


def test_want_names_outputs(no_device):
    """As for the per-frame estimator: a bare string is one name, the order asked in does not matter, and an empty or unknown ``want``
    is refused in fixed words, by the host-buffer call and by the device-resident one."""
    from commpy_amd import deviceops
    p = OfdmPilots(**GOOD)
    Y0 = np.zeros((0, 3, 3, 8))
    assert [a.shape for a in ofdm_estimate_tv_batch(Y0, p, want='h_sym')] == [(0, 3, 8, 3, 2)]
    assert [a.shape for a in ofdm_estimate_tv_batch(Y0, p, want=['h', 'y'])] == [(0, 19, 3), (0, 19, 3, 2)]
    for call in (lambda w: ofdm_estimate_tv_batch(Y0, p, want=w), lambda w: deviceops.ofdm_estimate_tv_dev(p, None, 1, 3, want=w)):
        for bad in ((), [], '', 'x', ('y', 'x'), (None,), 'h_sc'):
            with pytest.raises(ValueError) as e:
                call(bad)
            assert str(e.value) == "want must name at least one of 'y', 'h', 'h_sym'"


def test_engine_checks_without_device():
    """cpx_pilots_create_tv and cpx_pilots_estimate_tv report argument errors before the device is looked for."""
    lib = _lib.load()
    P = _lib.ptr
    i32 = lambda *v: np.array(v, np.int32)
    h = ctypes.c_void_p()
    ones = np.ones(64, complex)

    def create(nsc, nsym, nt, sym, sc, tx, val, w, v):
        val = np.asarray(val, complex)
        return lib.cpx_pilots_create_tv(nsc, nsym, nt, len(sym), P(i32(*sym)), P(i32(*sc)), P(i32(*tx)), P(val), P(np.asarray(w, complex)),
                                        None if v is None else P(np.asarray(v, complex)), ctypes.byref(h))
    # cpx_pilots_create's own checks
    for args in ((3, 1, 1, [0], [0], [0], [1]), (4, 0, 1, [0], [0], [0], [1]), (4, 1, 1, [1], [0], [0], [1]), (4, 1, 1, [0, 0], [2, 2], [0, 0], [1, 1]),
                 (4, 1, 2, [0, 0], [1, 2], [0, 0], [1, 1]), (4, 1, 1, [0], [0], [0], [0])):
        assert create(*args, ones, ones) == _lib.CPX_EINVAL and _lib.last_error().startswith("ofdm_pilots:") and not h.value, args
    assert create(4, 1, 1, [0], [0], [0], [1], [1, 1, np.inf, 1], ones) == _lib.CPX_EINVAL
    assert _lib.last_error() == "ofdm_pilots: the interpolation matrices hold a value that is not finite"
    assert create(4, 1, 2000, [0], [0], [0], [1], ones, ones) == _lib.CPX_ELIMIT
    # the time matrices: staggered, null, not finite
    stag = (8, 3, 2, [0, 0, 2, 1, 0], [0, 4, 0, 4, 1], [0, 0, 0, 0, 1], [1, 1j, -1, 1, 1])
    assert create(*stag, ones, ones) == _lib.CPX_EINVAL and not h.value
    assert _lib.last_error() == ("ofdm_pilots: antenna 0 has pilots on 1 of its 2 pilot subcarriers in symbol 1 (time tracking needs the same "
                                 "subcarriers on every pilot symbol)")
    rect = (8, 3, 2, [0, 0, 2, 2, 0], [0, 4, 0, 4, 1], [0, 0, 0, 0, 1], [1, 1j, -1, 1, 1])
    assert create(*rect, ones, None) == _lib.CPX_EINVAL and _lib.last_error() == "ofdm_pilots: null time matrices (v_re_im)" and not h.value
    v = np.ones(9, complex)                                                         # V_0 [3][2], then V_1 [3][1]
    for bad in (np.nan, np.inf, 1j * np.nan):
        v[8] = bad
        assert create(*rect, ones, v) == _lib.CPX_EINVAL and not h.value
        assert _lib.last_error() == "ofdm_pilots: the time matrices hold a value that is not finite"
    x = np.zeros(64)
    assert lib.cpx_pilots_estimate_tv(None, P(x), 1, 1, P(x), None, None) == _lib.CPX_EINVAL and _lib.last_error() == "ofdm_estimate_tv: null plan"
    assert lib.cpx_pilots_estimate_tv_dev(None, P(x), 1, 1, P(x), None, None, None) == _lib.CPX_EINVAL
    assert _lib.last_error() == "ofdm_estimate_tv: null plan"
    if _lib.device_count() > 0:
        return
    v[8] = 1.0
    assert create(*rect, ones, v) == _lib.CPX_ENODEV and _lib.last_error().startswith("no HIP device available")


def test_entry_point_fails_loudly_without_device():
    if _lib.device_count() > 0:
        pytest.skip("a HIP device is present")
    p = OfdmPilots.comb(52, 4, 2, 4, [0, 2], 'linear', time_interp='linear')
    with pytest.raises(_lib.EngineError):
        ofdm_estimate_tv_batch(np.zeros((1, 2, 4, 52)), p)


def _exported(path):
    """Names of the defined global functions in the dynamic symbol table of an ELF64 little-endian shared object."""
    with open(path, "rb") as f:
        data = f.read()
    assert data[:6] == b"\x7fELF\x02\x01"
    shoff, = struct.unpack_from("<Q", data, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", data, 0x3A)
    sections = [struct.unpack_from("<IIQQQQIIQQ", data, shoff + i * shentsize) for i in range(shnum)]
    names = set()
    for sh in sections:
        if sh[1] != 11:                                                             # SHT_DYNSYM
            continue
        stroff = sections[sh[6]][4]
        for off in range(sh[4], sh[4] + sh[5], 24):
            st_name, st_info, _, st_shndx = struct.unpack_from("<IBBH", data, off)
            if st_shndx != 0 and st_info & 15 == 2 and st_info >> 4 in (1, 2):      # defined, a function, global or weak
                names.add(data[stroff + st_name:data.index(b"\0", stroff + st_name)].decode())
    return names


def test_header_declares_what_the_library_exports():
    text = open(os.path.join(ROOT, "include", "commpy_amd.h")).read()
    declared = set(re.findall(r"\b(cpx_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    exported = {n for n in _exported(_lib.load()._name) if n.startswith("cpx_")}
    assert {"cpx_pilots_create_tv", "cpx_pilots_estimate_tv", "cpx_pilots_estimate_tv_dev", "cpx_pilots_estimate"} <= exported
    assert exported <= declared, sorted(exported - declared)
