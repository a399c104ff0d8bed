"""The optional outputs of every entry point that takes ``want``, pinned on the host against a recording stand-in for the library:
which output arguments reach the C-ABI, how large the arrays and device buffers behind them are, and what comes back.  Nothing is
computed: the stand-in records the arguments of every call and returns 0."""
import ctypes
import math
import types

import numpy as np
import pytest

from commpy_amd import _lib, channels, deviceops, equalizers, modulation, sync
from commpy_amd.channelcoding import (BCHCode, PolarCode, ProductCode, RSCode, Trellis, bch, bch_decode, chase_decode, ldpc_layered,
                                      ldpc_layered_decode, polar, polar_decode, productcode, rs, rs_decode, tailbiting, tailbiting_decode,
                                      tpc_decode)
import ldpc_layered_model

SERVED = ('cpx_malloc', 'cpx_free', 'cpx_device_count', 'cpx_get_device', 'cpx_last_error')


class Recorder:
    """Every ``cpx_*`` entry point records its positional arguments and returns 0; ``cpx_malloc`` hands out made-up addresses and a
    handle creator a made-up handle."""

    def __init__(self):
        self.calls = []                                 # (name, args) of every call but the SERVED ones and handle (de)construction
        self.top = 0x10000

    def fresh(self):
        self.top += 0x100
        return self.top

    def cpx_malloc(self, ref, nbytes):
        ref._obj.value = self.fresh()
        return 0

    def cpx_device_count(self, n):
        n._obj.value = 1
        return 0

    def cpx_last_error(self):
        return b''

    def __getattr__(self, name):
        if not name.startswith('cpx_'):
            raise AttributeError(name)

        def entry(*args):
            if name.endswith('_create'):
                args[-1]._obj.value = self.fresh()
            elif name not in SERVED and not name.endswith('_destroy'):
                self.calls.append((name, args))
            return 0
        return entry

    def args_of(self, entry):
        return [args for name, args in self.calls if name == entry]


@pytest.fixture
def lib(monkeypatch):
    rec = Recorder()
    monkeypatch.setattr(_lib, 'load', lambda: rec)
    # one made-up handle for every host object, kept nowhere: nothing is left to destroy once the real library is back
    monkeypatch.setattr(_lib.DeviceHandles, 'get', lambda self: ctypes.c_void_p(0x40))
    return rec


def nbytes(shape, dtype):
    return math.prod(shape) * np.dtype(dtype).itemsize


def address(arg):
    return None if arg is None else arg.value


def check(lib, entry, run, names, slots, table, dev, one=False, bare='single', copied=(), zeroed=True):
    """``run(want)`` for every single name, all names and all names reversed: the arguments of ``entry`` at ``slots[name]`` are
    non-null exactly for the wanted names and point at what is returned, which has the shape and dtype (the byte size, for a device
    buffer) of ``table[name]`` and is ordered as ``names``; then the invalid name."""
    for want in [(n,) for n in names] + [names[0], tuple(names), tuple(names)[::-1]]:
        lib.calls.clear()
        got = run(want)
        wanted = [n for n in names if n in ((want,) if isinstance(want, str) else want)]
        single = {'single': len(wanted) == 1, 'never': False, 'y-only': wanted == ['y']}[bare]
        if single:
            assert not isinstance(got, tuple) or isinstance(table[wanted[0]], list), (want, got)
            got = (got,)
        assert isinstance(got, tuple) and len(got) == len(wanted), (want, got)
        calls = lib.args_of(entry)
        assert len(calls) == 1, (want, lib.calls)
        for name in names:
            args = [calls[0][i] for i in np.atleast_1d(slots[name])]
            if name not in wanted:
                assert all(a is None for a in args), (want, name)
                continue
            part = got[wanted.index(name)]
            members, specs = (part, table[name]) if isinstance(table[name], list) else ((part,), [table[name]])
            assert isinstance(members, tuple) and len(members) == len(specs)
            for arg, member, (shape, dtype) in zip(args, members, specs):
                assert arg is not None and address(arg), (want, name)
                if dev:
                    assert isinstance(member, deviceops.DeviceBuf)
                    assert member.nbytes == nbytes(shape, dtype), (want, name, member.nbytes)
                    assert address(arg) == member.ptr.value
                else:
                    assert isinstance(member, np.generic if one and len(shape) == 1 else np.ndarray)
                    assert member.shape == (shape[1:] if one else shape) and member.dtype == np.dtype(dtype), (want, name, member.shape)
                    assert not zeroed or not member.any()
                    assert name in copied or isinstance(member, np.generic) or address(arg) == member.ctypes.data
    with pytest.raises(ValueError) as e:
        run(('nope',))
    assert str(e.value) == 'want must name at least one of ' + ', '.join("'%s'" % n for n in names)


def check_empty(lib, run, names, table, dev, calls=False, bare='single'):
    """``B = 0``: nothing reaches the library, yet every result is there, empty."""
    lib.calls.clear()
    got = run(tuple(names))
    assert bool(lib.calls) == calls, lib.calls
    assert isinstance(got, tuple) and len(got) == len(names)
    for name, part in zip(names, got):
        members, specs = (part, table[name]) if isinstance(table[name], list) else ((part,), [table[name]])
        for member, (shape, dtype) in zip(members, specs):
            assert math.prod(shape) == 0
            if dev:
                assert member.nbytes == 0 and member.ptr.value
            else:
                assert member.shape == shape and member.dtype == np.dtype(dtype)
    got = run((names[0],))
    assert isinstance(got, tuple) == (bare == 'never' or isinstance(table[names[0]], list))


def buf():
    return deviceops.DeviceBuf(8)


def bpsk():
    return modulation.PSKModem(2)


# ---- equalisers: BPSK, L = 2, n = 3, nf = 2, nb = 1 ----------------------------------------------------------------------------------
L, N, NF, NB = 2, 3, 2, 1


def mlse_table(B, m=1):
    return {'indices': ((B, N), np.int32), 'bits': ((B, N * m), np.uint8), 'metric': ((B,), np.float64), 'llr': ((B, N * m), np.float64)}


def mmse_table(B, m=1):
    return {'indices': ((B, N), np.int32), 'bits': ((B, N * m), np.uint8), 'estimate': ((B, N), np.complex128),
            'llr': ((B, N * m), np.float64), 'noise': ((B,), np.float64), 'ff': ((B, NF), np.complex128), 'fb': ((B, NB), np.complex128),
            'gain': ((B,), np.float64)}


MLSE_SLOTS = dict(zip(equalizers.WANT, range(11, 15)))
MMSE_SLOTS = dict(zip(equalizers.MMSE_WANT, range(14, 22)))


def test_mlse_host(lib):
    md, h = bpsk(), np.array([1.0, 0.5])
    run = lambda B: lambda want: equalizers.mlse_equalize_batch(np.zeros((B, N + L - 1), complex), h, md, noise_var=1.0, want=want)
    check(lib, 'cpx_mlse', run(2), equalizers.WANT, MLSE_SLOTS, mlse_table(2), False)
    check(lib, 'cpx_mlse', lambda want: equalizers.mlse_equalize_batch(np.zeros(N + L - 1, complex), h, md, noise_var=1.0, want=want),
          equalizers.WANT, MLSE_SLOTS, mlse_table(1), False, one=True)
    check_empty(lib, run(0), equalizers.WANT, mlse_table(0), False)


def test_mlse_dev(lib):
    md = bpsk()
    run = lambda B: lambda want: deviceops.mlse_equalize_dev(md, buf(), buf(), False, B, N, L, d_noise_var=buf(), want=want)
    check(lib, 'cpx_mlse_dev', run(2), equalizers.WANT, MLSE_SLOTS, mlse_table(2), True)
    check_empty(lib, run(0), equalizers.WANT, mlse_table(0), True)


def test_mmse_host(lib):
    md, h = bpsk(), np.array([1.0, 0.5])
    run = lambda B: lambda want: equalizers.mmse_equalize_batch(np.zeros((B, N + L - 1), complex), h, md, 1.0, NF, NB, want=want)
    check(lib, 'cpx_mmse_equalize', run(2), equalizers.MMSE_WANT, MMSE_SLOTS, mmse_table(2), False)
    check(lib, 'cpx_mmse_equalize', lambda want: equalizers.mmse_equalize_batch(np.zeros(N + L - 1, complex), h, md, 1.0, NF, NB, want=want),
          equalizers.MMSE_WANT, MMSE_SLOTS, mmse_table(1), False, one=True)
    check_empty(lib, run(0), equalizers.MMSE_WANT, mmse_table(0), False)
    for call in (lambda: equalizers.mmse_equalize_batch(np.zeros((2, N + L - 1), complex), h, md, None, NF, NB),
                 lambda: deviceops.mmse_equalize_dev(md, buf(), buf(), False, 2, N, L, None, False, NF, NB)):
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == 'noise_var is required'


def test_mmse_dev(lib):
    md = bpsk()
    run = lambda B: lambda want: deviceops.mmse_equalize_dev(md, buf(), buf(), False, B, N, L, buf(), False, NF, NB, want=want)
    check(lib, 'cpx_mmse_equalize_dev', run(2), equalizers.MMSE_WANT, MMSE_SLOTS, mmse_table(2), True)
    check_empty(lib, run(0), equalizers.MMSE_WANT, mmse_table(0), True)


def test_equaliser_input_errors_keep_their_texts(lib):
    md = bpsk()
    for f in (lambda y, h: equalizers.mlse_equalize_batch(y, h, md), lambda y, h: equalizers.mmse_equalize_batch(y, h, md, 1.0, NF)):
        for y, h, text in ((np.array(['a']), np.ones(2), "y must hold numbers, got dtype <U1"),
                           (np.zeros(4), np.array(['a']), "h must hold numbers, got dtype <U1"),
                           (np.zeros((1, 1, 4)), np.ones(2), 'y must be [B, n_y] or 1-D, got 3 dimensions'),
                           (np.zeros((2, 4)), np.ones((3, 2)), 'y is [2, n_y]: h must be [L] or [2, L], got shape (3, 2)'),
                           (np.zeros((2, 4)), np.ones((1, 1, 2)), 'y is [2, n_y]: h must be [L] or [2, L], got shape (1, 1, 2)')):
            with pytest.raises(ValueError) as e:
                f(y, h)
            assert str(e.value) == text
    assert lib.calls == []


# ---- tail-biting codes: 4 states, rate 1/2, T = 4 ----------------------------------------------------------------------------------
T = 4
TBCC_SLOTS = dict(zip(tailbiting.WANT, range(6, 10)))


def tbcc_table(B, k=1):
    return {'bits': ((B, T * k), np.uint8), 'wraps': ((B,), np.int32), 'tailbiting': ((B,), np.uint8), 'metric': ((B,), np.float64)}


def trellis():
    return Trellis(np.array([2]), np.array([[5, 7]]))


def test_tailbiting_host(lib):
    tr = trellis()
    run = lambda shape: lambda want: tailbiting_decode(np.zeros(shape), tr, want=want)
    check(lib, 'cpx_tbcc_decode', run((2, 2 * T)), tailbiting.WANT, TBCC_SLOTS, tbcc_table(2), False)
    check(lib, 'cpx_tbcc_decode', run((2 * T,)), tailbiting.WANT, TBCC_SLOTS, tbcc_table(1), False, one=True)
    check_empty(lib, run((0, 2 * T)), tailbiting.WANT, tbcc_table(0), False)


def test_tailbiting_dev(lib):
    tr = trellis()
    run = lambda B: lambda want: deviceops.tailbiting_decode_dev(tr, buf(), B, T, want=want)
    check(lib, 'cpx_tbcc_decode_dev', run(2), tailbiting.WANT, TBCC_SLOTS, tbcc_table(2), True)
    check_empty(lib, run(0), tailbiting.WANT, tbcc_table(0), True)


# ---- layered LDPC: the smallest plan of the host tests ------------------------------------------------------------------------------
LDPC_SLOTS = dict(zip(ldpc_layered.WANT, range(8, 12)))


def ldpc_table(B, n_v=8):
    return {'bits': ((B, n_v), np.int8), 'llr': ((B, n_v), np.float64), 'iters': ((B,), np.int32), 'converged': ((B,), np.uint8)}


def small_code():
    return ldpc_layered_model.params_from_code(ldpc_layered_model.code_from_rows(8, [[0, 1, 2], [2, 3, 4], [4, 5, 6], [6, 7]]))


def test_ldpc_layered_host(lib):
    code = small_code()
    run = lambda shape: lambda want: ldpc_layered_decode(np.zeros(shape), code, 3, want=want)
    check(lib, 'cpx_ldpc_layered_decode', run((2, 8)), ldpc_layered.WANT, LDPC_SLOTS, ldpc_table(2), False)
    check(lib, 'cpx_ldpc_layered_decode', run((8,)), ldpc_layered.WANT, LDPC_SLOTS, ldpc_table(1), False, one=True)
    check_empty(lib, run((0, 8)), ldpc_layered.WANT, ldpc_table(0), False)


def test_ldpc_layered_dev(lib):
    code = small_code()
    run = lambda B: lambda want: deviceops.ldpc_layered_decode_dev(code, buf(), B, 3, want=want)
    check(lib, 'cpx_ldpc_layered_decode_dev', run(2), ldpc_layered.WANT, LDPC_SLOTS, ldpc_table(2), True)
    check_empty(lib, run(0), ldpc_layered.WANT, ldpc_table(0), True)


# ---- polar codes: N = 8 ----------------------------------------------------------------------------------------------------------------
POLAR_SLOTS = {'bits': 4, 'crc': 5, 'metric': 6, 'u_llr': 7, 'list': (8, 9, 10)}


def polar_table(B, code, Ls, dev):
    return {'bits': ((B, code.A), np.uint8), 'crc': ((B,), np.uint8 if dev else bool), 'metric': ((B,), np.float64),
            'u_llr': ((B, code.N), np.float64), 'list': [((B, Ls, code.K), np.uint8), ((B, Ls), np.float64), ((B,), np.int32)]}


@pytest.mark.parametrize('dev', [False, True])
def test_polar(lib, dev):
    code = PolarCode(8, 4)
    entry = 'cpx_polar_decode_dev' if dev else 'cpx_polar_decode'
    if dev:
        run = lambda B, Ls: lambda want: deviceops.polar_decode_dev(code, buf(), B, Ls, want=want)
    else:
        run = lambda B, Ls: lambda want: polar_decode(np.zeros((B, 8)), code, Ls, want=want)
    check(lib, entry, run(2, 1), polar.WANT, POLAR_SLOTS, polar_table(2, code, 1, dev), dev, copied=('crc',))
    with pytest.raises(ValueError) as e:                # 'u_llr' is defined for successive cancellation only
        run(2, 2)(('bits', 'u_llr'))
    assert str(e.value) == "'u_llr' is defined for list_size = 1 only"
    if not dev:
        one = lambda want: polar_decode(np.zeros(8), code, 2, want=want)
        got = one(('list', 'bits'))
        assert got[0].shape == (4,) and isinstance(got[1], tuple) and [v.shape for v in got[1]] == [(2, 4), (2,), ()]
        assert isinstance(one('list'), tuple) and len(one('list')) == 3 and one('crc').dtype == bool
    check_empty(lib, run(0, 1), polar.WANT, polar_table(0, code, 1, dev), dev)
    for bad in (True, 1.0, -1):
        with pytest.raises(ValueError) as e:
            deviceops.polar_decode_dev(code, buf(), bad)
        assert str(e.value) == 'B = %r, need an integer >= 0' % (bad,)
    with pytest.raises(ValueError) as e:
        PolarCode(8, 0)
    assert str(e.value) == 'K = 0, need an integer >= 1'


def test_polar_list_arguments(lib):
    """With a list every name but 'u_llr', which stays null."""
    code = PolarCode(8, 4)
    for dev, entry in ((False, 'cpx_polar_decode'), (True, 'cpx_polar_decode_dev')):
        names = tuple(n for n in polar.WANT if n != 'u_llr')
        for want in [(n,) for n in names] + [names, names[::-1]]:
            lib.calls.clear()
            got = deviceops.polar_decode_dev(code, buf(), 2, 2, want=want) if dev else polar_decode(np.zeros((2, 8)), code, 2, want=want)
            (args,) = lib.args_of(entry)
            for name in polar.WANT:
                assert all((args[i] is not None) == (name in want) for i in np.atleast_1d(POLAR_SLOTS[name])), (want, name)
            wanted = [n for n in names if n in want]
            got = got if len(wanted) > 1 else (got,)
            table = polar_table(2, code, 2, dev)
            for name, part in zip(wanted, got):
                for member, (shape, dtype) in zip(*((part, table[name]) if name == 'list' else ((part,), [table[name]]))):
                    assert (member.nbytes == nbytes(shape, dtype)) if dev else (member.shape == shape and member.dtype == np.dtype(dtype))


# ---- BCH, Chase, product codes and Reed-Solomon: the (7, 4) Hamming code, RS(7, 5) --------------------------------------------------
def word_table(B, code, first, dtype):
    return {first: ((B, code.k), dtype), 'codeword': ((B, code.n), dtype), 'errors': ((B,), np.int32)}


def test_bch_decode(lib):
    code = BCHCode(7, 1)
    slots = dict(zip(bch.WANT, (3, 4, 5)))
    run = lambda shape: lambda want: bch_decode(np.zeros(shape, np.uint8), code, want=want)
    check(lib, 'cpx_bch_decode', run((2, 7)), bch.WANT, slots, word_table(2, code, 'bits', np.uint8), False)
    check(lib, 'cpx_bch_decode', run((7,)), bch.WANT, slots, word_table(1, code, 'bits', np.uint8), False, one=True)
    check_empty(lib, run((0, 7)), bch.WANT, word_table(0, code, 'bits', np.uint8), False)
    run = lambda B: lambda want: deviceops.bch_decode_dev(code, buf(), B, want=want)
    check(lib, 'cpx_bch_decode_dev', run(2), bch.WANT, slots, word_table(2, code, 'bits', np.uint8), True)
    check_empty(lib, run(0), bch.WANT, word_table(0, code, 'bits', np.uint8), True)


def test_rs_decode(lib):
    code = RSCode(7, 5)
    slots = dict(zip(rs.WANT, (4, 5, 6)))
    run = lambda shape: lambda want: rs_decode(np.zeros(shape, np.uint16), code, want=want)
    check(lib, 'cpx_rs_decode', run((2, 7)), rs.WANT, slots, word_table(2, code, 'symbols', np.uint16), False)
    check(lib, 'cpx_rs_decode', run((7,)), rs.WANT, slots, word_table(1, code, 'symbols', np.uint16), False, one=True)
    check_empty(lib, run((0, 7)), rs.WANT, word_table(0, code, 'symbols', np.uint16), False)
    run = lambda B: lambda want: deviceops.rs_decode_dev(code, buf(), B, want=want)
    check(lib, 'cpx_rs_decode_dev', run(2), rs.WANT, slots, word_table(2, code, 'symbols', np.uint16), True)
    check_empty(lib, run(0), rs.WANT, word_table(0, code, 'symbols', np.uint16), True)


def chase_table(rows, k, span):
    return {'bits': (rows + (k,), np.uint8), 'codeword': (span, np.uint8), 'extrinsic': (span, np.float64), 'metric': (rows, np.float64),
            'candidates': (rows, np.int32)}


def test_chase_host(lib):
    code = BCHCode(7, 1)
    slots = dict(zip(bch.CHASE_WANT, range(7, 12)))
    run = lambda shape: lambda want: chase_decode(np.zeros(shape), code, 2, 1.0, want=want)
    check(lib, 'cpx_chase_bch', run((2, 7)), bch.CHASE_WANT, slots, chase_table((2,), 4, (2, 7)), False)
    check(lib, 'cpx_chase_bch', run((7,)), bch.CHASE_WANT, slots, chase_table((1,), 4, (1, 7)), False, one=True)
    check_empty(lib, run((0, 7)), bch.CHASE_WANT, chase_table((0,), 4, (0, 7)), False)


def test_chase_dev(lib):
    code = BCHCode(7, 1)
    slots = dict(zip(bch.CHASE_WANT, range(11, 16)))
    run = lambda B: lambda want: deviceops.bch_chase_dev(code, buf(), B, 2, 1.0, want=want)
    check(lib, 'cpx_chase_bch_dev', run(2), bch.CHASE_WANT, slots, chase_table((2,), 4, (2, 7)), True)
    check_empty(lib, run(0), bch.CHASE_WANT, chase_table((0,), 4, (0,)), True)
    # strided: 'codeword' and 'extrinsic' are as large as the extent the strides span, (B - 1) sb + (n - 1) si + (J - 1) sj + 1
    strided = lambda want, **kw: deviceops.bch_chase_dev(code, buf(), 2, 2, 1.0, want=want, J=2, strides=(20, 1, 2), **kw)
    check(lib, 'cpx_chase_bch_dev', strided, bch.CHASE_WANT, slots, chase_table((2, 2), 4, (20 + 12 + 1 + 1,)), True)
    mine = deviceops.DeviceBuf(8 * 34)
    lib.calls.clear()
    got = strided(('extrinsic', 'bits'), d_extrinsic=mine)
    assert got[1] is mine and lib.args_of('cpx_chase_bch_dev')[0][13].value == mine.ptr.value
    assert strided('extrinsic', d_extrinsic=mine) is mine
    with pytest.raises(ValueError) as e:
        strided('bits', d_extrinsic=mine)
    assert str(e.value) == "d_extrinsic needs 'extrinsic' in want"


def test_tpc(lib):
    code = ProductCode(BCHCode(7, 1), BCHCode(7, 1))
    block = lambda B: {'bits': ((B, 4, 4), np.uint8), 'codeword': ((B, 7, 7), np.uint8), 'extrinsic': ((B, 7, 7), np.float64)}
    for dev, names in ((True, productcode.TPC_DEV_WANT), (False, productcode.TPC_WANT)):
        for want in [(n,) for n in names] + [names[0], names, names[::-1]]:
            lib.calls.clear()
            if dev:
                got = deviceops.tpc_decode_dev(code, buf(), 2, iters=2, want=want)
            else:
                got = tpc_decode(np.zeros((2, 7, 7)), code, iters=2, want=want)
            wanted = [n for n in names if n in want]
            assert isinstance(got, tuple) == (len(wanted) > 1)
            got = dict(zip(wanted, got if len(wanted) > 1 else (got,)))
            calls = lib.args_of('cpx_chase_bch_dev')
            assert len(calls) == 4
            # the decision is asked of the last half-iteration alone, and only where it is needed; the soft output always, in place
            word = 'codeword' in want or 'bits' in want
            assert [c[12] is not None for c in calls] == [False, False, False, word]
            assert all(c[11] is None and c[14] is None and c[15] is None for c in calls)
            assert len({c[13].value for c in calls}) == 1 and all(c[2].value == c[13].value for c in calls)
            for name, v in got.items():
                shape, dtype = block(2)[name]
                if dev:
                    assert v.nbytes == nbytes(shape, dtype)
                    assert v.ptr.value == calls[-1][12 if name == 'codeword' else 13].value
                else:
                    assert v.shape == shape and v.dtype == np.dtype(dtype)
        with pytest.raises(ValueError) as e:
            deviceops.tpc_decode_dev(code, buf(), 2, want='nope') if dev else tpc_decode(np.zeros((2, 7, 7)), code, want='nope')
        assert str(e.value) == 'want must name at least one of ' + ', '.join("'%s'" % n for n in names)
        check_empty(lib, (lambda want: deviceops.tpc_decode_dev(code, buf(), 0, want=want)) if dev else
                    (lambda want: tpc_decode(np.zeros((0, 7, 7)), code, want=want)), names, block(0), dev)
    got = tpc_decode(np.zeros((7, 7)), code, iters=1, want=productcode.TPC_WANT)
    assert [v.shape for v in got] == [(4, 4), (7, 7), (7, 7)]


# ---- the OFDM estimators, the fading channel and the timing metric: their own return rules --------------------------------------------
def pilots():
    return types.SimpleNamespace(ndata=3, nt=2, nsc=4, nsym=2, handle=lambda: ctypes.c_void_p(0x40))


@pytest.mark.parametrize('fn, entry, third', [(deviceops.ofdm_estimate_dev, 'cpx_pilots_estimate_dev', 'h_sc'),
                                              (deviceops.ofdm_estimate_tv_dev, 'cpx_pilots_estimate_tv_dev', 'h_sym')])
def test_ofdm_estimate_dev(lib, fn, entry, third):
    """Always a tuple, in the order (y, h, third); the C-ABI takes (third, y, h).  An empty batch is passed on to the engine."""
    p, nr = pilots(), 2
    table = lambda B: {'y': ((B, p.ndata, nr), np.complex128), 'h': ((B, p.ndata, nr, p.nt), np.complex128),
                       'h_sc': ((B, p.nsc, nr, p.nt), np.complex128), 'h_sym': ((B, p.nsym, p.nsc, nr, p.nt), np.complex128)}
    names, slots = ('y', 'h', third), {third: 4, 'y': 5, 'h': 6}
    run = lambda B: lambda want: fn(p, buf(), B, nr, want=want)
    check(lib, entry, run(2), names, slots, table(2), True, bare='never')
    check_empty(lib, run(0), names, table(0), True, calls=True, bare='never')


def test_fading_channel_dev(lib):
    """A bare buffer for ``want == ('y',)`` alone; without 'y' the input is not passed either.  An empty batch is passed on."""
    nt, nr, n, pdp = 1, 2, 3, np.ones(2)
    table = lambda B, nblk: {'y': ((B, nr, n + 1), np.complex128), 'g': ((B, nblk, nr, nt, 2), np.complex128)}
    run = lambda B: lambda want: deviceops.fading_channel_dev(buf(), B, nt, nr, n, pdp, 0.01, hold=2, want=want)
    check(lib, 'cpx_fading_channel_dev', run(2), ('y', 'g'), {'y': 16, 'g': 17}, table(2, 2), True, bare='y-only')
    for want, passed in ((('y',), True), (('g',), False), (('g', 'y'), True)):
        lib.calls.clear()
        run(2)(want)
        assert (lib.args_of('cpx_fading_channel_dev')[0][0] is not None) == passed
    check_empty(lib, run(0), ('y', 'g'), table(0, 1), True, calls=True, bare='y-only')
    assert isinstance(run(2)(('g',)), tuple) and isinstance(run(2)(('y',)), deviceops.DeviceBuf)


def test_fading_multipath_batch(lib):
    nr, n, pdp = 2, 3, np.ones(2)
    table = lambda B, nblk: {'y': ((B, nr, n + 1), np.complex128), 'g': ((B, nblk, nr, 1, 2), np.complex128)}
    run = lambda B: lambda want: channels.fading_multipath_batch(np.zeros((B, 1, n)), nr, pdp, 0.01, hold=2, want=want)
    check(lib, 'cpx_fading_channel', run(2), ('y', 'g'), {'y': 16, 'g': 17}, table(2, 2), False, bare='y-only')
    lib.calls.clear()
    run(2)(('g',))
    assert lib.args_of('cpx_fading_channel')[0][0] is None
    check_empty(lib, run(0), ('y', 'g'), table(0, 1), False, bare='y-only')
    siso = channels.fading_multipath_batch(np.zeros((2, n)), 1, pdp, 0.01, want=('y', 'g'))
    assert siso[0].shape == (2, n + 1) and siso[1].shape == (2, n + 1, 1, 1, 2)


def test_sync_metric_batch(lib):
    """Always a tuple (m, e, p); the C-ABI takes (p, e, m)."""
    table = lambda B: {'m': ((B, 3), np.float64), 'e': ((B, 3), np.float64), 'p': ((B, 3), np.complex128)}
    run = lambda B: lambda want: sync.sync_metric_batch(np.zeros((B, 4), complex), 1, 1, want=want)
    check(lib, 'cpx_sync_metric', run(2), ('m', 'e', 'p'), {'p': 6, 'e': 7, 'm': 8}, table(2), False, bare='never')
    check_empty(lib, run(0), ('m', 'e', 'p'), table(0), False, bare='never')


# ---- the helper itself -----------------------------------------------------------------------------------------------------------------
def test_results_module(lib):
    from commpy_amd import _results
    shapes = {'a': ((2, 3), np.complex128), 'b': ((2,), np.int32), 'c': ((2, 5), np.uint8), 'd': ((0, 4), np.float64)}
    res, p = _results.outputs(('c', 'a'), shapes)
    assert list(res) == ['a', 'c'] and res['a'].shape == (2, 3) and res['a'].dtype == np.complex128 and not res['c'].any()
    assert p('a').value == res['a'].ctypes.data and p('b') is None and p('d') is None
    assert [v.shape for v in _results.returned(res, True)] == [(3,), (5,)] and _results.returned(res)[1] is res['c']
    assert _results.returned({'b': res['c']}) is res['c'] and _results.returned({'b': res['c']}, one=True).shape == (5,)
    bufs, q = _results.device_outputs(('d', 'c', 'b', 'a'), shapes)
    assert list(bufs) == ['a', 'b', 'c', 'd'] and [b.nbytes for b in bufs.values()] == [96, 8, 10, 0]
    assert all(q(k).value == bufs[k].ptr.value for k in bufs)
    mine = deviceops.DeviceBuf(10)
    bufs, q = _results.device_outputs(('a', 'c'), shapes, {'c': mine, 'a': None})
    assert bufs['c'] is mine and q('c').value == mine.ptr.value and q('b') is None and bufs['a'].nbytes == 96
    assert _results.returned(bufs) == (bufs['a'], mine)
    assert lib.calls == []


def test_one_table_serves_both_flavours():
    """The device buffers are sized by the tables the host arrays are made from."""
    md = bpsk()
    assert equalizers.mlse_shapes(2, N, 1) == mlse_table(2) and equalizers.mmse_shapes(2, N, 1, NF, NB) == mmse_table(2)
    assert tailbiting.shapes(2, T, 1) == tbcc_table(2) and ldpc_layered.shapes(2, 8) == ldpc_table(2)
    assert bch.chase_shapes((2,), 4, (2, 7)) == chase_table((2,), 4, (2, 7))
    assert list(equalizers.mmse_shapes(2, N, 1, NF, NB)) == list(equalizers.MMSE_WANT) and md.num_bits_symbol == 1
