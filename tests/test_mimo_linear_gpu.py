"""The linear MIMO kernels of csrc/mimo_linear.hip against the NumPy model of tests/mimo_linear_model.py (checked without a GPU by
tests/test_mimo_linear_host.py): every shape class of both kernels, xhat and nu within the bound the model file derives, LLRs
under the K-best rule, indices exactly except where the MODEL calls a vector a near-tie, a cross-check against the exhaustive ML
kernel on unitary channels, isolation of failed vectors, bit identity across everything the contract lists, and exact ties."""
import ctypes

import numpy as np
import pytest

import mimo_linear_model as L
from commpy_amd import _lib
from commpy_amd.deviceops import DeviceBuf
from commpy_amd.modulation import Modem, QAMModem, _linear_run, linear_batch, mimo_ml_batch
from mimo_model import assert_llr

pytestmark = pytest.mark.gpu
ALL = ('idx', 'llr', 'xhat', 'nu')
_modems = {}


def modem_of(m):
    if m not in _modems:
        _modems[m] = Modem(L.BPSK, reorder_as_gray=False) if m == 2 else QAMModem(m)
    return _modems[m]


def kernel_of(nt):
    return "mimo_linear_kernel<%d>" % nt if nt <= 8 else "mimo_linear_wave_kernel"


def run(y, h, md, reg, noise_var=L.NOISE_VAR, want=ALL):
    with np.errstate(all="ignore"):
        out = _linear_run(y, h, md, reg, noise_var, want)
    nt = np.shape(h)[-1]
    note = _lib.last_kernel()
    assert kernel_of(nt) in note and ("x%d" % nt) in note and ("m %d" % md.m) in note, note
    return out


def same_bits(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in a) and set(a) == set(b)


# ---- against the model -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("i", range(len(L.CASES)), ids=[L.case_id(c) for c in L.CASES])
def test_matches_model(gpu, i):
    c = L.CASES[i]
    nr, nt, m, B, shared = c
    md = modem_of(m)
    Es = float(np.mean(L._sq(md.constellation)))
    # LLRs and indices on the well-conditioned set, xhat and nu on both
    for smax, kmax in ((L.SMAX_LLR, L.KAPPA_LLR), (L.SMAX_XHAT, L.KAPPA_XHAT)):
        y, h, const, want = L.case(i, smax)
        assert np.array_equal(const, md.constellation) and (y.dtype == np.float64) == (m == 2)
        for me, w in want.items():
            reg = L.case_reg(c, me, const)
            kap = L.kappa(h, reg, B)
            assert kap.max() <= kmax and not w["bad"].any()
            got = run(y, h, md, reg)
            bound = L.K_BOUND * nt * nr * L.EPS * kap
            ex, en = L.rel_err(got["xhat"], w["xhat"]), L.rel_err(got["nu"], w["nu"])
            print("%s %s smax %g: kappa <= %.3g, xhat err / bound <= %.3g, nu err / bound <= %.3g  [%s]" % (
                L.case_id(c), me, smax, kap.max(), (ex / bound).max(), (en / bound).max(), _lib.last_kernel()))
            assert np.all(ex <= bound) and np.all(en <= bound)
            if smax == L.SMAX_LLR:
                assert_llr(got["llr"], w["llr"])
                keep = w["margin"] >= L.MARGIN_MIN * Es
                assert np.sum(~keep) <= L.MARGIN_CAP * B
                assert np.array_equal(got["idx"][keep], w["idx"][keep])
                sym = linear_batch(y, h, md, L.NOISE_VAR, me, 'hard', reg)
                assert np.array_equal(sym, md.constellation[got["idx"]])


@pytest.mark.parametrize("nr,nt,B", [(2, 2, L.WRAP_REG_B), (9, 9, L.WRAP_WAVE_B)], ids=["lane", "wave"])
def test_grid_wrap(gpu, nr, nt, B):
    """A batch just past one full pass of the grid-stride loop: the vectors of the second pass against the model, and the whole
    batch bit for bit against the same vectors run in small batches."""
    md = modem_of(4)
    y, h = L.conditioned_inputs(20261102, B, nr, nt, md.constellation, False, L.SMAX_LLR)
    reg = L.NOISE_VAR / md.Es
    got = run(y, h, md, reg)
    first = B - (65 if nt <= 8 else 70)                         # the second pass starts here
    sel = np.concatenate((np.arange(130), np.arange(first - 64, B)))
    w = L.linear_model(y[sel], h[sel], md.constellation, reg, L.NOISE_VAR)
    bound = L.K_BOUND * nt * nr * L.EPS * L.kappa(h[sel], reg)
    assert np.all(L.rel_err(got["xhat"][sel], w["xhat"]) <= bound) and np.all(L.rel_err(got["nu"][sel], w["nu"]) <= bound)
    assert_llr(got["llr"][sel], w["llr"])
    keep = w["margin"] >= L.MARGIN_MIN * md.Es
    assert keep.all() and np.array_equal(got["idx"][sel], w["idx"])
    tail = run(y[first - 3:], h[first - 3:], md, reg)             # the same vectors at other positions, in another batch size
    assert same_bits({k: v[first - 3:] for k, v in got.items()}, tail)


def test_agrees_with_ml_on_unitary_channels(gpu):
    """H = a Q with Q unitary: |y - H x|^2 = a^2 |Q^H y / a - x|^2 decouples per stream, so zero forcing decides as the
    exhaustive ML kernel does on every vector whose decision is not a near-tie."""
    for m, n, B in ((4, 4, 300), (16, 3, 300), (2, 5, 200)):
        md = modem_of(m)
        rs = np.random.RandomState(77 + m)
        q = np.linalg.qr(rs.randn(B, n, n) + (0 if m == 2 else 1j) * rs.randn(B, n, n))[0]
        h = q * (0.5 + rs.rand(B))[:, None, None]
        x = md.constellation[rs.randint(0, m, (B, n))]
        y = np.matmul(h, x[:, :, None])[:, :, 0] + 0.8 * (rs.randn(B, n) + (0 if m == 2 else 1j) * rs.randn(B, n))
        zf = linear_batch(y, h, md, 0.1, 'zf')
        ml = mimo_ml_batch(y, h, md)
        w = L.linear_model(y, h, md.constellation, 0.0, 0.1)
        keep = w["margin"] >= L.MARGIN_MIN * md.Es
        assert np.sum(~keep) <= L.MARGIN_CAP * B and np.sum(zf != x) > 0          # noisy enough to make errors
        assert np.array_equal(zf[keep], ml[keep])


# ---- isolation ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nr,nt", [(4, 4), (10, 9)], ids=["lane", "wave"])
@pytest.mark.parametrize("where", [0, 63, 140], ids=["lane0", "lane63", "last_partial_workgroup"])
@pytest.mark.parametrize("fault", ["nan_y", "inf_h", "singular"])
def test_failed_vector_is_isolated(gpu, nr, nt, where, fault):
    md, B = modem_of(16), 150
    y0, h0 = L.conditioned_inputs(31, B, nr, nt, md.constellation, False, L.SMAX_LLR)
    clean = run(y0, h0, md, 0.0)
    y, h = y0.copy(), h0.copy()
    if fault == "nan_y":
        y[where, nr - 1] = np.nan
    elif fault == "inf_h":
        h[where, 1, nt - 1] = np.inf
    else:
        h[where, :, nt - 1] = h[where, :, 0]                      # two equal columns: exactly singular under zero forcing
    got = run(y, h, md, 0.0)
    assert np.isnan(got["xhat"][where].view(np.float64)).all() and np.isnan(got["nu"][where]).all()
    assert np.isnan(got["llr"][where]).all() and not got["idx"][where].any()
    others = np.arange(B) != where
    assert same_bits({k: v[others] for k, v in got.items()}, {k: v[others] for k, v in clean.items()})
    assert not np.isnan(got["llr"][others]).any()


@pytest.mark.parametrize("nr,nt", [(3, 4), (8, 9)], ids=["lane", "wave"])
def test_more_streams_than_antennas(gpu, nr, nt):
    """nt > nr: zero forcing fails on every vector (A is singular), MMSE does not -- and a shared H behaves as its replicas."""
    md, B = modem_of(4), 70
    y, h = L.conditioned_inputs(32, B, nr, nt, md.constellation, True, 4.0)
    zf = run(y, h, md, 0.0)
    assert np.isnan(zf["xhat"].view(np.float64)).all() and np.isnan(zf["nu"]).all() and np.isnan(zf["llr"]).all()
    assert not zf["idx"].any()
    mm = run(y, h, md, 1.0)
    assert np.isfinite(mm["llr"]).all() and np.isfinite(mm["nu"]).all()
    # one failing H among good ones, reg = 0: vector 5 alone has a rank-deficient square H
    y, h = L.conditioned_inputs(33, B, nt, nt, md.constellation, False, 4.0)
    clean = run(y, h, md, 0.0)
    h = h.copy()
    h[5, nt - 1, :] = 0                                           # a zero row leaves rank nt - 1: nr effectively below nt
    got = run(y, h, md, 0.0)
    others = np.arange(B) != 5
    assert np.isnan(got["llr"][5]).all() and not got["idx"][5].any()
    assert same_bits({k: v[others] for k, v in got.items()}, {k: v[others] for k, v in clean.items()})


# ---- bit identity ------------------------------------------------------------------------------------------------------------------

def _dev_run(md, y, h, reg, noise_var, stream=None, want=ALL):
    lib = _lib.load()
    B, nr = y.shape
    nt, nb = h.shape[-1], md.num_bits_symbol
    d_y, d_h = DeviceBuf.from_array(y), DeviceBuf.from_array(h)
    shapes = {'idx': ((B, nt), np.int32), 'llr': ((B, nt * nb), np.float64), 'xhat': ((B, nt), np.complex128), 'nu': ((B, nt), np.float64)}
    bufs = {k: DeviceBuf(int(np.prod(shapes[k][0])) * np.dtype(shapes[k][1]).itemsize) for k in want}
    _lib.check(lib.cpx_mimo_linear_dev(md._device_handle(), d_y.ptr, d_h.ptr, int(h.ndim == 3), B, nr, nt, reg, noise_var,
                                       *[bufs[k].ptr if k in bufs else None for k in ALL], stream))
    _lib.check(lib.cpx_stream_sync(stream))
    return {k: bufs[k].to_array(*shapes[k]) for k in want}


@pytest.mark.parametrize("nr,nt,m", [(4, 4, 16), (5, 3, 64), (8, 8, 4), (10, 9, 4)], ids=["4x4", "5x3", "8x8", "10x9_wave"])
def test_bit_identity(gpu, nr, nt, m):
    md, B = modem_of(m), 333
    y = np.ascontiguousarray(L.conditioned_inputs(41, B, nr, nt, md.constellation, False, L.SMAX_LLR, real=(m == 2))[0],
                             dtype=np.complex128)
    _, h1 = L.conditioned_inputs(42, 1, nr, nt, md.constellation, True, L.SMAX_LLR)
    h1 = np.ascontiguousarray(h1, dtype=np.complex128)
    reg = 0.05
    ref = run(y, h1, md, reg)                                     # shared H
    rep = np.ascontiguousarray(np.broadcast_to(h1, (B, nr, nt)))
    assert same_bits(run(y, rep, md, reg), ref)                   # ... replicated per vector
    for lo, hi in ((0, 1), (0, 64), (1, 66), (64, 127), (100, 333), (332, 333)):     # batch sizes and positions
        part = run(y[lo:hi], rep[lo:hi], md, reg)
        assert same_bits(part, {k: v[lo:hi] for k, v in ref.items()}), (lo, hi)
    perm = np.random.RandomState(1).permutation(B)
    assert same_bits(run(y[perm], h1, md, reg), {k: v[perm] for k, v in ref.items()})
    for k in ALL:                                                 # one output at a time
        assert run(y, h1, md, reg, want=(k,))[k].tobytes() == ref[k].tobytes(), k
    assert same_bits(_dev_run(md, y, rep, reg, L.NOISE_VAR), ref)                     # the device form, default stream
    lib = _lib.load()
    streams = [ctypes.c_void_p(), ctypes.c_void_p()]
    for s in streams:
        _lib.check(lib.cpx_stream_create(ctypes.byref(s)))
    try:
        for s in streams:
            assert same_bits(_dev_run(md, y, h1, reg, L.NOISE_VAR, s), ref)
    finally:
        for s in streams:
            lib.cpx_stream_destroy(s)


# ---- exact ties --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [3, 9], ids=["lane", "wave"])
def test_exact_ties_go_to_the_lowest_index(gpu, n):
    """H = I (real) and y midway between points: A = I, L = I, xhat = y exactly, every distance exact."""
    md = modem_of(16)
    c = md.constellation
    rs = np.random.RandomState(3)
    y = np.zeros((40, n), complex)                                # the origin: four points tie on every stream
    y[1:20] = c[rs.randint(0, 16, (19, n))] + rs.choice([1.0, -1.0, 1j, -1j], (19, n))        # one-axis midpoints
    y[20:] = c[rs.randint(0, 16, (20, n))] + rs.choice([1 + 1j, 1 - 1j, -1 + 1j, -1 - 1j], (20, n))
    inside = (np.abs(y.real) <= 3) & (np.abs(y.imag) <= 3)
    y = np.where(inside, y, 0)
    got = run(y, np.eye(n), md, 0.0)
    assert np.array_equal(got["xhat"], y) and np.all(got["nu"] == L.NOISE_VAR)
    d = L._sq(y[:, :, None] - c[None, None, :])
    assert np.all(np.sum(d == d.min(axis=2, keepdims=True), axis=2) >= 2)            # every decision is a tie
    assert np.array_equal(got["idx"], np.argmin(d, axis=2))                           # argmin: the first minimum
    w = L.linear_model(y, np.eye(n), c, 0.0, L.NOISE_VAR)
    assert np.array_equal(got["idx"], w["idx"]) and np.array_equal(got["llr"], w["llr"])
