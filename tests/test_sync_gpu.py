"""The timing / frequency-offset synchroniser on the MI355X (csrc/sync.hip) against the NumPy model of sync_model.py.

Tolerances, derived rather than tuned.  On Gaussian-integer samples (|re|, |im| <= 64) every product and every partial sum is an
integer far below 2^53, so P and E are exact whatever the order of summation and must equal the model bit for bit; M is five
roundings (two quotients, two squares, one sum; at most 4 x 2^-53 relative, 2 ulp) from |P|^2 / E^2: the issue's 4 ulp.  On random samples P and E stay within the issue's bound
2 (W + 2048 + 8) 2^-53 sqrt(2) sum |y_i| |y_{i+D}| over [d - 2048, d + W + 2048) (sync_model.bound).  The kernel's tile is 1024, so the
issue's nd list covers its edges.

The figures the tests print (shares of the bound, end-to-end errors) are recorded in profiles/sync_tests_mi355x.txt and DESIGN.md 4.14."""
import ctypes
import itertools

import numpy as np
import pytest

import sync_model as M
from commpy_amd import _lib, modulation
from commpy_amd.channels import multipath_batch
from commpy_amd.deviceops import DeviceBuf, multipath_dev, ofdm_estimate_dev, sync_align_dev, sync_estimate_dev
from commpy_amd.modulation import OfdmPilots, QAMModem, linear_batch, ofdm_estimate_batch, ofdm_map_batch, ofdm_rx_batch, ofdm_tx_batch
from commpy_amd.sync import frame_sync_batch, schmidl_cox_preamble, sync_align_batch, sync_estimate_batch, sync_metric_batch

pytestmark = pytest.mark.gpu
I64MAX = 2 ** 63 - 1


def cplx(rs, *shape):
    return rs.randn(*shape) + 1j * rs.randn(*shape)


def gint(rs, *shape):
    """Gaussian integers, |re|, |im| <= 64."""
    return rs.randint(-64, 65, shape) + 1j * rs.randint(-64, 65, shape)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def user_stream(gpu):
    lib = _lib.load()
    st = ctypes.c_void_p()
    _lib.check(lib.cpx_stream_create(ctypes.byref(st)))
    yield st
    lib.cpx_stream_sync(st)
    lib.cpx_stream_destroy(st)


def check_m(Mdev, P, E):
    """M within 4 ulp of |P|^2 / E^2 (extended precision), exactly +0 where E is 0."""
    ref = M.metric_of(P.astype(M.CLD), E.astype(M.LD))
    assert np.all(np.abs(Mdev.astype(M.LD) - ref) <= 4 * np.spacing(ref.astype(float)))
    assert not np.any(np.signbit(Mdev[E == 0])) and np.all(Mdev[E == 0] == 0)


def check_search(y, D, W, Mdev, Pdev, search=None):
    """estimate against the DEVICE's own metric: first argmax, the peak's bits, the step's 8 ulp of pi / D."""
    d, peak, step = sync_estimate_batch(y, D, W, search)
    lo, hi = (0, None) if search is None else search
    assert np.array_equal(d, M.first_argmax(Mdev, lo, hi))
    rows = np.arange(len(d))
    assert same_bits(peak, Mdev[rows, d])
    P = Pdev[rows, d]
    assert np.all(np.abs(step + np.arctan2(P.imag, P.real) / D) <= 8 * 2.0 ** -53 * np.pi / D)
    return d, peak, step


# ---- exact on Gaussian integers -----------------------------------------------------------------------------------------------
NDS, WS, DS, NRS = [1, 2, 1023, 1024, 1025, 2047, 2049, 4100], [1, 2, 16, 1000, 1024, 1025, 3000], [1, 16, 1024, 2500], [1, 2, 3]
# 40 of the issue's combinations: every nd with five windows, lags and antenna counts rotating; then windows of whole tiles (no
# remainder, with and without tiles in between) and the largest lag and window the issue names
EXACT = [(nd, WS[(i + j) % 7], DS[(i + 2 * j) % 4], NRS[(i + j) % 3]) for i, nd in enumerate(NDS) for j in range(5)] + \
        [(2049, 2048, 16, 1), (1025, 4096, 1, 2), (2, 8192, 8192, 1), (1500, 5000, 3, 1)]


@pytest.mark.parametrize("nd, W, D, nr", EXACT)
def test_exact_on_gaussian_integers(gpu, nd, W, D, nr):
    rs = np.random.RandomState(nd * 7 + W)
    y = gint(rs, 2, nr, nd + D + W - 1)
    Mdev, E, P = sync_metric_batch(y, D, W, want=('m', 'e', 'p'))
    totals = W // 1024 >= 2 or (W // 1024 >= 1 and W % 1024 > 0)
    assert _lib.last_kernel() == ("sync_totals_kernel+" if totals else "") + "sync_metric_kernel"
    Pm, Em, _ = M.metric(y, D, W)
    assert P.shape == (2, nd) and same_bits(P, Pm) and same_bits(E, Em)
    check_m(Mdev, P, E)
    check_search(y, D, W, Mdev, P)


# ---- random samples: the summation bound --------------------------------------------------------------------------------------
RANDOM = [(1, 1, 1, 1), (1025, 16, 16, 2), (2049, 1000, 1, 3), (1023, 1025, 1024, 1), (4100, 3000, 2500, 2), (2047, 1024, 16, 1),
          (4100, 2, 1, 1), (1024, 5000, 16, 1)]
_shares = {}


def bound_shares(y, D, W):
    P, E = sync_metric_batch(y, D, W, want=('e', 'p'))[::-1]
    Pm, Em = M.windows(y, D, W)
    bp, be = M.bound(y, D, W)
    ep, ee = np.abs(P.astype(M.CLD) - Pm).astype(float), np.abs(E.astype(M.LD) - Em).astype(float)
    assert np.all(ep <= bp) and np.all(ee <= be)
    return np.max(ep / bp), np.max(ee / be)


@pytest.mark.parametrize("nd, W, D, nr", RANDOM)
def test_random_within_bound(gpu, nd, W, D, nr):
    y = cplx(np.random.RandomState(nd + W + D), 2, nr, nd + D + W - 1)
    sp, se = bound_shares(y, D, W)
    _shares[(nd, W, D, nr)] = (sp, se)
    print("sync bound", (nd, W, D, nr), "largest share of the bound: P %.2e, E %.2e" % (sp, se),
          "| so far: P %.2e, E %.2e" % tuple(np.max(list(_shares.values()), axis=0)))


@pytest.mark.parametrize("W, D", [(16, 16), (1000, 16), (1500, 64)])
def test_loud_half_does_not_leak(gpu, W, D):
    """The first half of the row is 1e8 times louder than the second: a window more than 2048 positions into the quiet half has a
    bound that knows nothing of the loud one, and must keep it."""
    n = 9000
    y = cplx(np.random.RandomState(W), 1, 2, n)
    y[:, :, :n // 2] *= 1e8
    sp, se = bound_shares(y, D, W)
    print("sync bound, loud half", (W, D), "largest share of the bound: P %.2e, E %.2e" % (sp, se))


# ---- the search ---------------------------------------------------------------------------------------------------------------
def test_search_ranges(gpu):
    D, W = 16, 32
    y = cplx(np.random.RandomState(2), 3, 2, 5000)
    Mdev, P = sync_metric_batch(y, D, W, want=('m', 'p'))
    nd = Mdev.shape[1]
    for search in (None, (0, I64MAX), (100, 101), (1023, 1024), (1024, 1025), (1000, 1100), (1023, 1025), (1500, 3000), (-5, 10),
                   (nd - 1, 10 ** 9), (2047, 4097)):
        d, _, _ = check_search(y, D, W, Mdev, P, search)
        assert np.all(d >= 0)
    assert _lib.last_kernel() == "sync_search_kernel+sync_finish_kernel"
    # with totals between the window's ends
    D, W = 8, 2500
    Mdev, P = sync_metric_batch(y, D, W, want=('m', 'p'))
    for search in (None, (1100, 1101), (900, 2100)):
        check_search(y, D, W, Mdev, P, search)
    assert _lib.last_kernel() == "sync_totals_kernel+sync_search_kernel+sync_finish_kernel"


def test_search_ties_zeros_and_nans(gpu):
    D = W = 64
    n = 4000
    rs = np.random.RandomState(3)
    half = gint(rs, 2, D)
    half[half == 0] = 1 + 1j
    y = np.zeros((3, 2, n), complex)
    for at in (700, 2900):                                  # two identical preambles, in different tiles: M = 1 exactly at both
        y[0, :, at:at + D] = half
        y[0, :, at + D:at + 2 * D] = half
    y[2] = np.nan
    Mdev, P = sync_metric_batch(y, D, W, want=('m', 'p'))
    assert Mdev[0, 700] == 1.0 and Mdev[0, 2900] == 1.0 and np.count_nonzero(Mdev[0] >= 1.0) == 2
    d, peak, step = sync_estimate_batch(y, D, W)
    assert list(d) == [700, 0, -1]
    assert peak[0] == 1.0 and step[0] == 0 and peak[1] == 0 and not np.signbit(peak[1]) and step[1] == 0
    assert np.isnan(peak[2]) and np.isnan(step[2])
    d, peak, _ = sync_estimate_batch(y, D, W, (701, n))
    assert list(d) == [2900, 701, -1] and peak[0] == 1.0


# ---- bit identity -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D, W", [(32, 32), (16, 1100)])           # without and with the totals launch
def test_bit_identity(gpu, user_stream, D, W):
    lib = _lib.load()
    rs = np.random.RandomState(4)
    B, nr, n, nout = 7, 2, 3000, 2500
    y = cplx(rs, B, nr, n)
    nd = n - D - W + 1
    start, step = rs.randint(-50, 600, B).astype(np.int64), rs.randn(B) * 1e-2
    d_y, d_start, d_step = DeviceBuf.from_array(y), DeviceBuf.from_array(start), DeviceBuf.from_array(step)

    def device_calls(st):
        d_P, d_E, d_M = DeviceBuf(B * nd * 16), DeviceBuf(B * nd * 8), DeviceBuf(B * nd * 8)
        _lib.check(lib.cpx_sync_metric_dev(d_y.ptr, B, nr, n, D, W, d_P.ptr, d_E.ptr, d_M.ptr, st))
        d_d, d_pk, d_st = sync_estimate_dev(d_y, B, nr, n, D, W, stream=st)
        d_out = sync_align_dev(d_y, B, nr, n, d_start, d_step, nout, stream=st)
        _lib.check(lib.cpx_stream_sync(st))
        return (d_M.to_array((B, nd), np.float64), d_E.to_array((B, nd), np.float64), d_P.to_array((B, nd), np.complex128),
                d_d.to_array((B,), np.int64), d_pk.to_array((B,), np.float64), d_st.to_array((B,), np.float64),
                d_out.to_array((B, nr, nout), np.complex128))

    host = sync_metric_batch(y, D, W, want=('m', 'e', 'p')) + sync_estimate_batch(y, D, W) + (sync_align_batch(y, start, step, nout),)
    for st in (None, user_stream):                          # the _dev form, on the null stream and on a user's
        assert all(same_bits(a, b) for a, b in zip(device_calls(st), host))
    for row in (2, 5):                                      # B = 1 against places 0 and last of B = 7
        alone = sync_metric_batch(y[row:row + 1], D, W, want=('m', 'e', 'p')) + sync_estimate_batch(y[row:row + 1], D, W) + \
            (sync_align_batch(y[row:row + 1], start[row:row + 1], step[row:row + 1], nout),)
        assert all(same_bits(a[0], b[row]) for a, b in zip(alone, host))
        for order in ([row] + [i for i in range(B) if i != row], [i for i in range(B) if i != row] + [row]):
            place = order.index(row)
            moved = sync_metric_batch(y[order], D, W, want=('m', 'e', 'p')) + sync_estimate_batch(y[order], D, W) + \
                (sync_align_batch(y[order], start[order], step[order], nout),)
            assert all(same_bits(a[place], b[row]) for a, b in zip(moved, host))
    names = dict(zip('mep', host[:3]))
    for k in (1, 2):                                        # every subset of (P, E, M)
        for want in itertools.combinations('mep', k):
            out = sync_metric_batch(y, D, W, want=want)
            assert len(out) == k and all(same_bits(a, names[w]) for a, w in zip(out, want))


def test_nan_and_inf_stay_in_their_row(gpu):
    D, W = 16, 1100
    y = cplx(np.random.RandomState(5), 3, 2, 4000)
    clean = sync_metric_batch(y, D, W, want=('m', 'e', 'p')) + sync_estimate_batch(y, D, W)
    for bad, at in ((np.nan, 1500), (np.inf, 10), (-np.inf + 1j, 3999)):
        yb = y.copy()
        yb[1, 1, at] = bad
        out = sync_metric_batch(yb, D, W, want=('m', 'e', 'p')) + sync_estimate_batch(yb, D, W)
        for a, b in zip(out, clean):
            assert same_bits(a[[0, 2]], b[[0, 2]])
        Mrow, d = out[0][1], out[3][1]
        assert np.isnan(Mrow).any()
        assert d == M.first_argmax(Mrow[None])[0]           # -1, or the first argmax of the row's finite values
        if d >= 0:
            assert same_bits(out[4][1], Mrow[d])
        else:
            assert np.isnan(out[4][1]) and np.isnan(out[5][1])


# ---- grid wrap and 64-bit offsets ---------------------------------------------------------------------------------------------
def test_more_rows_than_the_grid(gpu):
    B, n, D, W = 70001, 8, 2, 3
    y = gint(np.random.RandomState(6), B, 1, n)
    Mdev, E, P = sync_metric_batch(y, D, W, want=('m', 'e', 'p'))
    Pm, Em, _ = M.metric(y, D, W)
    assert same_bits(P, Pm) and same_bits(E, Em)
    check_m(Mdev, P, E)
    check_search(y, D, W, Mdev, P)
    check_search(y[:, 0], D, W, Mdev, P, (1, 3))


def _poke(buf, start, arr):
    _lib.check(_lib.load().cpx_memcpy_h2d(ctypes.c_void_p(buf.ptr.value + start * arr.itemsize), _lib.ptr(arr), arr.nbytes))


def _peek(buf, start, count, dtype):
    out = np.zeros(count, dtype)
    _lib.check(_lib.load().cpx_memcpy_d2h(_lib.ptr(out), ctypes.c_void_p(buf.ptr.value + start * out.itemsize), out.nbytes))
    return out


def test_large_row(gpu):
    """One row of 2^27 + 5 samples (2 GB): 131 073 tiles, more than the grid, and offsets past 2^31 bytes.  An integer preamble sits
    in the last 1000 samples of an otherwise silent row; the tail of M and d^ are compared."""
    lib = _lib.load()
    n, D, W = 2 ** 27 + 5, 32, 32
    nd = n - D - W + 1
    rs = np.random.RandomState(7)
    half = gint(rs, D)
    half[half == 0] = 1 - 1j
    tail = np.zeros(2000, complex)
    at = 2000 - 1000 + 300
    tail[at:at + 2 * D] = np.concatenate([half, half])
    tail[1900:1950] = gint(rs, 50)                          # and something that is not a preamble
    d_y, d_M = DeviceBuf(16 * n), DeviceBuf(8 * nd)
    _lib.check(lib.cpx_memset(d_y.ptr, 0, 16 * n))
    _poke(d_y, n - 2000, tail)
    _lib.check(lib.cpx_sync_metric_dev(d_y.ptr, 1, 1, n, D, W, None, None, d_M.ptr, None))
    d_d, d_pk, d_st = sync_estimate_dev(d_y, 1, 1, n, D, W)
    _lib.check(lib.cpx_stream_sync(None))
    Pm, Em, _ = M.metric(tail[None, None], D, W)
    got = _peek(d_M, nd - Pm.shape[1], Pm.shape[1], np.float64)
    check_m(got[None], Pm, Em)
    assert got[at] == 1.0 and np.count_nonzero(got >= 1.0) == 1
    assert not _peek(d_M, 0, 5000, np.float64).any() and not _peek(d_M, 2 ** 26 - 2500, 5000, np.float64).any()
    assert d_d.to_array((1,), np.int64)[0] == n - 2000 + at and d_pk.to_array((1,), np.float64)[0] == 1.0
    assert d_st.to_array((1,), np.float64)[0] == 0
    for b in (d_y, d_M):
        b.free()


# ---- align --------------------------------------------------------------------------------------------------------------------
def test_align_equals_freq_offset(gpu):
    lib = _lib.load()
    rs = np.random.RandomState(8)
    B, nr, n = 3, 2, 2500
    y, step = cplx(rs, B, nr, n), np.array([0.3, -1e-3, 2.5e4])
    want = np.zeros_like(y)
    per_row = np.repeat(step, nr)
    _lib.check(lib.cpx_freq_offset(_lib.ptr(y), B * nr, n, _lib.ptr(per_row), 1, _lib.ptr(want)))
    assert same_bits(sync_align_batch(y, 0, step, n), want)
    assert _lib.last_kernel() == "sync_align_kernel"
    assert same_bits(sync_align_batch(y[:, 0], np.zeros(B, int), step, n), want[:, 0])
    # a NaN step stays in its row
    bad = step.copy()
    bad[1] = np.nan
    out = sync_align_batch(y, 0, bad, n)
    assert same_bits(out[[0, 2]], want[[0, 2]]) and np.isnan(out[1]).all()


def test_align_gathers_exactly(gpu):
    rs = np.random.RandomState(9)
    B, nr, n, nout = 6, 2, 1500, 2100                       # nout > n
    y = cplx(rs, B, nr, n)
    start = np.array([-700, 0, 37, n - 1, n, -nout - 5], dtype=np.int64)       # negative, inside, the last sample, past the end, all before
    out = sync_align_batch(y, start, None, nout)
    assert same_bits(out, M.align(y, start, None, nout))     # the zeros are +0
    assert same_bits(sync_align_batch(y, -3, None, 10), M.align(y, [-3] * B, None, 10))
    # the offset argument of the device form is added to start inside the kernel
    d_y, d_start = DeviceBuf.from_array(y), DeviceBuf.from_array(start + 16)
    d_out = sync_align_dev(d_y, B, nr, n, d_start, None, nout, offset=-16)
    assert same_bits(d_out.to_array((B, nr, nout), np.complex128), out)
    step = rs.randn(B) * 0.01
    rot = sync_align_batch(y, start, step, nout)
    ref = M.align(y, start, step, nout)
    assert np.max(np.abs(rot - ref)) <= 4 * 2.0 ** -53 * np.max(np.abs(y)) * (1 + nout * np.max(np.abs(step)))
    d_step = DeviceBuf.from_array(step)
    d_out = sync_align_dev(d_y, B, nr, n, d_start, d_step, nout, offset=-16)
    assert same_bits(d_out.to_array((B, nr, nout), np.complex128), rot)


# ---- end to end ---------------------------------------------------------------------------------------------------------------
E2E = {
    "siso": dict(nfft=64, nsc=52, cp=16, nsym=4, nt=1, nr=1, L=4, m=16, count=156),
    "2x2": dict(nfft=64, nsc=52, cp=16, nsym=4, nt=2, nr=2, L=4, m=16, count=312),
    "2x3": dict(nfft=256, nsc=200, cp=32, nsym=3, nt=2, nr=3, L=6, m=64, count=800),
}


def frame(c, rs):
    """(pilots, modem, data indices [1, ndata, nt], tx [1, nt, (nsym + 1)(nfft + cp)]): block pilots on all of symbol 0, antenna t on
    the subcarriers k % nt == t, and the same Schmidl-Cox preamble from every antenna ahead of the frame."""
    nfft, nsc, cp, nsym, nt = c["nfft"], c["nsc"], c["cp"], c["nsym"], c["nt"]
    k = np.arange(nsc)
    p = OfdmPilots(nsc, nsym, nt, np.zeros(nsc, int), k, k % nt, np.exp(0.5j * np.pi * np.random.RandomState(nsc).randint(0, 4, nsc)),
                   ('taps', cp + c["L"], nfft))
    md = QAMModem(c["m"])
    idx = rs.randint(0, c["m"], size=(1, p.ndata, nt))
    assert idx.size == c["count"]
    grid = ofdm_map_batch(md.constellation[idx], p)                                # [1, nt, nsym, nsc]
    pre = np.broadcast_to(schmidl_cox_preamble(nfft, nsc), (1, nt, 1, nsc))
    full = np.concatenate([pre, grid], axis=2)
    tx = ofdm_tx_batch(full.reshape(nt, nsym + 1, nsc), nfft, cp).reshape(1, nt, -1)
    return p, md, idx, tx


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("case", sorted(E2E))
def test_end_to_end_noise_free(gpu, case, seed):
    lib = _lib.load()
    c = E2E[case]
    nfft, nsc, cp, nsym, nt, nr, L = c["nfft"], c["nsc"], c["cp"], c["nsym"], c["nt"], c["nr"], c["L"]
    rs = np.random.RandomState(seed)
    p, md, idx, tx = frame(c, rs)
    g = cplx(rs, 1, nr, nt, L) * np.sqrt(0.5) * np.exp(-0.7 * np.arange(L))
    delay = int(rs.randint(0, 100))
    eps = rs.uniform(-0.45, 0.45) / (nfft // 2)                                    # cycles per sample
    rx = multipath_batch(tx, g)
    rows = np.concatenate([np.zeros((1, nr, delay)), rx, np.zeros((1, nr, 37))], axis=2)
    n = rows.shape[2]
    shifted, step_in = np.zeros_like(rows), np.full(nr, 2 * np.pi * eps)
    _lib.check(lib.cpx_freq_offset(_lib.ptr(rows), nr, n, _lib.ptr(step_in), 1, _lib.ptr(shifted)))
    nout = (nsym + 1) * (nfft + cp)
    aligned, d_hat, peak, step = frame_sync_batch(shifted, nfft, cp, nout)
    eps_hat = -step[0] / (2 * np.pi)
    Y = ofdm_rx_batch(aligned.reshape(nr, nout), nfft, nsc, cp).reshape(1, nr, nsym + 1, nsc)[:, :, 1:]
    y, h = ofdm_estimate_batch(np.ascontiguousarray(Y), p)
    det = linear_batch(y.reshape(-1, nr), h.reshape(-1, nr, nt), md, 0, method='zf', output_type='hard')
    wrong = int(np.count_nonzero(det.reshape(1, p.ndata, nt) != md.constellation[idx]))
    print("sync end to end", case, seed, "delay %d, d^ %d (plateau %d..%d), peak 1 - %.1e, |eps^ - eps| = %.1e, wrong %d of %d"
          % (delay, d_hat[0], delay + L - 1, delay + cp, 1 - peak[0], abs(eps_hat - eps), wrong, idx.size))
    assert delay + L - 1 <= d_hat[0] <= delay + cp                                  # the ISI-free plateau
    assert abs(eps_hat - eps) <= 1e-12
    assert wrong == 0


def test_device_chain_matches_staged_host_calls(gpu, user_stream):
    """multipath -> frequency offset -> awgn -> sync_estimate -> sync_align (offset = -cp added to d^ inside the kernel) -> ofdm_rx ->
    ofdm_estimate on one stream, nothing copied to the host in between, against the same stages called one by one on host arrays."""
    lib = _lib.load()
    st = user_stream
    c = dict(E2E["2x2"], nr=2)
    nfft, nsc, cp, nsym, nt, nr, L = c["nfft"], c["nsc"], c["cp"], c["nsym"], c["nt"], c["nr"], c["L"]
    rs = np.random.RandomState(11)
    B = 3
    frames = [frame(c, rs) for _ in range(B)]
    p = frames[0][0]
    per = (nsym + 1) * (nfft + cp)
    n_tx = 100 + per + 37
    tx = np.zeros((B, nt, n_tx), complex)
    for b, delay in enumerate((0, 41, 99)):
        tx[b, :, delay:delay + per] = frames[b][3][0]
    g = cplx(rs, B, nr, nt, L) * np.sqrt(0.5) * np.exp(-0.7 * np.arange(L))
    n = n_tx + L - 1
    step_in = np.repeat(2 * np.pi * rs.uniform(-0.45, 0.45, B) / (nfft // 2), nr)
    sigma, seed, sid = 1e-5, 5, 3
    plan = modulation._ofdm_plan(nfft, nsc, cp).handle()

    def awgn(d_in, d_out, stream):
        _lib.check(lib.cpx_awgn_dev(d_in.ptr, B * nr * n, sigma, sigma, seed, sid, d_out.ptr, stream))

    # staged: every stage on host arrays
    rx = multipath_batch(tx, g)
    shifted = np.zeros_like(rx)
    _lib.check(lib.cpx_freq_offset(_lib.ptr(rx), B * nr, n, _lib.ptr(step_in), 1, _lib.ptr(shifted)))
    d_clean, d_noisy = DeviceBuf.from_array(shifted), DeviceBuf(shifted.nbytes)
    awgn(d_clean, d_noisy, None)
    noisy = d_noisy.to_array(rx.shape, np.complex128)
    assert not same_bits(noisy, shifted)
    d_hat, peak, step = sync_estimate_batch(noisy, nfft // 2, nfft // 2)
    aligned = sync_align_batch(noisy, d_hat - cp, step, per)
    Y = ofdm_rx_batch(aligned.reshape(B * nr, per), nfft, nsc, cp)
    # the chain
    d_tx, d_g, d_step_in = DeviceBuf.from_array(tx), DeviceBuf.from_array(g), DeviceBuf.from_array(step_in)
    d_sh, d_rxn, d_Y = DeviceBuf(rx.nbytes), DeviceBuf(rx.nbytes), DeviceBuf(Y.nbytes)
    d_rx = multipath_dev(d_tx, d_g, 1, B, nt, nr, n_tx, L, stream=st)
    _lib.check(lib.cpx_freq_offset_dev(d_rx.ptr, B * nr, n, d_step_in.ptr, 1, d_sh.ptr, st))
    awgn(d_sh, d_rxn, st)
    d_d, d_pk, d_st = sync_estimate_dev(d_rxn, B, nr, n, nfft // 2, nfft // 2, stream=st)
    d_al = sync_align_dev(d_rxn, B, nr, n, d_d, d_st, per, offset=-cp, stream=st)
    _lib.check(lib.cpx_ofdm_rx_dev(plan, d_al.ptr, B * nr, per, d_Y.ptr, st))
    _lib.check(lib.cpx_stream_sync(st))
    assert same_bits(d_d.to_array((B,), np.int64), d_hat) and same_bits(d_st.to_array((B,), np.float64), step)
    assert same_bits(d_al.to_array(aligned.shape, np.complex128), aligned)
    assert same_bits(d_Y.to_array(Y.shape, np.complex128), Y)
    # the frame's own estimator takes it from there: symbol 0 of Y is the preamble, which the estimator's frame does not hold, so the
    # frame's symbols are copied out on the device before it runs
    Yf = np.ascontiguousarray(Y.reshape(B, nr, nsym + 1, nsc)[:, :, 1:])
    d_Yf = DeviceBuf(Yf.nbytes)
    sym = nsc * 16
    for row in range(B * nr):
        _lib.check(lib.cpx_memcpy_d2d_async(ctypes.c_void_p(d_Yf.ptr.value + row * nsym * sym),
                                            ctypes.c_void_p(d_Y.ptr.value + (row * (nsym + 1) + 1) * sym), nsym * sym, st))
    d_yd, d_hd = ofdm_estimate_dev(p, d_Yf, B, nr, stream=st)
    _lib.check(lib.cpx_stream_sync(st))
    y, h = ofdm_estimate_batch(Yf, p)
    assert same_bits(d_yd.to_array(y.shape, np.complex128), y) and same_bits(d_hd.to_array(h.shape, np.complex128), h)
    for b, delay in enumerate((0, 41, 99)):
        assert delay + L - 1 <= d_hat[b] <= delay + cp
