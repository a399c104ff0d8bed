"""OFDM transmit / receive on the MI355X (csrc/ofdm.hip) against the extended-precision model (ofdm_model.py): derived error
bounds, output coverage and guard words, grid wrap of both kernels, the direct DFT up to its limit size, batched RX with
leftover samples, non-finite isolation.  Each test prints what it measured (pytest -s shows it); DESIGN 4.9 records the figures."""
import ctypes
import time

import numpy as np
import pytest

import ofdm_model as om
from commpy_amd import _lib
from commpy_amd.modulation import ofdm_rx, ofdm_rx_batch, ofdm_tx_batch
from ofdm_model import LD, U
from test_ofdm_gpu import DevBuf, _plan
from test_ofdm_host import prefix_len

pytestmark = [pytest.mark.gpu, om.requires_longdouble]

uLD = LD(U)


def cplx(rs, *shape):
    return rs.randn(*shape) + 1j * rs.randn(*shape)


def note(fmt, *args):
    print("ofdm-measure: " + fmt % args)


def spw(nfft):
    """Symbols per workgroup of the fast kernel."""
    return max(1, 4096 // nfft)


def nsc_default(nfft):
    return max(2, 2 * int(0.4 * nfft))


def tx_split(t, nfft, cp):
    """[B, nsym * (P + nfft)] -> (prefix [B, nsym, P], body [B, nsym, nfft]); the prefix must be the body's tail, bit for bit."""
    P = prefix_len(nfft, cp)
    t = t.reshape(t.shape[0], -1, P + nfft)
    prefix, body = t[:, :, :P], t[:, :, P:]
    assert prefix.tobytes() == np.ascontiguousarray(body[:, :, nfft - P:]).tobytes()
    return prefix, body


def rx_unique(got, nfft, nsc):
    """got [.., nsc] -> (got at one position per distinct bin, those bins); a bin that is output twice must be the same twice."""
    bin_of = om.rx_bin_of(nfft, nsc)
    uniq, first, inv = np.unique(bin_of, return_index=True, return_inverse=True)
    one = got[..., first]
    assert np.ascontiguousarray(one[..., inv]).tobytes() == np.ascontiguousarray(got).tobytes()
    return one, uniq


# ---- 1. accuracy of the fast kernel under bound (a) ----------------------------------------------------------------------------------
def fast_tx_error(t, x, nfft, cp):
    """Per-symbol ||got - ref||_2 / (u ||ref||_2) of TX, asserted under fast_bound; returns the largest."""
    _, body = tx_split(t, nfft, cp)
    _, ref = tx_split(om.ref_tx_batch(x, nfft, cp), nfft, cp)
    err, size = om.norm2(body - ref), om.norm2(ref)
    assert np.all(err <= om.fast_bound(nfft) * uLD * size), float(np.max(err / (uLD * size)))
    return float(np.max(err / (uLD * size)))


def fast_rx_error(r, y, nfft, nsc, cp):
    """The same for RX.  The bound is on the whole transform, so the error of the bins RX returns is set against the norm of
    all nfft bins, sqrt(nfft) ||samples||_2 (Parseval)."""
    got, bins = rx_unique(r, nfft, nsc)
    ref = om.ref_rx_batch(y, nfft, nsc, cp, bins=bins)
    size = np.sqrt(LD(nfft)) * om.norm2(om.rx_bodies(y, nfft, cp).astype(om.CLD))
    err = om.norm2(got - ref)
    assert np.all(err <= om.fast_bound(nfft) * uLD * size), float(np.max(err / (uLD * size)))
    return float(np.max(err / (uLD * size)))


@pytest.mark.parametrize("nfft", [2 ** k for k in range(1, 14)])
def test_fast_kernel_is_inside_its_derived_bound(gpu, nfft):
    """One full tile and a partial one (SPW + 1 symbols), every nsc / cp edge, TX and RX, each symbol under bound (a)."""
    rs = np.random.RandomState(nfft)
    nsym = spw(nfft) + 1
    worst_tx = worst_rx = 0.0
    for nsc in sorted({v for v in (2, nfft, 2 * (nfft - 1), 2 * int(0.4 * nfft)) if v >= 2 and v // 2 <= nfft - 1}):
        x = cplx(rs, 1, nsym, nsc)
        for cp in sorted({0, 1, nfft // 4}):
            t = ofdm_tx_batch(x, nfft, cp)
            assert "ofdm_fast_kernel<%d,tx>" % nfft in _lib.last_kernel()
            worst_tx = max(worst_tx, fast_tx_error(t, x, nfft, cp))
            y = t + 0.1 * float(np.sqrt(np.mean(np.abs(t) ** 2))) * cplx(rs, *t.shape)
            r = ofdm_rx_batch(y, nfft, nsc, cp)
            assert "ofdm_fast_kernel<%d,rx>" % nfft in _lib.last_kernel()
            assert r.shape == (1, y.shape[1] // (nfft + cp), nsc)
            worst_rx = max(worst_rx, fast_rx_error(r, y, nfft, nsc, cp))
    note("fast nfft=%d largest per-symbol error tx %.2f u, rx %.2f u, bound %.1f u", nfft, worst_tx, worst_rx, om.fast_bound(nfft))


# ---- 2. scaling by a power of two is exact ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nfft", [64, 8192, 100, 1536])
def test_power_of_two_scaling_is_exact(gpu, nfft):
    """x 2^40 and x 2^-40 give the outputs times 2^40 / 2^-40 exactly: no absolute threshold, no flush in the arithmetic."""
    rs = np.random.RandomState(nfft)
    nsc, cp = nsc_default(nfft), nfft // 4
    x = cplx(rs, 1, 3, nsc)
    y = cplx(rs, 1, 3 * (nfft + cp) + 5)
    t, r = ofdm_tx_batch(x, nfft, cp), ofdm_rx_batch(y, nfft, nsc, cp)
    assert np.all(np.isfinite(t.view(float))) and np.all(t != 0) and np.all(r != 0)
    for s in (2.0 ** 40, 2.0 ** -40):
        assert ofdm_tx_batch(x * s, nfft, cp).tobytes() == (t * s).tobytes()
        assert ofdm_rx_batch(y * s, nfft, nsc, cp).tobytes() == (r * s).tobytes()


# ---- 3. sparse inputs under bound (b), every output element ----------------------------------------------------------------------------
FAST_SPARSE = [16, 64, 512, 4096, 8192]
DFT_SPARSE = [3, 2049, 4100, 12288, 16384, 65536]


def factors_of(nfft):
    return om.fast_factors(nfft) if nfft in FAST_SPARSE else 1


def kernel_of(nfft, way):
    return ("ofdm_fast_kernel<%d,%s>" if nfft in FAST_SPARSE else "ofdm_dft_kernel<%d,%s>") % (nfft, way)


def sparse_cases(nfft, places, rs):
    """[(index, value), ..] lists: 1 - 2j alone at each place, then three values at once (the first, the middle, the last)."""
    cases = [[(p, 1 - 2j)] for p in places]
    three = sorted({places[0], places[len(places) // 2], places[-1]})
    cases.append([(p, complex(*rs.randn(2))) for p in three])
    return cases


def call_per_symbol(fn, arr, per_call):
    """fn over the symbols of arr [1, nsym, ..] in groups of per_call, the outputs joined along the symbol axis."""
    return np.concatenate([fn(arr[:, i:i + per_call]) for i in range(0, arr.shape[1], per_call)], axis=1)


@pytest.mark.parametrize("nfft", FAST_SPARSE + DFT_SPARSE)
def test_sparse_rx_every_bin(gpu, nfft):
    """Impulses in time: every bin RX returns is within bound (b) of x W^(k n0) in extended precision.  nsc = 2 (nfft - 1) returns
    bins 1 .. nfft - 1 (twice); one sample of prefix holds a value that must not be read."""
    rs = np.random.RandomState(nfft)
    nsc, cp = 2 * (nfft - 1), 1
    chunk_edge = () if nfft in FAST_SPARSE else (2047, 2048)              # either side of the direct DFT's first LDS chunk
    places = sorted({n for n in (0, 1, nfft - 1) + chunk_edge if n < nfft})
    cases = sparse_cases(nfft, places, rs)
    y = np.zeros((1, len(cases), nfft + cp), complex)
    y[:, :, 0] = 7.0 - 3.0j
    for i, case in enumerate(cases):
        for n0, v in case:
            y[0, i, cp + n0] = v
    t0 = time.perf_counter()
    per_call = 1 if nfft >= 16384 else len(cases)
    r = call_per_symbol(lambda part: ofdm_rx_batch(part.reshape(1, -1), nfft, nsc, cp), y, per_call)
    dt = time.perf_counter() - t0
    assert kernel_of(nfft, "rx") in _lib.last_kernel()
    got, bins = rx_unique(r, nfft, nsc)
    ref = om.ref_rx_batch(y.reshape(1, -1), nfft, nsc, cp, bins=bins)
    worst = 0.0
    for i, case in enumerate(cases):
        l1 = LD(sum(abs(v) for _, v in case))
        err = np.abs(got[0, i] - ref[0, i]) / (uLD * l1)
        bound = om.sparse_bound(len(case), factors_of(nfft))
        assert np.all(err <= bound), (case, float(np.max(err)), bound)
        worst = max(worst, float(np.max(err)))
    note("sparse rx nfft=%d: %d symbols in %.2f s, largest element error %.2f u sum|x| (bound %.1f for one impulse)",
         nfft, len(cases), dt, worst, om.sparse_bound(1, factors_of(nfft)))


@pytest.mark.parametrize("nfft", FAST_SPARSE + DFT_SPARSE)
def test_sparse_tx_every_sample(gpu, nfft):
    """Single subcarriers (the first, the two either side of the fold, the last) and three at once: every sample TX returns,
    prefix included, is within bound (b) of the tone in extended precision."""
    rs = np.random.RandomState(nfft + 1)
    nsc, cp = nsc_default(nfft), 1
    h = nsc // 2
    cases = sparse_cases(nfft, sorted({0, h - 1, h, nsc - 1}), rs)
    x = np.zeros((1, len(cases), nsc), complex)
    for i, case in enumerate(cases):
        for sc, v in case:
            x[0, i, sc] = v
    t0 = time.perf_counter()
    per_call = 1 if nfft >= 16384 else len(cases)
    t = call_per_symbol(lambda part: ofdm_tx_batch(part, nfft, cp).reshape(1, part.shape[1], -1), x, per_call)
    dt = time.perf_counter() - t0
    assert kernel_of(nfft, "tx") in _lib.last_kernel()
    t = t.reshape(1, -1)
    tx_split(t, nfft, cp)
    ref = om.ref_tx_batch(x, nfft, cp)
    got, ref = t.reshape(len(cases), -1), ref.reshape(len(cases), -1)
    inexact = nfft & (nfft - 1) != 0
    worst = 0.0
    for i, case in enumerate(cases):
        l1 = LD(sum(abs(v) for _, v in case)) / nfft
        err = np.abs(got[i] - ref[i]) / (uLD * l1)
        bound = om.sparse_bound(len(case), factors_of(nfft), inexact)
        assert np.all(err <= bound), (case, float(np.max(err)), bound)
        worst = max(worst, float(np.max(err)))
    note("sparse tx nfft=%d: %d symbols in %.2f s, largest element error %.2f u sum|x| / N (bound %.1f for one subcarrier)",
         nfft, len(cases), dt, worst, om.sparse_bound(1, factors_of(nfft), inexact))


# ---- 4. dense input on the direct DFT: the two assertions of (c) -------------------------------------------------------------------
def dense_check(got, ref, walk, l1, N):
    """got, ref, walk [nsym, nbins], l1 [nsym, 1] = sum|x| of each symbol's transform: every element under dense_bound, and the
    error norm over all of them within DENSE_RATIO_LIMIT of the float64 index-order sum's.  Returns (ratio, error in u)."""
    assert got.shape == ref.shape == walk.shape and got.size >= 64
    assert np.all(np.abs(got - ref) <= om.dense_bound(N) * uLD * l1), float(np.max(np.abs(got - ref) / (uLD * l1)))
    e_got = float(np.sqrt(np.sum(om.norm2(got - ref) ** 2)))
    e_walk = float(np.sqrt(np.sum(om.norm2(walk - ref) ** 2)))
    assert e_got <= om.DENSE_RATIO_LIMIT * e_walk, (e_got, e_walk)
    return e_got / e_walk, float(np.max(om.norm2(got - ref) / (uLD * om.norm2(ref))))


def dense_shape(nfft):
    """(symbols, the step between the bins compared): all bins up to 4100, 64 of them above; at least 64 bins in all."""
    nsym = 1 if nfft >= 16384 else max(2, -(-64 // (nfft - 1)))
    return nsym, (1 if nfft <= 4100 else nfft // 64)


@pytest.mark.parametrize("way", ["tx", "rx"])
@pytest.mark.parametrize("nfft", sorted(DFT_SPARSE + [1536]))
def test_dense_direct_dft(gpu, nfft, way):
    rs = np.random.RandomState(nfft)
    nsc, cp = 2 * (nfft - 1), 1
    nsym, step = dense_shape(nfft)
    t0 = time.perf_counter()
    if way == "tx":
        x = cplx(rs, 1, nsym, nsc)
        t = ofdm_tx_batch(x, nfft, cp)
        dt = time.perf_counter() - t0
        _, body = tx_split(t, nfft, cp)
        pick = np.arange(0, nfft, step)[:64 if step > 1 else nfft]
        F = om.tx_bins(x, nfft)
        got, ref = body[0][:, pick], om.ref_tx_batch(x, nfft, cp, samples=pick)[0]
        walk = om.dft_f64_index_order(F[0], pick, inverse=True)
        l1 = np.sum(np.abs(F[0]), axis=-1, keepdims=True).astype(LD) / nfft
    else:
        y = cplx(rs, 1, nsym * (nfft + cp) + 3)
        r = ofdm_rx_batch(y, nfft, nsc, cp)
        dt = time.perf_counter() - t0
        one, bins = rx_unique(r, nfft, nsc)                             # bins 1 .. nfft - 1
        sel = np.arange(0, bins.size, step)[:64 if step > 1 else bins.size]
        pick = bins[sel]
        body = om.rx_bodies(y, nfft, cp)[0]
        got, ref = one[0][:, sel], om.ref_rx_batch(y, nfft, nsc, cp, bins=pick)[0]
        walk = om.dft_f64_index_order(body, pick)
        l1 = np.sum(np.abs(body), axis=-1, keepdims=True).astype(LD)
    assert "ofdm_dft_kernel<%d,%s>" % (nfft, way) in _lib.last_kernel()
    ratio, err = dense_check(got, ref, walk, l1, nfft)
    note("dense %s nfft=%d: %d symbol(s) in %.2f s, %d bins compared, error norm / float64 index-order sum's = %.3f, "
         "largest per-symbol error %.1f u", way, nfft, nsym, dt, got.shape[1], ratio, err)


# ---- 5. every output element written, and nothing else ------------------------------------------------------------------------------
GUARD = 4096                                     # doubles either side of the result
GUARD_WORD = np.uint64(0x7FF8DEADBEEF0001)        # NaN payloads no computation produces
FILL_WORD = np.uint64(0x7FF8F111F111F111)


def guarded_call(call, n_out):
    """Runs call(out pointer) on a device buffer of GUARD sentinels, n_out complex results pre-filled with a second sentinel,
    GUARD sentinels; returns the result after checking that both guards are untouched and no result word still holds the fill."""
    lib = _lib.load()
    host = np.full(2 * GUARD + 2 * n_out, FILL_WORD, np.uint64)
    host[:GUARD] = GUARD_WORD
    host[GUARD + 2 * n_out:] = GUARD_WORD
    with DevBuf(host) as buf:
        call(ctypes.c_void_p(buf.p.value + GUARD * 8))
        _lib.check(lib.cpx_stream_sync(None))
        back = buf.get()
    assert np.all(back[:GUARD] == GUARD_WORD), "write in front of the output"
    assert np.all(back[GUARD + 2 * n_out:] == GUARD_WORD), "write behind the output"
    res = back[GUARD:GUARD + 2 * n_out]
    missing = np.flatnonzero(res == FILL_WORD)
    assert missing.size == 0, "%d output words never written, the first at %d" % (missing.size, missing[0])
    return res.view(np.complex128)


def guard_cases(nfft):
    if nfft & (nfft - 1) == 0 and nfft <= 8192:
        s = spw(nfft)
        return sorted({n for n in (1, s - 1, s, s + 1, 2 * s + 1) if n >= 1})
    return [1, 3]


@pytest.mark.parametrize("nfft", [2, 64, 2048, 4096, 8192, 3, 100, 2049])
def test_output_coverage_and_guard_words(gpu, nfft):
    """The _dev entry points write their whole output and not a word outside it, at every fill of the last tile; the result is
    bit-identical to the host entry points'."""
    lib = _lib.load()
    rs = np.random.RandomState(nfft)
    for nsym in guard_cases(nfft):
        nsc = nsc_default(nfft)
        x = cplx(rs, 1, nsym, nsc)
        for cp in (1, nfft + 3):
            plan = _plan(nfft, nsc, cp)
            n_out = nsym * (prefix_len(nfft, cp) + nfft)
            with DevBuf(x) as dx:
                got = guarded_call(lambda out: _lib.check(lib.cpx_ofdm_tx_dev(plan, dx.p, 1, nsym, out, None)), n_out)
            assert got.tobytes() == ofdm_tx_batch(x, nfft, cp).tobytes()
        cp = 1
        ny = nsym * (nfft + cp) + 2
        y = cplx(rs, 1, ny)
        for nsc in sorted({2, 2 * (nfft - 1)}):
            plan = _plan(nfft, nsc, cp)
            with DevBuf(y) as dy:
                got = guarded_call(lambda out: _lib.check(lib.cpx_ofdm_rx_dev(plan, dy.p, 1, ny, out, None)), nsym * nsc)
            assert got.tobytes() == ofdm_rx_batch(y, nfft, nsc, cp).tobytes()


# ---- 6. batched RX with samples left over after the last whole block ---------------------------------------------------------------
@pytest.mark.parametrize("nfft, nsc, cp, rows", [(64, 52, 16, 23), (100, 60, 10, 2)])
@pytest.mark.parametrize("left", ["1", "S-1"])
def test_batched_rx_with_leftover(gpu, nfft, nsc, cp, rows, left):
    """B = 3 rows of rows * S + r samples (at nfft = 64, 69 symbols: a tile boundary inside row 2).  Against the model; each row
    bit-equal to ofdm_rx of that row alone; and NaN in everything RX must not read (prefixes, leftovers) changes no bit."""
    rs = np.random.RandomState(nfft)
    S = nfft + cp
    r = 1 if left == "1" else S - 1
    y = cplx(rs, 3, rows * S + r)
    got = ofdm_rx_batch(y, nfft, nsc, cp)
    assert got.shape == (3, rows, nsc)
    if nfft == 64:
        note("batched rx nfft=64 left=%s: largest per-symbol error %.2f u", left, fast_rx_error(got, y, nfft, nsc, cp))
    else:
        body = om.rx_bodies(y, nfft, cp).reshape(-1, nfft)
        bins = om.rx_bin_of(nfft, nsc)
        ratio, err = dense_check(got.reshape(-1, nsc), om.ref_rx_batch(y, nfft, nsc, cp).reshape(-1, nsc),
                                 om.dft_f64_index_order(body, bins), np.sum(np.abs(body), axis=-1, keepdims=True).astype(LD), nfft)
        note("batched rx nfft=%d left=%s: error norm / float64 index-order sum's = %.3f, largest per-symbol error %.1f u",
             nfft, left, ratio, err)
    for b in range(3):
        assert ofdm_rx(y[b], nfft, nsc, cp).T.tobytes() == got[b].tobytes()
    pos = np.arange(rows * S + r)
    unread = np.broadcast_to((pos >= rows * S) | (pos % S < cp), y.shape)
    assert int(unread.sum()) == 3 * (rows * cp + r)
    for junk in (0.0, complex(np.nan, np.nan), complex(np.inf, -np.inf)):
        z = y.copy()
        z[unread] = junk
        assert ofdm_rx_batch(z, nfft, nsc, cp).tobytes() == got.tobytes()


# ---- 7. a non-finite sample stays in its symbol ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nfft, nsc, cp, B, nsym, hit", [(64, 52, 16, 2, 65, 5), (64, 52, 16, 2, 65, 129), (12, 8, 3, 1, 3, 1)])
@pytest.mark.parametrize("bad", ["nan", "inf"])
def test_non_finite_stays_in_its_symbol(gpu, nfft, nsc, cp, B, nsym, hit, bad):
    """One input element of one symbol is nan + nan j, or has +inf as its real part (at nfft = 64 the symbol shares a workgroup
    and its LDS image with 63 others, or sits in the partial last tile).  Every other symbol is bit-identical to the clean run.
    NaN: every output element of the hit symbol is NaN in both parts.  inf: which elements of the hit symbol become inf and which
    NaN (inf - inf, inf * 0) is nobody's contract; asserted is only that it makes no finite wrong claim: each real or imaginary
    part is non-finite or equals the clean run's."""
    rs = np.random.RandomState(nfft + hit)
    b, i = divmod(hit, nsym)
    S = nfft + cp
    x = cplx(rs, B, nsym, nsc)
    y = cplx(rs, B, nsym * S + 2)
    xb, yb = x.copy(), y.copy()
    for arr, at in ((xb, (b, i, nsc // 2 + 1)), (yb, (b, i * S + cp + 7))):
        arr[at] = complex(np.nan, np.nan) if bad == "nan" else complex(np.inf, arr[at].imag)
    per = prefix_len(nfft, cp) + nfft
    runs = ((ofdm_tx_batch(x, nfft, cp).reshape(B * nsym, per), ofdm_tx_batch(xb, nfft, cp).reshape(B * nsym, per)),
            (ofdm_rx_batch(y, nfft, nsc, cp).reshape(B * nsym, nsc), ofdm_rx_batch(yb, nfft, nsc, cp).reshape(B * nsym, nsc)))
    for clean, dirty in runs:
        assert np.all(np.isfinite(clean.view(float)))
        others = np.arange(B * nsym) != hit
        assert dirty[others].tobytes() == clean[others].tobytes()
        parts, want = dirty[hit].view(float), clean[hit].view(float)
        if bad == "nan":
            assert np.all(np.isnan(parts))
        else:
            assert not np.all(np.isfinite(parts))
            assert np.all(~np.isfinite(parts) | (parts == want))


# ---- 8. grid wrap of the direct DFT -----------------------------------------------------------------------------------------------------
def test_dft_grid_wrap(gpu):
    """(3, 2, 1) with 65535 + 70 symbols: the last 70 go to workgroups on their second turn.  Every symbol against the model under
    bound (b) (TX: two nonzero bins and a rounded 1 / 3; RX: three samples), and the error norm over all of them under (c)."""
    nfft, nsc, cp, nsym = 3, 2, 1, 65535 + 70
    rs = np.random.RandomState(8)
    x = cplx(rs, 1, nsym, nsc)
    t0 = time.perf_counter()
    t = ofdm_tx_batch(x, nfft, cp)
    assert "ofdm_dft_kernel<3,tx>" in _lib.last_kernel()
    y = t + 0.1 * cplx(rs, *t.shape)
    r = ofdm_rx_batch(y, nfft, nsc, cp)
    dt = time.perf_counter() - t0
    assert "ofdm_dft_kernel<3,rx>" in _lib.last_kernel()
    _, body = tx_split(t, nfft, cp)
    F = om.tx_bins(x, nfft)[0]
    _, ref = tx_split(om.ref_tx_batch(x, nfft, cp), nfft, cp)
    l1 = np.sum(np.abs(F), axis=-1, keepdims=True).astype(LD) / nfft
    err = np.abs(body[0] - ref[0]) / (uLD * l1)
    assert np.all(err <= om.sparse_bound(2, 1, True)), (int(np.argmax(np.max(err, axis=-1))), float(np.max(err)))
    ratio_tx, _ = dense_check(body[0], ref[0], om.dft_f64_index_order(F, np.arange(nfft), inverse=True), l1, nfft)
    samples = om.rx_bodies(y, nfft, cp)[0]
    ref = om.ref_rx_batch(y, nfft, nsc, cp)[0]
    l1 = np.sum(np.abs(samples), axis=-1, keepdims=True).astype(LD)
    err_rx = np.abs(r[0] - ref) / (uLD * l1)
    assert np.all(err_rx <= om.sparse_bound(3, 1)), (int(np.argmax(np.max(err_rx, axis=-1))), float(np.max(err_rx)))
    ratio_rx, _ = dense_check(r[0], ref, om.dft_f64_index_order(samples, om.rx_bin_of(nfft, nsc)), l1, nfft)
    note("dft grid wrap: %d symbols tx + rx in %.2f s, largest element error tx %.2f rx %.2f u sum|x|, ratio (c) tx %.3f rx %.3f",
         nsym, dt, float(np.max(err)), float(np.max(err_rx)), ratio_tx, ratio_rx)


# ---- 9. grid wrap of the fast kernel ------------------------------------------------------------------------------------------------------
def test_fast_grid_wrap(gpu):
    """TX at (4096, 2, 1) with 65536 + 64 symbols, one tile each: 65 tiles go to workgroups on their second turn.  The 4.3 GB
    output stays on the device; the symbols either side of the wrap, the last and 50 random ones are read back and held to bound
    (a), then RX of the whole buffer returns 2 bins per symbol: the read-back symbols against ref_rx under (a), and every symbol
    against its input under twice the bound (TX's error goes through RX's transform, unitary up to the scale, and RX adds its
    own; both are relative to the norm of the whole transform, which here is the norm of the two inputs)."""
    lib = _lib.load()
    nfft, nsc, cp = 4096, 2, 1
    nsym = 65536 + 64
    per = cp + nfft
    plan = _plan(nfft, nsc, cp)
    rs = np.random.RandomState(9)
    x = cplx(rs, 1, nsym, nsc)
    picks = np.unique(np.concatenate([[0, 65534, 65535, 65536, 65537, nsym - 1], rs.choice(nsym, 50, replace=False)]))
    bound = om.fast_bound(nfft)
    t0 = time.perf_counter()
    ptrs = {}
    try:
        for name, nbytes in (("x", x.nbytes), ("tx", nsym * per * 16), ("rx", x.nbytes)):
            ptrs[name] = ctypes.c_void_p()
            _lib.check(lib.cpx_malloc(ctypes.byref(ptrs[name]), nbytes))
        _lib.check(lib.cpx_memcpy_h2d(ptrs["x"], _lib.ptr(x), x.nbytes))
        _lib.check(lib.cpx_ofdm_tx_dev(plan, ptrs["x"], 1, nsym, ptrs["tx"], None))
        assert "ofdm_fast_kernel<4096,tx>" in _lib.last_kernel()
        _lib.check(lib.cpx_ofdm_rx_dev(plan, ptrs["tx"], 1, nsym * per, ptrs["rx"], None))
        assert "ofdm_fast_kernel<4096,rx>" in _lib.last_kernel()
        _lib.check(lib.cpx_stream_sync(None))
        r = np.zeros((nsym, nsc), complex)
        _lib.check(lib.cpx_memcpy_d2h(_lib.ptr(r), ptrs["rx"], r.nbytes))
        t = np.zeros((picks.size, per), complex)
        for row, s in enumerate(picks):
            _lib.check(lib.cpx_memcpy_d2h(_lib.ptr(t[row:row + 1]), ctypes.c_void_p(ptrs["tx"].value + int(s) * per * 16), per * 16))
    finally:
        for p in ptrs.values():
            lib.cpx_free(p)
    dt = time.perf_counter() - t0
    worst_tx = fast_tx_error(t.reshape(1, -1), x[:, picks], nfft, cp)
    worst_rx = fast_rx_error(r[picks][None], t.reshape(1, -1), nfft, nsc, cp)
    size = om.norm2(x[0].astype(om.CLD))
    trip = om.norm2(r - x[0]) / (uLD * size)
    assert np.all(trip <= 2 * bound), (int(np.argmax(trip)), float(np.max(trip)), 2 * bound)
    note("fast grid wrap: %d symbols tx + rx and read-back in %.2f s; %d symbols tx %.2f u, rx %.2f u (bound %.1f); round trip of "
         "all %.2f u (bound %.1f)", nsym, dt, picks.size, worst_tx, worst_rx, bound, float(np.max(trip)), 2 * bound)
