"""Demodulation at the edges, on every kernel path, against the float64 reference.

Hard decisions.  The reference rule is ``abs(y - c[:, None]).argmin(0)``: the first minimum wins (ties go to the lowest label)
and a symbol whose every distance is inf or NaN gets label 0.  The inputs are built, not drawn: exact points, exact midpoints
between grid levels, boundaries a few ulps off, boundaries with a huge other component, every {finite, +-inf, NaN} pair,
components beyond the overflow of hypot, subnormal offsets and -0.0 (tests/demod_edges.py), scattered among noisy symbols in
arrays of 1 .. 4099 symbols so that the scan fallback and the per-axis fast decision share a wave.  The contract
(tests/demod_edges.py, checked by exact rational arithmetic):

* only one label within 2 ulps of the exact minimum distance, or every distance the same non-finite value: the kernel's label
  is the reference's (``oracle.demodulate(.., 'hard')``), exactly;
* several labels at bit-identical distances (an exact tie): the lowest of them;
* several labels within 2 ulps only through rounding (a near-boundary symbol next to a huge other component, where the
  reference's own hypot rounding turns a near-tie into a tie): a label of that band.  The device hypot (ocml) is not guaranteed
  to round like the host's (glibc), so bit equality with the reference cannot be promised there; the count of such symbols is
  printed, and the large-magnitude inputs must produce some.

Soft decisions.  The same symbols through every float64 soft kernel, for noise variances from 5e-324 to inf, 0, negative and
NaN: NaN and +-inf exactly where the reference has them, finite values within 1e-9.  In the "fp32-fast" precision mode the
contract is weaker by design (csrc/demod.hip): a symbol with a NaN or inf component, or one whose every squared distance
overflows float64, gets no finite LLR; where the reference is finite (and below 600 in magnitude) the mode's own tolerance of
tests/test_fp32_fast_gpu.py holds; where the reference is -inf / NaN only because every exponential underflows, the mode gives
the LLR the formula defines and is not checked.
"""
import ctypes

import numpy as np
import pytest

import oracle
from demod_edges import BIG, EXACT, ROUND, TIE, edge_symbols, hard_contract, labels_of, same_soft, scatter
from helpers import make_trellis

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 255, 256, 257, 4099)
NOISE_VARS = (0.5, 1e-295, 1e295, 0.0, -0.5, np.inf, np.nan, 5e-324)


def _grid(nh, xs, ys):
    """A separable grid as given: label (a << nh) | b -> xs[a] + 1j ys[b] (no Gray re-indexing)."""
    from commpy_amd.modulation import Modem
    R = 1 << nh
    lab = np.arange(R * R)
    return Modem(np.asarray(xs, float)[lab >> nh] + 1j * np.asarray(ys, float)[lab & (R - 1)], reorder_as_gray=False)


def _modem(name):
    from commpy_amd.modulation import Modem, PSKModem, QAMModem
    kind, _, arg = name.partition(":")
    if kind == "qam":
        return QAMModem(int(arg))
    if kind == "qam_unit":                                          # QAMModem's table scaled to unit energy
        q = QAMModem(int(arg))
        return Modem(q.constellation / np.sqrt(q.Es), reorder_as_gray=False)
    if kind == "psk":
        return PSKModem(int(arg))
    if kind == "uneven16":                                          # unequal spacing, unsorted levels, non-Gray labels
        return _grid(2, [0.75, -3.0, 2.5, -0.5], [-1.25, 4.0, 0.0, -6.0])
    if kind == "uneven64":
        return _grid(3, [3.75, -7.0, 0.5, -1.25, 8.0, -4.5, 1.0, -2.0], [-0.25, 6.5, -3.0, 2.0, -8.0, 0.0, 4.25, -1.5])
    if kind == "degenerate16":                                      # a repeated grid line: must stay on the generic kernel
        return _grid(2, [-3.0, -1.0, -1.0, 3.0], [-3.0, -1.0, 1.0, 3.0])
    if kind == "random":
        rs = np.random.RandomState(int(arg))
        return Modem((rs.randn(int(arg)) + 1j * rs.randn(int(arg))) * 1.5, reorder_as_gray=False)
    raise KeyError(name)


SEP = [("qam:%d" % m, m) for m in (4, 16, 64, 256)] + [("qam_unit:%d" % m, m) for m in (4, 16, 64, 256)] + \
      [("uneven16", 16), ("uneven64", 64)]
GENERIC = ["psk:%d" % m for m in (2, 4, 8, 16, 32, 64, 128, 256)] + ["random:64", "degenerate16"]
ANY = ["qam:1024", "random:512"]


def _nh(m):
    return int(np.log2(m)) // 2


def _violations(c, y, got, ref):
    """Indices that break the hard-decision contract, and the number of symbols in the rounding band."""
    kind, band, _ = hard_contract(c, y)
    bad = [i for i in range(len(got))
           if not (got[i] == ref[i] if kind[i] == EXACT else
                   got[i] == min(band[i]) if kind[i] == TIE else int(got[i]) in band[i])]
    return bad, kind


def _run_hard(name, want_kernel, sizes, seed):
    from commpy_amd import _lib
    md = _modem(name)
    c, nb = md.constellation, md.num_bits_symbol
    rs = np.random.RandomState(seed)
    edges, cls = edge_symbols(c, rs)
    kinds_e, _, _ = hard_contract(c, edges)
    assert np.any(kinds_e[cls == "big"] == ROUND), "the large-magnitude inputs put no symbol in the rounding band"
    total_round = 0
    for n in sizes:
        y, _ = scatter(c, edges, n, rs)
        got = labels_of(md.demodulate(y, "hard"), nb)
        assert _lib.last_kernel().startswith(want_kernel), (name, _lib.last_kernel())
        ref = labels_of(oracle.demodulate(c, y, "hard"), nb)
        bad, kind = _violations(c, y, got, ref)
        total_round += int(np.sum(kind == ROUND))
        assert not bad, (name, n, [(y[i], int(got[i]), int(ref[i]), int(kind[i])) for i in bad[:8]], len(bad))
    print("%s: %d symbols in the rounding band, all inside it" % (name, total_round))


@pytest.mark.parametrize("name,m", SEP, ids=[s[0] for s in SEP])
def test_hard_separable_edges(gpu, name, m):
    _run_hard(name, "demod_hard_sep_kernel<%d>" % _nh(m), SIZES, m)


@pytest.mark.parametrize("name", GENERIC)
def test_hard_generic_edges(gpu, name):
    _run_hard(name, "demod_hard_kernel", SIZES, 7)


@pytest.mark.parametrize("name", ANY)
def test_hard_large_constellation_edges(gpu, name):
    _run_hard(name, "demod_hard_any_kernel", (1, 65, 2500), 11)


def _dev(arr):
    from commpy_amd.devicelink import DeviceBuf
    return DeviceBuf.from_array(arr)


def _stream():
    from commpy_amd import _lib
    st = ctypes.c_void_p()
    _lib.check(_lib.load().cpx_stream_create(ctypes.byref(st)))
    return st


@pytest.mark.parametrize("m", (4, 16, 64, 256))
def test_hard_device_entry_odd_pointers_guard_bytes_own_stream(gpu, m):
    """cpx_demod_hard_dev writing at byte offsets 0, 1, 2, 3 and 5 (the byte-store branch of demod_hard_sep_kernel) on a stream
    of its own: the bits of the host entry, and the guard bytes in front of and behind the output untouched."""
    from commpy_amd import _lib
    from commpy_amd.devicelink import DeviceBuf
    from commpy_amd.modulation import QAMModem
    so = _lib.load()
    md = QAMModem(m)
    nb = md.num_bits_symbol
    rs = np.random.RandomState(m + 1)
    edges, _ = edge_symbols(md.constellation, rs)
    y, _ = scatter(md.constellation, edges, 4099, rs)
    want = md.demodulate(y, "hard")
    d_y = _dev(y)
    st = _stream()
    try:
        for off in (0, 1, 2, 3, 5):
            nbytes = 16 + y.size * nb + 64
            fill = np.full(nbytes, 0x5A, np.uint8)
            d_o = DeviceBuf.from_array(fill)
            _lib.check(so.cpx_demod_hard_dev(md._device_handle(), d_y.ptr, y.size, ctypes.c_void_p(d_o.ptr.value + 8 + off), st))
            assert _lib.last_kernel() == "demod_hard_sep_kernel<%d>" % _nh(m)
            _lib.check(so.cpx_stream_sync(st))
            out = d_o.to_array(nbytes, np.uint8)
            lo, hi = 8 + off, 8 + off + y.size * nb
            assert np.array_equal(out[lo:hi].view(np.int8), want), (m, off)
            assert np.all(out[:lo] == 0x5A) and np.all(out[hi:] == 0x5A), (m, off)
    finally:
        so.cpx_stream_destroy(st)


FUSED = [("psk:8", 0), ("qam:4", 1), ("qam:16", 2), ("qam:64", 3), ("qam:256", 4)]


@pytest.mark.parametrize("tname", ["t57", "k7_133_171"])
@pytest.mark.parametrize("name,nh", FUSED, ids=["nh%d" % f[1] for f in FUSED])
def test_fused_hard_demod_viterbi_edges(gpu, name, nh, tname):
    """demodulate_viterbi_hard on codewords that carry edge symbols -- NaN and +-inf in either component, exact boundaries,
    overflow -- against the oracle pair viterbi_decode(demodulate(y, 'hard')) codeword by codeword (only symbols whose hard
    decision the contract pins exactly: the rounding band is left to the element-wise tests)."""
    from commpy_amd import _lib
    from commpy_amd.channelcoding import conv_encode_batch
    md = _modem(name)
    tr = make_trellis(tname)
    c, nb = md.constellation, md.num_bits_symbol
    rs = np.random.RandomState(17 + nh)
    edges, _ = edge_symbols(c, rs)
    kind, _, _ = hard_contract(c, edges)
    pool = edges[kind != ROUND]
    must = np.array([complex(np.nan, 0.3), complex(0.3, np.nan), complex(np.inf, -0.3), complex(0.3, np.inf),
                     complex(-np.inf, 1.0), complex(1.0, -np.inf), complex(np.nan, np.inf), complex(1.3e308, -1.5e308)])
    B, nmsg = 24, 50 * tr.k
    coded = conv_encode_batch(rs.randint(0, 2, (B, nmsg)), tr)
    pad = (-coded.shape[1]) % nb
    coded = np.concatenate([coded, np.zeros((B, pad), coded.dtype)], axis=1)
    s = md.modulate(coded.reshape(-1)).reshape(B, -1)
    N0 = md.Es / 10 ** 0.9
    y = s + np.sqrt(N0 / 2) * (rs.randn(*s.shape) + 1j * rs.randn(*s.shape))
    nsym = y.shape[1]
    for b in range(B):
        k = int(rs.randint(1, 6))
        pos = rs.choice(nsym, k + 1, replace=False)
        y[b, pos[:k]] = pool[rs.randint(0, pool.size, k)]
        y[b, pos[k]] = must[b % must.size]
    bits = oracle.demodulate(c, y.reshape(-1), "hard").reshape(B, -1).astype(np.float64)
    for tb in (None, 12):
        got = md.demodulate_viterbi_hard(y, tr, tb)
        assert "demod" in _lib.last_kernel(), _lib.last_kernel()
        want = oracle.viterbi_decode(bits, tr, tb, "hard")
        bad = [b for b in range(B) if not np.array_equal(got[b], want[b])]
        assert not bad, (name, tname, tb, bad)


# ---- soft decisions -------------------------------------------------------------------------------------------------------------


def _soft_inputs(c, seed):
    rs = np.random.RandomState(seed)
    edges, _ = edge_symbols(c, rs, big=BIG)
    y, _ = scatter(c, edges, 2 * edges.size + 65, rs)
    return y


def _check_soft(got, want, what):
    bad = same_soft(got, want)
    assert bad.size == 0, (what, bad.size, [(int(i), got[i], want[i]) for i in bad[:6]])


@pytest.mark.parametrize("mode", [None, "libm", "plain"])
@pytest.mark.parametrize("m", (4, 16, 64, 256))
def test_soft_separable_edges(gpu, m, mode):
    from commpy_amd import _lib
    from commpy_amd.modulation import QAMModem
    md = QAMModem(m)
    y = _soft_inputs(md.constellation, m)
    with _lib.forced_path("demod", mode):
        for nv in NOISE_VARS:
            got = md.demodulate(y, "soft", nv)
            k = _lib.last_kernel()
            rcp = 1e-290 < nv < 1e290
            assert k.startswith("demod_soft_sep_kernel<%d,%s" % (_nh(m), "rcp" if rcp else "div")), (k, nv)
            _check_soft(got, oracle.demodulate(md.constellation, y, "soft", nv), (m, mode, nv, k))


@pytest.mark.parametrize("name", ["psk:2", "psk:8", "psk:32", "random:16", "degenerate16"])
def test_soft_generic_edges(gpu, name):
    """demod_soft_gen_kernel (16-byte aligned output) and the literal demod_soft_kernel ('libm' path)."""
    from commpy_amd import _lib
    md = _modem(name)
    y = _soft_inputs(md.constellation, 3)
    for mode, kern in ((None, "demod_soft_gen_kernel<"), ("libm", "demod_soft_kernel<")):
        with _lib.forced_path("demod", mode):
            for nv in NOISE_VARS:
                got = md.demodulate(y, "soft", nv)
                assert _lib.last_kernel().startswith(kern), (_lib.last_kernel(), mode)
                _check_soft(got, oracle.demodulate(md.constellation, y, "soft", nv), (name, mode, nv))


@pytest.mark.parametrize("name", ["qam:16", "qam:64", "psk:8"])
def test_soft_literal_kernel_through_8_byte_aligned_output(gpu, name):
    """An output pointer that is 8- but not 16-byte aligned takes the literal demod_soft_kernel on every constellation; the scaled
    device entry with scale -1 gives exactly the negated LLRs (the sign convention of the LDPC decoder)."""
    from commpy_amd import _lib
    from commpy_amd.devicelink import DeviceBuf
    so = _lib.load()
    md = _modem(name)
    nb = md.num_bits_symbol
    y = _soft_inputs(md.constellation, 5)
    d_y = _dev(y)
    d_o = DeviceBuf(8 * (y.size * nb + 2))
    for nv in NOISE_VARS:
        want = oracle.demodulate(md.constellation, y, "soft", nv)
        for scale in (1.0, -1.0):
            _lib.check(so.cpx_demod_soft_scaled_dev(md._device_handle(), d_y.ptr, y.size, nv, scale,
                                                    ctypes.c_void_p(d_o.ptr.value + 8), None))
            assert _lib.last_kernel().startswith("demod_soft_kernel<%d,%s" % (nb, "rcp" if 1e-290 < nv < 1e290 else "div"))
            out = d_o.to_array(y.size * nb + 1, np.float64)[1:]
            _check_soft(out, scale * want, (name, nv, scale))


@pytest.mark.parametrize("name", ["qam:64", "psk:8", "random:32"])
def test_soft_scaled_device_entry_sign_flip(gpu, name):
    """cpx_demod_soft_scaled_dev with scale -1 on the fast kernels (16-byte aligned output): the negated reference."""
    from commpy_amd import _lib
    from commpy_amd.devicelink import DeviceBuf
    so = _lib.load()
    md = _modem(name)
    nb = md.num_bits_symbol
    y = _soft_inputs(md.constellation, 6)
    d_y = _dev(y)
    d_o = DeviceBuf(8 * y.size * nb)
    st = _stream()
    try:
        for nv in NOISE_VARS:
            _lib.check(so.cpx_demod_soft_scaled_dev(md._device_handle(), d_y.ptr, y.size, nv, -1.0, d_o.ptr, st))
            assert "demod_soft_sep_kernel" in _lib.last_kernel() or "demod_soft_gen_kernel" in _lib.last_kernel()
            _lib.check(so.cpx_stream_sync(st))
            _check_soft(d_o.to_array(y.size * nb, np.float64), -oracle.demodulate(md.constellation, y, "soft", nv), (name, nv))
    finally:
        so.cpx_stream_destroy(st)


@pytest.mark.parametrize("name", ANY)
def test_soft_large_constellation_edges(gpu, name):
    from commpy_amd import _lib
    md = _modem(name)
    rs = np.random.RandomState(9)
    edges, _ = edge_symbols(md.constellation, rs, big=(1e3, 1e150))
    y = edges[rs.choice(edges.size, 300, replace=False)]
    for nv in NOISE_VARS:
        got = md.demodulate(y, "soft", nv)
        assert _lib.last_kernel().startswith("demod_soft_any_kernel<%d>" % md.num_bits_symbol), _lib.last_kernel()
        _check_soft(got, oracle.demodulate(md.constellation, y, "soft", nv), (name, nv))


@pytest.mark.parametrize("name", ["qam:4", "qam:16", "qam:64", "qam:256", "psk:8", "random:16"])
def test_soft_fp32_fast_edges(gpu, name):
    """The weaker contract of the "fp32-fast" mode (see the module docstring); noise variances outside its float32 range keep
    the float64 kernels and their full contract."""
    import commpy_amd
    from commpy_amd import _lib
    md = _modem(name)
    c, nb = md.constellation, md.num_bits_symbol
    y = _soft_inputs(c, 4)
    bad_in = ~(np.isfinite(y.real) & np.isfinite(y.imag))
    with np.errstate(all="ignore"):
        overflow = np.all(np.isinf(np.abs(y[:, None] - c[None, :]) ** 2), axis=1)
    must_nonfinite = np.repeat(bad_in | overflow, nb)
    with commpy_amd.precision("fp32-fast"):
        for nv in (0.5, 2.0, 1e-295, 0.0, np.inf, np.nan):
            got = md.demodulate(y, "soft", nv)
            k = _lib.last_kernel()
            ref = oracle.demodulate(c, y, "soft", nv)
            if "_f32_kernel" not in k:
                assert not (1e-30 < nv < 1e30), (k, nv)
                _check_soft(got, ref, (name, nv, k))
                continue
            assert not np.any(np.isfinite(got[must_nonfinite])), (name, nv, np.nonzero(np.isfinite(got) & must_nonfinite)[0][:8])
            fin = np.isfinite(ref) & (np.abs(ref) < 600)
            err = np.abs(got - ref)[fin] - (2e-5 + 4e-6 * np.abs(ref[fin]))
            assert not np.any(err > 0) and np.all(np.isfinite(got[fin])), (name, nv, float(np.max(err)))
