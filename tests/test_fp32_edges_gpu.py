"""The fp32-fast kernels at small shapes and edges, each against its float32 model (tests/fp32_model.py): bit for bit where the arithmetic
is add / compare / min (Viterbi, LDPC min-sum), within a measured bound against the model (LDPC sum-product) and within the derived
bound against a long-double reference (demodulator).  tests/test_fp32_fast_gpu.py holds the statistical contract at workload sizes."""
import numpy as np
import pytest

import fp32_model as M
import oracle
from helpers import ldpc_params, make_trellis
from test_fp32_model_host import CUSTOM4, outliers
from test_ldpc_layered_host import random_code

pytestmark = pytest.mark.gpu

# the five built-in 64-state pairs (csrc/viterbi_cw.hip BUILTIN_PAIRS): (133,171) and (171,133) in both polynomial formats and the
# Wifi80211 generators as shipped
K7_CODES = {
    "133_171": ([[0o133, 0o171]], "MSB"), "171_133": ([[0o171, 0o133]], "MSB"),
    "133_171_lsb": ([[0o133, 0o171]], "LSB"), "171_133_lsb": ([[0o171, 0o133]], "LSB"), "wifi_decimal": ([[133, 171]], "MSB"),
}
BATCHES = (1, 63, 64, 65, 257)
# T = L + 5 trellis steps for a 64-state code, so no input has fewer than 6: around the smallest, around tb_depth (29 .. 31) and around
# the 96-step flush of the fused kernel (95 .. 97, 193 = two flushes and one step)
STEPS = (6, 7, 29, 30, 31, 95, 96, 97, 193)
DEPTHS = (2, 15, 30)


@pytest.fixture
def lib():
    from commpy_amd import _lib
    _lib.set_precision("fp32-fast")
    yield _lib
    _lib.set_precision(None)
    _lib.viterbi_set_path(None)
    _lib.ldpc_set_path(None)
    _lib.demod_set_path(None)


def _k7(name):
    from commpy_amd.channelcoding.convcode import Trellis
    g, fmt = K7_CODES[name]
    return Trellis(np.array([6]), np.array(g), polynomial_format=fmt)


def _received(tr, rs, B, T, termination, dtype, sigma=0.9):
    """A noisy batch with T trellis steps: 'term' encodes T - 11 message bits with the tail, 'cont' T - 5 bits without one."""
    from commpy_amd.channelcoding import conv_encode_batch
    msgs = rs.randint(0, 2, (B, T - 11 if termination == "term" else T - 5)).astype(np.uint8)
    coded = conv_encode_batch(msgs, tr, termination)
    assert coded.shape[1] == 2 * (T - 5)
    y = 2.0 * coded - 1.0 + sigma * rs.randn(*coded.shape)
    return (y > 0).astype(np.float64) if dtype == "hard" else (2.0 / sigma ** 2) * y if dtype == "soft" else y


def _fused_f32(lib, x, tr, tb, dtype):
    from commpy_amd.channelcoding import viterbi_decode
    got = viterbi_decode(x, tr, tb, dtype)
    assert "viterbi_cw_fused_kernel" in lib.last_kernel() and ",f32" in lib.last_kernel(), lib.last_kernel()
    return got


# ---- Viterbi --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("code", sorted(K7_CODES))
@pytest.mark.parametrize("dtype", ["hard", "soft", "unquantized"])
def test_viterbi_bits_are_the_float32_models(gpu, lib, code, dtype):
    """Every (steps, depth, batch size) triple; the termination alternates ('term' needs T >= 12)."""
    tr = _k7(code)
    lib.viterbi_set_path("cw!")
    rs = np.random.RandomState(len(code) + len(dtype))
    n = 0
    for T in STEPS:
        for tb in DEPTHS:
            for B in BATCHES:
                termination = "term" if n % 2 == 0 and T >= 12 else "cont"
                n += 1
                x = _received(tr, rs, B, T, termination, dtype)
                got = _fused_f32(lib, x, tr, tb, dtype)
                want = M.viterbi(x, tr, tb, dtype)
                assert np.array_equal(got, want), (T, tb, B, termination, int((got != want).sum()))


@pytest.mark.parametrize("dtype", ["soft", "unquantized"])
def test_viterbi_exact_float32_ties_keep_the_models_order(gpu, lib, dtype):
    """+-1-valued 'unquantized' samples (metrics 0 and 4) and integer 'soft' LLRs with +-500 and beyond (clipped): every metric is a
    small integer, candidates tie exactly and several states share the minimum -- the first predecessor and the first state win."""
    tr = _k7("133_171")
    lib.viterbi_set_path("cw!")
    rs = np.random.RandomState(12)
    if dtype == "unquantized":
        x = 2.0 * rs.randint(0, 2, (65, 2 * 92)) - 1.0
    else:
        x = rs.randint(-3, 4, (65, 2 * 92)).astype(np.float64)
        x[rs.rand(*x.shape) < 0.05] = 500.0
        x[rs.rand(*x.shape) < 0.05] = -500.0
        x[rs.rand(*x.shape) < 0.03] = 1e6
        x[rs.rand(*x.shape) < 0.03] = -np.inf
    for tb in (15, 30):
        want, stats = M.viterbi(x, tr, tb, dtype, want_stats=True)
        print("%s tb %d: %d exact candidate ties, %d steps with several best states" % (dtype, tb, stats["select_ties"], stats["best_ties"]))
        assert stats["select_ties"] >= 20000 and stats["best_ties"] >= 500
        assert np.array_equal(_fused_f32(lib, x, tr, tb, dtype), want)


@pytest.mark.parametrize("dtype,seed", [("soft", 0), ("unquantized", 0)])
def test_viterbi_follows_float32_where_float64_decides_otherwise(gpu, lib, dtype, seed):
    """Inputs on a coarse grid plus a perturbation below float32's resolution of the path metrics (seeds searched on the CPU): float64
    tells the near-ties apart, float32 rounds them -- the two models decode differently, and the kernel follows the float32 one."""
    tr = _k7("133_171")
    lib.viterbi_set_path("cw!")
    rs = np.random.RandomState(seed)
    x = np.round(3 * rs.randn(64, 120)) + 1e-6 * rs.randn(64, 120) if dtype == "soft" else \
        np.round(4 * rs.randn(64, 120)) / 4 + 1e-7 * rs.randn(64, 120)
    f32, f64 = M.viterbi(x, tr, None, dtype), M.viterbi(x, tr, None, dtype, dtype=np.float64)
    assert (f32 != f64).any(axis=1).sum() >= 5
    assert np.array_equal(_fused_f32(lib, x, tr, None, dtype), f32)


def test_viterbi_hands_back_to_float64(gpu, lib):
    """Depths above the default (the 64-slot ring), the two-kernel form and the smaller built-in codes have no float32 variant: no
    ',f32' in the note and the float64 oracle's bits."""
    from commpy_amd.channelcoding import viterbi_decode
    rs = np.random.RandomState(4)
    tr = _k7("133_171")
    x = _received(tr, rs, 65, 97, "term", "soft")
    for path, tb in (("cw!", 31), ("cw!", 48), ("cw2!", 30)):
        lib.viterbi_set_path(path)
        got = viterbi_decode(x, tr, tb, "soft")
        assert "viterbi_cw_" in lib.last_kernel() and "f32" not in lib.last_kernel(), lib.last_kernel()
        assert np.array_equal(got, oracle.viterbi_decode_mt(x, tr, tb, "soft"))
    lib.viterbi_set_path("cw")
    for name in ("t57", "k5_23_35"):
        small = make_trellis(name)
        from commpy_amd.channelcoding import conv_encode_batch
        coded = conv_encode_batch(rs.randint(0, 2, (65, 80)).astype(np.uint8), small)
        xs = 2.0 * (2.0 * coded - 1.0 + 0.8 * rs.randn(*coded.shape))
        got = viterbi_decode(xs, small, None, "soft")
        assert "f32" not in lib.last_kernel(), lib.last_kernel()
        assert np.array_equal(got, oracle.viterbi_decode_mt(xs, small, None, "soft"))


@pytest.mark.parametrize("dtype", ["hard", "soft", "unquantized"])
def test_viterbi_special_values_stay_in_their_rows(gpu, lib, dtype):
    """NaN, +-inf and 1e30 (its 'unquantized' metric overflows float32) in some rows: every other row as in a clean run, bit for bit.
    The rows themselves follow the model where it is defined: all of them for 'unquantized', all but NaN for 'soft' (a NaN codeword is
    decoded again in float64: the oracle's bits), none for 'hard' (the conversion to an integer is undefined there)."""
    tr = _k7("133_171")
    lib.viterbi_set_path("cw!")
    rs = np.random.RandomState(21)
    clean = _received(tr, rs, 130, 110, "term", dtype)
    x = clean.copy()
    special = {3: np.nan, 63: np.inf, 64: -np.inf, 65: 1e30, 100: np.nan, 129: -1e30}
    for row, v in special.items():
        x[row, [7, 40 + row % 9, 150]] = v
    base = _fused_f32(lib, clean, tr, None, dtype)
    got = _fused_f32(lib, x, tr, None, dtype)
    others = np.setdiff1d(np.arange(130), list(special))
    assert np.array_equal(got[others], base[others])
    if dtype == "hard":
        return
    want = M.viterbi(x, tr, None, dtype)
    for row, v in special.items():
        if dtype == "soft" and np.isnan(v):
            assert np.array_equal(got[row], oracle.viterbi_decode(x[row], tr, None, "soft")), row
        else:
            assert np.array_equal(got[row], want[row]), row


# ---- LDPC -----------------------------------------------------------------------------------------------------------------------------
_codes = {}


def _ldpc(name):
    """(parameter dictionary, model tables); 'irregular': 130 variables, checks of every degree 2 .. 32 -- rows padded to cpad = 32 > their
    degree, column tables of 64-variable groups with different trip counts."""
    if name not in _codes:
        if name == "irregular":
            import ldpc_layered_model
            code = random_code(np.random.RandomState(31), 130, list(range(2, 33)) + [3, 5, 8, 13, 21, 4, 6])
            p = ldpc_layered_model.params_from_code(code)
            import scipy.sparse as sp                                 # the decoder only reads the matrix: given, it is not derived
            p["parity_check_matrix"] = sp.csr_matrix((np.ones(len(code.edge_var), np.int8), (code.edge_check, code.edge_var)),
                                                     shape=(code.n_c, code.n_v))
        else:
            p = ldpc_params(name)
        _codes[name] = (p, M.LdpcTables.from_params(p))
    return _codes[name]


def _ldpc_rows(p, seed):
    """Eight blocks: a codeword on arrival, four noisy all-zero words of growing noise (early, late, never converging), pure noise,
    one with +-inf and values beyond the clip, and (last) one with a NaN."""
    n = int(p["n_vnodes"])
    rs = np.random.RandomState(seed)
    rows = [np.abs(2.0 + rs.randn(n)) + 0.01]
    rows += [2.0 * (1.0 + s * rs.randn(n)) / s ** 2 for s in (0.5, 0.7, 0.85, 1.0)]
    rows += [3.0 * rs.randn(n)]
    r = 2.0 * (1.0 + 0.7 * rs.randn(n)) / 0.49
    r[[0, 5, n - 1]] = [np.inf, -np.inf, 1e9]
    r[[9, 11]] = [-777.0, 500.5]
    rows += [r]
    r = 2.0 * (1.0 + 0.7 * rs.randn(n)) / 0.49
    r[n // 2] = np.nan
    rows += [r]
    return np.array(rows)


def _decode(lib, llr, p, alg, iters, kernel):
    from commpy_amd.channelcoding import ldpc_bp_decode
    flat = llr.reshape(-1).copy()
    dec, out, its = ldpc_bp_decode(flat, p, alg, iters, return_iterations=True)
    assert kernel in lib.last_kernel(), lib.last_kernel()
    B = llr.shape[0]
    return dec.reshape(-1, B).T, out.reshape(-1, B).T, its, flat.reshape(llr.shape)


@pytest.mark.parametrize("name", ["gallager96", "n1944", "irregular"])
@pytest.mark.parametrize("iters", [1, 2, 7, 50])
def test_minsum_is_the_float32_model_bit_for_bit(gpu, lib, name, iters):
    p, tab = _ldpc(name)
    lib.ldpc_set_path("resident")
    llr = _ldpc_rows(p, 40 + iters)
    want = M.ldpc_decode(llr[:7], tab, "MSA", iters)
    assert want["iters"][0] == 0 and want["iters"].max() == iters
    for rows in (slice(0, 8), slice(1, 2), slice(4, 7)):                 # B = 8, 1 and 3
        dec, out, its, clipped = _decode(lib, llr[rows], p, "MSA", iters, "ldpc_resident_f32_kernel<MSA>")
        idx = np.arange(8)[rows]
        keep = idx < 7                                                   # the NaN block: below
        assert np.array_equal(its[keep], want["iters"][idx[keep]])
        assert np.array_equal(out[keep].view(np.int64), want["out"][idx[keep]].view(np.int64))
        assert np.array_equal(dec[keep], want["dec"][idx[keep]])
        assert np.array_equal(clipped[keep].view(np.int64), want["llr"][idx[keep]].view(np.int64))
    # the caller's array after the call, and the block with a NaN (decoded again by the float64 NaN-exact kernel): as in fp64-parity
    dec, out, its, clipped = _decode(lib, llr, p, "MSA", iters, "ldpc_resident_f32_kernel<MSA>")
    lib.set_precision(None)
    dec64, out64, its64, clipped64 = _decode(lib, llr, p, "MSA", iters, "ldpc_resident_kernel<MSA")
    assert np.array_equal(clipped.view(np.int64), clipped64.view(np.int64)) and np.isinf(llr[6]).any() and not np.isinf(clipped).any()
    assert np.array_equal(out[7].view(np.int64), out64[7].view(np.int64)) and np.array_equal(dec[7], dec64[7]) and its[7] == its64[7]


def test_minsum_more_blocks_than_the_resident_grid(gpu, lib):
    """5000 blocks of the 96-bit code: the persistent grid holds at most 16 workgroups per compute unit, so slots are refilled."""
    p, tab = _ldpc("gallager96")
    lib.ldpc_set_path("resident")
    base = _ldpc_rows(p, 3)[:5]
    want = M.ldpc_decode(base, tab, "MSA", 7)
    dec, out, its, _ = _decode(lib, np.tile(base, (1000, 1)), p, "MSA", 7, "ldpc_resident_f32_kernel<MSA>")
    assert np.array_equal(its, np.tile(want["iters"], 1000))
    assert np.array_equal(out.view(np.int64), np.tile(want["out"], (1000, 1)).view(np.int64))
    assert np.array_equal(dec, np.tile(want["dec"], (1000, 1)))


# Sum-product: worst |out_llrs - model| measured on an MI355X over the seeds below (printed by the test), times four for v_exp_f32 /
# v_log_f32 / v_rcp_f32 against NumPy's correctly rounded float32 functions.  DESIGN.md 4.3 records the same figures.
SPA_TOL = {1: 4 * 4.8e-6, 2: 4 * 2.5e-5}                                # measured: 4.77e-6 (irregular code), 2.48e-5 (irregular code)
SPA_SEEDS = (50, 51, 52)


def _spa_rows(p, seed):
    """Twelve blocks with |LLR| <= 8: half noisy all-zero words, half pure noise."""
    n = int(p["n_vnodes"])
    rs = np.random.RandomState(seed)
    return np.concatenate([np.clip(2.0 * (1.0 + 0.8 * rs.randn(6, n)) / 0.64, -8, 8), rs.uniform(-8, 8, (6, n))])


@pytest.mark.parametrize("name", ["gallager96", "n1944", "irregular"])
@pytest.mark.parametrize("iters", [1, 2])
def test_sum_product_is_within_the_measured_bound_of_the_float32_model(gpu, lib, name, iters):
    """Measured on an MI355X, worst |out_llrs - model| over the three seeds: one iteration 3.8e-6 / 3.1e-6 / 4.8e-6 ((96,48) / (1944,1296) /
    irregular), two iterations 1.6e-5 / 2.9e-6 / 2.5e-5; SPA_TOL is four times the worst of each row (the test prints its own figure).  dec_word is exact wherever the model's LLR is further than the tolerance from zero, and the iteration count of every
    block whose check passes never read a |Q| within the tolerance of zero; the margin excludes under 1 % of the positions."""
    p, tab = _ldpc(name)
    lib.ldpc_set_path("resident")
    tol, worst, excluded, total = SPA_TOL[iters], 0.0, 0, 0
    for seed in SPA_SEEDS:
        llr = _spa_rows(p, seed)
        want = M.ldpc_decode(llr, tab, "SPA", iters)
        dec, out, its, _ = _decode(lib, llr, p, "SPA", iters, "ldpc_resident_f32_kernel<SPA>")
        assert np.all(np.isfinite(out))
        worst = max(worst, float(np.abs(out - want["out"]).max()))
        sure = np.abs(want["out"]) > tol
        excluded += int((~sure).sum())
        total += sure.size
        assert np.array_equal(dec[sure], want["dec"][sure])
        safe = want["margin"] > tol
        assert 2 * safe.sum() >= len(safe) and np.array_equal(its[safe], want["iters"][safe])
    print("fp32-fast SPA %s, %d iteration(s): worst |out_llrs - float32 model| %.3e (tolerance %.1e); %d of %d positions inside the margin" % (
        name, iters, worst, tol, excluded, total))
    assert excluded <= 0.01 * total
    assert worst <= tol, worst


def test_sum_product_tiny_messages_make_no_nan(gpu, lib):
    """A block with LLRs 1e-30 .. 1e-6 and one exact zero between ordinary blocks.  tanh(m / 2) = (1 - e) / (1 + e), e = exp(-|m|),
    is 0 in float32 for every |m| below 3e-8, and 1 / 0 times a product that holds the same zero is NaN: before the kernel took m / 2
    for tiny messages, 1e-30, 1e-10, -1e-9 and 2e-8 each made a NaN (measured on an MI355X: NaN at all five positions up to 2e-8).
    Now only the exact zero does, as in the model; the float64 resident decoder makes a NaN there and nowhere the float32 one is finite
    (its ratio-domain row also loses 1e-30, e^1e-30 being 1: NaN at the zero and at 1e-30)."""
    p, tab = _ldpc("gallager96")
    lib.ldpc_set_path("resident")
    llr = _spa_rows(p, 60)[:5]
    plain = llr.copy()
    # No two of them share a check.  (Two tiny LLRs in one check send each other messages below float32's resolution of the other
    # messages; Q - R then cancels to an exact zero, which is NaN in any precision -- float64 merely needs them 1e9 times smaller.)
    pos = [2, 3, 4, 5, 7, 10]
    checks = lambda v: set(np.nonzero((tab.row_q == v).any(axis=1))[0])
    assert all(not (checks(a) & checks(b)) for a in pos for b in pos if a < b)
    llr[2, pos] = [0.0, 1e-30, 1e-10, -1e-9, 2e-8, 1e-6]
    for iters in (1, 2):
        want = M.ldpc_decode(llr, tab, "SPA", iters)
        dec, out, its, _ = _decode(lib, llr, p, "SPA", iters, "ldpc_resident_f32_kernel<SPA>")
        _, base, _, _ = _decode(lib, plain, p, "SPA", iters, "ldpc_resident_f32_kernel<SPA>")
        lib.set_precision(None)
        _, out64, _, _ = _decode(lib, llr, p, "SPA", iters, "ldpc_resident_kernel<SPA")
        lib.set_precision("fp32-fast")
        print("fp32-fast SPA, tiny messages, %d iteration(s): NaN at %s, float64 at %s" % (
            iters, np.nonzero(np.isnan(out[2]))[0].tolist(), np.nonzero(np.isnan(out64[2]))[0].tolist()))
        assert np.isnan(out[2, 2]) and np.isnan(out64[2, 2])
        assert not np.any(np.isnan(out) & ~np.isnan(out64))              # NaN only where the float64 resident decoder's is
        assert np.array_equal(np.isnan(out), np.isnan(want["out"]))      # and exactly where the model's is: what the exact zero reaches
        if iters == 1:
            assert np.array_equal(np.nonzero(np.isnan(out[2]))[0], [2])
        others = [0, 1, 3, 4]
        assert np.array_equal(out[others].view(np.int64), base[others].view(np.int64))


# ---- demodulator ----------------------------------------------------------------------------------------------------------------------
DEMOD_CASES = [("qam", 4), ("qam", 16), ("qam", 64), ("qam", 256), ("psk", 2), ("psk", 8), ("psk", 16), ("custom", 4)]
SIZES = (1, 63, 64, 65, 257)
SNRS_DB = (0.0, 10.0, 20.0, 28.0, 40.0)


def _modem(kind, m):
    from commpy_amd.modulation import Modem, PSKModem, QAMModem
    return QAMModem(m) if kind == "qam" else PSKModem(m) if kind == "psk" else Modem(CUSTOM4, reorder_as_gray=False)


def _soft(lib, md, y, N0, kind):
    got = md.demodulate(y, "soft", N0)
    assert ("demod_soft_sep_f32_kernel" if kind == "qam" else "demod_soft_f32_kernel") in lib.last_kernel(), lib.last_kernel()
    return got


def test_demod_measure_A(gpu, lib):
    """The constant of the bound: the worst error next to the constellation (scale 1, max_a t_a <= 32 nats), all eight constellations,
    0 .. 40 dB.  Measured on an MI355X: see fp32_model.DEMOD_A, which is four times the figure this test prints."""
    worst = 0.0
    for kind, m in DEMOD_CASES:
        md = _modem(kind, m)
        for snr_db in SNRS_DB:
            y, N0 = outliers(md.constellation, snr_db, 1.0, 2000, m + int(snr_db))
            near = np.repeat(M.demod_exponents(md.constellation, y, N0).max(axis=1) <= 32, md.num_bits_symbol)
            err = np.abs(_soft(lib, md, y, N0, kind) - M.demod_ref(md.constellation, y, N0)).astype(np.float64)
            worst = max(worst, float(err[near].max(initial=0.0)))
    print("fp32-fast demodulator: worst |error| next to the constellation %.3e; A = %.1e" % (worst, M.DEMOD_A))
    assert 4 * worst <= M.DEMOD_A


@pytest.mark.parametrize("kind,m", DEMOD_CASES)
@pytest.mark.parametrize("scale", [1, 3, 10, 30])
def test_demod_is_within_the_derived_bound_everywhere(gpu, lib, kind, m, scale):
    """Every LLR against the long-double reference, no magnitude mask: 0 .. 40 dB, partial waves, samples up to 30 times the
    constellation's size.  The re-summation branch (a bit subset that flushes to zero against the nearest point) is taken."""
    md = _modem(kind, m)
    c = md.constellation
    transcription = M.demod_sep_f32 if kind == "qam" else M.demod_gen_f32
    worst, worst_old, resummed = 0.0, 0.0, 0
    for i, snr_db in enumerate(SNRS_DB):
        Ns = SIZES[(i + scale) % 5]
        y, N0 = outliers(c, snr_db, float(scale), Ns, 7 * m + scale)
        ref, bound = M.demod_ref(c, y, N0), M.demod_bound(c, y, N0)
        resummed += transcription(c, y, N0, want_stats=True)[1]["resummed"]
        got = _soft(lib, md, y, N0, kind)
        assert got.shape == ref.shape and np.all(np.isfinite(got))
        ratio = np.abs(got - ref).astype(np.float64) / bound
        worst = max(worst, float(ratio.max()))
        worst_old = max(worst_old, float((np.abs(got - ref).astype(np.float64) / (2e-5 + 4e-6 * np.abs(ref).astype(np.float64))).max()))
        assert np.all(ratio <= 1.0), (snr_db, Ns, float(ratio.max()))
    print("fp32-fast demod %s-%d x%d: worst error / bound %.3f (/ the allowance 2e-5 + 4e-6 |LLR|: %.2f); %d subsets re-summed" % (
        kind, m, scale, worst, worst_old, resummed))
    assert resummed > 0 or m == 2


@pytest.mark.parametrize("kind,m", [("qam", 16), ("qam", 256), ("psk", 8), ("custom", 4)])
def test_demod_scaled_entry_and_special_values(gpu, lib, kind, m):
    """scale = -1 through cpx_demod_soft_scaled_dev: the negated LLRs.  A NaN, +-inf or 1e39 (beyond float32) component makes every LLR
    of its symbol NaN and moves no other symbol."""
    from commpy_amd.devicelink import DeviceBuf
    md = _modem(kind, m)
    so, nb = lib.load(), md.num_bits_symbol
    for Ns in SIZES:
        y, N0 = outliers(md.constellation, 12.0, 1.0, Ns, m + Ns)
        plain = _soft(lib, md, y, N0, kind)
        d_y, d_l = DeviceBuf(y.nbytes), DeviceBuf(Ns * nb * 8)
        lib.check(so.cpx_memcpy_h2d(d_y.ptr, lib.ptr(y), y.nbytes))
        lib.check(so.cpx_demod_soft_scaled_dev(md._device_handle(), d_y.ptr, Ns, N0, -1.0, d_l.ptr, None))
        assert "_f32_kernel" in lib.last_kernel()
        neg = np.empty(Ns * nb)
        lib.check(so.cpx_memcpy_d2h(lib.ptr(neg), d_l.ptr, neg.nbytes))
        assert np.array_equal(neg, -plain)
        re, im = y.real.copy(), y.imag.copy()
        where = sorted(set(int(v) % Ns for v in (0, 5, 62, 63, 64, 200, Ns - 1)))
        values = [(re, np.nan), (im, np.nan), (re, np.inf), (im, -np.inf), (re, 1e39), (im, -1e39), (re, -np.inf)]
        for s, (part, v) in zip(where, values):
            part[s] = v
        bad = np.empty(Ns, np.complex128)
        bad.real, bad.imag = re, im
        got = _soft(lib, md, bad, N0, kind).reshape(Ns, nb)
        hit = np.zeros(Ns, bool)
        hit[where[:len(values)]] = True
        assert np.isnan(got[hit]).all()
        assert np.array_equal(got[~hit].view(np.int64), plain.reshape(Ns, nb)[~hit].view(np.int64))
