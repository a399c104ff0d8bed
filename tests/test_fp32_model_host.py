"""The float32 models of the fp32-fast kernels (tests/fp32_model.py) without a GPU: against the float64 oracle wherever float32 is
exact, against the long-double demodulator, and the demodulator's derived error bound on the float32 transcription of both kernels."""
import numpy as np
import pytest

import fp32_model as M
import oracle
from helpers import ldpc_params, make_trellis

K7 = ("k7_133_171", "wifi_decimal_133_171")


def _encode(msgs, tr, termination="term"):
    from commpy_amd.channelcoding import conv_encode_batch
    return conv_encode_batch(msgs, tr, termination)


# ---- Viterbi --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", K7)
@pytest.mark.parametrize("tb", [None, 2, 15, 40])
def test_viterbi_model_hard_is_the_oracle(name, tb):
    """0/1 input: the metrics are Hamming distances, exact in float32 -- the model IS the reference's decision rule."""
    tr = make_trellis(name)
    rs = np.random.RandomState(3)
    for length in (14, 62, 202):
        if tb and tb > length // 2 + 6:                                # beyond T + 1 steps the reference never runs a traceback
            continue
        x = rs.randint(0, 2, (9, length)).astype(np.float64)           # random words: ties at every step
        got, stats = M.viterbi(x, tr, tb, "hard", want_stats=True)
        want = np.stack([oracle.viterbi_decode(r, tr, tb, "hard") for r in x])
        assert np.array_equal(got, want)
        assert stats["select_ties"] > 100 and stats["best_ties"] > 10


@pytest.mark.parametrize("name", K7)
@pytest.mark.parametrize("dtype", ["hard", "soft", "unquantized"])
@pytest.mark.parametrize("termination", ["term", "cont"])
def test_viterbi_model_decodes_clean_words(name, dtype, termination):
    tr = make_trellis(name)
    msgs = np.random.RandomState(5).randint(0, 2, (7, 70)).astype(np.uint8)
    coded = _encode(msgs, tr, termination).astype(np.float64)
    x = coded if dtype == "hard" else (8.0 * (2 * coded - 1) if dtype == "soft" else 2 * coded - 1)
    got = M.viterbi(x, tr, None, dtype)
    n = 70 if termination == "term" else 70 - 30                       # 'cont': the last bits have no tail behind them
    assert np.array_equal(got[:, :n], msgs[:, :n])


def test_viterbi_model_float64_twin_follows_the_oracle_on_unquantized():
    """The same rule run in float64 (the twin the near-tie search uses) is the float64 oracle: squared distances, no exp / log."""
    tr = make_trellis("k7_133_171")
    rs = np.random.RandomState(6)
    x = 2.0 * rs.randint(0, 2, (6, 120)) - 1 + 0.8 * rs.randn(6, 120)
    want = np.stack([oracle.viterbi_decode(r, tr, None, "unquantized") for r in x])
    assert np.array_equal(M.viterbi(x, tr, None, "unquantized", dtype=np.float64), want)


# ---- LDPC -----------------------------------------------------------------------------------------------------------------------------
def _codeword_llrs(p, rs, B, scale):
    """All-zero codeword: positive LLRs, multiples of 1/8 -- exact in float32, and so is every sum the decoder forms of them."""
    n = int(p["n_vnodes"])
    return np.round(8 * (scale + 1.2 * scale * rs.randn(B, n))) / 8


@pytest.mark.parametrize("name", ["gallager96", "n1944"])
@pytest.mark.parametrize("iters", [1, 2])
def test_minsum_model_on_dyadic_input_is_the_float64_oracle(name, iters):
    p = ldpc_params(name)
    tab = M.LdpcTables.from_params(p)
    llr = _codeword_llrs(p, np.random.RandomState(7), 5, 2.0)
    llr[0] = np.abs(llr[0]) + 0.125                                     # a codeword on arrival: returned unchanged
    assert np.array_equal(llr.astype(np.float32).astype(np.float64), llr)
    got = M.ldpc_decode(llr, tab, "MSA", iters)
    dec, out, its = oracle.ldpc_bp_decode(llr.reshape(-1).copy(), p, "MSA", iters, return_iters=True)
    assert got["iters"][0] == 0 and got["iters"][1:].min() >= 1
    assert np.array_equal(got["iters"], its)
    assert np.array_equal(got["out"].view(np.int64), np.ascontiguousarray(out.T).view(np.int64))
    assert np.array_equal(got["dec"], dec.T)


@pytest.mark.parametrize("alg", ["MSA", "SPA"])
def test_ldpc_models_return_the_codeword(alg):
    p = ldpc_params("gallager96")
    tab = M.LdpcTables.from_params(p)
    llr = np.full((3, 96), 6.0)                                         # noise-free all-zero word
    llr[1, 5] = -1.0                                                    # one and two unreliable bits: corrected
    llr[2, [7, 50]] = -0.5
    got = M.ldpc_decode(llr, tab, alg, 20)
    assert not got["dec"].any() and got["iters"][0] == 0 and np.array_equal(got["out"][0], llr[0])
    assert 1 <= got["iters"][1] < 20 and 1 <= got["iters"][2] < 20


def test_spa_model_tiny_messages_are_finite():
    """|m| down to the smallest normal float: tanh(m / 2) = m / 2 stays non-zero, no 1 / 0; only an exact zero gives inf * 0 = NaN."""
    p = ldpc_params("gallager96")
    tab = M.LdpcTables.from_params(p)
    llr = np.random.RandomState(2).randn(2, 96) * 3
    llr[0, [0, 20, 40, 60, 80]] = [1e-30, 1e-10, -1e-9, 2e-8, 1e-6]
    got = M.ldpc_decode(llr, tab, "SPA", 2)
    assert np.all(np.isfinite(got["out"]))
    llr[0, 3] = 0.0
    got = M.ldpc_decode(llr, tab, "SPA", 1)
    assert np.array_equal(np.nonzero(np.isnan(got["out"][0]))[0], [3]) and np.all(np.isfinite(got["out"][1]))


def test_sum_product_margin_excludes_under_one_percent():
    """The seeds of the GPU comparison: the model's LLR lies within the tolerance of zero (where dec_word may differ) at under 1 % of the
    positions, and most blocks never show a check pass a |Q| that close (so their iteration counts are compared)."""
    import test_fp32_edges_gpu as G
    for name in ("gallager96", "n1944", "irregular"):
        p, tab = G._ldpc(name)
        for iters in (1, 2):
            inside = total = safe = blocks = 0
            for seed in G.SPA_SEEDS:
                want = M.ldpc_decode(G._spa_rows(p, seed), tab, "SPA", iters)
                inside += int((np.abs(want["out"]) <= G.SPA_TOL[iters]).sum())
                total += want["out"].size
                safe += int((want["margin"] > G.SPA_TOL[iters]).sum())
                blocks += len(want["margin"])
            assert inside <= 0.01 * total and 2 * safe >= blocks, (name, iters, inside, total, safe, blocks)


# ---- demodulator ----------------------------------------------------------------------------------------------------------------------
def _modem(kind, M_):
    from commpy_amd.modulation import PSKModem, QAMModem
    return QAMModem(M_) if kind == "qam" else PSKModem(M_)


CUSTOM4 = np.array([1.0 + 0.25j, -0.5 + 1.5j, -1.0 - 0.25j, 0.5 - 1.5j])          # contains -c with every c; not axis-separable


def outliers(c, snr_db, scale, Ns, seed):
    """Constellation points plus noise at Es/N0, then the whole sample multiplied by ``scale``: far from every point for scale > 1."""
    rs = np.random.RandomState(seed)
    Es = float(np.mean(np.abs(c) ** 2))
    N0 = Es / 10 ** (snr_db / 10)
    y = c[rs.randint(0, len(c), Ns)] + np.sqrt(N0 / 2) * (rs.randn(Ns) + 1j * rs.randn(Ns))
    return scale * y, N0


@pytest.mark.parametrize("kind,M_", [("qam", 4), ("qam", 16), ("qam", 64), ("psk", 2), ("psk", 8), ("psk", 16)])
def test_long_double_reference_is_the_float64_oracle(kind, M_):
    c = _modem(kind, M_).constellation
    seen = 0
    for snr_db in (0.0, 10.0, 20.0, 30.0):
        y, N0 = outliers(c, snr_db, 1.0, 400, M_)
        want = oracle.demodulate(c, y, "soft", N0)
        got = M.demod_ref(c, y, N0)
        ok = np.isfinite(want) & (np.abs(want) < 600)
        seen += int(ok.sum())
        assert np.all(np.abs(got[ok].astype(np.float64) - want[ok]) <= 1e-12)
        assert np.all(np.isfinite(got))
    assert seen > 1000


GRID = [("qam", 16, 10.0), ("qam", 64, 20.0), ("qam", 256, 28.0)]


@pytest.mark.parametrize("kind,M_,snr_db", GRID)
@pytest.mark.parametrize("scale", [1, 3, 10, 30])
def test_derived_bound_holds_for_the_transcription_on_the_outlier_grid(kind, M_, snr_db, scale):
    """The bound A + K 2^-24 max_a t_a (derived in fp32_model's docstring) on the float32 transcription of BOTH kernels against the long-double
    reference, twelve cells; beside it the old allowance 2e-5 + 4e-6 |LLR|, which holds next to the constellation only."""
    c = _modem(kind, M_).constellation
    y, N0 = outliers(c, snr_db, float(scale), 3000, 100 * M_ + scale)
    ref = M.demod_ref(c, y, N0)
    bound = M.demod_bound(c, y, N0)
    old = 2e-5 + 4e-6 * np.abs(ref.astype(np.float64))
    over_old = 0.0
    for name, fn in (("sep", M.demod_sep_f32), ("gen", M.demod_gen_f32)):
        got = fn(c, y, N0)
        err = np.abs(got - ref).astype(np.float64)
        over_old = max(over_old, float((err / old).max()))
        print("%s-%d %g dB x%d %s: worst error / derived bound %.3f, / old allowance %.2f (worst |err| %.3g, worst |LLR| %.3g)" % (
            kind, M_, snr_db, scale, name, (err / bound).max(), (err / old).max(), err.max(), np.abs(ref).max()))
        assert np.all(np.isfinite(got))
        assert np.all(err <= bound), (name, float((err / bound).max()))
    if scale >= 10:
        assert over_old > 1.0                                           # the old contract is false out here


def test_transcriptions_take_the_resummation_branch_and_stay_finite():
    for c, fn in ((_modem("qam", 64).constellation, M.demod_sep_f32), (_modem("psk", 8).constellation, M.demod_gen_f32),
                  (CUSTOM4, M.demod_gen_f32)):
        y, N0 = outliers(c, 40.0, 1.0, 257, 9)
        got, stats = fn(c, y, N0, want_stats=True)
        assert stats["resummed"] > 100
        ref = M.demod_ref(c, y, N0)
        assert np.all(np.abs(got - ref) <= M.demod_bound(c, y, N0))
        assert np.array_equal(fn(c, y, N0, scale=-1.0), -got)
