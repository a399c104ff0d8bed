"""The NumPy models of tests/mimo_model.py, pinned without a GPU: they reproduce every ML, K-best and soft K-best case of the
reference's goldens (tests/golden/mimo.npz), they are exact on the tie inputs (bit for bit equal to an evaluation in rational
arithmetic, with the intended ties really present), and no random case of tests/test_mimo_model_gpu.py loses more than 2 % of
its vectors to the near-tie screen."""
import os
import time
from fractions import Fraction

import numpy as np
import pytest

import mimo_model as M
from commpy_amd.modulation import QAMModem

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mimo.npz"))
ML_GOLD = sorted({k[:-4] for k in G.files if k.startswith("ml_") and k.endswith("_out")})
KB_GOLD = sorted({k[:-4] for k in G.files if k.startswith("kb_") and k.endswith("_out")})
SOFT_GOLD = sorted({k[:-4] for k in G.files if k.startswith("kbs_") and k.endswith("_out")})


def const_of(m):
    return M.BPSK if m == 2 else QAMModem(m).constellation


def test_goldens_are_all_here():
    assert len(ML_GOLD) == 7 and len(KB_GOLD) == 7 and len(SOFT_GOLD) == 3


@pytest.mark.parametrize("case", ML_GOLD)
def test_ml_model_reproduces_golden(case):
    ys, hs, want, c = G[case + "_y"], G[case + "_h"], G[case + "_out"], G[case + "_const"]
    for y, h, w in zip(ys, hs, want):
        idx, gap = M.ml_model(y, h, c)
        assert np.array_equal(c[idx], w) and gap > M.GAP_MIN


@pytest.mark.parametrize("case", KB_GOLD)
def test_kbest_model_reproduces_golden(case):
    K = int(case.split("_K")[1])
    ys, hs, want, c = G[case + "_y"], G[case + "_h"], G[case + "_out"], G[case + "_const"]
    for y, h, w in zip(ys, hs, want):
        cand, n, gap = M.kbest_model(y, h, c, K)
        assert n == len(cand) == min(K, len(c) ** h.shape[1])
        assert np.array_equal(c[cand[0]], w) and gap > M.GAP_MIN


@pytest.mark.parametrize("case", SOFT_GOLD)
def test_kbest_llr_model_reproduces_golden(case):
    nv = float(G[case + "_noise_var"])
    ys, hs, want, c = G[case + "_y"], G[case + "_h"], G[case + "_out"], G[case + "_const"]
    assert np.array_equal(c, QAMModem(16).constellation)          # index bits are then the labels of the goldens' demode
    got = np.array([M.kbest_llr_model(y, h, c, M.kbest_model(y, h, c, 16)[0], nv) for y, h in zip(ys, hs)])
    M.assert_llr(got, want)


# ---- the tie inputs: the float64 model is exact on them, and the ties are there -------------------------------------------------
TIES = M.tie_inputs(const_of(4), const_of(16))
# equal minima of the ML metric per vector
ML_MINIMA = {"qpsk_3x3_K3": [8, 2, 1, 2, 2, 4, 4], "qam16_2x2_K4": [4, 2, 2, 2, 2, 4, 4], "qpsk_2I_K3": [64, 2, 2, 4]}
ML_MINIMA["qpsk_3x3_K2"] = ML_MINIMA["qpsk_3x3_K5"] = ML_MINIMA["qpsk_3x3_K3"]
ML_MINIMA["qam16_2x2_K6"] = ML_MINIMA["qam16_2x2_K4"]
# (vector, level) pairs, level 0 the first (antenna nt - 1), where a K-best tie straddles the keep / drop boundary
KB_STRADDLES = {
    "qpsk_3x3_K3": [(0, 0), (0, 2), (1, 0), (5, 0), (5, 2), (6, 0), (6, 2)],
    "qpsk_3x3_K2": [(0, 0), (0, 2), (2, 0), (2, 1), (3, 0), (4, 0), (5, 0), (5, 1), (6, 2)],
    "qpsk_3x3_K5": [(0, 1), (0, 2), (3, 1), (4, 1), (5, 1), (5, 2), (6, 2)],      # level 1 is an inner level
    "qam16_2x2_K4": [(2, 1)],
    "qam16_2x2_K6": [(0, 0), (0, 1), (4, 0), (5, 0), (5, 1), (6, 0), (6, 1)],
    "qpsk_2I_K3": [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 1), (2, 2), (3, 0)],
}


def _same(floats, exact):
    return len(floats) == len(exact) and all(Fraction(float(a)) == b for a, b in zip(floats, exact))


@pytest.mark.parametrize("name", [t[0] for t in TIES])
def test_tie_inputs_exact_and_tied(name):
    _, ys, h, c, K = next(t for t in TIES if t[0] == name)
    assert np.all(np.diag(h).real > 0) and not np.any(np.tril(h, -1))
    straddles, final_ties = [], 0
    for v, y in enumerate(ys):
        met = M.ml_metrics(y, h, c)
        idx, _ = M.ml_model(y, h, c)
        idx_x, met_x = M.ml_exact(y, h, c)
        assert np.array_equal(idx, idx_x) and _same(met, met_x)
        assert int(np.sum(met == met.min())) == sum(mx == min(met_x) for mx in met_x) == ML_MINIMA[name][v]
        levels = []
        cand, n, _ = M.kbest_model(y, h, c, K, levels)
        cand_x, n_x, levels_x = M.kbest_exact(y, h, c, K)
        assert n == n_x and np.array_equal(cand, cand_x)
        assert len(levels) == len(levels_x) == h.shape[1]
        for lvl, ((child, nk), (child_x, nk_x)) in enumerate(zip(levels, levels_x)):
            assert nk == nk_x and _same(child, child_x)
            s = sorted(child_x)
            if len(s) > nk and s[nk - 1] == s[nk]:
                straddles.append((v, lvl))
            if lvl == len(levels) - 1:
                final_ties += sum(a == b for a, b in zip(s[:nk - 1], s[1:nk]))
    assert straddles == KB_STRADDLES[name]
    assert final_ties > 0                                       # ties inside the list that is returned, every case


# ---- the near-tie screen of the GPU file's random cases ------------------------------------------------------------------------
@pytest.mark.parametrize("shared", [True, False], ids=["sharedH", "ownH"])
@pytest.mark.parametrize("i", range(len(M.ML_CASES)), ids=[M.ml_case_id(c) for c in M.ML_CASES])
def test_ml_cases_screen_cap(i, shared):
    t0 = time.perf_counter()
    keep = M.ml_case(i, shared, const_of(M.ML_CASES[i][2]))[3]
    out = int(np.sum(~keep))
    print("ML %s %s: %d of %d screened out (model %.2f s)" % (M.ml_case_id(M.ML_CASES[i]), "shared H" if shared else "own H", out,
                                                             keep.size, time.perf_counter() - t0))
    assert out <= M.SCREEN_CAP * keep.size


@pytest.mark.parametrize("shared", [True, False], ids=["sharedH", "ownH"])
@pytest.mark.parametrize("i", range(len(M.KB_CASES)), ids=[M.kb_case_id(c) for c in M.KB_CASES])
def test_kbest_cases_screen_cap(i, shared):
    t0 = time.perf_counter()
    _, _, lists, counts, keep, llr = M.kb_case(i, shared, const_of(M.KB_CASES[i][2]))
    nr, nt, m, K, B, _ = M.KB_CASES[i]
    out = int(np.sum(~keep))
    print("K-best %s %s: %d of %d screened out (model %.2f s)" % (M.kb_case_id(M.KB_CASES[i]), "shared H" if shared else "own H",
                                                                 out, B, time.perf_counter() - t0))
    assert out <= M.SCREEN_CAP * B
    assert np.all(counts == min(K, m ** nt)) and lists.shape == (B, min(K, m ** nt), nt) and lists.min() >= 0
    if K == 1 and m > 2:                                        # one survivor: every bit misses a value
        assert np.all(np.isinf(llr[0.3]))


def test_wrap_case_screen_cap():
    y, h, want, keep = M.wrap_case(const_of(4))
    print("wrap: %d of %d compared vectors screened out" % (int(np.sum(~keep)), keep.size))
    assert np.sum(~keep) <= M.SCREEN_CAP * keep.size and keep[M.WRAP_NAN]
    assert np.all(want["ml"][M.WRAP_NAN] == 0) and np.all(want["hard"][M.WRAP_NAN] == 0) and np.all(np.isnan(want["soft"][M.WRAP_NAN]))
    assert np.all(np.isfinite(want["soft"][M.WRAP_SEL != M.WRAP_NAN]) | np.isinf(want["soft"][M.WRAP_SEL != M.WRAP_NAN]))
