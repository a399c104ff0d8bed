"""The MIMO kernels of csrc/mimo.hip against the NumPy models of tests/mimo_model.py (pinned without a GPU by
tests/test_mimo_model_host.py): random cases at the shapes where a lane-strided loop takes a second pass, the direct ML kernel,
the natural global K-best path, the candidate list's order and count, the LDS paths' grid wrap, exact metric ties and NaN / inf.

Indices, list order and count are compared exactly; LLRs under the rule of tests/test_mimo_gpu.py.  A vector of a random case
is left out where the MODEL calls it a near-tie (gap <= 1e-9, a condition on the input); at most 2 % of a case may be."""
import time

import numpy as np
import pytest

import mimo_model as M
from commpy_amd import _lib
from commpy_amd.modulation import Modem, QAMModem, _kbest_list, kbest_batch, mimo_ml_batch

pytestmark = pytest.mark.gpu
_modems = {}


def modem_of(m):
    if m not in _modems:
        _modems[m] = Modem(M.BPSK, reorder_as_gray=False) if m == 2 else QAMModem(m)
    return _modems[m]


def _note(want):
    note = _lib.last_kernel()
    assert want in note, note
    return note


def _kbest_all(y, h, md, K, want_note):
    """hard symbols, (list, count), {noise_var: LLRs} of one batch, each launch leaving ``want_note``."""
    with np.errstate(all="ignore"):
        hard = kbest_batch(y, h, md, K)
        note = _note(want_note)
        lst = _kbest_list(y, h, md, K)
        _note(want_note)
        soft = {}
        for nv in M.NOISE_VARS:
            soft[nv] = kbest_batch(y, h, md, K, nv, 'soft')
            _note(want_note)
    return hard, lst, soft, note


@pytest.mark.parametrize("shared", [True, False], ids=["sharedH", "ownH"])
@pytest.mark.parametrize("i", range(len(M.ML_CASES)), ids=[M.ml_case_id(c) for c in M.ML_CASES])
def test_ml_matches_model(gpu, i, shared):
    nr, nt, m, B, real, kernel = M.ML_CASES[i]
    md = modem_of(m)
    y, h, want, keep = M.ml_case(i, shared, md.constellation)
    assert (y.dtype == np.float64) == real and np.sum(~keep) <= M.SCREEN_CAP * B
    t0 = time.perf_counter()
    got = mimo_ml_batch(y, h, md)
    dt = time.perf_counter() - t0
    print("ML %s %s: %s, %d of %d screened out, %.3f s" % (M.ml_case_id(M.ML_CASES[i]), "shared H" if shared else "own H",
                                                         _note(kernel), int(np.sum(~keep)), B, dt))
    assert np.array_equal(got[keep], md.constellation[want][keep])


@pytest.mark.parametrize("shared", [True, False], ids=["sharedH", "ownH"])
@pytest.mark.parametrize("i", range(len(M.KB_CASES)), ids=[M.kb_case_id(c) for c in M.KB_CASES])
def test_kbest_matches_model(gpu, i, shared):
    nr, nt, m, K, B, path = M.KB_CASES[i]
    md = modem_of(m)
    y, h, lists, counts, keep, llr = M.kb_case(i, shared, md.constellation)
    assert np.sum(~keep) <= M.SCREEN_CAP * B
    runs = [(False, "kbest_kernel<%s>" % path)] + ([(True, "kbest_kernel<global>")] if path == "lds" else [])
    for forced, kernel in runs:
        t0 = time.perf_counter()
        if forced:
            with _lib.forced_path("kbest", "general"):
                hard, (cand, count), soft, note = _kbest_all(y, h, md, K, kernel)
        else:
            hard, (cand, count), soft, note = _kbest_all(y, h, md, K, kernel)
        print("K-best %s %s%s: %s, %d of %d screened out, 4 launches %.3f s" % (
            M.kb_case_id(M.KB_CASES[i]), "shared H" if shared else "own H", " forced general" if forced else "", note,
            int(np.sum(~keep)), B, time.perf_counter() - t0))
        assert np.array_equal(hard[keep], md.constellation[lists[:, 0]][keep])
        assert cand.shape == lists.shape and np.array_equal(count, counts)      # the count holds for a near-tie too
        assert np.array_equal(cand[keep], lists[keep])
        for nv in M.NOISE_VARS:
            M.assert_llr(soft[nv][keep], llr[nv][keep])
    if K == 1 and m > 2:
        assert np.all(np.isinf(soft[0.3]))                                      # one survivor: every bit misses a value


def test_grid_wrap_on_lds_paths(gpu):
    """B = 2^20 + 70 > grid_for(B): workgroups 0..69 of the LDS-resident kernels take a second vector on the state the first
    left behind -- a NaN vector among the first ones."""
    md = modem_of(4)
    c = md.constellation
    y, h, want, keep = M.wrap_case(c)
    sel = M.WRAP_SEL
    ys, hs = np.ascontiguousarray(y[sel]), np.ascontiguousarray(h[sel])
    t0 = time.perf_counter()
    with np.errstate(all="ignore"):
        big = {"hard": kbest_batch(y, h, md, M.WRAP_K)}
        _note("kbest_kernel<lds>")
        big["soft"] = kbest_batch(y, h, md, M.WRAP_K, M.WRAP_NOISE_VAR, 'soft')
        _note("kbest_kernel<lds>")
        big["ml"] = mimo_ml_batch(y, h, md)
        _note("mimo_ml_kernel<table>")
        small = {"hard": kbest_batch(ys, hs, md, M.WRAP_K), "soft": kbest_batch(ys, hs, md, M.WRAP_K, M.WRAP_NOISE_VAR, 'soft'),
                 "ml": mimo_ml_batch(ys, hs, md)}
    print("wrap: three launches of %d vectors and three of %d in %.2f s" % (M.WRAP_B, sel.size, time.perf_counter() - t0))
    for k in ("hard", "soft", "ml"):
        assert np.array_equal(big[k][sel], small[k], equal_nan=True), k          # bit for bit
    assert np.array_equal(big["ml"][sel][keep], c[want["ml"]][keep])
    assert np.array_equal(big["hard"][sel][keep], c[want["hard"]][keep])
    M.assert_llr(big["soft"][sel][keep], want["soft"][keep])
    after = int(np.flatnonzero(sel == (1 << 20) + M.WRAP_NAN)[0])
    assert keep[after] and np.all(np.isnan(big["soft"][M.WRAP_NAN])) and not np.any(np.isnan(big["soft"][(1 << 20) + M.WRAP_NAN]))


TIES = M.tie_inputs(QAMModem(4).constellation, QAMModem(16).constellation)


@pytest.mark.parametrize("name", [t[0] for t in TIES])
def test_exact_ties(gpu, name):
    """Metric ties that are exact in float64 (tests/test_mimo_model_host.py proves the model exact on them): ML takes the first
    minimum in hypothesis order, K-best orders equal metrics by the child position -- inside the list, across the keep / drop
    boundary, at an inner level and at the last.  No screening."""
    _, ys, h, c, K = next(t for t in TIES if t[0] == name)
    md = modem_of(len(c))
    nt = h.shape[1]
    ml = np.array([M.ml_exact(y, h, c)[0] for y in ys])
    kb = [M.kbest_model(y, h, c, K) for y in ys]
    lists = np.array([M.pad_list(r[0], min(K, len(c) ** nt)) for r in kb])
    counts = np.array([r[1] for r in kb])
    for hh in (h, np.ascontiguousarray(np.broadcast_to(h, (len(ys),) + h.shape))):       # shared, one per vector
        assert np.array_equal(mimo_ml_batch(ys, hh, md), c[ml])
        for forced in (False, True):
            if forced:
                with _lib.forced_path("kbest", "general"):
                    hard, (cand, count) = kbest_batch(ys, hh, md, K), _kbest_list(ys, hh, md, K)
                    _note("kbest_kernel<global>")
            else:
                hard, (cand, count) = kbest_batch(ys, hh, md, K), _kbest_list(ys, hh, md, K)
                _note("kbest_kernel<lds>")
            assert np.array_equal(hard, c[lists[:, 0]])
            assert np.array_equal(count, counts) and np.array_equal(cand, lists)


def test_nan_and_inf_vectors(gpu):
    """A NaN in y, +inf in y and a NaN in a vector's own H inside an ordinary batch: those three equal the model (np.argmin:
    the first NaN; a stable argsort: NaN last, equal metrics by position), every other vector is bit-identical to the batch
    without them."""
    md = modem_of(16)
    c = md.constellation
    K, nv = M.SPECIAL_K, 0.3
    y0, h0, y, h = M.special_inputs(c)
    bad = sorted(M.SPECIAL.values())
    rest = np.setdiff1d(np.arange(M.SPECIAL_B), bad)

    def run(yy, hh):
        with np.errstate(all="ignore"):
            return {"ml": mimo_ml_batch(yy, hh, md), "hard": kbest_batch(yy, hh, md, K), "list": _kbest_list(yy, hh, md, K),
                    "soft": kbest_batch(yy, hh, md, K, nv, 'soft')}

    clean = run(y0, h0)
    outs = [run(y, h)]
    _note("kbest_kernel<lds>")
    with _lib.forced_path("kbest", "general"):
        outs.append(run(y, h))
        _note("kbest_kernel<global>")
    for got in outs:
        assert np.array_equal(got["ml"][rest], clean["ml"][rest]) and np.array_equal(got["hard"][rest], clean["hard"][rest])
        assert np.array_equal(got["list"][0][rest], clean["list"][0][rest]) and np.array_equal(got["list"][1], clean["list"][1])
        assert np.array_equal(got["soft"][rest], clean["soft"][rest], equal_nan=True)
        assert np.all(np.isfinite(got["soft"][rest]) | np.isinf(got["soft"][rest]))
        for b in bad:
            assert np.array_equal(got["ml"][b], c[M.ml_model(y[b], h[b], c)[0]]), b
            cand, n, _ = M.kbest_model(y[b], h[b], c, K)
            assert np.array_equal(got["hard"][b], c[cand[0]]), b
            assert got["list"][1][b] == n and np.array_equal(got["list"][0][b], M.pad_list(cand, K)), b
            assert np.array_equal(got["soft"][b], M.kbest_llr_model(y[b], h[b], c, cand, nv), equal_nan=True), b
