"""MIMO detection on the MI355X (csrc/mimo.hip): the reference's goldens (tests/golden/mimo.npz), cross-checks without the
reference on large batches, the general kernel against the LDS-resident one, and the K-best link of test_links.py."""
import os

import numpy as np
import pytest

from commpy_amd import _lib
from commpy_amd.channels import MIMOFlatChannel
from commpy_amd.links import LinkModel, mimo_receiver
from commpy_amd.modulation import Modem, QAMModem, kbest, kbest_batch, mimo_ml, mimo_ml_batch

pytestmark = pytest.mark.gpu
G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mimo.npz"))
ML_CASES = sorted({k[:-4] for k in G.files if k.startswith("ml_") and k.endswith("_out")})
KB_CASES = sorted({k[:-4] for k in G.files if k.startswith("kb_") and k.endswith("_out")})
SOFT_CASES = sorted({k[:-4] for k in G.files if k.startswith("kbs_") and k.endswith("_out")})


def _rnd(rs, *shape):
    return (rs.randn(*shape) + 1j * rs.randn(*shape)) / np.sqrt(2)


def _q16_dem(symbs, md=QAMModem(16)):
    return md.demodulate(symbs, 'hard')


@pytest.mark.parametrize("case", ML_CASES)
def test_ml_golden(gpu, case):
    ys, hs, want, c = G[case + "_y"], G[case + "_h"], G[case + "_out"], G[case + "_const"]
    for y, h, w in zip(ys, hs, want):
        assert np.array_equal(mimo_ml(y, h, c), w)
    batch = mimo_ml_batch(ys, hs, c)                                   # one H per vector
    assert np.array_equal(batch, want)
    assert np.array_equal(mimo_ml_batch(ys, hs[0], c), np.array([mimo_ml(y, hs[0], c) for y in ys]))   # shared H


@pytest.mark.parametrize("case", KB_CASES)
def test_kbest_hard_golden(gpu, case):
    K = int(case.split("_K")[1])
    ys, hs, want, c = G[case + "_y"], G[case + "_h"], G[case + "_out"], G[case + "_const"]
    for y, h, w in zip(ys, hs, want):
        got = kbest(y, h, c, K)
        assert got.dtype == w.dtype and np.array_equal(got, w)
    md = Modem(c, reorder_as_gray=False)
    assert np.array_equal(kbest_batch(ys, hs, md, K), want)
    assert np.array_equal(kbest_batch(ys, hs[0], md, K), np.array([kbest(y, hs[0], c, K) for y in ys]))


def _assert_llr(got, want):
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.array_equal(np.where(np.isfinite(want), 0, got), np.where(np.isfinite(want), 0, want), equal_nan=True)
    fin = np.isfinite(want)
    assert np.all(np.abs(got[fin] - want[fin]) <= 1e-9 * np.maximum(1, np.abs(want[fin])))


@pytest.mark.parametrize("case", SOFT_CASES)
def test_kbest_soft_golden(gpu, case):
    nv = float(G[case + "_noise_var"])
    ys, hs, want, c = G[case + "_y"], G[case + "_h"], G[case + "_out"], G[case + "_const"]
    with np.errstate(divide="ignore", invalid="ignore"):
        single = np.array([kbest(y, h, c, 16, nv, 'soft', _q16_dem) for y, h in zip(ys, hs)])
        batch = kbest_batch(ys, hs, QAMModem(16), 16, nv, 'soft')
    _assert_llr(single, want)
    _assert_llr(batch, want)


def test_kbest_full_width_equals_ml(gpu):
    """K >= m^(nt-1) keeps every hypothesis at the last antenna: K-best is then ML, up to metric ties."""
    rs = np.random.RandomState(5)
    md = QAMModem(16)
    B = 4096
    h = _rnd(rs, B, 4, 4)
    y = np.einsum('bij,bj->bi', h, md.constellation[rs.randint(0, 16, (B, 4))]) + 0.7 * _rnd(rs, B, 4)
    ml = mimo_ml_batch(y, h, md)
    kb = kbest_batch(y, h, md, 16 ** 3)
    diff = np.flatnonzero(np.any(ml != kb, axis=1))
    ties = 0
    for b in diff:                                         # only an exact-metric tie may separate them
        d_ml = np.linalg.norm(y[b] - h[b] @ ml[b]) ** 2
        d_kb = np.linalg.norm(y[b] - h[b] @ kb[b]) ** 2
        assert abs(d_ml - d_kb) <= 1e-12 * max(d_ml, d_kb), (b, d_ml, d_kb)
        ties += 1
    print("K-best (full width) vs ML: %d of %d vectors differ by a metric tie" % (ties, B))


def test_ml_qpsk_brute_force(gpu):
    rs = np.random.RandomState(6)
    md = QAMModem(4)
    B = 2048
    h = _rnd(rs, B, 4, 4)
    y = np.einsum('bij,bj->bi', h, md.constellation[rs.randint(0, 4, (B, 4))]) + 0.8 * _rnd(rs, B, 4)
    digits = (np.arange(256)[:, None] >> (2 * np.arange(3, -1, -1))) & 3   # antenna 0 the most significant digit
    hyp = md.constellation[digits]                                          # [256, 4]
    metric = np.sum(np.abs(y[:, None, :] - np.einsum('bij,hj->bhi', h, hyp)) ** 2, axis=2)
    want = hyp[np.argmin(metric, axis=1)]
    assert np.array_equal(mimo_ml_batch(y, h, md), want)


def test_kbest_large_batch_matches_single(gpu):
    rs = np.random.RandomState(7)
    md = QAMModem(16)
    B = 1 << 20
    h = _rnd(rs, B, 4, 4)
    y = np.einsum('bij,bj->bi', h, md.constellation[rs.randint(0, 16, (B, 4))]) + 0.5 * _rnd(rs, B, 4)
    hard = kbest_batch(y, h, md, 16)
    with np.errstate(divide="ignore", invalid="ignore"):
        soft = kbest_batch(y, h, md, 16, 0.25, 'soft')
        for b in rs.choice(B, 48, replace=False):
            assert np.array_equal(kbest(y[b], h[b], md.constellation, 16), hard[b])
            _assert_llr(kbest(y[b], h[b], md.constellation, 16, 0.25, 'soft', _q16_dem), soft[b])


@pytest.mark.parametrize("nr,nt,m,K", [(4, 4, 16, 16), (6, 4, 16, 8), (3, 2, 64, 5), (4, 4, 4, 64)])
def test_kbest_general_equals_fast(gpu, nr, nt, m, K):
    rs = np.random.RandomState(nr * 100 + K)
    md = QAMModem(m)
    B = 3000
    h = _rnd(rs, B, nr, nt)
    y = np.einsum('bij,bj->bi', h, md.constellation[rs.randint(0, m, (B, nt))]) + 0.6 * _rnd(rs, B, nr)
    with np.errstate(divide="ignore", invalid="ignore"):
        fast = (kbest_batch(y, h, md, K), kbest_batch(y, h, md, K, 0.3, 'soft'))
        assert "kbest_kernel<lds>" in _lib.last_kernel(), _lib.last_kernel()
        with _lib.forced_path("kbest", "general"):
            general = (kbest_batch(y, h, md, K), kbest_batch(y, h, md, K, 0.3, 'soft'))
            assert "kbest_kernel<global>" in _lib.last_kernel(), _lib.last_kernel()
    assert np.array_equal(fast[0], general[0])
    assert np.array_equal(fast[1], general[1], equal_nan=True)


def _link(batched):
    q16 = QAMModem(16)
    chan = MIMOFlatChannel(4, 4)
    chan.uncorr_rayleigh_fading(complex)

    def receiver(y, h, constellation, noise_var):
        return q16.demodulate(kbest(y, h, constellation, 16), 'hard')
    rx = mimo_receiver(q16, 'kbest', 16) if batched else receiver
    return LinkModel(q16.modulate, chan, rx, q16.num_bits_symbol, q16.constellation, q16.Es)


@pytest.mark.parametrize("batched", [False, True])
def test_kbest_link_matches_reference(gpu, batched):
    model = _link(batched)
    np.random.seed(8071996)
    BERs, BEs, _, _ = model.link_performance_full_metrics(G["link_snrs"], int(G["link_tx_max"]), int(G["link_err_min"]),
                                                          int(G["link_send_chunk"]), 1)
    assert np.array_equal(BEs, G["link_BEs"]), (BEs, G["link_BEs"])
    np.testing.assert_allclose(BERs, G["link_BERs"], rtol=1e-15)
