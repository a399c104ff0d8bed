"""Best-first soft MIMO detection on the MI355X (csrc/mimo.hip, best_first_kernel): the reference's goldens
(tests/golden/best_first.npz) through the single-vector and both batched forms, the workspace path against the LDS path, a
large batch against the single-vector form, and the third link of test_links.py (LDPC (1440,720), 16-QAM, 4x4 Rayleigh)."""
import os

import numpy as np
import pytest

from commpy_amd import _lib
from commpy_amd.channelcoding.ldpc import ldpc_bp_decode, triang_ldpc_systematic_encode
from commpy_amd.channels import MIMOFlatChannel
from commpy_amd.links import LinkModel, link_performance, mimo_receiver
from commpy_amd.modulation import Modem, QAMModem, best_first_batch, best_first_detector
from helpers import ldpc_params

pytestmark = pytest.mark.gpu
G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "best_first.npz"))
CASES = sorted({k[:-4] for k in G.files if k.startswith("bf_") and k.endswith("_out")})


def _rnd(rs, *shape):
    return (rs.randn(*shape) + 1j * rs.randn(*shape)) / np.sqrt(2)


def _assert_llr(got, want):
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.array_equal(np.where(np.isfinite(want), 0, got), np.where(np.isfinite(want), 0, want), equal_nan=True)
    fin = np.isfinite(want)
    assert np.all(np.abs(got[fin] - want[fin]) <= 1e-9 * np.maximum(1, np.abs(want[fin])))


def _table_demode(const, labels):
    """demode from a stored label table: the bits of each point, looked up by equality."""
    def demode(symbs):
        idx = np.argmax(np.asarray(symbs).reshape(-1)[:, None] == const[None, :], axis=1)
        return labels[idx].reshape(-1)
    return demode


def _case(case):
    return (G[case + "_y"], G[case + "_h"], G[case + "_out"], G[case + "_const"], G[case + "_labels"],
            tuple(int(s) for s in G[case + "_stacks"]), float(G[case + "_llr_max"]))


def test_goldens_present():
    assert len(CASES) >= 18, CASES
    assert all(len(G[c + "_out"]) >= 20 for c in CASES)
    # the wide-stack cases must test something the narrow stacks do not
    assert int(G["bf_qam16_4x4_s64_64_64_differ_from_135"]) + int(G["bf_qam16_4x4_s4096_4096_4096_differ_from_135"]) > 0


@pytest.mark.parametrize("case", CASES)
def test_best_first_golden(gpu, case):
    ys, hs, want, c, labels, stacks, llr_max = _case(case)
    demode = _table_demode(c, labels)
    with np.errstate(invalid="ignore"):
        single = np.array([best_first_detector(y, h, c, stacks, 0.1, demode, llr_max) for y, h in zip(ys, hs)])
    _assert_llr(single, want)
    md = Modem(c, reorder_as_gray=False)
    _assert_llr(best_first_batch(ys, hs, md, stacks, llr_max, labels), want)            # one H per vector
    shared = best_first_batch(ys, hs[0], md, stacks, llr_max, labels)                  # one H for the batch
    for b in range(0, len(ys), 7):
        _assert_llr(shared[b], best_first_detector(ys[b], hs[0], c, stacks, 0.1, demode, llr_max))


def test_large_stacks_take_the_workspace(gpu):
    ys, hs, _, c, labels, stacks, llr_max = _case("bf_qam16_4x4_s4096_4096_4096")
    best_first_batch(ys[:2], hs[:2], Modem(c, reorder_as_gray=False), stacks, llr_max, labels)
    assert "best_first_kernel<global>" in _lib.last_kernel(), _lib.last_kernel()


def test_modem_labels_by_default(gpu):
    ys, hs, want, c, labels, stacks, llr_max = _case("bf_qam16_4x4_135_n1")
    q16 = QAMModem(16)
    assert np.array_equal(q16.constellation, c)
    _assert_llr(best_first_batch(ys, hs, q16, stacks, llr_max), want)
    dem = lambda s: q16.demodulate(s, 'hard')  # noqa: E731
    _assert_llr(np.array([best_first_detector(y, h, c, stacks, 0.0, dem, llr_max) for y, h in zip(ys[:10], hs[:10])]), want[:10])


def test_noise_var_has_no_effect(gpu):
    ys, hs, _, c, labels, stacks, llr_max = _case("bf_qam16_4x4_135_n2")
    demode = _table_demode(c, labels)
    for y, h in zip(ys[:12], hs[:12]):
        a = best_first_detector(y, h, c, stacks, 0.01, demode, llr_max)
        b = best_first_detector(y, h, c, stacks, 7.5, demode, llr_max)
        assert np.array_equal(a, b)


def test_no_leaf_gives_nan(gpu):
    rs = np.random.RandomState(3)
    md = QAMModem(16)
    h = _rnd(rs, 3, 4, 4)
    y = _rnd(rs, 3, 4)
    y[1, 2] = np.nan
    out = best_first_batch(y, h, md, (1, 3, 5), 500)
    assert np.all(np.isnan(out[1])) and np.all(np.isfinite(out[[0, 2]]))
    with pytest.raises(ValueError):
        best_first_detector(y[1], h[1], md.constellation, (1, 3, 5), 0.1, lambda s: md.demodulate(s, 'hard'), 500)


@pytest.mark.parametrize("nr,nt,m,stacks", [(4, 4, 16, (1, 3, 5)), (3, 4, 64, (4, 16)), (8, 8, 4, (2, 2, 3, 3, 4, 4, 5)),
                                            (2, 2, 16, (16,))])
def test_general_equals_lds(gpu, nr, nt, m, stacks):
    rs = np.random.RandomState(nr * 10 + m)
    md = QAMModem(m)
    B = 3000
    h = _rnd(rs, B, nr, nt)
    y = np.einsum('bij,bj->bi', h, md.constellation[rs.randint(0, m, (B, nt))]) + 0.6 * _rnd(rs, B, nr)
    fast = best_first_batch(y, h, md, stacks, 500)
    assert "best_first_kernel<lds>" in _lib.last_kernel(), _lib.last_kernel()
    with _lib.forced_path("best_first", "general"):
        general = best_first_batch(y, h, md, stacks, 500)
        assert "best_first_kernel<global>" in _lib.last_kernel(), _lib.last_kernel()
    assert np.array_equal(fast, general, equal_nan=True)


def test_large_batch_matches_single(gpu):
    rs = np.random.RandomState(9)
    md = QAMModem(16)
    B = 1 << 20
    h = _rnd(rs, B, 4, 4)
    y = np.einsum('bij,bj->bi', h, md.constellation[rs.randint(0, 16, (B, 4))]) + 0.5 * _rnd(rs, B, 4)
    batch = best_first_batch(y, h, md, (1, 3, 5), 500)
    assert np.all(np.isfinite(batch))
    dem = lambda s: md.demodulate(s, 'hard')  # noqa: E731
    for b in rs.choice(B, 48, replace=False):
        assert np.array_equal(best_first_detector(y[b], h[b], md.constellation, (1, 3, 5), 0.25, dem, 500), batch[b])


def _link(batched):
    q16 = QAMModem(16)
    chan = MIMOFlatChannel(4, 4)
    chan.uncorr_rayleigh_fading(complex)
    ldpc = ldpc_params("wimax1440")

    def modulate(bits):
        return q16.modulate(triang_ldpc_systematic_encode(bits, ldpc, False).reshape(-1, order='F'))

    def decoder(llrs):
        return ldpc_bp_decode(llrs, ldpc, 'MSA', 15)[0][:720].reshape(-1, order='F')

    def demode(symbs):
        return q16.demodulate(symbs, 'hard')

    def receiver(y, h, constellation, noise_var):
        return best_first_detector(y, h, constellation, (1, 3, 5), noise_var, demode, 500)
    rx = mimo_receiver(q16, 'best_first') if batched else receiver
    return LinkModel(modulate, chan, rx, q16.num_bits_symbol, q16.constellation, q16.Es, decoder, 0.5)


@pytest.mark.parametrize("batched", [False, True])
def test_best_first_link_matches_reference(gpu, batched):
    model = _link(batched)
    np.random.seed(8071996)
    BERs, BEs, _, _ = model.link_performance_full_metrics(G["link_snrs"], int(G["link_tx_max"]), int(G["link_err_min"]),
                                                          int(G["link_send_chunk"]), 0.5)
    assert np.array_equal(BEs, G["link_BEs"]), (BEs, G["link_BEs"])
    np.testing.assert_allclose(BERs, G["link_BERs"], rtol=1e-15)


@pytest.mark.slow
def test_best_first_link_performance(gpu):
    """test_links.py:61-86 and :92-99, the reference's own assertion on the third link."""
    model = _link(True)
    snrs = np.arange(17, 20)
    np.random.seed(8071996)
    BERs = link_performance(model, snrs, 5e5, 200, 720, model.rate)
    np.testing.assert_allclose(BERs, (1.7e-1, 1e-1, 2.5e-3), rtol=2)
    full = model.link_performance_full_metrics(snrs, 2500, 200, 720, model.rate)
    np.testing.assert_allclose(full[0], (1.7e-1, 1e-1, 2.5e-3), rtol=2)
