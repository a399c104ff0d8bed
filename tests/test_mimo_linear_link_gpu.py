"""The linear detectors inside the two link layers: ``mimo_receiver('zf' | 'mmse')`` under ``LinkModel`` and
``DeviceMimoLink(detector='zf' | 'mmse')``, uncoded and LDPC-coded, against ``linear_batch`` and the NumPy model of
tests/mimo_linear_model.py on the link's own kept arrays -- exact counts, no statistical tolerance."""
import numpy as np
import pytest

import mimo_linear_model as L
from commpy_amd.channelcoding.ldpc import ldpc_bp_decode
from commpy_amd.channels import MIMOFlatChannel
from commpy_amd.devicelink import DeviceMimoLink
from commpy_amd.links import LinkModel, mimo_receiver
from commpy_amd.modulation import QAMModem, linear_batch
from helpers import ldpc_params

pytestmark = pytest.mark.gpu


def _rayleigh(nr=4, nt=4):
    ch = MIMOFlatChannel(nt, nr)
    ch.uncorr_rayleigh_fading(complex)
    return ch


def _bits_of(symbols, md):
    labels = np.argmax(symbols.reshape(-1)[:, None] == md.constellation[None, :], axis=1)
    return ((labels[:, None] >> np.arange(md.num_bits_symbol - 1, -1, -1)) & 1).reshape(-1)


@pytest.mark.parametrize("detector", ["zf", "mmse"])
def test_receiver_in_link_model_gives_linear_batch_bits(gpu, detector):
    md = QAMModem(16)
    inner, seen = mimo_receiver(md, detector), []

    def receive(y, h, constellation, noise_var):
        out = inner(y, h, constellation, noise_var)
        seen.append((np.array(y), np.array(h), noise_var, np.array(out)))
        return out
    receive.batched = True
    np.random.seed(11)
    model = LinkModel(md.modulate, _rayleigh(), receive, md.num_bits_symbol, md.constellation, md.Es)
    ber = model.link_performance([8.0], 16 * 40 * 4, 10 ** 9, 16 * 40)
    assert len(seen) == 4 and 0 < ber[0] < 0.5
    for y, h, noise_var, out in seen:
        assert y.shape == (40, 4) and h.shape == (40, 4, 4)
        # the complex channel's noise has variance noise_var / 2 (quirk B7): the MMSE regulariser is noise_var / (2 Es)
        reg = 0.0 if detector == "zf" else noise_var / (2 * md.Es)
        assert np.array_equal(out, _bits_of(linear_batch(y, h, md, noise_var, detector, 'hard', reg), md))
    soft = mimo_receiver(md, detector, output_type='soft')
    y, h, noise_var, _ = seen[0]
    reg = 0.0 if detector == "zf" else noise_var / (2 * md.Es)
    assert np.array_equal(soft(y, h, md.constellation, noise_var), linear_batch(y, h, md, noise_var, detector, 'soft', reg).reshape(-1))


@pytest.mark.parametrize("detector", ["zf", "mmse"])
def test_device_link_keeps_what_linear_batch_gives(gpu, detector):
    md = QAMModem(16)
    link = DeviceMimoLink(md, _rayleigh(), detector=detector)
    link.keep_rx = True
    errs = link.run_batch(14.0, 300)
    rx = link.last_rx
    noise_var = rx['noise_std'] ** 2
    reg = 0.0 if detector == "zf" else noise_var / (2 * md.Es)
    assert errs.shape == (300,) and errs.sum() > 0
    want = linear_batch(rx['y'], rx['h'], md, noise_var, detector, 'hard', reg)
    assert np.array_equal(md.constellation[rx['idx']], want)
    assert np.array_equal(errs, (_bits_of(want, md).reshape(rx['msg'].shape) != rx['msg']).sum(axis=1))


def test_uncoded_qpsk_point_counts_what_the_model_counts(gpu):
    """One 4x4 QPSK point at a high SNR: the link's error count against the host model on the link's own y and H."""
    md = QAMModem(4)
    link = DeviceMimoLink(md, _rayleigh(), detector='mmse', send_chunk=800)
    link.keep_rx = True
    errs = link.run_batch(30.0, 200)
    rx = link.last_rx
    noise_var = rx['noise_std'] ** 2
    w = L.linear_model(rx['y'], rx['h'], md.constellation, noise_var / (2 * md.Es), noise_var)
    assert not w["bad"].any() and np.all(w["margin"] >= L.MARGIN_MIN * md.Es)     # no decision of this batch is a near-tie
    bits = ((w["idx"].reshape(-1)[:, None] >> np.array([1, 0])) & 1).reshape(rx['msg'].shape)
    model_errs = (bits != rx['msg']).sum(axis=1)
    print("4x4 QPSK MMSE at 30 dB: %d bit errors in %d bits (model: %d)" % (errs.sum(), rx['msg'].size, model_errs.sum()))
    assert np.array_equal(errs, model_errs)
    assert errs.sum() / rx['msg'].size < 0.02


def test_ldpc_coded_point_decodes(gpu):
    """One (1440, 720) LDPC-coded 4x4 QPSK point: the soft output reaches the decoder with the right sign and layout.  At this
    SNR the MODEL's LLRs of the kept batch decode without a block error on the host, so the link must count none."""
    md, ldpc = QAMModem(4), ldpc_params("wimax1440")
    link = DeviceMimoLink(md, _rayleigh(), detector='mmse', output_type='soft', ldpc_params=ldpc, send_chunk=720)
    link.keep_rx = True
    T = 12
    errs = link.run_batch(16.0, T)
    rx = link.last_rx
    noise_var = rx['noise_std'] ** 2
    w = L.linear_model(rx['y'], rx['h'], md.constellation, noise_var / (2 * md.Es), noise_var)
    assert not w["bad"].any() and rx['llr'].shape == w["llr"].shape
    assert np.mean(np.signbit(rx['llr']) == np.signbit(w["llr"])) > 0.999          # same sign convention, same layout
    assert np.mean((rx['llr'].reshape(T, -1) < 0) == (rx['tx'] == 1)) > 0.8       # negative: bit 1
    vpt = link.vectors_per_tx
    for t in range(T):
        dec = ldpc_bp_decode(w["llr"][t * vpt:(t + 1) * vpt].reshape(-1).copy(), ldpc, 'MSA', 15)[0]
        assert np.array_equal(dec[:720].reshape(-1, order='F'), rx['msg'][t])      # the model's LLRs decode cleanly
    assert not errs.any()
