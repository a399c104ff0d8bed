"""Host side of the MIMO feature: MIMOFlatChannel, max_log_approx and bit_lvl_repr against the reference's goldens
(tests/golden/mimo.npz, tests/golden/make_golden_mimo.py), argument errors, and the new entry points' lack of a CPU fallback."""
import os

import numpy as np
import pytest

from commpy_amd import _lib
from commpy_amd.channels import MIMOFlatChannel
from commpy_amd.modulation import QAMModem, bit_lvl_repr, kbest, kbest_batch, max_log_approx, mimo_ml, mimo_ml_batch

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mimo.npz"))
SETUPS = {
    "default": lambda ch: None,
    "rayleigh_c": lambda ch: ch.uncorr_rayleigh_fading(complex),
    "rayleigh_f": lambda ch: ch.uncorr_rayleigh_fading(float),
    "expo_rayleigh": lambda ch: ch.expo_corr_rayleigh_fading(np.exp(0.3j), np.exp(-0.7j), 0.2, 0.4),
    "rician": lambda ch: ch.uncorr_rician_fading(ch.specular_compo(0.4, 0.5, 1.1, 0.25), 3.0),
    "expo_rician": lambda ch: ch.expo_corr_rician_fading(ch.specular_compo(0.2, 0.1, 0.9, 0.3), 2.0, np.exp(0.5j),
                                                         np.exp(0.1j), 0.1, 0.3),
}


@pytest.mark.parametrize("name", sorted(SETUPS))
def test_mimo_channel_matches_reference(name):
    ch = MIMOFlatChannel(4, 3, noise_std=0.2)
    SETUPS[name](ch)
    msg = G["chan_msg"].real if name in ("default", "rayleigh_f") else G["chan_msg"]
    np.random.seed(77)
    out = ch.propagate(msg)
    assert ch.isComplex == bool(G["chan_%s_iscomplex" % name])
    assert out.shape == G["chan_%s_out" % name].shape == (8, 3)
    np.testing.assert_allclose(ch.channel_gains, G["chan_%s_gains" % name], rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(out, G["chan_%s_out" % name], rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(ch.k_factor, G["chan_%s_kfactor" % name], rtol=1e-12)


def test_mimo_channel_checks():
    np.testing.assert_allclose(MIMOFlatChannel(4, 3).specular_compo(0.4, 0.5, 1.1, 0.25), G["chan_specular"], rtol=1e-13)
    with pytest.raises(ValueError):
        MIMOFlatChannel(2, 2, fading_param=(np.zeros((2, 2)), 2 * np.identity(2), np.identity(2)))
    ch = MIMOFlatChannel(2, 2, 0.1)
    with pytest.raises(TypeError):
        ch.propagate(np.array([1j, 1]))               # complex message, real channel
    with pytest.raises(ValueError):
        ch.expo_corr_rayleigh_fading(2.0, 1.0)
    with pytest.raises(AssertionError):
        MIMOFlatChannel(2, 2).propagate(np.ones(4))   # noise_std not set


def test_max_log_approx_and_bit_lvl_repr():
    q16 = QAMModem(16)
    hard = {tuple(p): i for i, p in enumerate(np.c_[q16.constellation.real, q16.constellation.imag])}

    def demode(symbs):                                # host labels: no device needed
        idx = [hard[(s.real, s.imag)] for s in symbs]
        return ((np.array(idx)[:, None] >> np.arange(3, -1, -1)) & 1).reshape(-1)
    got = max_log_approx(G["mla_y"], G["mla_h"], 0.3, G["mla_pts"], demode)
    want = G["mla_out"]
    assert np.array_equal(np.isinf(got), np.isinf(want))
    fin = np.isfinite(want)
    np.testing.assert_allclose(got[fin], want[fin], rtol=1e-12)
    np.testing.assert_allclose(bit_lvl_repr(G["blr_h"], G["blr_w"]), G["blr_out"], rtol=1e-14)
    with pytest.raises(ValueError):
        bit_lvl_repr(G["blr_h"], [1, 2, 3])


def test_kbest_argument_errors():
    c = QAMModem(4).constellation
    with pytest.raises(ValueError):
        kbest(np.zeros(2, complex), np.ones((2, 3), complex), c, 4)           # nt > nr
    with pytest.raises(ValueError):
        kbest(np.zeros(2, complex), np.ones((2, 2), complex), c, 4, output_type='soft-ish')
    with pytest.raises(ValueError):
        kbest_batch(np.zeros((3, 2), complex), np.ones((2, 3), complex), QAMModem(4), 4)


def test_mimo_entry_points_fail_without_device():
    if _lib.device_count() > 0:
        pytest.skip("a HIP device is present")
    c = QAMModem(4).constellation
    y, h = np.zeros(2, complex), np.eye(2, dtype=complex)
    for call in (lambda: mimo_ml(y, h, c), lambda: kbest(y, h, c, 4), lambda: mimo_ml_batch(y[None], h, c),
                 lambda: kbest_batch(y[None], h, QAMModem(4), 4, 0.1, 'soft')):
        with pytest.raises(_lib.EngineError):
            call()
