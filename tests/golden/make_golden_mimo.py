#!/usr/bin/env python3
"""Generate tests/golden/mimo.npz from the LIVE reference (MIMO detectors, MIMOFlatChannel, the K-best link).

Run in the build container only (the GPU box has no reference checkout):

    python tests/golden/make_golden_mimo.py

Reference entry points exercised (file:line in the reference checkout):
  mimo_ml                 commpy/modulation.py:299
  kbest                   commpy/modulation.py:325
  bit_lvl_repr            commpy/modulation.py:568
  max_log_approx          commpy/modulation.py:599
  MIMOFlatChannel         commpy/channels.py:242
  LinkModel               commpy/links.py:67 (the 4x4 16-QAM hard K-best link of commpy/tests/test_links.py:44-59)

The reference breaks K-best ties with NumPy's unstable argsort and ML ties with argmin over norms, so a vector whose answer
hangs on a near-tie is not a fair exact-equality fixture: a vector is kept only when the reference's output is unchanged
under three relative 1e-10 perturbations of y; the number dropped is stored next to each case (``<case>_dropped``).
"""
import os
import sys
import warnings

os.environ.setdefault("MPLBACKEND", "Agg")
sys.dont_write_bytecode = True
REF = os.environ.get("COMMPY_REFERENCE", "/root/reference")
sys.path.insert(0, REF)

import numpy as np  # noqa: E402

warnings.simplefilter("ignore")

from commpy.channels import MIMOFlatChannel  # noqa: E402
from commpy.links import LinkModel  # noqa: E402
from commpy.modulation import QAMModem, PSKModem, bit_lvl_repr, kbest, max_log_approx, mimo_ml  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = {}


def rnd_c(rs, *shape):
    return (rs.randn(*shape) + 1j * rs.randn(*shape)) / np.sqrt(2)


def same(a, b, soft):
    if not soft:
        return np.array_equal(a, b, equal_nan=True)
    fin = np.isfinite(b)      # soft: the same +-inf / NaN pattern and finite values within 1e-6 (they move with y themselves)
    return (np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.where(fin, 0, a), np.where(fin, 0, b), equal_nan=True)
            and np.allclose(a[fin], b[fin], rtol=1e-6, atol=1e-6))


def stable(fn, y, rs, soft=False):
    """fn(y), or None when a relative 1e-10 perturbation of y changes it (NaN patterns compared as equal)."""
    base = np.asarray(fn(y))
    for _ in range(3):
        e = (rs.randn(*y.shape) + (1j * rs.randn(*y.shape) if np.iscomplexobj(y) else 0)) * 1e-10 * np.max(np.abs(y))
        if not same(np.asarray(fn(y + e)), base, soft):
            return None
    return base


def case(name, nr, nt, const, n, fn, rs, real=False, noise=0.3, soft=False):
    ys, hs, outs, dropped = [], [], [], 0
    for _ in range(n):
        h = rs.randn(nr, nt) if real else rnd_c(rs, nr, nt)
        x = const[rs.randint(0, len(const), nt)]
        y = h.dot(x) + noise * (rs.randn(nr) if real else rnd_c(rs, nr))
        out = stable(lambda yy: fn(yy, h), y, rs, soft)
        if out is None:
            dropped += 1
            continue
        ys.append(y), hs.append(h), outs.append(out)
    OUT[name + "_y"], OUT[name + "_h"], OUT[name + "_out"] = np.array(ys), np.array(hs), np.array(outs)
    OUT[name + "_const"] = np.asarray(const)
    OUT[name + "_dropped"] = np.array(dropped)
    print("%-24s kept %3d dropped %d" % (name, len(ys), dropped))


def main():
    rs = np.random.RandomState(20261015)
    bpsk = np.array([-1.0, 1.0])
    qpsk, q16, q64 = QAMModem(4), QAMModem(16), QAMModem(64)
    # ---- mimo_ml
    ml = lambda c: (lambda y, h: mimo_ml(y, h, c))  # noqa: E731
    case("ml_bpsk_real_3x3", 3, 3, bpsk, 40, ml(bpsk), rs, real=True)
    case("ml_qpsk_2x2", 2, 2, qpsk.constellation, 60, ml(qpsk.constellation), rs)
    case("ml_qpsk_4x4", 4, 4, qpsk.constellation, 60, ml(qpsk.constellation), rs)
    case("ml_qam16_2x2", 2, 2, q16.constellation, 60, ml(q16.constellation), rs, noise=0.6)
    case("ml_qam16_4x4", 4, 4, q16.constellation, 24, ml(q16.constellation), rs, noise=0.6)
    case("ml_qpsk_6x3", 6, 3, qpsk.constellation, 40, ml(qpsk.constellation), rs)
    case("ml_psk8_3x2", 3, 2, PSKModem(8).constellation, 40, ml(PSKModem(8).constellation), rs)
    # ---- kbest hard
    kb = lambda c, K: (lambda y, h: kbest(y, h, c, K))  # noqa: E731
    for K in (1, 4, 16, 64):
        case("kb_qam16_4x4_K%d" % K, 4, 4, q16.constellation, 80, kb(q16.constellation, K), rs, noise=0.6)
    case("kb_qam16_6x4_K8", 6, 4, q16.constellation, 60, kb(q16.constellation, 8), rs, noise=0.6)
    case("kb_qam64_2x2_K8", 2, 2, q64.constellation, 60, kb(q64.constellation, 8), rs, noise=1.0)
    case("kb_bpsk_real_4x4_K2", 4, 4, bpsk, 60, kb(bpsk, 2), rs, real=True)
    # ---- kbest soft with demode = modem.demodulate(., 'hard')
    dem = lambda symbs: q16.demodulate(symbs, 'hard')  # noqa: E731
    for i, nv in enumerate((0.0, 0.05, 0.5)):
        case("kbs_qam16_4x4_K16_nv%d" % i, 4, 4, q16.constellation, 40,
             lambda y, h, nv=nv: kbest(y, h, q16.constellation, 16, nv, 'soft', dem), rs, noise=0.6, soft=True)
        OUT["kbs_qam16_4x4_K16_nv%d_noise_var" % i] = np.array(nv)
    # ---- max_log_approx and bit_lvl_repr
    h = rnd_c(rs, 4, 4)
    pts = q16.constellation[rs.randint(0, 16, (4, 12))]
    y = rnd_c(rs, 4) * 2
    OUT["mla_y"], OUT["mla_h"], OUT["mla_pts"] = y, h, pts
    OUT["mla_out"] = max_log_approx(y, h, 0.3, pts, dem)
    w = np.array([1.0, 2.0, 0.5j, -1.0])
    OUT["blr_h"], OUT["blr_w"], OUT["blr_out"] = h, w, bit_lvl_repr(h, w)
    # ---- MIMOFlatChannel: seeded propagate for every fading setter
    msg = q16.constellation[rs.randint(0, 16, 30)]            # 30 symbols over 4 antennas: padding on the last vector
    OUT["chan_msg"] = msg
    setups = {
        "default": lambda ch: None,
        "rayleigh_c": lambda ch: ch.uncorr_rayleigh_fading(complex),
        "rayleigh_f": lambda ch: ch.uncorr_rayleigh_fading(float),
        "expo_rayleigh": lambda ch: ch.expo_corr_rayleigh_fading(np.exp(0.3j), np.exp(-0.7j), 0.2, 0.4),
        "rician": lambda ch: ch.uncorr_rician_fading(ch.specular_compo(0.4, 0.5, 1.1, 0.25), 3.0),
        "expo_rician": lambda ch: ch.expo_corr_rician_fading(ch.specular_compo(0.2, 0.1, 0.9, 0.3), 2.0, np.exp(0.5j),
                                                             np.exp(0.1j), 0.1, 0.3),
    }
    for name, setup in setups.items():
        ch = MIMOFlatChannel(4, 3, noise_std=0.2)
        setup(ch)
        m = msg.real if name in ("default", "rayleigh_f") else msg
        np.random.seed(77)
        OUT["chan_%s_out" % name] = ch.propagate(m)
        OUT["chan_%s_gains" % name] = ch.channel_gains
        OUT["chan_%s_kfactor" % name] = np.array(ch.k_factor)
        OUT["chan_%s_iscomplex" % name] = np.array(ch.isComplex)
    ch = MIMOFlatChannel(4, 3)
    OUT["chan_specular"] = ch.specular_compo(0.4, 0.5, 1.1, 0.25)
    # ---- the K-best link of test_links.py:44-59, per-transmission bit errors
    chan = MIMOFlatChannel(4, 4)
    chan.uncorr_rayleigh_fading(complex)

    def receiver(y, h, constellation, noise_var):
        return q16.demodulate(kbest(y, h, constellation, 16), 'hard')

    model = LinkModel(q16.modulate, chan, receiver, q16.num_bits_symbol, q16.constellation, q16.Es)
    snrs = np.array([12.0, 16.0])
    np.random.seed(8071996)
    BERs, BEs, CEs, NCs = model.link_performance_full_metrics(snrs, 12, 100, 128, 1)
    OUT["link_snrs"], OUT["link_BEs"], OUT["link_BERs"] = snrs, BEs, BERs
    OUT["link_tx_max"], OUT["link_err_min"], OUT["link_send_chunk"] = np.array(12), np.array(100), np.array(128)
    print("link BEs", BEs.tolist())
    path = os.path.join(HERE, "mimo.npz")
    np.savez_compressed(path, **OUT)
    print("wrote %s (%.1f kB, %d arrays)" % (path, os.path.getsize(path) / 1e3, len(OUT)))


if __name__ == "__main__":
    main()
