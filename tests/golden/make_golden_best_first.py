#!/usr/bin/env python3
"""Generate tests/golden/best_first.npz from the LIVE reference (soft-output best-first detection, idd_decoder, the third
link of test_links.py).

Run in the build container only (the GPU box has no reference checkout):

    python tests/golden/make_golden_best_first.py

Reference entry points exercised (file:line in the reference checkout):
  best_first_detector     commpy/modulation.py:422
  idd_decoder             commpy/links.py:345
  LinkModel               commpy/links.py:67 (the 4x4 16-QAM best-first LDPC link of commpy/tests/test_links.py:61-86)

The reference orders children with NumPy's unstable argsort and compares metrics against radii built from other metrics,
so a vector whose LLRs hang on a near-tie is not a fair fixture: a vector is kept only when its LLRs are unchanged under
three relative 1e-10 perturbations of y; the number dropped is stored next to each case (``<case>_dropped``).
Every case stores y [n, nr], h [n, nr, nt], the constellation, the label table demode(constellation) [m, log2 m], the stack
sizes, llr_max and the LLRs [n, nr * log2 m].
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

from commpy.channelcoding.ldpc import get_ldpc_code_params, ldpc_bp_decode, triang_ldpc_systematic_encode  # noqa: E402
from commpy.channels import MIMOFlatChannel  # noqa: E402
from commpy.links import LinkModel, idd_decoder  # noqa: E402
from commpy.modulation import PSKModem, QAMModem, best_first_detector  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = {}


# deterministic toy callbacks for idd_decoder -- tests/test_best_first_host.py defines the same ones
def toy_detector(y, h, constellation, noise_var, a_priori):
    z = h.conj().T.dot(y)
    return np.concatenate([z.real, z.imag]) * 0.75 + 0.5 * np.tanh(a_priori) - noise_var


def toy_decoder(llrs):
    return 1.5 * llrs + np.roll(llrs, 1) * 0.25 - 0.125


def toy_decision(llrs):
    return llrs * 1.0


def toy_inputs():
    rs = np.random.RandomState(345)
    nb_vect, nr, nt = 5, 3, 2
    y = rs.randn(nb_vect, nr) + 1j * rs.randn(nb_vect, nr)
    h = rs.randn(nb_vect, nr, nt) + 1j * rs.randn(nb_vect, nr, nt)
    return y, h, rs.randn(nb_vect * 2 * nt), 2 * nt


def rnd_c(rs, *shape):
    return (rs.randn(*shape) + 1j * rs.randn(*shape)) / np.sqrt(2)


def same(a, b):
    fin = np.isfinite(b)      # the same +-inf / NaN pattern and finite values within 1e-6 (they move with y themselves)
    return (np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.where(fin, 0, a), np.where(fin, 0, b), equal_nan=True)
            and np.allclose(a[fin], b[fin], rtol=1e-6, atol=1e-6))


def stable(fn, y, rs):
    """fn(y), or None when a relative 1e-10 perturbation of y changes it."""
    base = np.asarray(fn(y))
    for _ in range(3):
        e = (rs.randn(*y.shape) + (1j * rs.randn(*y.shape) if np.iscomplexobj(y) else 0)) * 1e-10 * np.max(np.abs(y))
        if not same(np.asarray(fn(y + e)), base):
            return None
    return base


def vectors(rs, n, nr, nt, const, noise, real=False):
    out = []
    for _ in range(n):
        h = rs.randn(nr, nt) if real else rnd_c(rs, nr, nt)
        x = const[rs.randint(0, len(const), nt)]
        nz = noise[rs.randint(len(noise))] if np.ndim(noise) else noise
        y = h.dot(x) + nz * (rs.randn(nr) if real else rnd_c(rs, nr))
        out.append((y, h))
    return out


def case(name, vecs, const, demode, stacks, llr_max, rs, noise_var=0.1):
    ys, hs, outs, dropped = [], [], [], 0
    for y, h in vecs:
        out = stable(lambda yy: best_first_detector(yy, h, const, stacks, noise_var, demode, llr_max), y, rs)
        if out is None:
            dropped += 1
            continue
        ys.append(y), hs.append(h), outs.append(out)
    OUT[name + "_y"], OUT[name + "_h"], OUT[name + "_out"] = np.array(ys), np.array(hs), np.array(outs, dtype=float)
    OUT[name + "_const"] = np.asarray(const)
    OUT[name + "_labels"] = np.asarray(demode(np.asarray(const))).reshape(len(const), -1).astype(np.uint8)
    OUT[name + "_stacks"] = np.array(stacks)
    OUT[name + "_llr_max"] = np.array(float(llr_max))
    OUT[name + "_dropped"] = np.array(dropped)
    print("%-30s kept %3d dropped %d" % (name, len(ys), dropped))
    return dict(zip([y.tobytes() for y in ys], outs))


def main():
    rs = np.random.RandomState(20261016)
    bpsk = np.array([-1.0, 1.0])
    qpsk, q16, q64, psk8 = QAMModem(4), QAMModem(16), QAMModem(64), PSKModem(8)
    dem = lambda md: (lambda s: md.demodulate(s, 'hard'))  # noqa: E731
    d16 = dem(q16)
    # ---- 4x4 16-QAM, (1, 3, 5), llr_max 500 at three noise levels
    for i, nz in enumerate((0.15, 0.4, 0.9)):
        case("bf_qam16_4x4_135_n%d" % i, vectors(rs, 60, 4, 4, q16.constellation, nz), q16.constellation, d16, (1, 3, 5), 500, rs)
    # ---- stack sizes, on ONE set of vectors (low and high noise): how often do wide stacks change the answer?
    vs = vectors(rs, 80, 4, 4, q16.constellation, np.array([0.3, 0.8, 1.2]))
    narrow = case("bf_qam16_4x4_s1_3_5", vs, q16.constellation, d16, (1, 3, 5), 500, rs)
    for st in ((1, 1, 1), (4, 8, 16), (64, 64, 64), (4096, 4096, 4096)):
        name = "bf_qam16_4x4_s%s" % "_".join(map(str, st))
        got = case(name, vs, q16.constellation, d16, st, 500, rs)
        diff = sum(1 for k, v in got.items() if k in narrow and not same(v, narrow[k]))
        OUT[name + "_differ_from_135"] = np.array(diff)
        print("   %d vectors differ from (1, 3, 5)" % diff)
    # ---- clipping
    case("bf_qam16_4x4_llr2", vectors(rs, 60, 4, 4, q16.constellation, 0.5), q16.constellation, d16, (1, 3, 5), 2.0, rs)
    case("bf_qam16_4x4_llrinf", vectors(rs, 60, 4, 4, q16.constellation, 0.5), q16.constellation, d16, (1, 3, 5), np.inf, rs)
    # ---- other shapes and constellations
    case("bf_qpsk_2x2", vectors(rs, 60, 2, 2, qpsk.constellation, 0.5), qpsk.constellation, dem(qpsk), (2,), 500, rs)
    case("bf_bpsk_real_3x3", vectors(rs, 60, 3, 3, bpsk, 0.6, real=True), bpsk, lambda s: (np.asarray(s) > 0).astype(int),
         (1, 2), 500, rs)
    case("bf_qpsk_8x8", vectors(rs, 40, 8, 8, qpsk.constellation, 0.5), qpsk.constellation, dem(qpsk), (1, 2, 3, 4, 5, 6, 7),
         500, rs)
    case("bf_qam64_4x4", vectors(rs, 40, 4, 4, q64.constellation, 0.3), q64.constellation, dem(q64), (1, 3, 5), 500, rs)
    case("bf_qam16_2x3", vectors(rs, 60, 2, 3, q16.constellation, 0.4), q16.constellation, d16, (3,), 500, rs)
    case("bf_qam16_3x4", vectors(rs, 60, 3, 4, q16.constellation, 0.4), q16.constellation, d16, (2, 4, 9), 500, rs)
    case("bf_psk8_3x3", vectors(rs, 60, 3, 3, psk8.constellation, 0.4), psk8.constellation, dem(psk8), (2, 3), 500, rs)
    case("bf_qam16_4x4_inv_labels", vectors(rs, 60, 4, 4, q16.constellation, 0.5), q16.constellation,
         lambda s: 1 - q16.demodulate(s, 'hard'), (1, 3, 5), 500, rs)
    # ---- idd_decoder with the deterministic toy callbacks above
    y, h, ap, bps = toy_inputs()
    OUT["idd_y"], OUT["idd_h"], OUT["idd_apriori"], OUT["idd_bps"] = y, h, ap, np.array(bps)
    for n_it in (1, 2, 3):
        OUT["idd_out_it%d" % n_it] = idd_decoder(toy_detector, toy_decoder, toy_decision, n_it)(y, h, None, 0.3, ap, bps)
    # ---- the third link of test_links.py:61-86, per-transmission bit errors
    ldpc = get_ldpc_code_params(os.path.join(REF, 'commpy/channelcoding/designs/ldpc/wimax/1440.720.txt'), True)
    chan = MIMOFlatChannel(4, 4)
    chan.uncorr_rayleigh_fading(complex)

    def modulate(bits):
        return q16.modulate(triang_ldpc_systematic_encode(bits, ldpc, False).reshape(-1, order='F'))

    def decoder(llrs):
        return ldpc_bp_decode(llrs, ldpc, 'MSA', 15)[0][:720].reshape(-1, order='F')

    def receiver(y, h, constellation, noise_var):
        return best_first_detector(y, h, constellation, (1, 3, 5), noise_var, d16, 500)

    model = LinkModel(modulate, chan, receiver, q16.num_bits_symbol, q16.constellation, q16.Es, decoder, 0.5)
    snrs = np.arange(17, 20)
    np.random.seed(8071996)
    BERs, BEs, CEs, NCs = model.link_performance_full_metrics(snrs, 24, 200, 720, 0.5)
    OUT["link_snrs"], OUT["link_BEs"], OUT["link_BERs"] = snrs, BEs, BERs
    OUT["link_tx_max"], OUT["link_err_min"], OUT["link_send_chunk"] = np.array(24), np.array(200), np.array(720)
    print("link BEs", BEs.tolist(), "BERs", BERs.tolist())
    path = os.path.join(HERE, "best_first.npz")
    np.savez_compressed(path, **OUT)
    print("wrote %s (%.1f kB, %d arrays)" % (path, os.path.getsize(path) / 1e3, len(OUT)))


if __name__ == "__main__":
    main()
