#!/usr/bin/env python3
"""Goldens of the waveform modules from the live reference (runs only where the reference checkout exists):

    python tests/golden/make_golden_waveform.py [REFERENCE_ROOT]

writes tests/golden/waveform.npz (taps of the four filter generators, pnsequence, zcsequence, add_frequency_offset) and
tests/golden/reference_fingerprints_waveform.json (statement fingerprints of filters.py, sequences.py, impairments.py in the
format of reference_fingerprints.json).  Data only.

A raised-cosine / root-raised-cosine case is kept only if min |1 - (2 alpha t / Ts)^2| (RC) or |1 - (4 alpha t / Ts)^2| (RRC)
over the samples that take the general formula is >= 1e-3, so that no golden rests on a 0/0 decided by the last bit of sin."""
import itertools
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
sys.path.insert(0, REF)
sys.path.insert(0, os.path.dirname(HERE))

sys.path.insert(0, HERE)

from commpy import filters, impairments, sequences  # noqa: E402
from make_golden_waveform_shared import FO_STRIDE, fo_input  # noqa: E402

NS = (16, 25, 32, 33, 64, 97, 128, 129)
ALPHAS = (0, 0.22, 0.25, 0.35, 0.5, 1)
TSFS = ((1, 4), (1, 8), (1e-3, 6e3), (1, 5), (0.5, 32), (1 / 3, 12))
PN = [(4, "1111", "1001"), (5, "10101", "00101"), (6, "100000", "000011"), (7, "1000000", "0000011"), (8, "10000001", "10001110"),
      (9, "000000001", "000010001"), (10, "1010101010", "0000001001"), (11, "1" * 11, "00000000101"),
      (12, "1" + "0" * 11, "100000101001"), (13, "0" * 12 + "1", "1000000001101"), (14, "1" * 14, "10000000101011"),
      (15, "1" * 15, "000000000000011"), (16, "1" + "0" * 15, "1000000000010110")]
ZC = [(1, 2, 0), (3, 20, 0), (7, 20, 3), (25, 139, 0), (29, 139, -4), (25, 839, 0), (129, 839, 11), (5, 4093, 0), (2047, 4093, 2)]
FO = [(1, 1e6, 1e3), (7, 1.0, 0.25), (1000, 8e3, -37.5), (1000, 1.0, 0.0), (4096, 1e3, 499.99), (100000, 2e6, 1.234e5),
      (100000, 1.0, 12345.678), (333, 48e3, -1e9)]


def margin(kind, N, alpha, Ts, Fs):
    t = (np.arange(N) - N / 2) * (1 / float(Fs))
    c = 2 if kind == "rc" else 4
    general = t != 0.0
    if alpha != 0:
        general &= np.abs(t) != Ts / (c * alpha)
    v = c * alpha * t[general] / Ts
    return float(np.min(np.abs(1 - v * v))) if v.size else 1.0


def main():
    out, kept, dropped = {}, 0, 0
    cases = []
    for N, alpha, (Ts, Fs) in itertools.product(NS, ALPHAS, TSFS):
        for kind, fn in (("rc", filters.rcosfilter), ("rrc", filters.rrcosfilter)):
            if margin(kind, N, alpha, Ts, Fs) < 1e-3:
                dropped += 1
                continue
            t, h = fn(N, alpha, Ts, Fs)
            i = len(cases)
            cases.append((0 if kind == "rc" else 1, N, alpha, Ts, Fs))
            out["tap_h_%d" % i] = h
            assert np.array_equal(out.setdefault("tap_t_%d_%r" % (N, float(Fs)), t), t)
            kept += 1
    for N, alpha, (Ts, Fs) in itertools.product((16, 33, 97), (0.22, 0.5, 1), TSFS[:3]):
        t, h = filters.gaussianfilter(N, alpha, Ts, Fs)
        i = len(cases)
        cases.append((2, N, alpha, Ts, Fs))
        out["tap_h_%d" % i] = h
        assert np.array_equal(out.setdefault("tap_t_%d_%r" % (N, float(Fs)), t), t)
        t, h = filters.rectfilter(N, Ts, Fs)
        i = len(cases)
        cases.append((3, N, 0.0, Ts, Fs))
        out["tap_h_%d" % i] = h
        assert np.array_equal(out.setdefault("tap_t_%d_%r" % (N, float(Fs)), t), t)
    out["tap_cases"] = np.array(cases, dtype=np.float64)       # kind (0 rc, 1 rrc, 2 gaussian, 3 rect), N, alpha, Ts, Fs
    for order, seed, mask in PN:
        length = min(2 ** order - 1 + 10, 3000)
        out["pn_%d_str" % order] = sequences.pnsequence(order, seed, mask, length)
        out["pn_%d_list" % order] = sequences.pnsequence(order, [int(c) for c in seed], tuple(int(c) for c in mask), length)
        out["pn_%d_arr" % order] = sequences.pnsequence(order, np.array([int(c) for c in seed]), np.array([int(c) for c in mask]), length)
    out["pn_cases"] = np.array([[o, int(s, 2), int(m, 2)] for o, s, m in PN])
    out["zc_cases"] = np.array(ZC)
    for i, (u, L, q) in enumerate(ZC):
        out["zc_%d" % i] = sequences.zcsequence(u, L, q)
    # the input of case i is fo_input(i, n) below (seeded, so it is not stored); of a long output every FO_STRIDE-th sample is kept
    out["fo_cases"] = np.array(FO, dtype=np.float64)
    for i, (n, Fs, df) in enumerate(FO):
        y = impairments.add_frequency_offset(fo_input(i, n), Fs, df)
        out["fo_y_%d" % i] = y if n <= 5000 else y[::FO_STRIDE]
    path = os.path.join(HERE, "waveform.npz")
    np.savez_compressed(path, **out)
    print("taps: kept %d, dropped %d (margin < 1e-3); wrote %s (%.1f kB)" % (kept, dropped, path, os.path.getsize(path) / 1e3))

    import test_no_verbatim_copies as nv
    files = {}
    for theirs in ("filters.py", "sequences.py", "impairments.py"):
        p = os.path.join(REF, "commpy", theirs)
        files[theirs] = {"statements": [nv.fingerprint(s) for s in nv._statements(p)],
                         "functions": {k: [nv.fingerprint(s) for s in v] for k, v in sorted(nv._functions(p).items())}}
    fp = os.path.join(HERE, "reference_fingerprints_waveform.json")
    with open(fp, "w") as f:
        json.dump({"what": "sha256(normalised statement)[:16] of the reference files, tests/test_waveform_host.py",
                   "python": "%d.%d" % sys.version_info[:2], "files": files}, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print("wrote %s" % fp)


if __name__ == "__main__":
    main()
