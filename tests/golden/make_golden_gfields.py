#!/usr/bin/env python3
"""Generate tests/golden/gfields.json from the LIVE reference: what ``GF`` of commpy/channelcoding/gfields.py returns.

Run where the reference checkout exists:

    python tests/golden/make_golden_gfields.py

Per m in 2, 3, 4, 5, 6, 8, for the whole field ``arange(2^m)``, the non-zero elements ``arange(1, 2^m)`` and one seeded subset with
repeats: ``tuple_to_power``, ``order`` and ``cosets`` (a list of lists); ``power_to_tuple`` of the exponents ``0 .. min(2 (2^m - 1), 62)``
(``2**i`` on NumPy integers wraps from i = 63 on, and the reference returns garbage there); sums of two seeded vectors.  ``minpolys`` and products are recorded for m <= 4 only: above, the reference's ``bitarray2dec`` raises
OverflowError under NumPy 2 (a product of 2 m - 1 > 8 bits accumulated in int8).  For the same reason ``cyclic_code_genpoly`` is
not recorded (tests/test_bch_host.py holds the lists of the reference's own test suite)."""
import json
import os
import sys
import warnings

sys.dont_write_bytecode = True
REF = os.environ.get("COMMPY_REFERENCE", "/root/reference")
sys.path.insert(0, REF)

import numpy as np  # noqa: E402

warnings.simplefilter("ignore")

from commpy.channelcoding.gfields import GF  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))


def methods(x, m, with_minpolys):
    g = GF(x, m)
    out = {"elements": x.tolist(), "tuple_to_power": g.tuple_to_power().elements.tolist(), "order": g.order().tolist(),
           "cosets": [c.elements.tolist() for c in g.cosets()]}
    if with_minpolys:
        out["minpolys"] = g.minpolys().tolist()
    return out


def main():
    out = {}
    for m in (2, 3, 4, 5, 6, 8):
        rs = np.random.RandomState(m)
        q = 2 ** m
        a, b = rs.randint(0, q, 40), rs.randint(0, q, 40)
        case = {"prim_poly": int(GF(1, m).prim_poly),
                "sets": [methods(x, m, m <= 4) for x in (np.arange(q), np.arange(1, q), rs.randint(0, q, 12))],
                "exponents": list(range(min(2 * (q - 1), 62) + 1)),
                "a": a.tolist(), "b": b.tolist(), "sum": (GF(a, m) + GF(b, m)).elements.tolist()}
        if m <= 4:
            case["product"] = (GF(a, m) * GF(b, m)).elements.tolist()
        case["power_to_tuple"] = GF(np.array(case["exponents"]), m).power_to_tuple().elements.tolist()
        out[str(m)] = case
        print("m = %d: %d cosets of the whole field" % (m, len(case["sets"][0]["cosets"])))
    path = os.path.join(HERE, "gfields.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print("wrote %s (%.1f kB)" % (path, os.path.getsize(path) / 1e3))


if __name__ == "__main__":
    main()
