#!/usr/bin/env python3
"""CPU baseline of the reference's best_first_detector (commpy/modulation.py:422-565): 4x4 16-QAM, stack sizes (1, 3, 5),
llr_max 500, the vectors of benchmarks/bench_mimo.py's best_first workload (noise 0.5, one H per vector), one process, one
vector at a time.  Needs the reference checkout (COMMPY_REFERENCE), so it runs where the goldens are made, not on the GPU
machine.  One JSON line.
    python benchmarks/ref_best_first_cpu.py [--vectors 200]"""
import argparse
import json
import os
import sys
import time
import warnings

sys.path.insert(0, os.environ.get("COMMPY_REFERENCE", "/root/reference"))
warnings.simplefilter("ignore")

import numpy as np  # noqa: E402
from commpy.modulation import QAMModem, best_first_detector  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vectors", type=int, default=200)
    a = ap.parse_args()
    rs = np.random.RandomState(11)
    md = QAMModem(16)
    dem = lambda s: md.demodulate(s, 'hard')  # noqa: E731
    B = a.vectors
    h = (rs.randn(B, 4, 4) + 1j * rs.randn(B, 4, 4)) / np.sqrt(2)
    x = md.constellation[rs.randint(0, 16, (B, 4))]
    y = np.einsum('bij,bj->bi', h, x) + 0.5 * (rs.randn(B, 4) + 1j * rs.randn(B, 4)) / np.sqrt(2)
    best_first_detector(y[0], h[0], md.constellation, (1, 3, 5), 0.25, dem, 500)      # warm-up
    t = time.perf_counter()
    for b in range(B):
        best_first_detector(y[b], h[b], md.constellation, (1, 3, 5), 0.25, dem, 500)
    s = time.perf_counter() - t
    print(json.dumps({"kernel": "reference best_first_detector (CPU)", "workload": "4x4 16-QAM stacks (1,3,5) llr_max 500",
                      "vectors": B, "seconds": s, "ms_per_vector": s * 1e3 / B, "value": B / s, "unit": "vectors/s",
                      "cores": 1, "numpy": np.__version__}))


if __name__ == "__main__":
    main()
