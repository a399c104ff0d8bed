"""What tests/golden/make_golden_waveform.py and the waveform tests share: the seeded inputs of the frequency-offset goldens
(stored as outputs only) and the stride at which a long output is kept."""
import numpy as np

FO_STRIDE = 61


def fo_input(i, n):
    """Complex (even i) or real (odd i) waveform of case i."""
    rs = np.random.RandomState(2026 + i)
    return rs.randn(n) + 1j * rs.randn(n) if i % 2 == 0 else rs.randn(n)
