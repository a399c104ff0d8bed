"""Pseudo-noise and Zadoff-Chu sequences (the reference's ``commpy/sequences.py``), host side.

Both generators are O(length) NumPy and sit outside any hot path, like ``Trellis`` and the LDPC design files: their output
feeds ``modulate`` or serves as the taps of a correlator (``filters.matched_filter``).
"""
import numpy as np

__all__ = ['pnsequence', 'zcsequence']


def pnsequence(pn_order, pn_seed, pn_mask, seq_length):
    """``seq_length`` outputs (int8) of the LFSR with ``pn_order`` delay elements (sequences.py:21).  ``pn_seed`` and ``pn_mask``
    are iterables of 0/1 of that length (string, list, tuple, array); ``seed[-1]`` is the first output and the feedback bit
    ``sum(register & mask) % 2`` enters at position 0."""
    for name, value in (('pn_seed', pn_seed), ('pn_mask', pn_mask)):
        if len(value) != pn_order:
            raise ValueError('%s has not the same length as pn_order' % name)
    reg = [int(c) for c in pn_seed]
    taps = [i for i, c in enumerate(pn_mask) if int(c)]
    out = np.empty(seq_length, np.int8)
    # the register as a growing history: hist[pn_order - 1 + i - j] is element j at step i, so nothing is shifted
    hist = reg[::-1] + [0] * seq_length
    top = pn_order - 1
    for i in range(seq_length):
        out[i] = hist[i]
        bit = 0
        for j in taps:
            bit ^= hist[top + i - j]
        hist[top + i + 1] = bit & 1
    return out


def zcsequence(u, seq_length, q=0):
    """Zadoff-Chu sequence of root ``u``, length ``seq_length`` and cyclic shift ``q`` (sequences.py:77): complex128
    ``exp(-1j pi u n (n + cf + 2 q) / seq_length)``, cf = seq_length % 2, the phase evaluated in that order."""
    for value in (u, seq_length, q):
        if float(value) != int(float(value)) if np.isfinite(value) else True:
            raise ValueError('%r is not an integer' % (value,))
    if not 0 < u < seq_length:
        raise ValueError('the root u = %d must lie in 1 .. seq_length - 1 = %d' % (u, seq_length - 1))
    u, seq_length = int(u), int(seq_length)
    if np.gcd(u, seq_length) != 1:
        raise ValueError('u = %d and seq_length = %d have a common divisor' % (u, seq_length))
    n = np.arange(seq_length)
    return np.exp(-1j * np.pi * u * n * (n + seq_length % 2 + 2. * q) / seq_length)
