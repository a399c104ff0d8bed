"""Plain NumPy model of the counter-based random stages of csrc/cpx_rng.h (philox4x32_10, u01, message_bits16, awgn_add) and of the
kernels that draw from them (random_bits_kernel, binary_channel_kernel, awgn_kernel in csrc/linksim.hip, mimo_channel_kernel in
csrc/mimo_channel.hip, link_front_kernel in csrc/demod.hip).  No GPU, no engine import.

Shared by tests/test_rng_model_host.py (which pins the model on the published Philox4x32-10 known-answer vectors, on mpmath and on
its own distribution) and tests/test_rng_gpu.py (which holds the kernels to it).

The contract modelled (include/commpy_amd.h, "Random streams"): every draw is a pure function of (seed, stream id, element index).

* ``philox``: Philox4x32-10 (Salmon et al., SC'11) on the counter ``(c0 c1 c2 c3) = (index lo, index hi, stream lo, stream hi)`` and
  the key ``(k0 k1) = (seed lo, seed hi)``: every 64-bit value is split low word first.  Ten rounds; the key is bumped by
  ``(9E3779B9, BB67AE85)`` after every round; multipliers ``D2511F53`` (on c0) and ``CD9E8D57`` (on c2).
* ``u01(hi, lo)``: the 53-bit integer ``m = ((hi >> 5) << 26 | lo >> 6) + 1`` in [1, 2^53], i.e. the top 27 bits of ``hi`` above the
  top 26 bits of ``lo``; the uniform is ``m 2^-53`` in (0, 1], exact in float64.
* message bits: bit j (LSB first) of the low 16 bits of word 0 at counter i is message bit ``16 i + j``.
* binary channels: two draws per counter, position ``2 i`` from words (0, 1), position ``2 i + 1`` from words (2, 3), each as
  ``u01(first, second)``.  A position is hit (flipped / erased) where ``(m - 1) 2^-53 <= p``: the [0, 1) draw of the reference's
  ``random(n) <= p``.
* Gaussian pair of counter i: ``u1 = u01(w0, w1)``, ``u2 = u01(w2, w3)``, ``rad = sqrt(-2 log u1)``,
  ``(n_re, n_im) = rad (cos 2 pi u2, sin 2 pi u2)``.  ``awgn`` adds ``(scale_re * rad) * cos`` and ``(scale_im * rad) * sin`` to the
  components of x, each product and the sum rounded to float64 in that order (the library is built without FMA contraction).

``sincos2pi`` reduces ``a = 2 u2`` in (0, 2] exactly: ``k = rint(2 a)``, ``r = a - k / 2`` in [-1/4, 1/4] is a multiple of 2^-52 and
exact in float64.  Sine and cosine of ``pi |r|`` are evaluated on [0, pi/4], where neither has a zero other than sin 0 = 0, and the
quadrant k permutes and negates them, so the relative error stays at the ulp level next to the zero crossings and u2 = 1/4, 1/2,
3/4, 1 give exact zeros and +-1.  ``rad``, the sine and the cosine are each evaluated in ``np.longdouble`` and rounded to float64 once
(where longdouble is wider than float64, as on x86: there each is within 0.51 ulp); the products are float64 operations in the
kernel's order.  tests/test_rng_model_host.py holds the result to 2 ulp of a 50-digit evaluation.

The AWGN bound.  The kernel's log, sqrt and sincospi are the HIP device library's; no accuracy table for them ships with the
toolkit, so the bound is measured as the contract of tests/test_rng_gpu.py lays down: ``AWGN_ULP_MEASURED`` is the largest
deviation between ``cpx_awgn_dev`` and ``awgn`` on zeros, in ulps of the noise term (relative: 2^-52 |term|), over the 2^21 + 5 draws of every (seed, stream)
of ``KEYS`` and both components; ``AWGN_ULP`` is twice that (a maximum over 2 10^6 samples underestimates the true maximum), and
``AWGN_ULP_CAP`` = 16 holds whatever was measured: more means another algorithm (a float32 intermediate is near 2^29 ulp).
The measurement uses the scales 2.0 and 0.5, which round nothing; with scales that are not powers of two (sqrt(1/2), 0.3) the same
runs gave at most 3.19, the product ``scale * rad`` rounding the kernel's and the model's slightly different ``rad`` apart.
"""
import numpy as np

M32 = np.uint64(0xFFFFFFFF)
PHILOX_M0, PHILOX_M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
PHILOX_W0, PHILOX_W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
TWO53 = 9007199254740992.0
ULP = 2.0 ** -52             # the relative ulp of the AWGN bound

# (seed, stream id) of the GPU comparisons: zero, small, a high word set in both, all ones
KEYS = ((0, 0), (7, 1), (2 ** 32 + 3, 2 ** 32 + 5), (2 ** 64 - 1, 2 ** 64 - 1))

AWGN_ULP_MEASURED = 2.84    # MI355X, ROCm 7.2: 2.839, 2.829, 2.840, 2.819 over the four KEYS (3 when counted in float64 spacings)
AWGN_ULP = 5.68             # twice the measured maximum
AWGN_ULP_CAP = 16.0


def _u64(v):
    """``v`` (Python ints up to 2^64 - 1, or an integer array) as a uint64 array."""
    if isinstance(v, np.ndarray):
        return v.astype(np.uint64, copy=False)
    return np.asarray(v, dtype=np.uint64)


def counters(first, n):
    """``first + 0 .. first + n - 1`` modulo 2^64 as uint64."""
    with np.errstate(over="ignore"):
        return _u64(int(first) % 2 ** 64) + np.arange(int(n), dtype=np.uint64)


def philox(ctr_lo, ctr_hi, key):
    """The four uint32 words (as uint64 arrays below 2^32) of Philox4x32-10 at counter (ctr_lo, ctr_hi) = (index, stream id) under
    ``key`` = seed.  The arguments broadcast against each other."""
    ctr_lo, ctr_hi, key = np.broadcast_arrays(_u64(ctr_lo), _u64(ctr_hi), _u64(key))
    c0, c1 = ctr_lo & M32, ctr_lo >> np.uint64(32)
    c2, c3 = ctr_hi & M32, ctr_hi >> np.uint64(32)
    k0, k1 = key & M32, key >> np.uint64(32)
    for _ in range(10):
        p0, p1 = PHILOX_M0 * c0, PHILOX_M1 * c2                  # 32 x 32 bits: below 2^64, no wrap
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + PHILOX_W0) & M32, (k1 + PHILOX_W1) & M32
    return c0, c1, c2, c3


def philox_words(c, k):
    """Known-answer form: counter words (c0, c1, c2, c3) and key words (k0, k1) -> the four output words as Python ints."""
    out = philox(c[0] | (c[1] << 32), c[2] | (c[3] << 32), k[0] | (k[1] << 32))
    return tuple(int(w) for w in out)


def u01(hi, lo):
    """(m, u): the 53-bit integer ``((hi >> 5) << 26 | lo >> 6) + 1`` in [1, 2^53] as uint64, and ``u = m 2^-53`` in (0, 1]."""
    hi, lo = _u64(hi), _u64(lo)
    m = (((hi >> np.uint64(5)) << np.uint64(26)) | (lo >> np.uint64(6))) + np.uint64(1)
    return m, m.astype(np.float64) * (1.0 / TWO53)


def message_bits(n, seed, stream):
    """The first ``n`` message bits of stream (seed, stream) as uint8: bit j of the low 16 bits of word 0 at counter i is bit 16 i + j."""
    w = philox(counters(0, (n + 15) // 16), stream, seed)[0]
    bits = (w[:, None] >> np.arange(16, dtype=np.uint64)[None, :]) & np.uint64(1)
    return bits.reshape(-1)[:n].astype(np.uint8)


def binary_draws(n, seed, stream):
    """The integers m in [1, 2^53] of the first ``n`` positions of a binary channel on stream (seed, stream): position 2 i from words
    (0, 1) of counter i, position 2 i + 1 from words (2, 3).  The draw compared with p is ``(m - 1) 2^-53``."""
    w = philox(counters(0, (n + 1) // 2), stream, seed)
    m = np.stack([u01(w[0], w[1])[0], u01(w[2], w[3])[0]], axis=1)
    return m.reshape(-1)[:n]


def binary_hits(n, p, seed, stream):
    """Bool [n]: where the binary channels flip / erase, ``(m - 1) 2^-53 <= p``.  Exact: m - 1 < 2^53 and p 2^53 are float64 values."""
    return (binary_draws(n, seed, stream) - np.uint64(1)).astype(np.float64) <= float(p) * TWO53


# pi to the precision of np.longdouble (float64(pi) + the next 53 bits); on x86 that is the 64-bit significand of the x87 format
PI_L = np.longdouble(np.pi) + np.longdouble(1.2246467991473532e-16)


def sincos2pi(u2):
    """(sin 2 pi u2, cos 2 pi u2) for u2 = m 2^-53 in (0, 1], by the exact quadrant reduction of the module docstring."""
    a = 2.0 * np.asarray(u2, dtype=np.float64)
    k = np.rint(2.0 * a)
    r = a - 0.5 * k                                              # exact; [-1/4, 1/4]
    t = PI_L * np.abs(r).astype(np.longdouble)                   # extended precision, rounded once: see the module docstring
    s, c = np.copysign(np.sin(t).astype(np.float64), r), np.cos(t).astype(np.float64)
    q = k.astype(np.int64) & 3                                   # sin(pi r + q pi/2), cos(pi r + q pi/2); 0.0 - x: no negative zero
    sn = np.choose(q, [s, c, 0.0 - s, 0.0 - c])
    cs = np.choose(q, [c, 0.0 - s, 0.0 - c, s])
    return sn, cs


def box_muller(m1, m2):
    """(rad, cos, sin) of the Gaussian pair whose uniforms are ``m1 2^-53`` and ``m2 2^-53`` (integers in [1, 2^53])."""
    u1, u2 = _u64(m1).astype(np.float64) * (1.0 / TWO53), _u64(m2).astype(np.float64) * (1.0 / TWO53)
    rad = np.sqrt(-2.0 * np.log(u1.astype(np.longdouble))).astype(np.float64)
    sn, cs = sincos2pi(u2)
    return rad, cs, sn


def gauss_uniforms(idx, seed, stream):
    """(m1, m2): the two 53-bit integers behind the Gaussian pair of every counter in ``idx``."""
    w = philox(idx, stream, seed)
    return u01(w[0], w[1])[0], u01(w[2], w[3])[0]


def gauss(idx, seed, stream):
    """(n_re, n_im), two independent N(0, 1) arrays: Box-Muller on words (0, 1) and (2, 3) of the counters ``idx``."""
    rad, cs, sn = box_muller(*gauss_uniforms(idx, seed, stream))
    return rad * cs, rad * sn


def _awgn_at(x, idx, scale_re, scale_im, seed, stream):
    x = np.asarray(x, dtype=np.complex128)
    rad, cs, sn = box_muller(*gauss_uniforms(idx, seed, stream))
    rad, cs, sn = (v.reshape(x.shape) for v in (rad, cs, sn))
    out = np.empty(x.shape, np.complex128)
    out.real = x.real + (scale_re * rad) * cs
    out.imag = x.imag + (scale_im * rad) * sn
    return out


def awgn(x, scale_re, scale_im, seed, stream, first=0):
    """``cpx_awgn_dev``: element i of the flat complex array uses counter ``first + i``."""
    x = np.asarray(x, dtype=np.complex128)
    return _awgn_at(x, counters(first, x.size), scale_re, scale_im, seed, stream)


def noise_terms(n, scale_re, scale_im, seed, stream, first=0):
    """What ``awgn`` adds, as a complex array [n] (``awgn`` of zeros)."""
    return awgn(np.zeros(int(n), np.complex128), scale_re, scale_im, seed, stream, first)


def mimo_fading(first_vector, V, nr, nt, seed, stream):
    """G [V, nr, nt] of ``cpx_mimo_channel_run_dev``: entry (v, r, a) from counter ``(first_vector + v) nr nt + r nt + a`` (modulo 2^64),
    scale sqrt(1/2) per component."""
    with np.errstate(over="ignore"):
        base = counters(first_vector, V) * np.uint64(nr * nt)
        idx = base[:, None] + np.arange(nr * nt, dtype=np.uint64)[None, :]
    s = np.sqrt(0.5)
    return _awgn_at(np.zeros((V, nr, nt), np.complex128), idx.reshape(-1), s, s, seed, stream)


def mimo_noise(first_vector, V, nr, seed, stream, scale=1.0):
    """The noise [V, nr] that ``cpx_mimo_channel_run_dev`` adds to H x: entry (v, r) from counter ``(first_vector + v) nr + r``."""
    with np.errstate(over="ignore"):
        base = counters(first_vector, V) * np.uint64(nr)
        idx = base[:, None] + np.arange(nr, dtype=np.uint64)[None, :]
    return _awgn_at(np.zeros((V, nr), np.complex128), idx.reshape(-1), scale, scale, seed, stream)


# ---- comparing a kernel's output with the model -----------------------------------------------------------------------------------

def two_sum(a, b):
    """(s, e) with s = fl(a + b) and s + e = a + b exactly (Knuth)."""
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def awgn_excess(y, x, noise, ulps):
    """Per component of the complex arrays: ``|y - (x + noise)| - (ulps 2^-52 |noise| + 2^-53 |y|)``, the amount by which the kernel's
    ``y`` misses the bound around the model's ``noise`` term on the input ``x``; <= 0 everywhere means within the bound.  An ulp is
    taken relative, ``2^-52 |noise|``, so that the bound does not depend on where in its binade a scale puts the term.  The model's
    sum is taken exactly (two_sum), so the only rounding allowed for is the kernel's final add; where x is zero that add is exact
    and the term is dropped."""
    out = []
    for yc, xc, nc in ((y.real, x.real, noise.real), (y.imag, x.imag, noise.imag)):
        s, e = two_sum(xc, nc)
        err = np.abs((yc - s) - e)
        out.append(err - (ulps * ULP * np.abs(nc) + np.where(xc == 0.0, 0.0, np.abs(yc) * 2.0 ** -53)))
    return np.stack(out)


def ulp_deviation(y, noise):
    """Largest ``|y - noise| / (2^-52 |noise|)`` over both components: the measurement behind ``AWGN_ULP_MEASURED`` (x = 0: nothing
    but the kernel's log, sqrt and sincospi separates the two)."""
    dev = 0.0
    for yc, nc in ((y.real, noise.real), (y.imag, noise.imag)):
        nz = nc != 0.0
        assert np.array_equal(yc[~nz], nc[~nz])
        dev = max(dev, float(np.max(np.abs(yc[nz] - nc[nz]) / (ULP * np.abs(nc[nz])))))
    return dev
