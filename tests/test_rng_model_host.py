"""tests/rng_model.py itself, and through it the contract of the counter-based random stages (csrc/cpx_rng.h): the published
Philox4x32-10 known-answer vectors, the bit layout of every derived draw restated with Python integers, Box-Muller against mpmath
at 50 digits, and the distribution and independence of what the contract generates.  No GPU: tests/test_rng_gpu.py holds the
kernels to this model, so the statistics live here and the GPU tests are equalities and an ulp bound."""
import math
from fractions import Fraction

import mpmath
import numpy as np
import pytest
from scipy.special import erfc, ndtr

import rng_model as R

M32 = 0xFFFFFFFF

# Random123's kat_vectors for philox4x32 with 10 rounds: (c0 c1 c2 c3), (k0 k1) -> four words
KNOWN_ANSWERS = (
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((M32, M32, M32, M32), (M32, M32), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
)


def _words(i, stream, seed):
    """Philox words of (index, stream id, seed) through the known-answer form: the low-word-first split written out."""
    return R.philox_words((i & M32, i >> 32, stream & M32, stream >> 32), (seed & M32, seed >> 32))


def _m(hi, lo):
    return ((hi >> 5) << 26 | lo >> 6) + 1


# ---- Philox and the integer draws -----------------------------------------------------------------------------------------------

def test_philox_known_answer_vectors():
    for c, k, want in KNOWN_ANSWERS:
        assert R.philox_words(c, k) == want, (c, k)


def test_philox_broadcasts_and_splits_low_word_first():
    idx = np.array([0, 1, 2 ** 32, 2 ** 33 + 5, 2 ** 64 - 1], dtype=np.uint64)
    for seed, stream in R.KEYS:
        got = R.philox(idx, stream, seed)
        for j, i in enumerate(int(v) for v in idx):
            assert tuple(int(w[j]) for w in got) == _words(i, stream, seed)
    # every high word matters: dropping the one of the index, the stream id or the seed would make these pairs equal
    base = R.philox_words((1, 0, 2, 0), (3, 0))
    assert len({base, R.philox_words((1, 1, 2, 0), (3, 0)), R.philox_words((1, 0, 2, 1), (3, 0)), R.philox_words((1, 0, 2, 0), (3, 1))}) == 4


def test_u01_end_points_and_bit_ranges():
    m, u = R.u01(0, 0)
    assert int(m) == 1 and float(u) == 2.0 ** -53
    m, u = R.u01(M32, M32)
    assert int(m) == 2 ** 53 and float(u) == 1.0
    for b in range(32):                                           # hi: bits 5..31 -> bits 26..52 of m - 1; lo: bits 6..31 -> bits 0..25
        assert int(R.u01(1 << b, 0)[0]) - 1 == ((1 << (b + 21)) if b >= 5 else 0)
        assert int(R.u01(0, 1 << b)[0]) - 1 == ((1 << (b - 6)) if b >= 6 else 0)
    rs = np.random.RandomState(1)
    hi, lo = rs.randint(0, 2 ** 32, 1000, dtype=np.uint64), rs.randint(0, 2 ** 32, 1000, dtype=np.uint64)
    m, u = R.u01(hi, lo)
    assert [int(v) for v in m] == [_m(int(h), int(l)) for h, l in zip(hi, lo)]
    assert all(Fraction(float(x)) == Fraction(int(v), 2 ** 53) for x, v in zip(u, m))


def test_message_bits_window():
    for seed, stream in R.KEYS:
        n = 16 * 3 + 5                                            # a ragged last counter
        want = [(_words(p // 16, stream, seed)[0] >> (p % 16)) & 1 for p in range(n)]
        got = R.message_bits(n, seed, stream)
        assert got.dtype == np.uint8 and got.tolist() == want
        assert R.message_bits(1, seed, stream).tolist() == want[:1]


def test_binary_draws_layout_and_threshold():
    for seed, stream in R.KEYS:
        n = 9
        want = []
        for p in range(n):
            w = _words(p // 2, stream, seed)
            want.append(_m(w[0], w[1]) if p % 2 == 0 else _m(w[2], w[3]))
        assert [int(v) for v in R.binary_draws(n, seed, stream)] == want
        for p in (0.0, 0.05, 0.5, 1.0, float(np.nextafter(1.0, 0.0)), (want[3] - 1) / 2.0 ** 53,
                  float(np.nextafter((want[3] - 1) / 2.0 ** 53, 0.0))):
            assert R.binary_hits(n, p, seed, stream).tolist() == [Fraction(m - 1, 2 ** 53) <= Fraction(p) for m in want], p
    assert R.binary_hits(1000, 1.0, 7, 1).all()
    assert R.binary_hits(1000, 0.0, 7, 1).sum() == 0             # a draw of exactly 0 has probability 2^-53


def test_counters_of_awgn_and_the_mimo_channel():
    first = 2 ** 33 + 5
    x = np.random.RandomState(2).randn(40) + 1j * np.random.RandomState(3).randn(40)
    whole = R.awgn(x, 2.0, 0.5, 7, 1)
    assert np.array_equal(R.awgn(x[11:], 2.0, 0.5, 7, 1, first=11), whole[11:])
    n_re, n_im = R.gauss(R.counters(0, 40), 7, 1)
    assert np.array_equal(whole.real, x.real + 2.0 * n_re) and np.array_equal(whole.imag, x.imag + 0.5 * n_im)   # powers of two
    assert np.array_equal(R.awgn(x, 0.0, 0.5, 7, 1).real, x.real)
    V, nr, nt = 7, 2, 3
    G = R.mimo_fading(first, V, nr, nt, 9, 2 ** 32 + 5)
    assert G.shape == (V, nr, nt)
    assert np.array_equal(G.reshape(-1), R.noise_terms(V * nr * nt, math.sqrt(0.5), math.sqrt(0.5), 9, 2 ** 32 + 5, first * nr * nt))
    N = R.mimo_noise(first, V, nr, 9, 4, 0.3)
    assert np.array_equal(N.reshape(-1), R.noise_terms(V * nr, 0.3, 0.3, 9, 4, first * nr))
    assert not np.array_equal(G, R.mimo_fading(5, V, nr, nt, 9, 2 ** 32 + 5))
    # the counter is taken modulo 2^64
    assert np.array_equal(R.mimo_noise(2 ** 63 + 1, 2, 2, 1, 1), R.noise_terms(4, 1.0, 1.0, 1, 1, 2).reshape(2, 2))
    assert R.counters(2 ** 64 - 1, 3).tolist() == [2 ** 64 - 1, 0, 1]


# ---- Box-Muller ---------------------------------------------------------------------------------------------------------------

def test_exact_quadrants_and_end_points():
    q = 2 ** 51
    sn, cs = R.sincos2pi(np.array([q, 2 * q, 3 * q, 4 * q]) / 2.0 ** 53)
    assert sn.tolist() == [1.0, 0.0, -1.0, 0.0] and cs.tolist() == [0.0, -1.0, 0.0, 1.0]
    rad, cs, sn = R.box_muller([1, 2 ** 53], [4 * q, 4 * q])
    assert abs(rad[0] ** 2 - 106 * math.log(2.0)) < 1e-13 and rad[1] == 0.0   # the largest |n| the contract can draw: 8.57 sigma
    # next to the crossings the small component is 2 pi d 2^-53 to the last bit or so, not the difference of two roundings
    sn, cs = R.sincos2pi(np.array([2 * q - 1, 2 * q + 1, q - 1, q + 1, 4 * q - 1, 1]) / 2.0 ** 53)
    tiny = 2.0 * math.pi * 2.0 ** -53
    assert np.all(np.abs(np.abs(np.array([sn[0], sn[1], cs[2], cs[3], sn[4], sn[5]])) / tiny - 1.0) <= 2.0 ** -51)
    assert sn[0] > 0 > sn[1] and cs[2] > 0 > cs[3] and sn[4] < 0 < sn[5]


@pytest.fixture(scope="module")
def stream_2_21():
    return R.gauss_uniforms(R.counters(0, 1 << 21), 7, 2)


def test_gauss_against_mpmath(stream_2_21):
    """About 2000 draws of the 2^21-draw stream (seed 7, stream 2) at 50 digits: the first 1900, the smallest u1 (the far tail), the
    u1 closest to 1 and the 16 u2 closest to each quadrant boundary; and the contract's own extremes."""
    m1, m2 = (v.astype(np.int64) for v in stream_2_21)            # m <= 2^53
    pick = set(range(1900)) | {int(np.argmin(m1)), int(np.argmax(m1))}
    for b in range(5):
        pick |= set(int(i) for i in np.argsort(np.abs(m2 - b * 2 ** 51))[:16])
    pick = sorted(pick)
    a1, a2 = [int(m1[i]) for i in pick], [int(m2[i]) for i in pick]
    for e1 in (1, 2, 2 ** 53 - 1, 2 ** 52):
        for e2 in (1, 2 ** 51 - 1, 2 ** 51 + 1, 2 ** 52 - 1, 2 ** 52 + 1, 3 * 2 ** 51 - 1, 3 * 2 ** 51 + 1, 2 ** 53 - 1, 12345):
            a1.append(e1)
            a2.append(e2)
    rad, cs, sn = R.box_muller(a1, a2)
    got = np.stack([rad * cs, rad * sn], axis=1)
    worst = 0.0
    with mpmath.workdps(50):
        for j, (i1, i2) in enumerate(zip(a1, a2)):
            r = mpmath.sqrt(-2 * mpmath.log(mpmath.mpf(i1) / 2 ** 53))
            ang = mpmath.mpf(i2) / 2 ** 52
            for want, g in ((r * mpmath.cospi(ang), got[j, 0]), (r * mpmath.sinpi(ang), got[j, 1])):
                assert want != 0
                ulp = float(np.spacing(abs(float(want))))
                worst = max(worst, float(abs(mpmath.mpf(float(g)) - want) / ulp))
    print("model vs mpmath over %d draws: max %.3f ulp" % (len(a1), worst))
    assert len(a1) >= 2000 and worst <= 2.0
    far = int(np.argmin(m1))
    print("far tail of the stream: u1 = %d 2^-53, rad = %.4f" % (m1[far], R.box_muller([m1[far]], [1])[0][0]))


# ---- the distribution the contract generates -----------------------------------------------------------------------------------

def test_normal_tails_and_ks():
    n_re, n_im = R.gauss(R.counters(0, 1 << 22), 7, 2)
    z = np.concatenate([n_re, n_im])
    N = z.size
    assert N == 1 << 23
    a = np.abs(z)
    for k in (1.0, 2.0, 3.0, 4.0, 4.5):
        want = N * float(erfc(k / math.sqrt(2.0)))
        got = int(np.count_nonzero(a > k))
        score = (got - want) / math.sqrt(want)
        print("beyond %.1f sigma: %d, expected %.1f, z = %+.2f" % (k, got, want, score))
        assert abs(score) <= 5.0, k
    z.sort()
    cdf = ndtr(z)
    i = np.arange(1, N + 1, dtype=np.float64)
    D = max(float(np.max(i / N - cdf)), float(np.max(cdf - (i - 1.0) / N)))
    print("Kolmogorov-Smirnov D sqrt(N) = %.3f" % (D * math.sqrt(N)))
    assert D * math.sqrt(N) < 1.95


def test_message_bit_balance_per_position():
    per = 1 << 20
    bits = R.message_bits(16 * per, 7, 1).reshape(per, 16)
    score = (bits.mean(axis=0) - 0.5) / (0.5 / math.sqrt(per))
    print("message bit balance, z per position:", np.round(score, 2).tolist())
    assert np.all(np.abs(score) <= 5.0)


@pytest.mark.parametrize("p", [0.05, 0.5])
def test_hit_rates(p):
    n = 1 << 22
    rate = R.binary_hits(n, p, 3, 1).mean()
    score = (rate - p) / math.sqrt(p * (1 - p) / n)
    print("hit rate at p = %g: z = %+.2f" % (p, score))
    assert abs(score) <= 5.0


# ---- independence: what a dropped word of the counter, the stream id or the seed would break -----------------------------------------

def _normals(first, seed, stream, n=1 << 20):
    return np.concatenate(R.gauss(R.counters(first, n), seed, stream))


def _corr(a, b):
    return float(np.mean((a - a.mean()) * (b - b.mean())) / (a.std() * b.std()))


@pytest.mark.parametrize("name,a,b", [
    ("streams s, s + 1", (0, 7, 2), (0, 7, 3)),
    ("streams s, s + 2^32", (0, 7, 2), (0, 7, 2 + 2 ** 32)),
    ("seeds k, k + 2^32", (0, 7, 2), (0, 7 + 2 ** 32, 2)),
    ("counters i, i + 2^32", (0, 7, 2), (2 ** 32, 7, 2)),
])
def test_normals_are_uncorrelated_across(name, a, b):
    x, y = _normals(*a), _normals(*b)
    c = _corr(x, y)
    print("%s: correlation %+.2e, bound %.2e" % (name, c, 5.0 / math.sqrt(x.size)))
    assert abs(c) <= 5.0 / math.sqrt(x.size)


def test_message_bits_and_next_streams_noise_sign_are_uncorrelated():
    """A device link draws its message bits on stream s and its noise on s + 1 with one seed, at the same counters."""
    n = 1 << 20
    w = R.philox(R.counters(0, n), 4, 7)[0]
    n_re, n_im = R.gauss(R.counters(0, n), 7, 5)
    worst = 0.0
    for comp in (n_re, n_im):
        sign = np.where(comp > 0, 1.0, -1.0)
        for j in range(16):
            bit = ((w >> np.uint64(j)) & np.uint64(1)).astype(np.float64) * 2.0 - 1.0
            worst = max(worst, abs(_corr(bit, sign)))
    print("message bit vs noise sign: largest |correlation| %.2e, bound %.2e" % (worst, 5.0 / math.sqrt(n)))
    assert worst <= 5.0 / math.sqrt(n)
