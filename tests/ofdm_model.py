"""Extended-precision model of OFDM transmit / receive (csrc/ofdm.hip) and the error bounds its tests assert.

Nothing here is taken from the package.  The transforms are written a second time in numpy.longdouble (64-bit mantissa on
x86-64, eps = 2^-63), so the model's own error is about a thousandth of u = 2^-53 and a comparison against it measures the
kernel alone.  The bin map and the prefix rule come from test_ofdm_host.py, which states them once for the whole suite.

The bounds are first-order worst cases derived from the kernels' operation sequences (the derivations stand beside them); they
are not fitted to what the kernels return.  Two facts are used throughout, with u = 2^-53:
  * a double rounded from an exact constant c has |c^ - c| <= u |c|, and so has a complex constant rounded by components;
  * a complex product computed from four multiplications and two additions has |fl(a b) - a b| <= sqrt(5) u |a b| (Brent,
    Percival and Zimmermann 2007); with the additions contracted into FMAs the constant is 2, so sqrt(5) holds either way.
    A complex addition has |fl(a + b) - (a + b)| <= u |a + b|.
"""
import functools

import numpy as np
import pytest

from test_ofdm_host import bin_map, prefix_len

LD = np.longdouble
CLD = np.clongdouble
U = 2.0 ** -53
EPS_LD = float(np.finfo(LD).eps)
LD_OK = EPS_LD < 2.0 ** -60
requires_longdouble = pytest.mark.skipif(
    not LD_OK, reason="numpy.longdouble has eps = %.3g >= 2^-60 here: no extended precision to model against" % EPS_LD)

PI_LD = LD("3.141592653589793238462643383279502884")
SQRT5 = 5.0 ** 0.5
ROT = 1.0 + SQRT5         # one rounded unit-modulus constant (u) applied by one complex multiplication (sqrt(5) u)


# ---- twiddles and transforms ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=64)
def twiddles_ld(N):
    """W[k] = e^{-2 pi i k / N}, k = 0..N-1, clongdouble.  4k = q N + r with q the nearest quarter turn (integers, exact), so
    cos / sin see |pi r / (2 N)| <= pi / 4 and the quarter turns are exact swaps and signs."""
    k = np.arange(N, dtype=np.int64)
    q = (4 * k + N // 2) // N
    r = 4 * k - q * N
    ang = PI_LD * r.astype(LD) / LD(2 * N)
    c, s = np.cos(ang), np.sin(ang)
    q &= 3
    re = np.choose(q, [c, -s, -c, s])          # e^{+i angle}
    im = np.choose(q, [s, c, -s, -c])
    w = np.empty(N, CLD)
    w.real, w.imag = re, -im
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=64)
def twiddles_f64(N):
    """The plan's table: twiddles_ld rounded to double by components."""
    w = twiddles_ld(N).astype(np.complex128)
    w.setflags(write=False)
    return w


def _fft_rec(x):
    N = x.shape[-1]
    if N == 1:
        return x
    F = _fft_rec(np.stack([x[..., 0::2], x[..., 1::2]], axis=-2))          # both halves as one batch: log2 N levels of NumPy
    E, O = F[..., 0, :], F[..., 1, :] * twiddles_ld(N)[:N // 2]
    return np.concatenate([E + O, E - O], axis=-1)


def fft_ld(x, inverse=False):
    """DFT over the last axis, power-of-two length, in clongdouble: recursive radix-2, decimation in time.  The inverse is
    conj(fft(conj(x))) / N, the division exact."""
    x = np.asarray(x).astype(CLD)
    N = x.shape[-1]
    assert N >= 1 and N & (N - 1) == 0, N
    if inverse:
        return np.conj(_fft_rec(np.conj(x))) / LD(N)
    return _fft_rec(x)


def dft_ld(x, bins=None, inverse=False):
    """Direct DFT over the last axis for any length, in clongdouble, for all output bins or those listed: out[..., j] =
    sum_n x[..., n] W^{(bins[j] n) mod N} (inverse: conj(W), then / N).  Exact zeros among the inputs are skipped, so a sparse
    input costs its nonzeros; otherwise one NumPy step per output bin."""
    x = np.asarray(x).astype(CLD)
    N = x.shape[-1]
    bins = np.arange(N, dtype=np.int64) if bins is None else np.asarray(bins, dtype=np.int64)
    w = np.conj(twiddles_ld(N)) if inverse else twiddles_ld(N)
    out = np.zeros(x.shape[:-1] + (bins.size,), CLD)
    nz = np.flatnonzero(np.any(x.reshape(-1, N) != 0, axis=0)).astype(np.int64)
    if nz.size < bins.size:
        for n in nz:
            out += x[..., n:n + 1] * w[(bins * n) % N]
    else:
        n = np.arange(N, dtype=np.int64)
        for j, k in enumerate(bins):
            out[..., j] = np.sum(x * w[(k * n) % N], axis=-1)
    return out / LD(N) if inverse else out


def dft_f64_index_order(x, bins, inverse=False):
    """The float64 sum a plain implementation of ofdm_dft_kernel's order gives: acc = 0, then acc += x[n] * T[(k n) mod N] for
    n = 0, 1, .. N-1 with T the double table (conjugated for the inverse), then * (1 / N) for the inverse.  Vectorised over the
    leading axes and the bins, one NumPy step per input sample.  Not bit-exact to the kernel (the compiler may contract products
    into FMAs): it is the yardstick of the dense-input check, a walk of the same length over the same terms."""
    x = np.asarray(x, dtype=np.complex128)
    N = x.shape[-1]
    bins = np.asarray(bins, dtype=np.int64)
    T = np.conj(twiddles_f64(N)) if inverse else twiddles_f64(N)
    acc = np.zeros(x.shape[:-1] + (bins.size,), np.complex128)
    idx = np.zeros(bins.size, np.int64)
    for n in range(N):
        acc += x[..., n:n + 1] * T[idx]
        idx += bins
        idx[idx >= N] -= N
    return acc * (1.0 / N) if inverse else acc


# ---- the contract of ofdm_tx / ofdm_rx over those transforms -----------------------------------------------------------------------
def tx_bins(x, nfft):
    """x [B, nsym, nsc] -> F [B, nsym, nfft]: the frequency-domain symbol TX transforms (bin map, the second write wins)."""
    x = np.asarray(x)
    bins = bin_map(nfft, x.shape[-1])
    F = np.zeros(x.shape[:-1] + (nfft,), x.dtype)
    used = bins >= 0
    F[..., used] = x[..., bins[used]]
    return F


def rx_bin_of(nfft, nsc):
    """The FFT bin that output element sc of RX carries: the top nsc / 2 bins first, then bins 1 .. nsc / 2."""
    h = nsc // 2
    return np.concatenate([np.arange(nfft - h, nfft), np.arange(1, h + 1)]).astype(np.int64)


def _pow2(n):
    return n & (n - 1) == 0


def ref_tx_batch(x, nfft, cp, samples=None):
    """x [B, nsym, nsc] -> clongdouble [B, nsym * (P + nfft)] like model_tx_batch; with `samples` (indices into a symbol's nfft
    body samples) -> [B, nsym, len(samples)], those body samples alone and no prefix."""
    x = np.asarray(x, dtype=complex)
    B = x.shape[0]
    F = tx_bins(x, nfft)
    if samples is not None:
        return dft_ld(F, samples, inverse=True)
    t = fft_ld(F, inverse=True) if _pow2(nfft) else dft_ld(F, inverse=True)
    P = prefix_len(nfft, cp)
    return np.concatenate([t[:, :, nfft - P:], t], axis=-1).reshape(B, -1)


def rx_bodies(y, nfft, cp):
    """y [B, n] -> [B, n // (nfft + cp), nfft]: the samples RX transforms (past each block's prefix; the leftover dropped)."""
    y = np.asarray(y)
    B, n = y.shape
    S = nfft + cp
    nsym = n // S
    return y[:, :nsym * S].reshape(B, nsym, S)[:, :, cp:cp + nfft]


def ref_rx_batch(y, nfft, nsc, cp, bins=None):
    """y [B, n] -> clongdouble [B, n // (nfft + cp), nsc] like model_rx_batch; with `bins` (FFT bin indices) ->
    [B, nsym, len(bins)], those bins of each symbol's transform instead of the nsc used ones."""
    body = rx_bodies(np.asarray(y, dtype=complex), nfft, cp)
    bins = rx_bin_of(nfft, nsc) if bins is None else np.asarray(bins, dtype=np.int64)
    if _pow2(nfft) and nfft <= 8192:                       # the sizes of the fast kernel: all bins at once
        return fft_ld(body)[:, :, bins]
    return dft_ld(body, bins)


# ---- bounds, in units of u = 2^-53 ---------------------------------------------------------------------------------------------------
def fast_passes(nfft):
    """log2 of the radix of each pass of ofdm_fast_kernel<log2 nfft>: radix 8 (16 at 8192), the first pass taking what is left."""
    logn = nfft.bit_length() - 1
    assert 2 <= nfft <= 8192 and 1 << logn == nfft, nfft
    logr = 4 if logn == 13 else 3
    first = logn % logr or logr
    return [first] + [logr] * ((logn - first) // logr)


def fast_bound(nfft):
    """(a)  Per symbol, ||got - ref||_2 <= fast_bound(nfft) u ||ref||_2 over the whole transform, to first order in u.

    The kernel is a product of stages, each a unitary map times a scalar (a radix-2 level is sqrt(2) times a unitary map, a
    twiddle stage is a unitary diagonal), so a stage whose computed output is off by a relative 2-norm error e adds e to the
    relative error of the result, and the stages' errors add (Higham, Accuracy and Stability of Numerical Algorithms, thm 24.2,
    is this argument for radix 2).  The stages of a pass of radix 2^l (dft_regs, then the next pass's twiddles):
      * l radix-2 levels, each one complex addition or subtraction per output: u each, l u.
      * after the subtraction, a rotation by e^{-+2 pi i m / 16}.  m = 0 and m = 4 (a swap and a sign) are exact, and the last two
        levels of every dft_regs have no other: max(0, l - 2) levels rotate by a rounded constant (u) through one product
        (sqrt(5) u): (1 + sqrt(5)) u each.
      * every pass but the first multiplies by W^(step r): a table entry where r is a power of two, else the product of up to
        three entries (r = 7: w4 (w2 w1); r = 15: w8 (w4 (w2 w1))): three rounded constants and two products to form it,
        (3 + 2 sqrt(5)) u, and one product to apply it: (3 + 3 sqrt(5)) u.
    The 1 / N of TX is a power of two: exact.  The reference's own error (some 2^-63 log2 N) is three digits below.
    At 8192 (passes 2, 16, 16, 16) this is 13 + 6 (1 + sqrt(5)) + 3 (3 + 3 sqrt(5)) = 61.5, i.e. 4.7 log2 N."""
    passes = fast_passes(nfft)
    levels = sum(passes)
    rotating = sum(max(0, l - 2) for l in passes)
    return levels + rotating * ROT + (len(passes) - 1) * 3 * ROT


def fast_factors(nfft):
    """The largest number of rounded unit-modulus constants, each applied by one complex product, between an input of
    ofdm_fast_kernel and an output: per pass of radix 2^l, max(0, l - 2) rotations by W16 constants (see fast_bound), and per
    pass after the first three table entries and three products (two to form W^(step r), one to apply it).  15 at 8192."""
    passes = fast_passes(nfft)
    return sum(max(0, l - 2) for l in passes) + 3 * (len(passes) - 1)


def sparse_bound(m, factors, inexact_scale=False):
    """(b)  For an input with m nonzero elements, every output element has |got - ref| <= sparse_bound u sum|x|, first order.

    An output is sum_n x_n c_n with |c_n| = 1, c_n the product of `factors` constants at most.  A zero input stays an exact
    zero through every product, and adding it is exact.  So:
      * each nonzero term carries `factors` rounded constants (u each) through `factors` products (sqrt(5) u each):
        factors (1 + sqrt(5)) u |x_n|, summed over n: factors (1 + sqrt(5)) u sum|x|;
      * in whatever order the kernel adds, at most m - 1 additions have two nonzero operands; each is off by u times a
        partial sum, itself <= sum|x|: (m - 1) u sum|x|;
      * the 1 / N of TX is exact for a power of two; otherwise (ofdm_dft_kernel at other sizes) 1.0 / N is rounded (u) and
        applied by one real multiplication per component (u): 2 u more (`inexact_scale`).
    factors = 1 for ofdm_dft_kernel (one table twiddle per term), fast_factors(nfft) for ofdm_fast_kernel."""
    return factors * ROT + (m - 1) + (2 if inexact_scale else 0)


def dense_bound(N):
    """(c), first assertion: every output element of ofdm_dft_kernel has |got - ref| <= (N + 3) u sum|x|.

    sparse_bound with m = N and one factor: N - 1 additions and (1 + sqrt(5)) u per term, N + 2.24, rounded up to N + 3.  (For
    TX at an N that is no power of two the rounded 1 / N adds 2 u to the strict worst case, which this figure does not carry:
    reaching N + 3 already takes every rounding of the sum at its extreme with the same sign.  sparse_bound carries the term,
    and is the one asserted where a bound of this kind is tight.)  The bound grows with N while the error of a sum of N
    random terms grows with sqrt(N): at 65536 it only catches a gross error, which is why a second assertion
    (DENSE_RATIO_LIMIT) stands beside it."""
    return N + 3


# (c), second assertion: over the bins compared, ||got - ref||_2 <= 4 ||dft_f64_index_order - ref||_2.  Both are sums of the same
# N terms per bin in the same order, rounded at the same places but for FMA contraction, so over >= 64 bins the two error norms
# are random walks of equal length and their ratio is near 1; the factor 4 is room for the contraction and for the walk's spread
# (the relative spread of an error norm over 64 complex bins is about 1 / sqrt(128)).  The library is built with contraction off
# today, and the ratios measured are within 6 % of 1; the factor stays, for a build that contracts.
DENSE_RATIO_LIMIT = 4.0


def norm2(a):
    """2-norm over the last axis, in the precision of a."""
    a = np.asarray(a)
    return np.sqrt(np.sum(a.real ** 2 + a.imag ** 2, axis=-1))
