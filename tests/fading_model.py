"""Plain NumPy model of the Doppler-fading multipath channel (csrc/fading.hip; the definitions are in include/commpy_amd.h, "Doppler-
fading multipath channel").  Built on rng_model.py; no GPU, no engine import.

Shared by tests/test_fading_host.py (which pins the model on exact rational arithmetic, on brute-force loops and on the statistics of
Clarke's model) and tests/test_fading_gpu.py (which holds the kernels to it).

Draws.  Path p = (((first_row + b) nr + r) nt + t) L + l; sinusoid s < Ns of path p uses counter p (Ns + 1) + s, the line of sight
counter p (Ns + 1) + Ns, all modulo 2^64.  u_a = u01(w0, w1), u_b = u01(w2, w3); nu = fd cos(2 pi u_a), phi = u_b; for the line of sight
nu = fd_los.  ``params`` evaluates the cosine as rng_model.sincos2pi does (exact quadrant reduction, np.longdouble, rounded once: within
0.51 ulp) and multiplies by fd in float64, the kernel's one multiply.

Gains.  From GIVEN float64 (nu, phi) and an integer tau the phase psi = nu tau + phi is reduced without the kernel's rounding:
``reduced_phase_exact`` does it in rational arithmetic (fractions.Fraction), ``reduced_phase`` for whole arrays: nu tau = p + e exactly
(Dekker's two-product in float64), p - rint(p) is exact, and the three small terms are added in np.longdouble, so that
|rho - rho_exact| <= 2^-62 where longdouble has a 64-bit significand (x86); tests/test_fading_host.py compares the two.  Sine and cosine
of 2 pi rho are then evaluated in np.longdouble on [0, pi/4] after the exact quadrant reduction and rounded to float64 once.  The sum
over s is the kernel's: plain float64 adds from +0 in ascending s; G = a_l S; where kf > 0 the line of sight is added as
c_l cos + G in np.longdouble, rounded once (the kernel's fma rounds once too).

The bound of the gains (``gain_bound``), per component, against the model evaluated on the DEVICE's own (nu, phi):
    a_l Ns (2 pi 2^-53 (fd tau + 1) + c 2^-52) + a_l (Ns^2 + Ns) 2^-53
      the kernel's psi = fma(nu, tau, phi) is rounded once: |d psi| <= 2^-53 |psi| <= 2^-53 (fd tau + 1), a phase error of 2 pi d psi per
      sinusoid; c 2^-52 is the device sincospi's distance from the model's value (measured, below); the Ns adds of partial sums of
      magnitude <= Ns round by at most Ns 2^-53 each and the product a_l S once.
    where kf > 0:  + c_l (2 pi 2^-53 (|fd_los| tau + 1) + c 2^-52) + (a_l Ns + c_l) 2^-52
      the same single-sinusoid term times c_l, and -- added to the issue's bound -- the final rounding of the fma in the kernel and of
      the sum in the model, each at most 2^-53 of a magnitude <= a_l Ns + c_l.
    + 2 pi 2^-62 (a_l Ns + c_l) for ``reduced_phase``.

The measured constants.  Neither cospi nor sincospi has a published accuracy table, so, as AWGN_ULP in rng_model.py:
``FADING_ULP_MEASURED`` is the largest |nu_device - nu_model| in relative ulps (2^-52 |nu_model|) over B nr nt L (Ns + 1) = 2^21 draws of
every (seed, stream) of rng_model.KEYS at fd = 0.5 (a power of two: the multiply rounds nothing); ``FADING_SINCOS_ULP_MEASURED`` is the
largest |G_device - G_model| / 2^-52 per component over the same keys at Ns = 1, pdp = 1, tau = 0, where G is the bare (cos, sin) of
2 pi phi.  The tests assert twice the measured value (a maximum over 2 10^6 samples underestimates the true one), under a cap of 16.
"""
from fractions import Fraction

import numpy as np

import rng_model as R

FADING_ULP_MEASURED = 1.00           # MI355X, ROCm 7.2: 1.000 over each of the four KEYS (the device's cospi is at most one float64 spacing off)
FADING_ULP = 2.0 * FADING_ULP_MEASURED
FADING_SINCOS_ULP_MEASURED = 0.50    # MI355X, ROCm 7.2: 0.500 over each of the four KEYS (one spacing of a value in [1/2, 1))
FADING_SINCOS_ULP = 2.0 * FADING_SINCOS_ULP_MEASURED
FADING_ULP_CAP = 16.0

L_ = np.longdouble


# ---- draws --------------------------------------------------------------------------------------------------------------------------
def draws(B, nr, nt, L, Ns, seed, stream, first_row=0):
    """(m_a, m_b): the 53-bit integers behind u_a and u_b of every counter, uint64 [B, nr, nt, L, Ns + 1]."""
    P = nr * nt * L
    with np.errstate(over="ignore"):
        path = R.counters((int(first_row) * P) % 2 ** 64, B * P)
        ctr = path[:, None] * np.uint64(Ns + 1) + np.arange(Ns + 1, dtype=np.uint64)[None, :]
    w = R.philox(ctr.reshape(-1), stream, seed)
    shape = (B, nr, nt, L, Ns + 1)
    return R.u01(w[0], w[1])[0].reshape(shape), R.u01(w[2], w[3])[0].reshape(shape)


def params(B, nr, nt, L, Ns, fd, fd_los, seed, stream, first_row=0):
    """float64 [B, nr, nt, L, Ns + 1, 2]: (nu, phi) of every sinusoid, the line of sight last."""
    m_a, m_b = draws(B, nr, nt, L, Ns, seed, stream, first_row)
    _, cs = R.sincos2pi(m_a.astype(np.float64) * (1.0 / R.TWO53))
    out = np.empty(m_a.shape + (2,), np.float64)
    out[..., 0] = float(fd) * cs
    out[..., Ns, 0] = float(fd_los)
    out[..., 1] = m_b.astype(np.float64) * (1.0 / R.TWO53)
    return out


def tap_scales(pdp, kf, Ns):
    """(a_l, c_l, los): a_l = sqrt(pdp / ((1 + kf) Ns)), c_l = sqrt(pdp kf / (1 + kf)), los = where the line of sight is added."""
    pdp = np.asarray(pdp, np.float64)
    kf = np.zeros_like(pdp) if kf is None else np.broadcast_to(np.asarray(kf, np.float64), pdp.shape)
    a = np.sqrt(pdp / ((1.0 + kf) * float(Ns)))
    c = np.sqrt(pdp * kf / (1.0 + kf))
    return a, c, (kf > 0) & (pdp > 0)


# ---- phases -------------------------------------------------------------------------------------------------------------------------
def reduced_phase_exact(nu, phi, tau):
    """rho = psi - round(psi) of psi = nu tau + phi, as a Fraction in [-1/2, 1/2]: no rounding anywhere."""
    psi = Fraction(float(nu)) * int(tau) + Fraction(float(phi))
    return psi - round(psi)


def _split(a):
    c = 134217729.0 * a                                          # 2^27 + 1 (Veltkamp)
    hi = c - (c - a)
    return hi, a - hi


def two_prod(a, b):
    """(p, e) with p = fl(a b) and p + e = a b exactly (Dekker; no overflow, e not below the subnormals)."""
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def reduced_phase(nu, phi, tau):
    """np.longdouble rho with |rho - reduced_phase_exact| <= 2^-62 (one of the two nearest integers is removed), arrays broadcast."""
    nu, phi, tau = np.broadcast_arrays(np.asarray(nu, np.float64), np.asarray(phi, np.float64), np.asarray(tau, np.float64))
    p, e = two_prod(nu, tau)
    s = ((p - np.rint(p)).astype(L_) + phi.astype(L_)) + e.astype(L_)
    return s - np.rint(s)


def phasor(rho):
    """(cos 2 pi rho, sin 2 pi rho) as float64 for np.longdouble rho in [-1/2, 1/2]: quadrant reduction, then [0, pi/4], rounded once."""
    a = 2 * np.asarray(rho, L_)
    k = np.rint(2 * a)
    r = a - k / 2                                                # exact; [-1/4, 1/4]
    t = R.PI_L * np.abs(r)
    s, c = np.copysign(np.sin(t), r).astype(np.float64), np.cos(t).astype(np.float64)
    q = np.mod(k.astype(np.int64), 4)
    return np.choose(q, [c, 0.0 - s, 0.0 - c, s]), np.choose(q, [s, c, 0.0 - s, 0.0 - c])


# ---- gains --------------------------------------------------------------------------------------------------------------------------
def gains_from_params(prm, pdp, kf, taus):
    """G complex128 [B, len(taus), nr, nt, L] from (nu, phi) = prm [B, nr, nt, L, Ns + 1, 2] at the integer times ``taus``."""
    prm = np.asarray(prm, np.float64)
    Ns = prm.shape[4] - 1
    a, c, los = tap_scales(pdp, kf, Ns)
    tau = np.asarray(taus, np.float64).reshape(1, -1, 1, 1, 1)
    nu, phi = prm[:, None, ..., 0], prm[:, None, ..., 1]          # [B, 1, nr, nt, L, Ns + 1]
    shape = (prm.shape[0], tau.size) + prm.shape[1:4]
    sre, sim = np.zeros(shape), np.zeros(shape)
    for s in range(Ns):
        cs, sn = phasor(reduced_phase(nu[..., s], phi[..., s], tau))
        sre, sim = sre + cs, sim + sn
    gre, gim = a * sre, a * sim
    if np.any(los):
        cs, sn = phasor(reduced_phase(nu[..., Ns], phi[..., Ns], tau))
        gre = np.where(los, (c.astype(L_) * cs + gre).astype(np.float64), gre)
        gim = np.where(los, (c.astype(L_) * sn + gim).astype(np.float64), gim)
    zero = (a == 0) & ~los
    return np.where(zero, 0.0, gre) + 1j * np.where(zero, 0.0, gim)


def block_times(t0, hold, nblk):
    return int(t0) + int(hold) * np.arange(int(nblk), dtype=np.int64)


def gains(B, nr, nt, pdp, fd, nblk, hold=1, t0=0, Ns=16, kf=None, fd_los=0.0, seed=0, stream=0, first_row=0):
    """The whole model: ``fading_gains_batch`` with the model's own (nu, phi)."""
    prm = params(B, nr, nt, len(pdp), Ns, fd, fd_los, seed, stream, first_row)
    return gains_from_params(prm, pdp, kf, block_times(t0, hold, nblk))


def gain_bound(pdp, kf, Ns, fd, fd_los, taus, c_ulp):
    """[len(taus), L]: the bound of the module docstring per component of G."""
    a, c, los = tap_scales(pdp, kf, Ns)
    tau = np.asarray(taus, np.float64)[:, None]
    one = lambda f: 2 * np.pi * 2.0 ** -53 * (abs(f) * tau + 1) + c_ulp * 2.0 ** -52
    b = a * Ns * one(fd) + a * (Ns * Ns + Ns) * 2.0 ** -53 + 2 * np.pi * 2.0 ** -62 * (a * Ns + c)
    return b + np.where(los, c * one(fd_los) + (a * Ns + c) * 2.0 ** -52, 0.0)


# ---- the time-varying convolution -----------------------------------------------------------------------------------------------------
def convolve(x, G, hold):
    """y[b][r][m] = sum_t sum_l G[b][m // hold][r][t][l] x[b][t][m - l]: per output a plain sum with its block's taps.  x [B, nt, n],
    G [B, nblk, nr, nt, L] or [nblk, nr, nt, L] -> [B, nr, n + L - 1]."""
    x, G = np.asarray(x, np.complex128), np.asarray(G, np.complex128)
    B, nt, n = x.shape
    G5 = np.broadcast_to(G, (B,) + G.shape[-4:])
    nr, L = G5.shape[2], G5.shape[4]
    y = np.zeros((B, nr, n + L - 1), np.complex128)
    blk = np.arange(n + L - 1) // int(hold)
    for l in range(L):
        taps = G5[..., l][:, blk[l:l + n]]                       # [B, n, nr, nt]
        y[:, :, l:l + n] += np.einsum("bmrt,btm->brm", taps, x)
    return y


def convolve_bound(x, G, hold):
    """[B, nr, n + L - 1]: 2 (nt L + 2) 2^-53 sqrt(2) sum_{t, l} |G[b][m // hold][r]| max|x[b]| (two float64 sums of nt L products of
    the same operands, as the static channel's mp_bound)."""
    x, G = np.asarray(x), np.asarray(G)
    B, nt, n = x.shape
    G5 = np.broadcast_to(G, (B,) + G.shape[-4:])
    L = G5.shape[4]
    blk = np.arange(n + L - 1) // int(hold)
    sg = np.sum(np.abs(G5), axis=(3, 4))[:, blk, :]              # [B, lout, nr]
    return 2 * (nt * L + 2) * 2.0 ** -53 * np.sqrt(2) * np.transpose(sg, (0, 2, 1)) * np.max(np.abs(x), axis=(1, 2))[:, None, None]


def conv_kernel(B, nt, nr, n, L, hold):
    """The kernel cpx_fading_convolve launches for this shape (csrc/fading.hip, launch_convolve)."""
    lout = n + L - 1
    sets = min((1024 - 2 + hold) // hold + 1, -(-lout // hold))
    if 2 * lout >= 1024 and sets * nr * nt * L <= 2048:
        return "fading_tiled_kernel<%d>" % (4 if nr >= 3 else nr)
    return "fading_direct_kernel"


# ---- statistics ---------------------------------------------------------------------------------------------------------------------
STAT_DELTAS = (0, 1, 5, 10, 20, 38, 50, 100, 200)


def autocorrelation(G0, Gd, pdp):
    """Mean over the paths of G(tau0 + d) conj(G(tau0)) / pdp[l]; G0, Gd [..., L]."""
    return np.mean(Gd * np.conj(G0) / np.asarray(pdp, np.float64))
