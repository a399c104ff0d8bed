"""The timing / carrier recovery model (tests/recovery_model.py) against independent truth, and the refusals of the Python layer and
the C-ABI; no GPU.

Bounds, with u = 2^-53 the unit roundoff of float64:
  * cubic interpolator on integer samples: the sums inside v3, v2 and v1 are small integers and therefore exact, so the longest path to
    the result is the constant S (1/6 rounded), the product with S, and three products and three sums of Horner's rule: 8 roundings.
    By the standard bound for Horner's rule with perturbed coefficients the result is within gamma_8 (|v3| mu^3 + |v2| mu^2 + |v1| mu +
    |x0|) of the exact value, gamma_k = k u / (1 - k u), v the exact coefficients.
  * linear interpolator on integer samples: x1 - x0 is exact, one product and one sum: gamma_2 (|x1 - x0| mu + |x0|).
  * unit_phasor: 2^-51 a part, as csrc/cpx_phasor.h and DESIGN 4.26 derive it (truncation < 2e-18, argument and 2 pi about 2^-53, Horner
    at most 2.6 * 2^-53); c^2 + s^2 is then within 2 * 2^-51 = 2^-50 of 1 to first order.
"""
import ctypes
from fractions import Fraction

import numpy as np
import pytest

import recovery_model as R
from commpy_amd import _lib, deviceops
from commpy_amd.modulation import PSKModem, QAMModem
from commpy_amd.recovery import RECOVERY_WANT, loop_gains, recovery_shapes, timing_recover_batch

U = 2.0 ** -53


def gamma(k):
    return Fraction(k) * Fraction(U) / (1 - Fraction(k) * Fraction(U))


# ---- interpolators --------------------------------------------------------------------------------------------------------------------
POLYS = [(1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1), (7, -3, 2, -1), (-5, 11, -4, 3), (1000, -999, 37, 13)]   # a0 .. a3
MUS = [Fraction(k, 64) for k in (0, 1, 21, 32, 43, 63)] + [Fraction(1, 2 ** 20), Fraction(2 ** 20 - 1, 2 ** 20)]


def poly(a, t):
    return sum(Fraction(c) * Fraction(t) ** i for i, c in enumerate(a))


@pytest.mark.parametrize("a", POLYS)
def test_cubic_reproduces_cubics(a):
    worst = Fraction(0)
    for base in (-4, 0, 9):
        xm, x0, x1, x2 = (poly(a, base + j) for j in (-1, 0, 1, 2))
        v3 = ((x2 - xm) + 3 * (x0 - x1)) / 6
        v2 = (x1 + xm) / 2 - x0
        v1 = ((6 * x1 - x2) - (3 * x0 + 2 * xm)) / 6
        for mu in MUS:
            exact = poly(a, base + mu)
            assert ((v3 * mu + v2) * mu + v1) * mu + x0 == exact           # the formula itself, in exact arithmetic
            got = R.farrow(*(np.float64(float(x)) for x in (xm, x0, x1, x2)), np.float64(float(mu)))
            bound = gamma(8) * (abs(v3) * mu ** 3 + abs(v2) * mu ** 2 + abs(v1) * mu + abs(x0))
            assert abs(Fraction(float(got)) - exact) <= bound, (a, base, mu)
            if bound:
                worst = max(worst, abs(Fraction(float(got)) - exact) / bound)
    print("cubic, coefficients %s: worst error / bound = %.3g" % (a, float(worst)))


@pytest.mark.parametrize("a", [p for p in POLYS if p[2] == 0 and p[3] == 0] + [(7, -3, 0, 0), (1000, -999, 0, 0)])
def test_linear_reproduces_lines(a):
    for base in (-4, 0, 9):
        x0, x1 = poly(a, base), poly(a, base + 1)
        for mu in MUS:
            exact = poly(a, base + mu)
            got = R.linear(np.float64(float(x0)), np.float64(float(x1)), np.float64(float(mu)))
            assert abs(Fraction(float(got)) - exact) <= gamma(2) * (abs(x1 - x0) * mu + abs(x0)), (a, base, mu)


def test_interpolate_reads_zero_outside_the_row():
    """Index -1 and index n_y read 0.0 and are used like any sample; ``inside`` says so."""
    y = np.array([[1.0 + 2.0j, 3.0 - 1.0j, -2.0 + 0.5j]])
    zr, zi, inside = R.interpolate(y.real.copy(), y.imag.copy(), np.array([0]), np.array([0.5]), True)
    assert not inside[0] and zr[0] == R.farrow(0.0, 1.0, 3.0, -2.0, 0.5) and zi[0] == R.farrow(0.0, 2.0, -1.0, 0.5, 0.5)
    zr, zi, inside = R.interpolate(y.real.copy(), y.imag.copy(), np.array([2]), np.array([0.25]), False)
    assert not inside[0] and zr[0] == -2.0 + 0.25 * 2.0 and zi[0] == 0.5 + 0.25 * -0.5
    assert R.interpolate(y.real.copy(), y.imag.copy(), np.array([1]), np.array([0.25]), False)[2][0]


# ---- the phasor -----------------------------------------------------------------------------------------------------------------------
def test_unit_phasor_against_long_double():
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63, "the reference needs an extended long double"
    special = np.array([0.0, 0.125, -0.125, 0.375, -0.375, 0.5, -0.5, 0.25, -0.25])
    near = np.concatenate([special, np.nextafter(special, 1.0), np.nextafter(special, -1.0), np.nextafter(np.nextafter(special, 1.0), 1.0),
                           np.nextafter(np.nextafter(special, -1.0), -1.0)])
    rs = np.random.RandomState(7)
    u = np.concatenate([near[np.abs(near) <= 0.5], rs.uniform(-0.5, 0.5, 100000), rs.uniform(-1e-3, 1e-3, 1000), [1e-300, -1e-300, 5e-324]])
    c, s = R.unit_phasor(u)
    two_pi = 2 * np.longdouble('3.14159265358979323846264338327950288')
    arg = two_pi * u.astype(np.longdouble)
    ec, es = np.abs(c - np.cos(arg)).max(), np.abs(s - np.sin(arg)).max()
    en = np.abs((c.astype(np.longdouble) ** 2 + s.astype(np.longdouble) ** 2) - 1).max()
    print("unit_phasor on %d arguments: cos within %.3g, sin within %.3g (bound 2^-51 = %.3g), |c^2 + s^2 - 1| within %.3g (bound %.3g)"
          % (u.size, ec, es, 2.0 ** -51, en, 2.0 ** -50))
    assert ec <= 2.0 ** -51 and es <= 2.0 ** -51 and en <= 2.0 ** -50
    # the quadrants are exact swaps and negations
    c, s = R.unit_phasor(np.array([0.0, 0.25, 0.5, -0.5, -0.25]))
    assert np.array_equal(c, [1.0, 0.0, -1.0, -1.0, 0.0]) and np.array_equal(s, [0.0, 1.0, 0.0, 0.0, -1.0])


# ---- the closed loop ------------------------------------------------------------------------------------------------------------------
def unit_energy(M):
    md = QAMModem(M)
    return md.constellation / np.sqrt(md.Es)


def loop_figures(out, sps):
    pos, ph = out['position'][0], out['phase'][0]
    step = np.diff(ph[-201:])
    return (pos[-1] - pos[-201]) / 200.0, float(np.mean(step - np.rint(step)))


@pytest.mark.parametrize("M,sps", [(4, 2), (4, 4), (16, 2), (16, 4)])
def test_gardner_locks(M, sps):
    """1500 raised-cosine symbols, roll-off 0.35, offset 0.3 symbol, sample clock 1.0004, phase 0.03 turn, 5e-4 cycle per symbol,
    sigma 0.02: no wrong decision in strobes 500 .. 1400; over the last 200 strobes the mean period is within 1e-4 sample of
    sps / 1.0004 and the mean phase step within 1e-4 of 5e-4 turn."""
    const = unit_energy(M)
    idx, y = R.rc_burst(const, 1500, sps, 10 * M + sps)
    out = R.recover(y, sps, const, 'gardner', 'cubic', 0.02 * sps, 2e-4 * sps, (0.05, 0.002), n=1400)
    assert not out['bad'].any() and out['count'][0] == 1399                    # strobe 0 reads index -1
    period, step = loop_figures(out, sps)
    print("gardner M=%d sps=%d: period %.6f samples (sent %.6f), phase step %.3e" % (M, sps, period, sps / 1.0004, step))
    assert np.array_equal(out['indices'][0, 500:1400], idx[500:1400])
    assert abs(period - sps / 1.0004) <= 1e-4 and abs(step - 5e-4) <= 1e-4


@pytest.mark.parametrize("sps", [2, 4])
def test_mueller_muller_with_training_locks(sps):
    """16-QAM, decision-directed timing and carrier: a 64-symbol training prefix settles the quarter-turn ambiguity.  The seeds were
    run on the CPU before they were written here: 163 and 165 give a period 1.6e-5 and 3.4e-5 sample off and no wrong decision."""
    const = unit_energy(16)
    idx, y = R.rc_burst(const, 1500, sps, 161 + sps, phase=0.2)
    out = R.recover(y, sps, const, 'mm', 'cubic', 0.02 * sps, 2e-4 * sps, (0.05, 0.002), idx[:64], n=1400)
    assert not out['bad'].any()
    period, step = loop_figures(out, sps)
    print("mm 16-QAM sps=%d: period %.6f samples (sent %.6f), phase step %.3e" % (sps, period, sps / 1.0004, step))
    assert np.array_equal(out['indices'][0, 500:1400], idx[500:1400])
    assert abs(period - sps / 1.0004) <= 1e-4 and abs(step - 5e-4) <= 1e-4


def test_model_rejects_rows_on_their_own():
    const = unit_energy(4)
    rows = np.stack([R.rc_burst(const, 40, 2, s, n_y=80)[1] for s in range(8)])
    kw = dict(k1=0.04, k2=4e-4, carrier=(0.05, 0.002), n=30)
    clean = R.recover(rows, 2, const, 'mm', 'cubic', training=np.zeros((8, 3), int), **kw)
    assert not clean['bad'].any()
    y, tr, k1, mu0, ph0, m0 = rows.copy(), np.zeros((8, 3), int), np.full(8, 0.04), np.zeros(8), np.zeros(8), np.zeros(8, int)
    y[0, 70] = np.nan                                              # behind the last sample any strobe reads
    tr[1, 2] = 4
    k1[2] = 1e6                                                    # the period leaves (0.5 sps, 1.5 sps)
    k1[3] = np.inf
    mu0[4] = 1.0
    ph0[5] = 0.75
    m0[6] = 80
    out = R.recover(y, 2, const, 'mm', 'cubic', k1, 4e-4, (0.05, 0.002), tr, 30, m0, mu0, ph0)
    assert out['bad'].tolist() == [True] * 7 + [False]
    assert not out['indices'][:7].any() and not out['bits'][:7].any() and not out['count'][:7].any()
    assert all(np.isnan(out[key][:7].view(np.float64)).all() for key in ('symbols', 'position', 'error', 'phase'))
    for key in RECOVERY_WANT:
        assert np.array_equal(out[key][7], clean[key][7])


# ---- gains ----------------------------------------------------------------------------------------------------------------------------
def test_loop_gains_by_hand():
    """damping 0.5, bandwidth 0.1: theta = 0.1, d = 1.11, k1 = 0.2 / 1.11 = 20/111, k2 = 0.04 / 1.11 = 4/111.  damping 1, bandwidth
    0.05, detector gain 2: theta = 0.05 / 1.25 = 0.04, d = 1.0816, k1 = 0.16 / 1.0816 / 2 = 25/338, k2 = 0.0064 / 1.0816 / 2 = 1/338."""
    assert loop_gains(0.1, 0.5) == pytest.approx((20 / 111, 4 / 111), rel=1e-14)
    assert loop_gains(0.05, 1.0, 2.0) == pytest.approx((25 / 338, 1 / 338), rel=1e-14)
    for bad in (lambda: loop_gains(0.0), lambda: loop_gains(0.01, 0.0), lambda: loop_gains(0.01, detector_gain=-1.0),
                lambda: loop_gains(float('nan'))):
        with pytest.raises(ValueError):
            bad()


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def no_device(monkeypatch):
    """Any attempt to load the engine fails the test: the refusals below must come from the host-side checks."""
    def boom(*a, **k):
        raise AssertionError("the engine was touched")
    monkeypatch.setattr(_lib, "load", boom)


class Duck:
    num_bits_symbol, Es = 2, 1.0

    def __init__(self, M):
        self.m, self.constellation = M, np.ones(M, complex)


def test_python_refusals(no_device):
    qpsk = QAMModem(4)
    y, tr, buf = np.zeros((2, 20), complex), np.zeros(4, int), object()
    rec = timing_recover_batch
    dev = lambda modem=None, B=2, n_y=20, sps=2, k1=buf, k2=buf, m0=buf, mu0=buf, ph=buf, **kw: deviceops.timing_recover_dev(
        buf, B, n_y, sps, k1, False, k2, False, m0, False, mu0, False, ph, False, modem, **kw)
    for bad, limit in (
            (lambda: rec(y, 1), '2 <= sps <= 8'),
            (lambda: rec(y, 2.5), 'sps must be an integer'),
            (lambda: rec(y, True), 'sps must be an integer'),
            (lambda: rec(y, 9), '2 <= sps <= 8'),
            (lambda: rec(y, 2, ted='zc'), "'gardner', 'mm'"),
            (lambda: rec(y, 2, interp='sinc'), "'linear', 'cubic'"),
            (lambda: rec(y, 2, n=0), '1 <= n <= 2^30'),
            (lambda: rec(y, 2, n=2 ** 30 + 1), '1 <= n <= 2^30'),
            (lambda: rec(np.zeros((2, 0), complex), 2, n=1), '1 <= n_y'),
            (lambda: rec(y, 2, ted='mm'), "ted = 'mm' needs a modem"),
            (lambda: rec(y, 2, carrier=(0.1, 0.01)), 'carrier needs a modem'),
            (lambda: rec(y, 2, training=tr), 'training needs a modem'),
            (lambda: rec(y, 2, want='indices'), "'indices' needs a modem"),
            (lambda: rec(y, 2, want=('symbols', 'bits')), "'bits' needs a modem"),
            (lambda: rec(y, 2, Duck(1)), '2 <= M <= 256'),
            (lambda: rec(y, 2, Duck(257)), '2 <= M <= 256'),
            (lambda: rec(y, 2, Duck(6), want='bits'), 'power of two'),
            (lambda: rec(y, 2, qpsk, want='phase'), "'phase' is wanted without carrier"),
            (lambda: rec(y, 2, qpsk, carrier=0.1), 'carrier must be None or (kc1, kc2)'),
            (lambda: rec(y, 2, qpsk, training=np.zeros(11, int)), '0 <= nt <= n'),
            (lambda: rec(y, 2, qpsk, training=np.zeros((3, 4), int)), 'training must be'),
            (lambda: rec(y, 2, qpsk, training=np.zeros(4)), 'integer labels'),
            (lambda: rec(y, 2, k1=-0.1), 'k1 >= 0'),
            (lambda: rec(y, 2, k2=np.array([0.1, -0.1])), 'k2 >= 0'),
            (lambda: rec(y, 2, k1=np.ones(3)), 'k1 must be a scalar or [B]'),
            (lambda: rec(y, 2, qpsk, carrier=(-1.0, 0.0)), 'kc1 >= 0'),
            (lambda: rec(y, 2, qpsk, carrier=(0.0, np.array([0.0, -1.0]))), 'kc2 >= 0'),
            (lambda: rec(y, 2, mu0=1.0), '0 <= mu0 < 1'),
            (lambda: rec(y, 2, mu0=-0.25), '0 <= mu0 < 1'),
            (lambda: rec(y, 2, phase0=0.6), '|phase0| <= 0.5'),
            (lambda: rec(y, 2, m0=20), '0 <= m0 < n_y'),
            (lambda: rec(y, 2, m0=np.array([0, -1])), '0 <= m0 < n_y'),
            (lambda: rec(y, 2, m0=0.5), 'm0 must hold integers'),
            (lambda: rec(y, 2, m0=np.zeros(3, int)), 'm0 must be a scalar or [B]'),
            (lambda: rec(np.zeros((2, 3, 4), complex), 2), '1-D'),
            (lambda: rec(y.astype(str), 2), 'numbers'),
            (lambda: rec(y, 2, want=()), 'want'),
            (lambda: rec(y, 2, want=('symbols', 'llr')), 'want'),
            (lambda: dev(sps=9), '2 <= sps <= 8'),
            (lambda: dev(sps=2.5), 'sps must be an integer'),
            (lambda: dev(ted='mm'), "ted = 'mm' needs a modem"),
            (lambda: dev(d_kc1=buf, d_kc2=buf), 'carrier needs a modem'),
            (lambda: dev(qpsk, d_kc1=buf), 'both kc1 and kc2'),
            (lambda: dev(qpsk, want='phase'), "'phase' is wanted without carrier"),
            (lambda: dev(want='indices'), "'indices' needs a modem"),
            (lambda: dev(Duck(6), want='bits'), 'power of two'),
            (lambda: dev(qpsk, nt=11, d_training=buf), '0 <= nt <= n'),
            (lambda: dev(qpsk, nt=4), 'training is required'),
            (lambda: dev(nt=4, d_training=buf), 'training needs a modem'),
            (lambda: dev(k1=None), 'k1 and k2 are required'),
            (lambda: dev(mu0=None), 'm0, mu0 and phase0 are required'),
            (lambda: dev(B=-1), 'B'),
            (lambda: dev(n_y=0, n=1), '1 <= n_y'),
            (lambda: dev(n=0), '1 <= n <= 2^30'),
            (lambda: dev(want='llr'), 'want')):
        with pytest.raises(ValueError) as err:
            bad()
        assert limit in str(err.value), (limit, str(err.value))


def test_shape_table_order_and_empty_batch(no_device):
    """``want`` in any order returns the results in the order of the table; ``B = 0`` makes no device call."""
    assert tuple(recovery_shapes(3, 5, 2)) == RECOVERY_WANT == ('symbols', 'indices', 'bits', 'position', 'error', 'phase', 'count')
    table = recovery_shapes(3, 5, 2)
    assert table['symbols'] == ((3, 5), np.complex128) and table['indices'] == ((3, 5), np.int32) and table['bits'] == ((3, 10), np.uint8)
    assert all(table[key] == ((3, 5), np.float64) for key in ('position', 'error', 'phase')) and table['count'] == ((3,), np.int32)
    got = timing_recover_batch(np.zeros((0, 20), complex), 2, QAMModem(16), carrier=(0.1, 0.01), training=np.zeros((0, 3), int),
                               want=('count', 'phase', 'bits', 'symbols', 'error', 'position', 'indices'))
    assert [(g.shape, g.dtype) for g in got] == [((0, 10), np.complex128), ((0, 10), np.int32), ((0, 40), np.uint8), ((0, 10), np.float64),
                                                 ((0, 10), np.float64), ((0, 10), np.float64), ((0,), np.int32)]
    single = timing_recover_batch(np.zeros((0, 21), complex), 3, want='position')
    assert single.shape == (0, 7) and single.dtype == np.float64


def c_call(lib, md, device_form, **over):
    """One call of the C-ABI with host pointers that are never followed past the limits (the host form reads the parameter values)."""
    val = lambda v: (ctypes.c_double * 2)(v, v)
    a = dict(B=2, n_y=20, n=10, sps=2, ted=0, interp=1, k1=val(0.1), k2=val(0.01), kc1=None, kc2=None, training=None, nt=0,
             m0=(ctypes.c_int64 * 2)(0, 0), mu0=val(0.0), phase0=val(0.0), symbols=ctypes.c_void_p(8), indices=None, bits=None, phase=None,
             batched=0)
    a.update(over)
    b = a['batched']
    args = [md, None, a['B'], a['n_y'], a['n'], a['sps'], a['ted'], a['interp'], a['k1'], b, a['k2'], b, a['kc1'], b, a['kc2'], b,
            a['training'], 0, a['nt'], a['m0'], b, a['mu0'], b, a['phase0'], b, a['symbols'], a['indices'], a['bits'], None, None, a['phase'],
            None]
    rc = lib.cpx_timing_recover_dev(*args, None) if device_form else lib.cpx_timing_recover(*args)
    return rc, _lib.last_error()


def test_c_abi_refuses_before_a_device_is_looked_for():
    """Every limit, in both forms, on a stand-in for the modem handle whose first two ints are M and the bits per symbol: the shared
    check reads nothing else of it, and returns before any device pointer is followed."""
    lib = _lib.load()
    qpsk, six = (ctypes.c_int * 64)(4, 2), (ctypes.c_int * 64)(6, 2)
    val = lambda a, b: (ctypes.c_double * 2)(a, b)
    some = ctypes.c_void_p(8)
    for device_form in (False, True):
        cases = [(None, dict(B=-1), 'B = -1'), (None, dict(ted=2), 'ted = 2'), (None, dict(interp=-1), 'interp = -1'),
                 (None, dict(sps=1), '2 <= sps <= 8'), (None, dict(sps=9), '2 <= sps <= 8'), (None, dict(n=0), '1 <= n <= 2^30'),
                 (None, dict(n=2 ** 30 + 1), '1 <= n <= 2^30'), (None, dict(n_y=0), '1 <= n_y <= 2^33'),
                 (None, dict(k1=None), 'k1 and k2 are required'), (qpsk, dict(kc1=val(0.1, 0.1)), 'both kc1 and kc2'),
                 (None, dict(mu0=None), 'm0, mu0 and phase0 are required'), (None, dict(ted=1), "'mm' needs a modem"),
                 (None, dict(kc1=val(0.1, 0.1), kc2=val(0.1, 0.1)), 'the carrier loop needs a modem'),
                 (None, dict(nt=2, training=some), 'training needs a modem'), (None, dict(indices=some), 'indices and bits need a modem'),
                 (None, dict(bits=some), 'indices and bits need a modem'), (qpsk, dict(phase=some), 'phase is asked for without'),
                 (qpsk, dict(nt=11, training=some), '0 <= nt <= n'), (qpsk, dict(nt=-1), '0 <= nt <= n'),
                 (None, dict(symbols=None), 'no output requested'), (six, dict(bits=some), 'power of two'),
                 ((ctypes.c_int * 64)(1, 1), {}, '2 <= M <= 256'), ((ctypes.c_int * 64)(257, 1), {}, '2 <= M <= 256')]
        if not device_form:                                    # values the host form can read
            cases += [(None, dict(k1=val(-0.1, 0.1)), 'k1 >= 0'), (None, dict(k2=val(0.1, -1.0), batched=1), 'k2 >= 0'),
                      (qpsk, dict(kc1=val(-1.0, 0.0), kc2=val(0.0, 0.0)), 'kc1 >= 0'), (None, dict(mu0=val(1.0, 0.0)), '0 <= mu0 < 1'),
                      (None, dict(mu0=val(0.0, -0.5), batched=1), '0 <= mu0 < 1'), (None, dict(phase0=val(0.75, 0.0)), '|phase0| <= 0.5'),
                      (None, dict(m0=(ctypes.c_int64 * 2)(20, 0)), '0 <= m0 < n_y'),
                      (None, dict(m0=(ctypes.c_int64 * 2)(0, -1), batched=1), '0 <= m0 < n_y')]
        for md, over, limit in cases:
            rc, msg = c_call(lib, md, device_form, **over)
            assert rc == _lib.CPX_EINVAL and limit in msg, (device_form, over, msg)


def test_fails_loudly_without_a_device():
    if _lib.device_count() == 0:
        with pytest.raises(_lib.EngineError):
            timing_recover_batch(np.zeros((2, 20), complex), 2)
        with pytest.raises(_lib.EngineError):
            timing_recover_batch(np.zeros((2, 20), complex), 2, PSKModem(2), 'mm')
