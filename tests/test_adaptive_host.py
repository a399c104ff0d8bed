"""The adaptive equalisers' NumPy model (tests/adaptive_model.py) against independent truth, and the refusals of the Python layer and
the C-ABI; no GPU.

The bound of test_rls_equals_regularised_least_squares: the RLS recursion with lambda = 1 is the matrix-inversion-lemma form of
``(delta I + X^H X) theta = X^H r``.  Each of its ``n`` steps does ``O(N)`` operations per element of ``P``, each rounded to
``2^-52`` relative, and an error in ``P`` reaches the taps amplified by at most ``kappa_2(Phi)``, ``Phi = delta I + X^H X``; hence
``K n N 2^-52 kappa_2(Phi)`` in relative 2-norm with ``K = 1``.  Measured with the operation order of the rule (printed by the test):
ratios to the bound 0.22 at (nf, nb, n) = (1, 0, 8) -- where the bound is 8 * 2^-52 and the difference, 4e-16, is two roundings, the
direct solve's own included -- then 5.5e-3, 2.6e-3 and 1.2e-3 at (6, 2, 60), (24, 8, 400) and (32, 0, 2000): none within a factor of 4
of the bound, so K stays 1.
"""
import ctypes
from fractions import Fraction

import numpy as np
import pytest

import adaptive_model as A
from commpy_amd import _lib, deviceops
from commpy_amd.equalizers import adaptive_equalize_batch
from commpy_amd.modulation import PSKModem, QAMModem

K = 1.0
CHANNEL_B = np.array([0.407, 0.815, 0.407])
THREE_TAPS = np.array([1.0, 0.3 + 0.2j, -0.1j])


def regressors(y, ref, nf, nb, d, sps, n):
    """``X [n, nf + nb]`` of one row, built without the model: row ``t`` is ``(y[t sps + d - i], i < nf; -ref[t - j], j = 1 .. nb)``."""
    X = np.zeros((n, nf + nb), dtype=np.complex128)
    for t in range(n):
        for i in range(nf):
            s = t * sps + d - i
            if 0 <= s < len(y):
                X[t, i] = y[s]
        for j in range(1, nb + 1):
            if t - j >= 0:
                X[t, nf + j - 1] = -ref[t - j]
    return X


@pytest.mark.parametrize("nf,nb,n", [(1, 0, 8), (6, 2, 60), (24, 8, 400), (32, 0, 2000)])
def test_rls_equals_regularised_least_squares(nf, nb, n):
    modem = QAMModem(4)
    rs = np.random.RandomState(100 + nf)
    idx = rs.randint(0, 4, n)
    ref = modem.constellation[idx]
    y = np.convolve(ref, THREE_TAPS)[:n] + 0.05 * (rs.randn(n) + 1j * rs.randn(n))
    delta, d = 0.01, A.default_delay(nf, nb)
    got = A.equalize(y, modem.constellation, idx, nf, nb, 'rls', forgetting=1.0, delta=delta)
    X = regressors(y, ref, nf, nb, d, 1, n)
    Phi = delta * np.eye(nf + nb) + X.conj().T @ X
    theta = np.linalg.solve(Phi, X.conj().T @ ref)
    mine = np.concatenate([got['ff'][0], got['fb'][0]])
    rel = np.linalg.norm(mine - theta) / np.linalg.norm(theta)
    bound = K * n * (nf + nb) * 2.0 ** -52 * np.linalg.cond(Phi)
    print("rls vs least squares (nf, nb, n) = (%d, %d, %d): relative difference %.3g, bound %.3g, ratio %.3g" % (nf, nb, n, rel, bound, rel / bound))
    assert rel <= bound


# ---- one step by hand, in exact rational arithmetic --------------------------------------------------------------------------------
def cmul(a, b):
    return (a[0] * b[0] - a[1] * b[1], a[0] * b[1] + a[1] * b[0])


def cadd(a, b):
    return (a[0] + b[0], a[1] + b[1])


def csub(a, b):
    return (a[0] - b[0], a[1] - b[1])


def conj(a):
    return (a[0], -a[1])


def frac(z):
    return (Fraction(z.real), Fraction(z.imag))


def by_hand(algorithm, y, const, labels, ff0, fb0, d, mu, eps, lam, delta):
    """Two steps of the equaliser with nf = 2, nb = 1 as the textbook writes them -- z = theta^T x with x = (y_{t+d}, y_{t+d-1}, -r_{t-1}),
    e = r - z, then the update -- in exact complex rationals.  Returns ``(theta, [z_0, z_1], [e_0, e_1])``."""
    theta = [frac(v) for v in ff0] + [frac(fb0[0])]
    P = [[(Fraction(1) / delta if i == j else Fraction(0), Fraction(0)) for j in range(3)] for i in range(3)]
    zs, es, zero = [], [], (Fraction(0), Fraction(0))
    sample = lambda s: frac(y[s]) if 0 <= s < len(y) else zero
    for t in range(2):
        r_prev = frac(const[labels[t - 1]]) if t >= 1 else zero
        x = [sample(t + d), sample(t + d - 1), (-r_prev[0], -r_prev[1])]
        z = zero
        for k in range(3):
            z = cadd(z, cmul(theta[k], x[k]))
        e = csub(frac(const[labels[t]]), z)
        if algorithm == 'rls':
            g = []
            for i in range(3):
                acc = zero
                for j in range(3):
                    acc = cadd(acc, cmul(P[i][j], conj(x[j])))
                g.append(acc)
            den = lam + sum(cmul(x[k], g[k])[0] for k in range(3))
            kap = [(g[i][0] / den, g[i][1] / den) for i in range(3)]
            theta = [cadd(theta[i], cmul(kap[i], e)) for i in range(3)]
            P = [[tuple(v / lam for v in csub(P[i][j], cmul(kap[i], conj(g[j])))) for j in range(3)] for i in range(3)]
        else:
            m = mu / (eps + sum(v[0] * v[0] + v[1] * v[1] for v in x)) if algorithm == 'nlms' else mu
            w = (m * e[0], m * e[1])
            theta = [cadd(theta[k], cmul(w, conj(x[k]))) for k in range(3)]
        zs.append(z)
        es.append(e)
    return theta, zs, es


@pytest.mark.parametrize("algorithm", ['lms', 'nlms', 'rls'])
def test_one_step_by_hand(algorithm):
    """Signs and conjugates: fb enters with a minus, no conjugate in z, conj(x) in the update.  All inputs are small Gaussian integers
    and dyadic parameters; for 'lms' and 'nlms' (eps = 0 and regressor energies 4 and 8) every value is dyadic and the model must equal
    the exact result; 'rls' divides by a den that is no power of two, so it must agree to 1e-13 relative."""
    const = np.array([1 + 1j, -1 + 1j, -1 - 1j, 1 - 1j])
    y = np.array([1 - 1j, 1 + 1j, 2j])                           # step 0: x = (y1, y0, 0), energy 4; step 1: x = (y2, y1, -r_0), energy 8
    labels, ff0, fb0 = [1, 3], np.array([1 + 0j, 0 + 1j]), np.array([1 - 1j])
    mu, eps, lam, delta = Fraction(1, 4), Fraction(0), Fraction(1, 2), Fraction(1, 4)
    theta, zs, es = by_hand(algorithm, y, const, labels, ff0, fb0, 1, mu, eps, lam, delta)
    got = A.equalize(y, const, labels, 2, 1, algorithm, step=None if algorithm == 'rls' else 0.25, forgetting=0.5, delta=0.25, eps=0.0,
                     delay=1, n=2, ff0=ff0, fb0=fb0)
    assert not got['bad'][0]
    mine = [(got['estimate'][0], zs), (got['error'][0], es), (np.concatenate([got['ff'][0], got['fb'][0]]), theta)]
    for values, exact in mine:
        for v, ex in zip(values, exact):
            if algorithm == 'rls':
                scale = max(abs(float(ex[0])), abs(float(ex[1])), 1.0)
                assert abs(v.real - float(ex[0])) <= 1e-13 * scale and abs(v.imag - float(ex[1])) <= 1e-13 * scale
            else:
                assert Fraction(v.real) == ex[0] and Fraction(v.imag) == ex[1], (v, ex)
    assert es[1] != (Fraction(0), Fraction(0)) and theta[2] != frac(fb0[0])      # the feedback tap took part and moved


# ---- behaviour ------------------------------------------------------------------------------------------------------------------
def errors_after(got, idx, nt):
    return int((got['indices'][0][nt:] != idx[nt:]).sum())


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_convergence_noise_free(seed):
    """16-QAM through (1, 0.3+0.2j, -0.1j), 600 symbols, 256 of them training: no symbol error afterwards."""
    modem = QAMModem(16)
    rs = np.random.RandomState(seed)
    n, nt = 600, 256
    idx = rs.randint(0, 16, n)
    y = np.convolve(modem.constellation[idx], THREE_TAPS)
    c = modem.constellation
    cases = [('lms 8,0', dict(nf=8, nb=0, algorithm='lms', step=0.002, delay=3)),
             ('lms 4,2', dict(nf=4, nb=2, algorithm='lms', step=0.002, delay=3)),
             ('nlms 8,0', dict(nf=8, nb=0, algorithm='nlms', step=0.5, delay=3)),
             ('rls 0.99', dict(nf=8, nb=0, algorithm='rls', forgetting=0.99, delta=0.01, delay=3)),
             ('rls 1', dict(nf=8, nb=0, algorithm='rls', forgetting=1.0, delta=0.01, delay=3))]
    for name, kw in cases:
        got = A.equalize(y, c, idx[:nt], n=n, **kw)
        assert not got['bad'][0]
        assert errors_after(got, idx, nt) == 0, (name, seed, errors_after(got, idx, nt))


@pytest.mark.parametrize("algorithm,kw", [('lms', dict(step=0.01)), ('rls', dict())])
def test_half_symbol_spacing(algorithm, kw):
    """QPSK, zero-stuffed by 2, through four T/2-spaced taps, noise-free: a T/2-spaced equaliser makes no error after 100 training symbols."""
    modem = QAMModem(4)
    rs = np.random.RandomState(4)
    n, nt = 400, 100
    idx = rs.randint(0, 4, n)
    up = np.zeros(2 * n, dtype=complex)
    up[::2] = modem.constellation[idx]
    y = np.convolve(up, np.array([0.2, 0.9, 0.5, -0.1 + 0.1j]))
    got = A.equalize(y, modem.constellation, idx[:nt], 8, 0, algorithm, delay=4, sps=2, n=n, **kw)
    assert not got['bad'][0] and errors_after(got, idx, nt) == 0, errors_after(got, idx, nt)


def test_ordering_on_channel_b():
    """The inputs of test_equalize_host.py::test_ordering_on_channel_b (QPSK, 14 dB, seed 14, 4000 symbols, nf = 16), nt = 200: feedback
    (nb = 2, delay 15) makes fewer errors than the linear equaliser (delay 8) for every algorithm, and RLS-DFE no more than LMS-DFE.
    Measured (nlms with mu = 0.1): LE 698 / 978 / 401 and DFE 99 / 266 / 18 symbol errors for lms / nlms / rls."""
    modem = QAMModem(4)
    rs = np.random.RandomState(14)
    n, nt = 4000, 200
    idx = rs.randint(0, 4, n)
    N0 = modem.Es / 10 ** 1.4
    y = np.convolve(modem.constellation[idx], CHANNEL_B) + np.sqrt(N0 / 2) * (rs.randn(n + 2) + 1j * rs.randn(n + 2))
    algs = {'lms': dict(step=0.005), 'nlms': dict(step=0.1), 'rls': dict(forgetting=0.999, delta=0.01)}
    count = {}
    for name, kw in algs.items():
        le = A.equalize(y, modem.constellation, idx[:nt], 16, 0, name, delay=8, n=n, **kw)
        dfe = A.equalize(y, modem.constellation, idx[:nt], 16, 2, name, delay=15, n=n, **kw)
        count[name] = (errors_after(le, idx, nt), errors_after(dfe, idx, nt))
    print("channel B, QPSK, 14 dB, %d symbols after %d of training, symbol errors (LE, DFE): %s" % (n - nt, nt, count))
    for name in algs:
        assert count[name][1] < count[name][0], (name, count)
    assert count['rls'][1] <= count['lms'][1], count


@pytest.mark.parametrize("algorithm,step", [('lms', 0.01), ('nlms', 0.3)])
def test_continuation(algorithm, step):
    """Two calls over the halves of a row, the second starting from the first's taps, equal one call bit for bit (nb = 0; delay = nf - 1,
    so that no step of the second half reaches back before its first sample)."""
    modem = QAMModem(16)
    rs = np.random.RandomState(6)
    n, nt, n1, nf = 120, 80, 50, 5
    idx = rs.randint(0, 16, n)
    y = np.convolve(modem.constellation[idx], THREE_TAPS) + 0.02 * (rs.randn(n + 2) + 1j * rs.randn(n + 2))
    kw = dict(nf=nf, nb=0, algorithm=algorithm, step=step, delay=nf - 1)
    whole = A.equalize(y, modem.constellation, idx[:nt], n=n, **kw)
    first = A.equalize(y, modem.constellation, idx[:n1], n=n1, **kw)
    second = A.equalize(y[n1:], modem.constellation, idx[n1:nt], n=n - n1, ff0=first['ff'][0], **kw)
    for key in ('indices', 'estimate', 'error'):
        joined = np.concatenate([first[key][0], second[key][0]])
        assert joined.tobytes() == whole[key][0].tobytes(), key
    assert second['ff'].tobytes() == whole['ff'].tobytes()


def test_model_rejects_rows_on_their_own():
    modem = QAMModem(4)
    rs = np.random.RandomState(9)
    idx = rs.randint(0, 4, (5, 40))
    y = modem.constellation[idx] + 0.1 * rs.randn(5, 40)
    good = A.equalize(y, modem.constellation, idx[:, :10], 3, 1, 'lms', step=0.05)
    y2, tr2, step2 = y.copy(), idx[:, :10].copy(), np.full(5, 0.05)
    y2[0, 39], tr2[1, 3], step2[2] = np.nan, 4, 1e200
    step2[3] = np.inf
    rej = A.equalize(y2, modem.constellation, tr2, 3, 1, 'lms', step=step2)
    assert rej['bad'].tolist() == [True, True, True, True, False]
    assert not rej['indices'][:4].any() and not rej['bits'][:4].any()
    for key in ('estimate', 'error', 'ff', 'fb'):
        assert np.isnan(rej[key][:4].real).all() and np.isnan(rej[key][:4].imag).all(), key
        assert rej[key][4].tobytes() == good[key][4].tobytes(), key
    three = np.exp(2j * np.pi * np.arange(3) / 3)                  # no power of two: every result but 'bits'
    idx3 = rs.randint(0, 3, 60)
    got = A.equalize(three[idx3] * (1 + 0.1j), three, idx3[:20], 2, 1, 'rls')
    assert 'bits' not in got and not got['bad'][0] and np.array_equal(got['indices'][0][20:], idx3[20:])


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def no_device(monkeypatch):
    """Any attempt to load the engine fails the test: the refusals below must come from the host-side checks."""
    def boom(*a, **k):
        raise AssertionError("the engine was touched")
    monkeypatch.setattr(_lib, "load", boom)


def test_python_refusals(no_device):
    qpsk = QAMModem(4)
    y, tr, buf = np.zeros((2, 20), complex), np.zeros(4, int), object()

    class Duck:
        num_bits_symbol, Es = 2, 1.0

        def __init__(self, M):
            self.m, self.constellation = M, np.ones(M, complex)
    eq = adaptive_equalize_batch
    dev = deviceops.adaptive_equalize_dev
    for bad, limit in (
            (lambda: eq(y, qpsk, tr, 0, step=0.1), '1 <= nf <= 64'),
            (lambda: eq(y, qpsk, tr, 65, step=0.1), '1 <= nf <= 64'),
            (lambda: eq(y, qpsk, tr, 4, -1, step=0.1), '0 <= nb <= 64'),
            (lambda: eq(y, qpsk, tr, 4, 65, step=0.1), '0 <= nb <= 64'),
            (lambda: eq(y, qpsk, tr, 30, 3, 'rls'), 'nf + nb <= 32'),
            (lambda: eq(y, qpsk, tr, 4, algorithm='cma', step=0.1), "'lms', 'nlms', 'rls'"),
            (lambda: eq(y, qpsk, tr, 4), 'step is required'),
            (lambda: eq(y, qpsk, tr, 4, algorithm='nlms'), 'step is required'),
            (lambda: eq(y, qpsk, tr, 4, algorithm='rls', step=0.1), "step is given with 'rls'"),
            (lambda: eq(y, qpsk, tr, 4, step=0.0), 'step must be positive'),
            (lambda: eq(y, qpsk, tr, 4, step=np.array([0.1, -0.1])), 'step must be positive'),
            (lambda: eq(y, qpsk, tr, 4, step=np.ones(3)), 'step must be a scalar or [B]'),
            (lambda: eq(y, qpsk, tr, 4, algorithm='rls', forgetting=0.0), 'forgetting must be positive'),
            (lambda: eq(y, qpsk, tr, 4, algorithm='rls', forgetting=1.5), 'forgetting must be at most 1'),
            (lambda: eq(y, qpsk, tr, 4, algorithm='rls', forgetting=np.ones(3)), 'forgetting must be a scalar or [B]'),
            (lambda: eq(y, qpsk, tr, 4, algorithm='rls', delta=0.0), 'delta must be positive'),
            (lambda: eq(y, qpsk, tr, 4, algorithm='rls', delta=np.array([1.0, -1.0])), 'delta must be positive'),
            (lambda: eq(y, qpsk, tr, 4, algorithm='nlms', step=0.1, eps=-1e-9), 'eps >= 0'),
            (lambda: eq(y, qpsk, tr, 4, step=0.1, delay=-1), '0 <= delay'),
            (lambda: eq(y, qpsk, tr, 4, step=0.1, sps=0), '1 <= sps <= 8'),
            (lambda: eq(y, qpsk, tr, 4, step=0.1, sps=9), '1 <= sps <= 8'),
            (lambda: eq(y, Duck(1), tr, 4, step=0.1), '2 <= M <= 256'),
            (lambda: eq(y, Duck(257), tr, 4, step=0.1), '2 <= M <= 256'),
            (lambda: eq(y, Duck(6), tr, 4, step=0.1, want='bits'), 'power of two'),
            (lambda: eq(np.zeros((2, 0), complex), qpsk, tr[:0], 4, step=0.1), '1 <= n'),
            (lambda: eq(y, qpsk, tr, 4, step=0.1, n=0), '1 <= n'),
            (lambda: eq(y, qpsk, tr, 4, step=0.1, n=2 ** 30 + 1), '1 <= n'),
            (lambda: eq(y, qpsk, np.zeros(21, int), 4, step=0.1), '0 <= nt <= n'),
            (lambda: eq(y, qpsk, tr, 4, step=0.1, sps=2, n=3), '0 <= nt <= n'),
            (lambda: eq(y, qpsk, np.zeros((3, 4), int), 4, step=0.1), 'training must be'),
            (lambda: eq(y, qpsk, np.zeros(4), 4, step=0.1), 'integer labels'),
            (lambda: eq(y, qpsk, tr, 4, step=0.1, ff0=np.zeros(3)), 'ff0 must be'),
            (lambda: eq(y, qpsk, tr, 4, 2, step=0.1, fb0=np.zeros((3, 2))), 'fb0 must be'),
            (lambda: eq(np.zeros((2, 3, 4), complex), qpsk, tr, 4, step=0.1), '1-D'),
            (lambda: eq(y.astype(str), qpsk, tr, 4, step=0.1), 'numbers'),
            (lambda: eq(y, qpsk, tr, 4, step=0.1, want=()), 'want'),
            (lambda: eq(y, qpsk, tr, 4, step=0.1, want=('indices', 'llr')), 'want'),
            (lambda: dev(qpsk, buf, 2, 20, buf, False, 4, 65, d_step=buf), '1 <= nf <= 64'),
            (lambda: dev(qpsk, buf, 2, 20, buf, False, 4, 4, 65, d_step=buf), '0 <= nb <= 64'),
            (lambda: dev(qpsk, buf, 2, 20, buf, False, 4, 30, 3, 'rls', d_forgetting=buf, d_delta=buf), 'nf + nb <= 32'),
            (lambda: dev(qpsk, buf, 2, 20, buf, False, 4, 4), 'step is required'),
            (lambda: dev(qpsk, buf, 2, 20, buf, False, 4, 4, 0, 'rls', d_step=buf), "step is given with 'rls'"),
            (lambda: dev(qpsk, buf, 2, 20, buf, False, 4, 4, 0, 'rls', d_delta=buf), 'forgetting and delta are required'),
            (lambda: dev(qpsk, buf, 2, 20, None, False, 4, 4, d_step=buf), 'training is required'),
            (lambda: dev(qpsk, buf, 2, 20, buf, False, 21, 4, d_step=buf), '0 <= nt <= n'),
            (lambda: dev(qpsk, buf, -1, 20, buf, False, 4, 4, d_step=buf), 'B'),
            (lambda: dev(qpsk, buf, 2, 20, buf, False, 4, 4, d_step=buf, sps=9), '1 <= sps <= 8'),
            (lambda: dev(qpsk, buf, 2, 20, buf, False, 4, 4, d_step=buf, eps=-1.0), 'eps >= 0'),
            (lambda: dev(Duck(6), buf, 2, 20, buf, False, 4, 4, d_step=buf, want='bits'), 'power of two'),
            (lambda: dev(qpsk, buf, 2, 20, buf, False, 4, 4, d_step=buf, want='llr'), 'want')):
        with pytest.raises(ValueError) as err:
            bad()
        assert limit in str(err.value), (limit, str(err.value))


def c_call(lib, md, device_form, **over):
    """One call of the C-ABI with host pointers that are never read: every limit is checked before them."""
    one = (ctypes.c_double * 1)(0.5)
    a = dict(B=2, n_y=20, n=20, sps=1, training=None, tr_batched=0, nt=0, nf=4, nb=0, delay=0, algorithm=0, step=one, step_batched=0,
             forgetting=None, fg_batched=0, delta=None, dl_batched=0, eps=1e-6, indices=ctypes.c_void_p(8))
    a.update(over)
    args = [md, None, a['B'], a['n_y'], a['n'], a['sps'], a['training'], a['tr_batched'], a['nt'], a['nf'], a['nb'], a['delay'],
            a['algorithm'], a['step'], a['step_batched'], a['forgetting'], a['fg_batched'], a['delta'], a['dl_batched'], a['eps'], None, 0,
            None, 0, a['indices'], a.get('bits'), None, None, None, None]
    rc = (lib.cpx_adaptive_equalize_dev(*args, None) if device_form else lib.cpx_adaptive_equalize(*args))
    return rc, _lib.last_error()


def test_c_abi_refuses_before_a_device_is_looked_for():
    """Every limit, in both forms, on a stand-in for the modem handle whose first two ints are M and the bits per symbol: the shared
    check reads nothing else of it, and returns before any pointer is followed."""
    lib = _lib.load()
    qpsk, six = (ctypes.c_int * 64)(4, 2), (ctypes.c_int * 64)(6, 2)
    val = lambda v: (ctypes.c_double * 2)(v, 0.5)
    for device_form in (False, True):
        rc, msg = c_call(lib, None, device_form)
        assert rc == _lib.CPX_EINVAL and msg == "adaptive_equalize: null pointer"
        cases = [(dict(B=-1), 'B = -1'), (dict(algorithm=3), 'algorithm = 3'), (dict(nf=0), '1 <= nf <= 64'), (dict(nf=65), '1 <= nf <= 64'),
                 (dict(nb=-1), '0 <= nb <= 64'), (dict(nb=65), '0 <= nb <= 64'),
                 (dict(algorithm=2, step=None, forgetting=val(1.0), delta=val(0.01), nf=30, nb=3), 'nf + nb <= 32'),
                 (dict(delay=-1), '0 <= delay'), (dict(sps=0), '1 <= sps <= 8'), (dict(sps=9), '1 <= sps <= 8'),
                 (dict(n=0), '1 <= n <= 2^30'), (dict(n=2 ** 30 + 1), '1 <= n <= 2^30'), (dict(n_y=-1), '0 <= n_y'),
                 (dict(nt=21), '0 <= nt <= n'), (dict(nt=-1), '0 <= nt <= n'), (dict(step=None), 'step is required'),
                 (dict(algorithm=2, forgetting=val(1.0), delta=val(0.01)), "step is given with 'rls'"),
                 (dict(algorithm=2, step=None, delta=val(0.01)), 'forgetting and delta are required'),
                 (dict(algorithm=2, step=None, forgetting=val(1.0)), 'forgetting and delta are required'),
                 (dict(algorithm=1, eps=-1.0), 'eps >= 0'), (dict(indices=None), 'no output requested')]
        if not device_form:                                    # values the host form can read
            cases += [(dict(step=val(0.0)), 'step > 0'), (dict(step=(ctypes.c_double * 2)(0.5, -1.0), step_batched=1), 'step > 0'),
                      (dict(algorithm=2, step=None, forgetting=val(1.5), delta=val(0.01)), '0 < forgetting <= 1'),
                      (dict(algorithm=2, step=None, forgetting=val(0.0), delta=val(0.01)), '0 < forgetting <= 1'),
                      (dict(algorithm=2, step=None, forgetting=val(1.0), delta=val(0.0)), 'delta > 0')]
        for over, limit in cases:
            rc, msg = c_call(lib, qpsk, device_form, **over)
            assert rc == _lib.CPX_EINVAL and limit in msg, (device_form, over, msg)
        rc, msg = c_call(lib, ctypes.cast(six, ctypes.c_void_p), device_form, bits=ctypes.c_void_p(8))
        assert rc == _lib.CPX_EINVAL and 'power of two' in msg
        for M in (1, 257):
            rc, msg = c_call(lib, (ctypes.c_int * 64)(M, 1), device_form)
            assert rc == _lib.CPX_EINVAL and '2 <= M <= 256' in msg


def test_fails_loudly_without_a_device():
    if _lib.device_count() == 0:
        with pytest.raises(_lib.EngineError):
            adaptive_equalize_batch(np.zeros((2, 11), complex), PSKModem(2), np.zeros(3, int), 4, step=0.1)
