"""Tail-biting convolutional codes without a GPU: the NumPy model tests/tbcc_model.py against brute force over every tail-biting code
word, the model's own arithmetic (its fused multiply-add, its 'soft' metric against the plain formula), the outcome classes of the
rule, and the host-side refusals (ValueError / CPX_EINVAL before any device is touched).

The rule is not maximum likelihood: how often it equals brute force is a property of the inputs, so the seeds below are chosen, and
the share is asserted: at most 5 % of the rows of a case may differ."""
import ctypes
import ctypes.util

import numpy as np
import pytest

import tbcc_model as M
from commpy_amd import _lib, deviceops
from commpy_amd.channelcoding import Trellis, tailbiting_decode, tailbiting_encode

T57, ROWS, MAX_WRAPS = 10, 150, 4


def code57():
    return Trellis(np.array([2]), np.array([[5, 7]]))


def lte_code():
    return Trellis(np.array([6]), np.array([[0o133, 0o171, 0o165]]))


def bpsk_llr(words, ebn0_db, rate, rs):
    """BPSK over AWGN at Eb/N0: LLRs log P1/P0 of the code bits."""
    sigma = np.sqrt(1.0 / (2.0 * rate * 10.0 ** (ebn0_db / 10.0)))
    y = (2.0 * words - 1.0) + sigma * rs.randn(*words.shape)
    return 2.0 * y / sigma ** 2


def outcome_classes(res, max_wraps):
    """Which of the rule's four ways to finish occur: one trip, an early stop after more than one, the remembered candidate, none."""
    return {'one trip': bool((res['wraps'] == 1).any()),
            'between': bool(((res['wraps'] > 1) & (res['wraps'] < max_wraps)).any()),
            'candidate': bool((res['outcome'] == M.OUTCOME_CANDIDATE).any()),
            'open': bool((res['tailbiting'][res['wraps'] > 0] == 0).any())}


@pytest.fixture(scope="module")
def every_word():
    return M.all_codewords(code57(), T57)


# ---- the model's arithmetic ---------------------------------------------------------------------------------------------------------
def test_model_fma_is_the_c_librarys():
    libm = ctypes.CDLL(ctypes.util.find_library("m"))
    libm.fma.restype, libm.fma.argtypes = ctypes.c_double, [ctypes.c_double] * 3
    rs = np.random.RandomState(0)
    a, b = rs.randn(20000) * np.exp(5 * rs.randn(20000)), rs.randn(20000)
    c = rs.randn(20000) * np.exp(5 * rs.randn(20000))
    c[:8000] = -(a[:8000] * b[:8000]) * (1 + 1e-10 * rs.randn(8000))          # cancellation: the product's low part decides
    c[8000:9000] = -(a[8000:9000] * b[8000:9000])
    want = np.array([libm.fma(x, y, z) for x, y, z in zip(a, b, c)])
    assert np.array_equal(M.fma(a, b, c), want)


def test_model_soft_metric_against_the_plain_formula():
    """exp below 1 ulp on either side, the sum's rounding, the logarithm below 1 ulp on either side: an error of a few 2^-53 relative
    to exp(r) + 1 >= 1, which moves its logarithm by as much in absolute terms -- bounded here by 4 * 2^-52 * max(1, log)."""
    rs = np.random.RandomState(1)
    r = np.concatenate([np.linspace(-500.0, 500.0, 200001), 10.0 * rs.randn(100000), [0.0, -0.0, 36.7, -36.7, 500.0, -500.0]])
    got, ref = M.soft_nll0(r), np.log(np.exp(r) + 1.0)
    assert np.all(np.abs(got - ref) <= 4 * 2.0 ** -52 * np.maximum(1.0, ref))
    assert np.mean(got == ref) > 0.9 and np.array_equal(M.soft_nll0(np.array([-500.0, -40.0])), [0.0, 0.0])


# ---- against brute force ------------------------------------------------------------------------------------------------------------
def brute_force_case(kind, seed, every_word):
    tr = code57()
    rs = np.random.RandomState(seed)
    msg = rs.randint(0, 2, (ROWS, T57))
    sent, closed = M.encode_batch(msg, tr)
    assert closed.all()
    if kind == 'hard':
        rx, dtype = (sent ^ (rs.rand(*sent.shape) < 0.08)).astype(float), 'hard'
    else:
        rx, dtype = bpsk_llr(sent, kind, 0.5, rs), 'soft'
    res = M.decode_batch(rx, tr, dtype, MAX_WRAPS)
    low = M.brute_force_minimum(rx, every_word[1], dtype)
    again, closes = M.encode_batch(res['bits'], tr)
    assert closes.all()
    direct = M.direct_metric(again, rx, dtype)
    tol = np.zeros(ROWS) if dtype == 'hard' else T57 * tr.n * 2.0 ** -52 * res['mmax']
    return res, low, direct, tol


@pytest.mark.parametrize("kind, seed, differing", [(0.0, 6, 2), (3.0, 3, 1), ('hard', 3, 2)])
def test_model_against_brute_force(every_word, kind, seed, differing):
    """(5, 7), T = 10, 150 rows: 'soft' at Eb/N0 = 0 and 3 dB, 'hard' with 8 % of the bits flipped, against all 2^10 code words."""
    assert every_word[1].shape == (1 << T57, 2 * T57)
    res, low, direct, tol = brute_force_case(kind, seed, every_word)
    tb = res['tailbiting'] == 1
    assert (res['wraps'] >= 1).all() and (res['wraps'] <= MAX_WRAPS).all()
    # a path that tail-bites is a code word, and its metric is that code word's
    if kind == 'hard':
        assert np.array_equal(res['metric'][tb], direct[tb])
    else:
        assert (np.abs(res['metric'] - direct)[tb] <= tol[tb]).all()
    assert (res['metric'][tb] >= low[tb] - tol[tb]).all()                      # never below the best code word
    assert (direct >= low - tol).all()
    differ = direct > low + tol                                                # the returned bits are not a best code word
    assert differ.sum() == differing and differ.sum() <= 0.05 * ROWS
    assert all(outcome_classes(res, MAX_WRAPS).values()), outcome_classes(res, MAX_WRAPS)
    assert (res['outcome'][~tb] == M.OUTCOME_OPEN).all() and (res['wraps'][res['outcome'] != M.OUTCOME_CLOSED] == MAX_WRAPS).all()


def test_model_on_the_lte_code():
    """(133, 171, 165), T = 40, 0 dB: every outcome class in 40 rows; noise-free rows stop after one trip with the message."""
    tr = lte_code()
    rs = np.random.RandomState(4)
    msg = rs.randint(0, 2, (40, 40))
    sent, closed = M.encode_batch(msg, tr)
    assert closed.all()
    res = M.decode_batch(bpsk_llr(sent, 0.0, 1.0 / 3.0, rs), tr, 'soft', MAX_WRAPS)
    assert all(outcome_classes(res, MAX_WRAPS).values()) and (res['outcome'] == M.OUTCOME_OPEN).sum() == 1
    for dtype, rx in (('unquantized', 2.0 * sent - 1.0), ('hard', sent.astype(float)), ('soft', 20.0 * (2.0 * sent - 1.0))):
        clean = M.decode_batch(rx, tr, dtype, MAX_WRAPS)
        assert (clean['wraps'] == 1).all() and (clean['tailbiting'] == 1).all() and np.array_equal(clean['bits'], msg)
        assert dtype == 'soft' or not clean['metric'].any()


def test_model_rejects_rows_and_encodes_like_two_walks():
    tr = code57()
    rs = np.random.RandomState(2)
    msg = rs.randint(0, 2, (6, T57))
    sent, _ = M.encode_batch(msg, tr)
    nxt, out = tr.next_state_table, tr.output_table
    for row, word in zip(msg, sent):                                           # the encoder, one bit at a time
        st = 0
        for u in row:
            st = nxt[st, u]
        first, bits = st, []
        for u in row:
            bits += [(out[st, u] >> 1) & 1, out[st, u] & 1]
            st = nxt[st, u]
        assert st == first and bits == word.tolist()
    rx = sent.astype(float)
    rx[1, 3], rx[3, 0], rx[4, 19] = np.nan, np.inf, -np.inf
    hard = M.decode_batch(rx, tr, 'hard', MAX_WRAPS)
    assert hard['wraps'].tolist() == [1, 0, 1, 0, 0, 1] and np.isnan(hard['metric'][[1, 3, 4]]).all()
    assert not hard['bits'][[1, 3, 4]].any() and np.array_equal(hard['bits'][[0, 2, 5]], msg[[0, 2, 5]])
    soft = M.decode_batch(rx, tr, 'soft', MAX_WRAPS)                           # an infinite LLR is clipped, not rejected
    assert soft['wraps'][1] == 0 and soft['wraps'][3] > 0 and soft['wraps'][4] > 0
    # a message shorter than the memory, and a recursive trellis, do not close
    assert not M.encode_batch(np.array([[1]]), tr)[1][0]
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        rsc = Trellis(np.array([2]), np.array([[1, 7]]), 5, "rsc")
    assert not M.encode_batch(rs.randint(0, 2, (64, 12)), rsc)[1].all()


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def no_device(monkeypatch):
    """Any attempt to load the engine fails the test: the refusals below must come from the host-side checks."""
    def boom(*a, **k):
        raise AssertionError("the engine was touched")
    monkeypatch.setattr(_lib, "load", boom)


def test_python_refusals(no_device):
    tr = code57()
    k2 = Trellis(np.array([1, 1]), np.array([[1, 0, 3], [0, 1, 2]]))
    table = lambda S, k, n: Trellis.from_tables(k, n, 0, np.zeros((S, 1 << k), int), np.zeros((S, 1 << k), int))
    ok, okx = np.zeros((2, 10), np.uint8), np.zeros((2, 20))
    buf = object()
    for bad, limit in (
            (lambda: tailbiting_encode(np.full((2, 10), 2), tr), '0 / 1'),
            (lambda: tailbiting_encode(np.full((2, 10), -1), tr), '0 / 1'),
            (lambda: tailbiting_encode(np.zeros((2, 10)), tr), 'integers'),
            (lambda: tailbiting_encode(np.zeros((2, 0), int), tr), 'T >= 1'),
            (lambda: tailbiting_encode(np.zeros((2, 3), int), k2), 'multiple of 2'),
            (lambda: tailbiting_encode(np.zeros((1, 8193), int), tr), 'T * k <= 8192'),
            (lambda: tailbiting_encode(np.zeros((1, 8194), int), k2), 'T * k <= 8192'),
            (lambda: tailbiting_encode(np.zeros((1, 2, 5), int), tr), '1-D or 2-D'),
            (lambda: tailbiting_encode(ok, table(128, 1, 2)), 'power of two from 2 to 64'),
            (lambda: tailbiting_encode(ok, table(1, 1, 2)), 'power of two from 2 to 64'),
            (lambda: tailbiting_encode(ok, table(24, 1, 2)), 'power of two from 2 to 64'),
            (lambda: tailbiting_encode(ok, table(4, 3, 4)), 'k <= 2'),
            (lambda: tailbiting_encode(ok, table(4, 1, 7)), 'n <= 6'),
            (lambda: tailbiting_decode(okx, table(4, 1, 7)), 'n <= 6'),
            (lambda: tailbiting_decode(okx, table(128, 1, 2)), 'power of two from 2 to 64'),
            (lambda: tailbiting_decode(np.zeros((2, 21)), tr), 'multiple of 2'),
            (lambda: tailbiting_decode(np.zeros((2, 0)), tr), 'T >= 1'),
            (lambda: tailbiting_decode(np.zeros((1, 2 * 8193)), tr), 'T * k <= 8192'),
            (lambda: tailbiting_decode(okx, tr, 'fuzzy'), 'decoding types'),
            (lambda: tailbiting_decode(okx, tr, max_wraps=0), 'from 1 to 32'),
            (lambda: tailbiting_decode(okx, tr, max_wraps=33), 'from 1 to 32'),
            (lambda: tailbiting_decode(okx, tr, max_wraps=2.0), 'from 1 to 32'),
            (lambda: tailbiting_decode(okx, tr, max_wraps=True), 'from 1 to 32'),
            (lambda: tailbiting_decode(okx, tr, want=()), 'want'),
            (lambda: tailbiting_decode(okx, tr, want=('bits', 'trips')), 'want'),
            (lambda: deviceops.tailbiting_encode_dev(tr, buf, 2, 0), 'T'),
            (lambda: deviceops.tailbiting_encode_dev(tr, buf, -1, 10), 'B'),
            (lambda: deviceops.tailbiting_encode_dev(table(128, 1, 2), buf, 2, 10), 'power of two from 2 to 64'),
            (lambda: deviceops.tailbiting_decode_dev(tr, buf, 2, 8193), 'T * k <= 8192'),
            (lambda: deviceops.tailbiting_decode_dev(tr, buf, 2, 10, max_wraps=40), 'from 1 to 32'),
            (lambda: deviceops.tailbiting_decode_dev(tr, buf, 2, 10, 'fuzzy'), 'decoding types'),
            (lambda: deviceops.tailbiting_decode_dev(tr, buf, 2, 10, want='origin'), 'want')):
        with pytest.raises(ValueError) as err:
            bad()
        assert limit in str(err.value), (limit, str(err.value))


def test_c_abi_refuses_null_pointers_before_a_device_is_looked_for():
    lib = _lib.load()
    assert lib.cpx_tbcc_encode(None, None, 2, 10, None, None) == _lib.CPX_EINVAL and _lib.last_error() == "tbcc_encode: null pointer"
    assert lib.cpx_tbcc_encode_dev(None, None, 2, 10, None, None, None) == _lib.CPX_EINVAL
    assert lib.cpx_tbcc_decode(None, None, 2, 10, 1, 4, None, None, None, None) == _lib.CPX_EINVAL
    assert _lib.last_error() == "tbcc_decode: null pointer"
    assert lib.cpx_tbcc_decode_dev(None, None, 2, 10, 1, 4, None, None, None, None, None) == _lib.CPX_EINVAL


def test_fails_loudly_without_a_device():
    if _lib.device_count() > 0:
        pytest.skip("a HIP device is present")
    with pytest.raises(_lib.EngineError):
        tailbiting_encode(np.zeros((2, 10), int), code57())
    with pytest.raises(_lib.EngineError):
        tailbiting_decode(np.zeros((2, 20)), code57())
