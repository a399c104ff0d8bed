"""DeviceMimoLink's argument and plan logic, and its link_performance stop rule, without a device: the transmission size is
rounded like LinkModel._prepare, every refusal is a ValueError raised before the engine is even loaded, and the batched stop
rule equals the reference's one-transmission-at-a-time rule (links.py:269-343) for integer and float send_max."""
from fractions import Fraction

import numpy as np
import pytest

from commpy_amd import devicelink
from commpy_amd.channels import MIMOFlatChannel
from commpy_amd.devicelink import DeviceMimoLink, _fading_matrices, _sequential_ber, mimo_channel_gpu
from commpy_amd.links import LinkModel
from commpy_amd.modulation import QAMModem
from helpers import ldpc_params


def _chan(nr=4, nt=4, kind=complex):
    ch = MIMOFlatChannel(nt, nr)
    ch.uncorr_rayleigh_fading(kind)
    return ch


@pytest.fixture
def no_engine(monkeypatch):
    """Any use of the engine fails the test: refusals must come first."""
    def refuse():
        raise AssertionError('the engine was loaded before the arguments were checked')
    monkeypatch.setattr(devicelink._lib, 'load', refuse)
    monkeypatch.setattr(devicelink._lib, 'require_device', refuse)


def _plan(modem, channel, **kw):
    """The plan DeviceMimoLink computes, with the device part of the constructor skipped."""
    link = DeviceMimoLink.__new__(DeviceMimoLink)
    link.modem, link.channel = modem, channel
    link.K = int(kw.pop('K', 16))
    link._plan(kw.pop('detector', 'kbest'), kw.pop('output_type', 'hard'), kw.pop('stack_size', (1, 3, 5)),
               kw.pop('ldpc_params', None), kw.pop('ldpc_alg', 'MSA'), kw.pop('send_chunk', 720))
    assert not kw
    return link


@pytest.mark.parametrize("m,nt,nr,chunk", [(16, 4, 4, 720), (4, 2, 3, 100), (64, 3, 3, 1000), (16, 4, 4, 5), (4, 1, 2, 7)])
def test_uncoded_chunk_rounds_like_link_model(m, nt, nr, chunk):
    md, ch = QAMModem(m), _chan(nr, nt)
    host = LinkModel(md.modulate, ch, None, md.num_bits_symbol, md.constellation, md.Es)
    want, _ = host._prepare(chunk, 200, 1)
    link = _plan(md, ch, send_chunk=chunk)
    assert link.send_chunk == want
    assert link.tx_bits == want and link.vectors_per_tx * nt * md.num_bits_symbol == want
    assert link.rate == 1


def test_coded_plan():
    md, ldpc = QAMModem(16), ldpc_params("wimax1440")
    ch = _chan()
    host = LinkModel(md.modulate, ch, None, md.num_bits_symbol, md.constellation, md.Es, None, 0.5)
    want, _ = host._prepare(1440, 200, 0.5)
    link = _plan(md, ch, detector='best_first', ldpc_params=ldpc, send_chunk=1440)
    assert link.send_chunk == want == 1440
    assert link.rate == Fraction(1, 2) and (link.k, link.n) == (720, 1440)
    assert link.codewords_per_tx == 2 and link.tx_bits == 2880 and link.vectors_per_tx == 180
    link = _plan(md, ch, detector='kbest', output_type='soft', ldpc_params=ldpc)
    assert link.vectors_per_tx == 90
    assert math_isclose(link.noise_std(17.0), np.sqrt(2 * 4 * md.Es / (0.5 * 10 ** 1.7)))


def math_isclose(a, b):
    return abs(a - b) <= 1e-12 * abs(b)


def test_default_batch_aims_at_a_million_vectors():
    link = _plan(QAMModem(16), _chan())
    link.tx_batch = max(1, devicelink._VECTORS_PER_LAUNCH // link.vectors_per_tx)
    assert 2 ** 18 <= link.tx_batch * link.vectors_per_tx <= 2 ** 20


REFUSED = [
    dict(detector='ml', output_type='soft'),
    dict(detector='kbest', output_type='soft'),                       # soft output without a code
    dict(detector='best_first'),                                       # ... likewise
    dict(detector='viterbi'),
    dict(detector='kbest', output_type='hard', ldpc=True),             # hard output into a decoder
    dict(detector='ml', ldpc=True),
    dict(detector='kbest', nr=3, nt=4),                                # K-best: more columns than rows
    dict(detector='kbest', K=0),
    dict(detector='ml', m=256, nr=4, nt=4),                            # 2^32 hypotheses
    dict(detector='best_first', ldpc=True, nr=1, nt=1),                # best-first: one antenna
    dict(detector='best_first', ldpc=True, nr=4, nt=3),                # more rows than columns
    dict(detector='best_first', ldpc=True, nr=3, nt=4),                # fewer LLRs than bits
    dict(detector='best_first', ldpc=True, stack_size=(1, 0, 5)),
    dict(detector='kbest', output_type='soft', ldpc=True, send_chunk=1000),   # not whole LDPC messages
    dict(detector='kbest', kind=float),                                # real channel
    dict(detector='kbest', ldpc=True, output_type='soft', ldpc_alg='BP'),
]


@pytest.mark.parametrize("case", REFUSED, ids=[str(i) for i in range(len(REFUSED))])
def test_refusals_come_before_the_engine(no_engine, case):
    case = dict(case)
    md = QAMModem(case.pop('m', 16))
    ch = _chan(case.pop('nr', 4), case.pop('nt', 4), case.pop('kind', complex))
    if case.pop('ldpc', False):
        case['ldpc_params'] = ldpc_params("wimax1440")
    with pytest.raises(ValueError):
        DeviceMimoLink(md, ch, **case)


def test_channel_refusals_come_before_the_engine(no_engine):
    md = QAMModem(16)
    ch = _chan()
    ch.noise_std = 0.1
    with pytest.raises(ValueError):
        mimo_channel_gpu(ch, md, np.zeros(17, np.uint8))
    real = _chan(kind=float)
    real.noise_std = 0.1
    with pytest.raises(ValueError):
        mimo_channel_gpu(real, md, np.zeros(16, np.uint8))
    with pytest.raises(ValueError):
        DeviceMimoLink(md, object())


def test_fading_matrices_are_propagates():
    from scipy.linalg import sqrtm
    ch = _chan(3, 2)
    a, bt, mean = _fading_matrices(ch)
    assert np.array_equal(a, np.eye(3)) and np.array_equal(bt, np.eye(2))   # the kernel then skips both products
    assert mean.shape == (3, 2) and not mean.any()
    ch.expo_corr_rician_fading(np.ones((3, 2), complex), 3.0, np.exp(0.4j), np.exp(0.1j), 0.2, 0.1)
    mean0, rt, rr = ch.fading_param
    a, bt, mean = _fading_matrices(ch)
    assert np.array_equal(a, sqrtm(rr)) and np.array_equal(bt, sqrtm(rt).T) and np.array_equal(mean, mean0)
    for arr in (a, bt, mean):
        assert arr.dtype == np.complex128 and arr.flags.c_contiguous


# ---- the stop rule -----------------------------------------------------------------------------------------------------------

def _reference_rule(counts, n_snr, send_max, err_min, chunk):
    """links.py:269-343, one transmission at a time: `counts[i]` is what SNR point i's transmissions produce, in order."""
    out = np.zeros(n_snr)
    for i in range(n_snr):
        it = iter(counts[i])
        sent = wrong = 0
        while sent < send_max and wrong < err_min:
            wrong += next(it)
            sent += chunk
        out[i] = wrong / sent
        if wrong < err_min:
            break
    return out


@pytest.mark.parametrize("send_max", [5e5, 500000, 7200.0, 7201, 719])
@pytest.mark.parametrize("tx_batch", [1, 7, 64, 100000])
def test_stop_rule_matches_the_reference(send_max, tx_batch):
    rs = np.random.RandomState(int(send_max) % 1000 + tx_batch)
    rates = [40.0, 3.0, 0.4, 0.05, 2.0]                                    # errors per transmission by point
    counts = [list(rs.poisson(r, 20000)) for r in rates]
    pos = [0] * len(rates)
    snrs = np.arange(len(rates), dtype=float)

    def run(snr, T):
        i = int(snr)
        out = counts[i][pos[i]:pos[i] + T]
        pos[i] += T
        return np.array(out, np.int32)
    got = _sequential_ber(snrs, send_max, 200, 720, tx_batch, run)
    want = _reference_rule(counts, len(rates), send_max, 200, 720)
    assert np.array_equal(got, want)
    assert got[0] > 0


def test_float_send_max_of_the_reference_tests():
    counts = [list(np.full(1000, 0))]
    got = _sequential_ber([0.0], 5e5, 200, 720, 64, lambda snr, T: np.zeros(T, np.int32))
    assert np.array_equal(got, _reference_rule(counts, 1, 5e5, 200, 720))
    with pytest.raises(ValueError):
        devicelink._whole(2.5)
    assert devicelink._whole(5e5) == 500000
