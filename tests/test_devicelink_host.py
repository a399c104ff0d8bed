"""The host side of commpy_amd.devicelink without a device: DeviceWifiLink's plan (sizes and index maps against the host
puncturing / depuncturing), the Viterbi call geometry against the expressions the links used to spell out, the fixed-budget sweep
rule against the loop both links used to carry, and the bookkeeping of buffer sets and one-shot allocations."""
import math

import numpy as np
import pytest

from commpy_amd import devicelink, deviceops
from commpy_amd.channelcoding.convcode import depuncturing, puncturing
from commpy_amd.channels import SISOFlatChannel
from commpy_amd.devicelink import DeviceWifiLink, _buffer_set, _fixed_budget_ber, _viterbi_geometry
from commpy_amd.links import LinkModel
from commpy_amd.wifi80211 import Wifi80211


def _plan(mcs, send_chunk=600, frame_aggregation=1, generator_matrix=None):
    """The plan DeviceWifiLink computes, with the device part of the constructor skipped."""
    link = DeviceWifiLink.__new__(DeviceWifiLink)
    link._plan(mcs, send_chunk, frame_aggregation, generator_matrix)
    return link


# ---- DeviceWifiLink's plan ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mcs", range(10))
@pytest.mark.parametrize("chunk,agg", [(600, 1), (1001, 1), (100, 3)])       # 1001 and 100 are rounded down for most codings
def test_wifi_plan_sizes_follow_the_host_chain(mcs, chunk, agg):
    link = _plan(mcs, chunk, agg, [[0o133, 0o171]])
    nb = link.modem.num_bits_symbol
    num, den = link.coding
    host = LinkModel(link.modem.modulate, SISOFlatChannel(fading_param=(1 + 0j, 0j)), None, nb, link.modem.constellation, link.modem.Es)
    assert link.send_chunk == host._prepare(chunk, 200, link.rate)[0]                      # links.py:203-214
    assert link.nbits == link.send_chunk * agg and link.ncoded == 2 * link.nbits
    pvec = Wifi80211._get_puncture_matrix(num, den)
    coded = np.random.RandomState(mcs).randint(0, 2, link.ncoded)
    if pvec is None:
        assert link.keep_idx is None and link.de_idx is None
        assert link.ntx == link.nde == link.ncoded
    else:
        sent = puncturing(coded, pvec)
        assert link.ntx == len(sent) and np.array_equal(coded[link.keep_idx], sent)
        assert link.nde == math.ceil(link.ntx * num / den * 2)                             # wifi80211.py's `shouldbe`
        ramp = np.arange(1.0, link.ntx + 1)
        want = depuncturing(ramp, pvec, link.nde)
        assert len(link.de_idx) == link.nde
        assert np.array_equal(np.where(link.de_idx >= 0, ramp[np.maximum(link.de_idx, 0)], 0.0), want)
    assert link.nsym * nb == link.ntx
    assert link.nde == link.ncoded                                                         # the decoder sees the mother code's length


def test_wifi_plan_rounds_a_chunk_that_needs_it():
    assert _plan(6, 600).send_chunk == 594                      # 64-QAM rate 3/4: frames of 9 information bits
    assert _plan(6, 5).send_chunk == 9                          # never below one such frame
    assert _plan(5, 1001).send_chunk == 1000


def test_wifi_plan_refuses_a_partial_symbol(monkeypatch):
    """A puncturing pattern the chunk rounding does not know of leaves 3 bits for a 4-bit symbol: ValueError, before any device."""
    def refuse():
        raise AssertionError('the engine was loaded before the arguments were checked')
    monkeypatch.setattr(devicelink._lib, 'load', refuse)
    monkeypatch.setattr(devicelink._lib, 'require_device', refuse)
    monkeypatch.setattr(Wifi80211, '_get_puncture_matrix', staticmethod(lambda numerator, denominator: [1, 1, 1, 0]))
    with pytest.raises(ValueError, match='integer number of symbols'):
        DeviceWifiLink(3, 2)


def test_wifi_noise_std_is_channels_py_74():
    link = _plan(5, 1200)
    for snr in (0.0, 13.5, np.float64(17.0), 20):
        assert link.noise_std(snr) == math.sqrt(2.0 * link.modem.Es / (link.rate * 10 ** (float(snr) / 10.0)))


# ---- the Viterbi call geometry ----------------------------------------------------------------------------------------------------

class _Tr:
    def __init__(self, k, n, m):
        self.k, self.n, self.total_memory = k, n, m


@pytest.mark.parametrize("m", [1, 2, 3, 6, 8])
def test_geometry_equals_the_expressions_it_replaces(m):
    for length in list(range(0, 260)) + [1199, 1200, 2399, 2400, 4801, 10 ** 6 + 1, 2 ** 31 + 3]:
        # DeviceWifiLink.run_batch / ber_sweep_batched: the rate-1/2 mother code
        L = int(length * 0.5)
        n_steps = int((L + m) / 1) - 1
        assert _viterbi_geometry(length, _Tr(1, 2, m)) == (L, n_steps, min(5 * m, L))
        # DeviceBscLink.__init__: any k = 1 code, given or default traceback depth
        for n in (2, 3, 4, 5, 7):
            tr = _Tr(1, n, m)
            L = int(length * tr.k / tr.n)
            n_steps = int((L + m) / tr.k) - 1
            assert _viterbi_geometry(length, tr, None) == (L, n_steps, min(5 * m, L))
            assert _viterbi_geometry(length, tr, 7.0) == (L, n_steps, 7)


# ---- the fixed-budget sweep ---------------------------------------------------------------------------------------------------------

def _old_loop(snrs_db, n_bits, bits_per_tx, tx_batch, run):
    """The loop DeviceWifiLink.ber_sweep and DeviceMimoLink.ber_sweep each carried."""
    out = []
    for snr in snrs_db:
        done, errs = 0, 0
        while done < n_bits:
            T = int(min(tx_batch, math.ceil((n_bits - done) / bits_per_tx)))
            e = run(float(snr), T)
            errs += int(e.sum())
            done += T * bits_per_tx
        out.append(errs / done)
    return np.array(out)


@pytest.mark.parametrize("n_bits", [1, 719, 720, 721, 50000, 1e5, 123456.5])
@pytest.mark.parametrize("tx_batch", [1, 7, 64, 4096])
def test_fixed_budget_sweep_equals_the_old_loop(n_bits, tx_batch):
    def recorder():
        rs, asked = np.random.RandomState(5), []

        def run(snr, T):
            assert type(snr) is float and type(T) is int
            asked.append((snr, T))
            return rs.poisson(30.0 / (1.0 + snr), (T, 2)).astype(np.int32)
        return run, asked
    snrs = np.array([0.0, 3.0, 6.5])
    run_new, asked_new = recorder()
    run_old, asked_old = recorder()
    got = _fixed_budget_ber(snrs, n_bits, 720, tx_batch, run_new)
    want = _old_loop(snrs, n_bits, 720, tx_batch, run_old)
    assert asked_new == asked_old and len(asked_new) >= 3
    assert got.dtype == want.dtype and np.array_equal(got, want) and got[0] > 0


def test_both_links_sweep_through_the_shared_rule(monkeypatch):
    calls = []
    monkeypatch.setattr(devicelink, '_fixed_budget_ber', lambda *a: calls.append(a) or 'ber')
    wifi = _plan(5, 1200, 2)
    assert wifi.ber_sweep([1.0], 5000, tx_batch=9) == 'ber' and wifi.ber_sweep([1.0], 5000) == 'ber'
    assert calls[0] == ([1.0], 5000, 2400, 9, wifi.run_batch) and calls[1][3] == 4096
    mimo = devicelink.DeviceMimoLink.__new__(devicelink.DeviceMimoLink)
    mimo.send_chunk, mimo.tx_batch = 720, 364
    assert mimo.ber_sweep([2.0], 1e4) == 'ber' and mimo.ber_sweep([2.0], 1e4, tx_batch=0) == 'ber'
    assert calls[2] == ([2.0], 1e4, 720, 364, mimo.run_batch) and calls[3][3] == 1
    with pytest.raises(ValueError):
        mimo.ber_sweep([2.0], 1e4, tx_batch=2.5)


# ---- buffer sets and one-shot allocations ---------------------------------------------------------------------------------------------

class _FakeBuf(deviceops.DeviceBuf):
    """A DeviceBuf that owns nothing: counts what would be allocated and freed."""
    live = 0

    def __init__(self, nbytes=0):
        self.nbytes, self.ptr = nbytes, True
        _FakeBuf.live += 1

    @classmethod
    def from_array(cls, arr):
        return cls(np.asarray(arr).nbytes)

    def free(self):
        if self.ptr:
            self.ptr = None
            _FakeBuf.live -= 1


def test_buffer_set_reuses_by_key_and_frees_the_old_set():
    _FakeBuf.live = 0
    link = type('Link', (), {'_bufs': {}})()
    first = _buffer_set(link, 8, lambda: {'a': _FakeBuf(), 'b': _FakeBuf()})
    assert _FakeBuf.live == 2 and link._bufs is first
    assert _buffer_set(link, 8, lambda: pytest.fail('same key: nothing is built')) is first
    second = _buffer_set(link, ('sweep', 8), lambda: {'a': _FakeBuf()})
    assert second is not first and link._bufs is second
    assert _FakeBuf.live == 1 and first['a'].ptr is None and first['b'].ptr is None
    assert _buffer_set(link, ('sweep', 8), lambda: pytest.fail('same key')) is second


def test_bsc_link_frees_its_previous_buffers(monkeypatch):
    monkeypatch.setattr(devicelink, 'DeviceBuf', _FakeBuf)
    _FakeBuf.live = 0
    link = devicelink.DeviceBscLink.__new__(devicelink.DeviceBscLink)
    link.nbits, link.ncoded, link.L, link._bufs = 64, 132, 66, {}
    a = link.buffers(10)
    assert link.buffers(10) is a and _FakeBuf.live == 5 and {'msg', 'coded', 'rx', 'dec', 'errs'} <= set(a)
    b = link.buffers(20)
    assert b is not a and _FakeBuf.live == 5 and a['rx'].ptr is None and b['rx'].nbytes == 20 * 132 * 8


def test_one_shot_frees_on_return_and_on_error(monkeypatch):
    monkeypatch.setattr(deviceops, 'DeviceBuf', _FakeBuf)
    monkeypatch.setattr(deviceops._lib, 'load', lambda: None)
    _FakeBuf.live = 0
    with deviceops._OneShot() as dev:
        dev.upload(np.zeros(4, np.uint8))
        out = dev.alloc(16)
        assert _FakeBuf.live == 2 and out.nbytes == 16
    assert _FakeBuf.live == 0
    with pytest.raises(RuntimeError):
        with deviceops._OneShot() as dev:
            dev.alloc(8)
            raise RuntimeError('the engine refused the call')
    assert _FakeBuf.live == 0
