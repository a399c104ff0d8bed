"""The polar codec on the GPU against tests/polar_model.py: every comparison is exact (``array_equal``), for the encoder, successive
cancellation and list decoding, at the sizes where the kernels change their path -- one word (N < 64), lanes and two words per lane in
the encoder; levels on one wave and on four, one and several paths per wave in the decoder."""
import ctypes

import numpy as np
import pytest

import polar_model as M
from commpy_amd import _lib, deviceops
from commpy_amd.channelcoding import PolarCode, polar_decode, polar_encode
from commpy_amd.deviceops import DeviceBuf
from test_polar_host import CRCS, MODEL_BLOCK_ERRORS, block_errors

pytestmark = pytest.mark.gpu
EVERYTHING = ("bits", "crc", "metric", "list")


def gaussian(seed, B, code, ebn0_db=2.0):
    return M.awgn_llrs(seed, code.frozen, code.crc, B, ebn0_db)[1]


def check_decode(code, llr, L):
    """Every output of the engine against the model, word by word."""
    want = EVERYTHING + (("u_llr",) if L == 1 else ())
    got = dict(zip([w for w in ("bits", "crc", "metric", "u_llr", "list") if w in want], polar_decode(llr, code, L, want=want)))
    ref = M.decode_batch(llr, code.frozen, L, code.crc)
    what = (code.N, code.K, code.crc, L)
    assert got["bits"].dtype == np.uint8 and np.array_equal(got["bits"], ref["bits"]), what
    assert np.array_equal(got["crc"], ref["crc_ok"].astype(bool)), what
    assert np.array_equal(got["metric"], ref["metric"]), what
    lb, lm, live = got["list"]
    assert np.array_equal(live, ref["live"]) and live.dtype == np.int32, what
    assert np.array_equal(lm, ref["list_metric"]), what
    assert np.array_equal(lb, ref["list_bits"]), what
    if L == 1:
        assert np.array_equal(got["u_llr"], ref["u_llr"]), what
    return ref


# ---- encoder ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [2, 4, 64, 128, 1024, 8192])
def test_encoder(gpu, N):
    rs = np.random.RandomState(N)
    for K in (1, N // 2, N):
        for crc in (None,) + tuple(g for g in (0xB, CRCS[6], CRCS[24]) if g.bit_length() - 1 < K)[-1:]:
            code = PolarCode(N, K, crc=crc)
            for B in (1, 3, 67):
                msg = rs.randint(0, 2, (B, code.A)).astype(np.uint8)
                x = polar_encode(msg, code)
                assert x.dtype == np.uint8 and x.shape == (B, N)
                assert np.array_equal(x, np.stack([M.encode(m, code.frozen, crc) for m in msg])), (N, K, crc, B)
            assert np.array_equal(polar_encode(msg[0], code), x[0])
    assert _lib.last_kernel() == "polar_encode_kernel"
    fz = np.ones(N, np.uint8)
    fz[[0, N - 1]] = 0                                                             # a caller's mask
    code = PolarCode(N, 2, frozen=fz)
    assert np.array_equal(polar_encode([[1, 0], [1, 1], [0, 1]], code), np.stack([M.encode(m, fz) for m in ([1, 0], [1, 1], [0, 1])]))


# ---- successive cancellation --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [2, 4, 32, 64, 128, 256, 1024, 8192])
def test_sc(gpu, N):
    few = 2 if N == 8192 else 4
    half = PolarCode(N, max(N // 2, 1))
    check_decode(half, gaussian(N, few, half), 1)
    assert _lib.last_kernel() == "polar_decode_kernel<1>"
    if N == 8192:
        return
    if N >= 32:
        crc_code = PolarCode(N, N // 2, crc=CRCS[11])
        check_decode(crc_code, gaussian(N + 1, 3, crc_code), 1)
    rs = np.random.RandomState(N)
    for code in (PolarCode(N, 1), PolarCode(N, N), PolarCode(N, 2, frozen=np.r_[0, np.ones(N - 2, np.uint8), 0][:N] if N > 2 else [0, 0])):
        llr = np.concatenate([rs.randn(1, N) + 0.5, np.zeros((1, N)), M.sign_llrs(N, 2, N)])
        check_decode(code, llr, 1)


# ---- list decoding ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N, L", [(4, 2), (8, 8), (32, 4), (64, 32), (128, 8), (256, 32), (1024, 8)])
def test_scl(gpu, N, L):
    big = N * L >= 8192
    code = PolarCode(N, N // 2)
    check_decode(code, np.concatenate([gaussian(L, 1 if big else 3, code), M.sign_llrs(N + L, 1 if big else 3, N)]), L)
    assert _lib.last_kernel() == "polar_decode_kernel<%d>" % L
    if N >= 32:
        crc_code = PolarCode(N, N // 2, crc=CRCS[11])
        check_decode(crc_code, gaussian(L + 1, 2 if big else 6, crc_code, 1.5), L)
    if not big:
        for K in sorted({1, max(L.bit_length() - 2, 1), N}):                       # K < log2 L: fewer live paths than L, padded rows
            small = PolarCode(N, K)
            ref = check_decode(small, np.concatenate([gaussian(K, 2, small), np.zeros((1, N))]), L)
            assert np.all(ref["live"] == min(L, 2 ** K))


def test_crc_selects_a_later_rank_or_none(gpu):
    code = PolarCode(128, 64, crc=CRCS[11])
    llr = gaussian(21, 16, code, 1.5)
    ref = check_decode(code, llr, 8)
    rank0_fails = np.array([M.crc_syndrome(row[0], code.crc_table) != 0 for row in ref["list_bits"]])
    assert (rank0_fails & (ref["crc_ok"] == 1)).sum() >= 2 and (ref["crc_ok"] == 0).sum() >= 2       # both cases are in the set


def test_ties_keep_the_models_order(gpu):
    """+-1-valued LLRs: integer metrics, many exactly equal -- the list order is the stable one at every rank."""
    code = PolarCode(128, 64)
    llr = M.sign_llrs(5, 6, 128)
    ref = check_decode(code, llr, 8)
    assert (np.diff(ref["list_metric"], axis=1) == 0).sum() >= 6
    small = PolarCode(32, 16)
    ref = check_decode(small, M.sign_llrs(6, 6, 32), 32)
    assert (np.diff(ref["list_metric"], axis=1) == 0).sum() >= 20


# ---- layout independence --------------------------------------------------------------------------------------------------------------
def test_batch_position_and_requested_outputs_do_not_matter(gpu):
    code = PolarCode(128, 64, crc=CRCS[11])
    llr = gaussian(3, 67, code, 2.0)
    for L in (1, 8):
        full = polar_decode(llr, code, L, want=EVERYTHING)
        for i in (0, 33, 66):
            alone = polar_decode(llr[i], code, L, want=EVERYTHING)
            assert np.array_equal(alone[0], full[0][i]) and alone[1] == full[1][i] and alone[2] == full[2][i]
            assert all(np.array_equal(a, f[i]) for a, f in zip(alone[3], full[3]))
        assert np.array_equal(polar_decode(llr, code, L), full[0])
        assert np.array_equal(polar_decode(llr, code, L, want="crc"), full[1])
        m, (lb, lm, live) = polar_decode(llr, code, L, want=("list", "metric"))
        assert np.array_equal(m, full[2]) and np.array_equal(lb, full[3][0]) and np.array_equal(lm, full[3][1]) and np.array_equal(live, full[3][2])
    u_llr, bits = polar_decode(llr, code, 1, want=("u_llr", "bits"))[::-1]
    assert np.array_equal(bits, polar_decode(llr, code, 1)) and np.array_equal(u_llr, polar_decode(llr, code, 1, want="u_llr"))


def test_batch_larger_than_the_resident_grid(gpu):
    code = PolarCode(8, 4)
    words = np.random.RandomState(8).randn(7, 8)
    ref = M.decode_batch(words, code.frozen, 2)
    reps = 1200                                                                    # 8400 words: the grid holds 8 per compute unit
    bits, metric = polar_decode(np.tile(words, (reps, 1)), code, 2, want=("bits", "metric"))
    assert np.array_equal(bits, np.tile(ref["bits"], (reps, 1))) and np.array_equal(metric, np.tile(ref["metric"], reps))
    msg = np.random.RandomState(9).randint(0, 2, (7, 4)).astype(np.uint8)
    assert np.array_equal(polar_encode(np.tile(msg, (reps * 2, 1)), code), np.tile(polar_encode(msg, code), (reps * 2, 1)))


def test_streams_and_device_buffers(gpu):
    code = PolarCode(256, 128, crc=CRCS[11])
    lib = _lib.load()
    msg = np.random.RandomState(4).randint(0, 2, (5, code.A)).astype(np.uint8)
    llr = gaussian(4, 5, code)
    host = polar_decode(llr, code, 8, want=EVERYTHING)
    streams = [ctypes.c_void_p() for _ in range(2)]
    for s in streams:
        _lib.check(lib.cpx_stream_create(ctypes.byref(s)))
    try:
        d_msg, d_llr = DeviceBuf.from_array(msg), DeviceBuf.from_array(llr)
        outs = [(deviceops.polar_encode_dev(code, d_msg, 5, stream=s), deviceops.polar_decode_dev(code, d_llr, 5, 8, want=EVERYTHING, stream=s))
                for s in streams + [None]]
        for s in streams + [None]:
            _lib.check(lib.cpx_stream_sync(s))
        for d_x, (d_bits, d_crc, d_metric, (d_lb, d_lm, d_live)) in outs:
            assert np.array_equal(d_x.to_array((5, 256), np.uint8), polar_encode(msg, code))
            assert np.array_equal(d_bits.to_array((5, code.A), np.uint8), host[0])
            assert np.array_equal(d_crc.to_array((5,), np.uint8).astype(bool), host[1])
            assert np.array_equal(d_metric.to_array((5,), np.float64), host[2])
            assert np.array_equal(d_lb.to_array((5, 8, 128), np.uint8), host[3][0])
            assert np.array_equal(d_lm.to_array((5, 8), np.float64), host[3][1])
            assert np.array_equal(d_live.to_array((5,), np.int32), host[3][2])
        d_u = deviceops.polar_decode_dev(code, d_llr, 5, want="u_llr")
        _lib.check(lib.cpx_stream_sync(None))
        assert np.array_equal(d_u.to_array((5, 256), np.float64), polar_decode(llr, code, want="u_llr"))
    finally:
        for s in streams:
            lib.cpx_stream_destroy(s)


# ---- isolation ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [1, 8])
def test_bad_rows_leave_the_others_alone(gpu, L):
    code = PolarCode(128, 64, crc=CRCS[11])
    llr = gaussian(7, 9, code)
    clean = polar_decode(llr, code, L, want=EVERYTHING)
    bad = llr.copy()
    bad[3] = np.nan
    bad[5] = np.where(np.arange(128) % 3 == 0, -np.inf, np.inf)
    got = polar_decode(bad, code, L, want=EVERYTHING)                              # the call returns
    keep = [i for i in range(9) if i not in (3, 5)]
    assert np.array_equal(got[0][keep], clean[0][keep]) and np.array_equal(got[1][keep], clean[1][keep])
    assert np.array_equal(got[2][keep], clean[2][keep])
    assert all(np.array_equal(g[keep], c[keep]) for g, c in zip(got[3], clean[3]))
    assert got[0][[3, 5]].max() <= 1 and got[3][0][[3, 5]].max() <= 1 and np.all(got[3][2] == min(L, 2 ** 64))


# ---- the link -----------------------------------------------------------------------------------------------------------------------
def test_block_errors_on_the_seeded_set(gpu):
    def engine(llr, L, with_crc):
        return polar_decode(llr, PolarCode(128, 64, crc=CRCS[11] if with_crc else None), L)
    assert block_errors(engine) == MODEL_BLOCK_ERRORS


def test_noise_free_qpsk_chain(gpu):
    from commpy_amd.modulation import QAMModem
    code, modem = PolarCode(256, 140, crc=CRCS[11]), QAMModem(4)
    msg = np.random.RandomState(2).randint(0, 2, (4, code.A)).astype(np.uint8)
    x = polar_encode(msg, code)
    llr1 = modem.demodulate(modem.modulate(x.reshape(-1)), "soft", 0.5)            # log P(1) / P(0): the decoder wants the opposite sign
    for L in (1, 4):
        bits, ok = polar_decode(-llr1.reshape(4, 256), code, L, want=("bits", "crc"))
        assert np.array_equal(bits, msg) and ok.all()
