"""commpy_amd -- MI355X-native communication-link engine with CommPy's Python API.

The modules of veeresht/CommPy 0.8.0, re-implemented as hand-written HIP kernels for gfx950 behind a ctypes C-ABI
(include/commpy_amd.h) where they have a hot path -- Viterbi, BCJR/MAP + turbo, LDPC belief propagation, PSK/QAM modulation and
hard/soft demodulation, MIMO detection, the fading channels (flat, static multipath and Doppler-fading multipath with time-varying
taps) and links, OFDM with timing / frequency-offset synchronisation,
pulse shaping / matched filtering / frequency offset of sampled waveforms, and equalisation of a multipath channel (MLSE / max-log MAP
on the trellis, MMSE linear and decision-feedback, and adaptive LMS / NLMS / RLS equalisers trained on a known prefix), and the
single-carrier synchroniser in front of them (symbol-timing recovery with a Gardner or Mueller-Mueller detector and a decision-directed
carrier PLL, one feedback loop per row) -- with the host-side descriptions either side of them (Trellis, interleavers, LDPC design files,
constellations, encoders, filter taps, PN and Zadoff-Chu sequences).  No PyTorch, no Triton, no CPU fallback: the device entry
points raise if the HIP library or the GPU is missing.

    from commpy_amd.channelcoding import Trellis, viterbi_decode, map_decode, turbo_decode, ldpc_bp_decode
    from commpy_amd.modulation import PSKModem, QAMModem, ofdm_tx, ofdm_rx
    from commpy_amd.modulation import OfdmPilots, ofdm_map_batch, ofdm_estimate_batch, ofdm_estimate_tv_batch
    from commpy_amd.filters import rrcosfilter, pulse_shape, matched_filter
    from commpy_amd.sequences import pnsequence, zcsequence
    from commpy_amd.impairments import add_frequency_offset
    from commpy_amd.sync import schmidl_cox_preamble, sync_estimate_batch, frame_sync_batch
    from commpy_amd.channels import multipath_batch, fading_multipath_batch, fading_gains_batch, tap_frequency_response
    from commpy_amd.equalizers import mlse_equalize_batch, mmse_equalize_batch, adaptive_equalize_batch
    from commpy_amd.recovery import timing_recover_batch, loop_gains
"""
__version__ = "0.3.0"

from commpy_amd import utilities  # noqa: F401



def set_precision(mode):
    """Precision mode of the engine: 'fp64-parity' (default: float64 in the reference's operation order, the mode every parity
    claim is made in) or 'fp32-fast' (float32 variants where a kernel has one; not bit-exact).  The switch is PROCESS-GLOBAL and affects
    two decoders: the large-batch Viterbi kernel (float32 path metrics) AND ``ldpc_bp_decode`` (float32 messages,
    hardware exp / log for sum-product, DESIGN.md 4.3: same decoded words on blocks that converge, NOT the 1e-5 LLR criterion).
    Enable it around the calls that should use it and reset it (``set_precision(None)``) afterwards.  Also settable through the
    environment variable CPX_PRECISION before the first call."""
    from commpy_amd import _lib
    _lib.set_precision(mode)


class precision:
    """``with commpy_amd.precision('fp32-fast'): ...`` -- the precision mode for the calls inside the block only; the previous mode is
    restored on the way out, exceptions included (round-4 answer to the process-global switch: enable it exactly around the decoder
    that should use it)."""

    def __init__(self, mode):
        self.mode = mode
        self._previous = None

    def __enter__(self):
        from commpy_amd import _lib
        self._previous = _lib.get_precision()
        _lib.set_precision(self.mode)
        return self

    def __exit__(self, *exc):
        from commpy_amd import _lib
        _lib.set_precision(self._previous)
        return False


__all__ = ["channelcoding", "modulation", "utilities", "parallel", "filters", "sequences", "impairments", "sync", "equalizers", "recovery", "set_precision", "precision"]
