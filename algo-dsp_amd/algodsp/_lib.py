"""ctypes loader for libalgodsp_hip.so (the C ABI declared in include/algodsp.h).

The product path is the HIP library only: if it cannot be loaded, or no
gfx950 device is visible, every create call raises -- there is no CPU
fallback anywhere in this package.
"""
from __future__ import annotations

import ctypes as C
import os
import pathlib

import numpy as np

_HERE = pathlib.Path(__file__).resolve().parent
LIB_PATH = _HERE.parent / "libalgodsp_hip.so"
HEADER_PATH = _HERE.parent.parent / "include" / "algodsp.h"

# status codes (include/algodsp.h)
AD_OK = 0
AD_ERR_EMPTY_INPUT = 1
AD_ERR_EMPTY_KERNEL = 2
AD_ERR_LENGTH_MISMATCH = 3
AD_ERR_INVALID_BLOCK_SIZE = 4
AD_ERR_INVALID_BLOCK_ORDER = 5
AD_ERR_EMPTY_IMPULSE_RESPONSE = 6
AD_ERR_STAGE_INDEX_OUT_OF_RANGE = 7
AD_ERR_INVALID_ARGUMENT = 8
AD_ERR_DIVISION_BY_ZERO = 9
AD_ERR_DEVICE = 100
AD_ERR_NO_DEVICE = 101
AD_ERR_INTERNAL = 102


class ADError(Exception):
    """Error returned through the C ABI; `code` is the AD_* status."""

    code = None

    def __init__(self, code: int, msg: str = ""):
        super().__init__(f"[{code}] {msg}")
        self.code = code


class ErrEmptyInput(ADError):
    pass


class ErrEmptyKernel(ADError):
    pass


class ErrLengthMismatch(ADError):
    pass


class ErrInvalidBlockSize(ADError):
    pass


class ErrInvalidBlockOrder(ADError):
    pass


class ErrEmptyImpulseResponse(ADError):
    pass


class ErrStageIndexOutOfRange(ADError):
    pass


class ErrInvalidArgument(ADError):
    pass


class ErrDivisionByZero(ADError):
    pass


class ErrDevice(ADError):
    pass


_BY_CODE = {
    AD_ERR_EMPTY_INPUT: ErrEmptyInput,
    AD_ERR_EMPTY_KERNEL: ErrEmptyKernel,
    AD_ERR_LENGTH_MISMATCH: ErrLengthMismatch,
    AD_ERR_INVALID_BLOCK_SIZE: ErrInvalidBlockSize,
    AD_ERR_INVALID_BLOCK_ORDER: ErrInvalidBlockOrder,
    AD_ERR_EMPTY_IMPULSE_RESPONSE: ErrEmptyImpulseResponse,
    AD_ERR_STAGE_INDEX_OUT_OF_RANGE: ErrStageIndexOutOfRange,
    AD_ERR_INVALID_ARGUMENT: ErrInvalidArgument,
    AD_ERR_DIVISION_BY_ZERO: ErrDivisionByZero,
}

class CompressorConfig(C.Structure):
    """ad_compressor_config (include/algodsp.h)."""

    _fields_ = [(n, C.c_double) for n in ("sample_rate", "threshold_db", "ratio", "knee_db", "attack_ms",
                                          "release_ms", "rms_window_ms", "makeup_db", "sidechain_low_cut_hz",
                                          "sidechain_high_cut_hz")] + \
               [(n, C.c_int) for n in ("topology", "detector_mode", "feedback_ratio_scale", "auto_makeup")]


class FdnConfig(C.Structure):
    """ad_fdn_config (include/algodsp.h); field k is parameter AD_FDN_* = k."""

    _fields_ = [(n, C.c_double) for n in ("sample_rate", "wet", "dry", "rt60_seconds", "damp", "pre_delay_seconds",
                                          "mod_depth_seconds", "mod_rate_hz")]


class DelayConfig(C.Structure):
    """ad_delay_config (include/algodsp.h)."""

    _fields_ = [(n, C.c_double) for n in ("sample_rate", "time_seconds", "feedback", "mix", "smooth_coeff")] + \
               [("mode", C.c_int), ("delay_samples", C.c_int64)]


class FlangerConfig(C.Structure):
    """ad_flanger_config (include/algodsp.h); field k is parameter AD_FLANGER_* = k."""

    _fields_ = [(n, C.c_double) for n in ("sample_rate", "rate_hz", "depth_seconds", "base_delay_seconds", "feedback",
                                          "mix")]


class PhaserConfig(C.Structure):
    """ad_phaser_config (include/algodsp.h); field k is parameter AD_PHASER_* = k."""

    _fields_ = [(n, C.c_double) for n in ("sample_rate", "rate_hz", "min_freq_hz", "max_freq_hz", "feedback", "mix")] + \
               [("stages", C.c_int)]


class TremoloConfig(C.Structure):
    """ad_tremolo_config (include/algodsp.h); field k is parameter AD_TREMOLO_* = k."""

    _fields_ = [(n, C.c_double) for n in ("sample_rate", "rate_hz", "depth", "smoothing_ms", "mix", "smoothing_coeff")]


class RingModConfig(C.Structure):
    """ad_ringmod_config (include/algodsp.h); field k is parameter AD_RINGMOD_* = k."""

    _fields_ = [(n, C.c_double) for n in ("sample_rate", "carrier_hz", "mix")]


class DistortionConfig(C.Structure):
    """ad_distortion_config (include/algodsp.h); field k (0..7) is parameter AD_DISTORTION_* = k, the ints
    are parameters 8..13 in their order."""

    _fields_ = [(n, C.c_double) for n in ("sample_rate", "drive", "mix", "output_level", "clip_level", "shape", "bias",
                                          "cheb_gain")] + [("cheb_weights", C.c_double * 16)] + \
               [(n, C.c_int) for n in ("mode", "approx", "cheb_order", "cheb_harmonic", "cheb_invert", "cheb_dc_bypass")]


class BitCrusherConfig(C.Structure):
    """ad_bitcrusher_config (include/algodsp.h); field k is parameter AD_BITCRUSHER_* = k."""

    _fields_ = [(n, C.c_double) for n in ("sample_rate", "bit_depth", "mix")] + [("downsample", C.c_int)]


class TransientConfig(C.Structure):
    """ad_transient_config (include/algodsp.h); field k is parameter AD_TRANSIENT_* = k."""

    _fields_ = [(n, C.c_double) for n in ("sample_rate", "attack_amount", "sustain_amount", "attack_ms", "release_ms",
                                          "attack_coeff", "release_coeff")]


class DeEsserConfig(C.Structure):
    """ad_deesser_config (include/algodsp.h); field k is parameter AD_DEESSER_* = k."""

    _fields_ = [(n, C.c_double) for n in ("sample_rate", "freq_hz", "q", "threshold_db", "ratio", "knee_db",
                                          "attack_ms", "release_ms", "range_db", "attack_coeff", "release_coeff")] + \
               [(n, C.c_int) for n in ("mode", "detector", "listen", "filter_order")]


class VocoderConfig(C.Structure):
    """ad_vocoder_config (include/algodsp.h); field k is parameter AD_VOCODER_* = k where the reference has a
    setter."""

    _fields_ = [(n, C.c_double) for n in ("sample_rate", "synth_q", "attack_ms", "release_ms", "input_level",
                                          "synth_level", "vocoder_level")] + \
               [(n, C.c_int) for n in ("downsample", "layout", "synth_q_set")]


VOCODER_MAX_BANDS = 32  # AD_VOCODER_MAX_BANDS


class VocoderTables(C.Structure):
    """ad_vocoder_tables (include/algodsp.h): what the reference caches for a config."""

    _fields_ = [("num_bands", C.c_int), ("num_groups", C.c_int), ("downsample_max", C.c_int),
                ("factors", C.c_int * VOCODER_MAX_BANDS), ("group_of_band", C.c_int * VOCODER_MAX_BANDS),
                ("group_factors", C.c_int * VOCODER_MAX_BANDS)] + \
               [(n, (C.c_double * 5) * VOCODER_MAX_BANDS) for n in ("analysis", "synthesis", "decimated",
                                                                    "antialias")] + \
               [("attack_coeff", C.c_double), ("release_coeff", C.c_double),
                ("ds_attack", C.c_double * VOCODER_MAX_BANDS), ("ds_release", C.c_double * VOCODER_MAX_BANDS)]


class LookaheadConfig(C.Structure):
    """ad_lookahead_config (include/algodsp.h); field k is parameter AD_LOOKAHEAD_* = k."""

    _fields_ = [(n, C.c_double) for n in ("sample_rate", "threshold_db", "release_ms", "lookahead_ms")]


class SpecFreezeConfig(C.Structure):
    """ad_specfreeze_config (include/algodsp.h); window points at frame_size coefficients."""

    _fields_ = [("sample_rate", C.c_double), ("mix", C.c_double)] + \
               [(n, C.c_int) for n in ("frame_size", "hop_size", "phase_mode", "frozen", "window_type")] + \
               [("window", C.POINTER(C.c_double))]


class PitchSpecConfig(C.Structure):
    """ad_pitchspec_config (include/algodsp.h); window and resample_taps point at the caller's tables."""

    _fields_ = [("sample_rate", C.c_double), ("pitch_ratio", C.c_double)] + \
               [(n, C.c_int) for n in ("frame_size", "analysis_hop", "window_type", "resample_quality")] + \
               [("window", C.POINTER(C.c_double)), ("resample_taps", C.POINTER(C.c_double)),
                ("n_resample_taps", C.c_int64)]


class FxNodeCfg(C.Structure):
    """ad_fx_node_cfg: a node's own config structure and its size."""

    _fields_ = [("config", C.c_void_p), ("bytes", C.c_int64)]


class DeconvOptionsC(C.Structure):
    """ad_deconv_options (include/algodsp.h)."""

    _fields_ = [("method", C.c_int), ("epsilon", C.c_double), ("noise_variance", C.c_double),
                ("signal_variance", C.c_double)]


_lib = None

c_double_p = C.POINTER(C.c_double)
c_float_p = C.POINTER(C.c_float)
c_int64_p = C.POINTER(C.c_int64)


def lib() -> C.CDLL:
    """Loads (once) and returns the HIP library; raises if it is missing."""
    global _lib
    if _lib is None:
        # PyTorch-ROCm bundles its own libamdhip64 (SONAME libamdhip64.so.7) and
        # refers to it by the unversioned name, so if our library pulled in
        # /opt/rocm's copy first the process would end up with two HIP/HSA
        # runtimes and torch would see no GPU.  Importing torch first makes the
        # dynamic linker bind our NEEDED libamdhip64.so.7 to torch's runtime:
        # one runtime, shared device pointers and streams.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        path = os.environ.get("ALGODSP_LIB", str(LIB_PATH))
        if not pathlib.Path(path).exists():
            raise ImportError(f"libalgodsp_hip.so not built at {path}; run `make -C algo-dsp_amd`")
        _lib = C.CDLL(path)
        _declare(_lib)
    return _lib


_NEWEST = ("ad_conv_multi_set_long_blocks", "ad_conv_multi_get_long_blocks")

# the effect handles whose create takes a config structure (csrc/fx_handle.hpp): a new kind is one entry here
_HANDLE_KINDS = (("fdn", FdnConfig), ("delay", DelayConfig), ("flanger", FlangerConfig), ("phaser", PhaserConfig),
                 ("tremolo", TremoloConfig), ("ringmod", RingModConfig), ("distortion", DistortionConfig),
                 ("bitcrusher", BitCrusherConfig), ("transient", TransientConfig), ("deesser", DeEsserConfig),
                 ("lookahead", LookaheadConfig), ("vocoder", VocoderConfig), ("specfreeze", SpecFreezeConfig),
                 ("pitchspec", PitchSpecConfig))


def _handle_prototypes(kind: str, cfg) -> dict:
    """The prototypes every kind of _HANDLE_KINDS has, {ad_<kind>_<name>: (restype, argtypes)}."""
    vp, i64, cp = C.c_void_p, C.c_int64, C.POINTER(cfg)
    common = {
        "default_config": (None, [cp, C.c_double]),
        "validate": (C.c_int, [cp]),
        "create": (C.c_int, [cp, C.c_int, C.c_int, C.POINTER(vp)]),
        "set_param": (C.c_int, [vp, C.c_int, C.c_double]),
        "get_config": (C.c_int, [vp, cp]),
        "process": (C.c_int, [vp, c_double_p, i64]),
        "process_device": (C.c_int, [vp, vp, i64, i64, vp]),
        "reset": (C.c_int, [vp]),
        "destroy": (None, [vp]),
    }
    return {f"ad_{kind}_{name}": proto for name, proto in common.items()}


def _declare(L: C.CDLL) -> None:
    vp = C.c_void_p
    i64 = C.c_int64
    sig = {
        "ad_last_error": (C.c_char_p, []),
        "ad_version": (C.c_int, []),
        "ad_device_count": (C.c_int, [C.POINTER(C.c_int)]),
        "ad_conv_stream_ols_create": (C.c_int, [c_double_p, i64, i64, C.c_int, C.POINTER(vp)]),
        "ad_conv_stream_ola_create": (C.c_int, [c_double_p, i64, i64, C.c_int, C.POINTER(vp)]),
        "ad_conv_process_block": (C.c_int, [vp, c_double_p, i64, c_double_p, i64]),
        "ad_conv_stream_ols32_create": (C.c_int, [c_float_p, i64, i64, C.c_int, C.POINTER(vp)]),
        "ad_conv_stream_ola32_create": (C.c_int, [c_float_p, i64, i64, C.c_int, C.POINTER(vp)]),
        "ad_conv_process_block32": (C.c_int, [vp, c_float_p, i64, c_float_p, i64]),
        "ad_conv_partitioned32_create": (C.c_int, [c_float_p, i64, C.c_int, C.c_int, C.c_int, C.POINTER(vp)]),
        "ad_conv_partitioned_process_block32": (C.c_int, [vp, c_float_p, i64, c_float_p, i64]),
        "ad_conv_ols_create": (C.c_int, [c_double_p, i64, i64, C.c_int, C.POINTER(vp)]),
        "ad_conv_ola_create": (C.c_int, [c_double_p, i64, i64, C.c_int, C.POINTER(vp)]),
        "ad_conv_process": (C.c_int, [vp, c_double_p, i64, c_double_p, i64]),
        "ad_conv_partitioned_create": (C.c_int, [c_double_p, i64, C.c_int, C.c_int, C.c_int, C.POINTER(vp)]),
        "ad_conv_partitioned_process_block": (C.c_int, [vp, c_double_p, i64, c_double_p, i64]),
        "ad_conv_stage_count": (C.c_int, [vp]),
        "ad_conv_stage_info": (C.c_int, [vp, C.c_int, c_int64_p, c_int64_p]),
        "ad_conv_reset": (C.c_int, [vp]),
        "ad_conv_block_size": (i64, [vp]),
        "ad_conv_kernel_len": (i64, [vp]),
        "ad_conv_fft_size": (i64, [vp]),
        "ad_conv_step_size": (i64, [vp]),
        "ad_conv_latency": (i64, [vp]),
        "ad_conv_set_host_io": (C.c_int, [vp, C.c_int, C.c_int]),
        "ad_conv_host_io_profile": (C.c_int, [vp, c_double_p, c_double_p, c_double_p]),
        "ad_conv_destroy": (None, [vp]),
        "ad_conv_direct": (C.c_int, [c_double_p, i64, c_double_p, i64, c_double_p, C.c_int]),
        "ad_conv_direct_circular": (C.c_int, [c_double_p, i64, c_double_p, i64, c_double_p, C.c_int]),
        "ad_conv_direct_device": (C.c_int, [C.c_void_p, i64, C.c_void_p, i64, C.c_void_p, C.c_void_p]),
        "ad_conv_convolve": (C.c_int, [c_double_p, i64, c_double_p, i64, C.c_int, c_double_p, i64, c_int64_p,
                                       C.c_int]),
        "ad_conv_multi_create": (C.c_int, [c_double_p, C.c_int, i64, i64, C.c_int, C.POINTER(C.c_int32), i64,
                                           C.c_int, C.POINTER(vp)]),
        "ad_conv_multi_set_schedule": (C.c_int, [vp, C.c_int, i64, i64]),
        "ad_conv_lowlat_stats": (C.c_int, [vp, c_int64_p, c_int64_p]),
        "ad_conv_multi_get_schedule": (C.c_int, [vp, C.POINTER(C.c_int), c_int64_p]),
        "ad_conv_multi_set_long_blocks": (C.c_int, [vp, C.c_int]),
        "ad_conv_multi_get_long_blocks": (C.c_int, [vp, C.POINTER(C.c_int)]),
        "ad_conv_multi_process_device": (C.c_int, [vp, vp, i64, i64, vp, i64, i64, vp]),
        "ad_conv_multi_process_device_segment": (C.c_int, [vp, vp, i64, i64, vp, i64, i64, i64, i64, vp]),
        "ad_conv_multi_process_device_mix": (C.c_int, [vp, vp, i64, i64, vp, i64, i64, C.c_int, i64, i64, vp]),
        "ad_conv_mixdown_device": (C.c_int, [vp, C.c_int, i64, i64, vp, i64, C.c_int, vp]),
        "ad_comm_get_unique_id": (C.c_int, [C.POINTER(C.c_uint8)]),
        "ad_comm_create": (C.c_int, [C.POINTER(C.c_uint8), C.c_int, C.c_int, C.c_int, C.POINTER(vp)]),
        "ad_comm_destroy": (None, [vp]),
        "ad_comm_rank": (C.c_int, [vp]),
        "ad_comm_size": (C.c_int, [vp]),
        "ad_mixdown_reduce": (C.c_int, [vp, vp, C.c_int, i64, i64, C.c_int, vp, i64, C.c_int, vp]),
        "ad_conv_ols_process_multi": (C.c_int, [vp, C.POINTER(c_double_p), C.POINTER(c_double_p), C.c_int, i64]),
        "ad_conv_multi_stream_create": (C.c_int, [c_double_p, C.c_int, i64, i64, C.c_int, C.POINTER(C.c_int32),
                                                  C.c_int, C.POINTER(vp)]),
        "ad_conv_multi_stream_process_block": (C.c_int, [vp, C.POINTER(c_double_p), C.POINTER(c_double_p), C.c_int,
                                                         i64]),
        "ad_conv_multi_stream_process_block_device": (C.c_int, [vp, vp, i64, vp, i64, vp]),
        "ad_conv_pc_multi_create": (C.c_int, [c_double_p, i64, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(vp)]),
        "ad_conv_pc_multi_process_device": (C.c_int, [vp, vp, i64, vp, i64, i64, vp]),
        "ad_conv_reverb_multi_create": (C.c_int, [c_double_p, i64, C.c_int, C.c_int, C.c_int, C.POINTER(vp)]),
        "ad_conv_reverb_multi_process_device": (C.c_int, [vp, vp, i64, i64, vp]),
        "ad_conv_reverb_multi_process": (C.c_int, [vp, c_double_p, i64]),
        "ad_conv_profile_enable": (C.c_int, [vp, C.c_int]),
        "ad_conv_profile_kernels": (C.c_int, [vp, C.c_int]),
        "ad_conv_profile_read": (C.c_int, [vp, c_double_p, c_int64_p, c_double_p]),
        "ad_compressor_default_config": (None, [C.POINTER(CompressorConfig), C.c_double]),
        "ad_compressor_validate": (C.c_int, [C.POINTER(CompressorConfig)]),
        "ad_fx_chain_create": (C.c_int, [C.c_int, C.c_int, C.POINTER(vp)]),
        "ad_fx_chain_set_eq": (C.c_int, [vp, c_double_p, C.c_int, C.c_int]),
        "ad_fx_eq_noise": (C.c_int, [c_double_p, C.c_int, C.c_int, c_double_p]),
        "ad_fx_chain_set_compressor": (C.c_int, [vp, C.POINTER(CompressorConfig)]),
        "ad_fx_chain_set_expander": (C.c_int, [vp, C.POINTER(CompressorConfig), C.c_int, C.c_double, C.c_double]),
        "ad_fx_chain_set_freeverb": (C.c_int, [vp, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double]),
        "ad_fx_chain_disable_freeverb": (C.c_int, [vp]),
        "ad_fx_chain_reset": (C.c_int, [vp]),
        "ad_fx_chain_process": (C.c_int, [vp, c_double_p, i64]),
        "ad_fx_chain_process_device": (C.c_int, [vp, vp, i64, i64, vp]),
        "ad_fx_chain_compressor_metrics": (C.c_int, [vp, C.c_int, c_double_p, c_double_p, c_double_p]),
        "ad_fx_chain_eq_state": (C.c_int, [vp, c_double_p, i64]),
        "ad_fx_chain_set_eq_state": (C.c_int, [vp, c_double_p, i64]),
        "ad_fx_chain_set_engine": (C.c_int, [vp, C.c_int, i64]),
        "ad_fx_chain_last_engine": (C.c_int, [vp, C.POINTER(C.c_int), C.POINTER(C.c_double)]),
        "ad_fx_chain_set_profiling": (C.c_int, [vp, C.c_int]),
        "ad_fx_chain_read_profile": (C.c_int, [vp, C.POINTER(C.c_ulonglong), C.c_int, C.POINTER(C.c_int)]),
        "ad_fx_chain_destroy": (None, [vp]),
        "ad_fx_graph_create": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.POINTER(vp)]),
        "ad_fx_graph_process": (C.c_int, [vp, c_double_p, i64]),
        "ad_fx_graph_process_device": (C.c_int, [vp, vp, i64, i64, vp]),
        "ad_fx_graph_reset": (C.c_int, [vp]),
        "ad_fx_graph_op_count": (C.c_int, [vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
        "ad_fx_graph_destroy": (None, [vp]),
        "ad_biquad_chain_process": (C.c_int, [c_double_p, c_double_p, C.c_double, c_double_p, C.c_int, C.c_int, i64,
                                              C.c_int]),
        "ad_conv_reverb_create": (C.c_int, [c_double_p, i64, C.c_int, C.c_int, C.POINTER(vp)]),
        "ad_conv_reverb_set_wet_dry": (C.c_int, [vp, C.c_double, C.c_double]),
        "ad_conv_reverb_process_inplace": (C.c_int, [vp, c_double_p, i64]),
        "ad_decode_f16": (C.c_int, [C.POINTER(C.c_uint16), i64, C.c_int, c_double_p, C.c_int]),
        "ad_decode_f16_device": (C.c_int, [vp, i64, C.c_int, vp, vp]),
        "ad_fir_create": (C.c_int, [c_double_p, i64, C.c_int, C.c_int, C.POINTER(vp)]),
        "ad_fir_process_block": (C.c_int, [vp, c_double_p, i64]),
        "ad_fir_process_block_to": (C.c_int, [vp, c_double_p, c_double_p, i64]),
        "ad_fir_process_device": (C.c_int, [vp, vp, i64, vp, i64, i64, vp]),
        "ad_fir_reset": (C.c_int, [vp]),
        "ad_fir_destroy": (None, [vp]),
        "ad_resampler_create": (C.c_int, [i64, i64, c_double_p, i64, C.c_int, C.c_int, C.POINTER(vp)]),
        "ad_resampler_predict_output_len": (C.c_int, [vp, i64, c_int64_p]),
        "ad_resampler_process": (C.c_int, [vp, c_double_p, i64, c_double_p, i64, c_int64_p]),
        "ad_resampler_process_device": (C.c_int, [vp, vp, i64, i64, vp, i64, i64, c_int64_p, vp]),
        "ad_resampler_reset": (C.c_int, [vp]),
        "ad_resampler_ratio": (C.c_int, [vp, c_int64_p, c_int64_p]),
        "ad_resampler_taps_per_phase": (C.c_int, [vp]),
        "ad_resampler_kernel_info": (C.c_int, [vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                               C.POINTER(C.c_int), C.POINTER(C.c_int), c_int64_p]),
        "ad_resampler_destroy": (None, [vp]),
        "ad_fdn_derived": (C.c_int, [vp, c_double_p, c_int64_p, c_int64_p, c_double_p]),
        "ad_fdn_kernel_info": (C.c_int, [vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
        "ad_delay_derived": (C.c_int, [vp, c_double_p, c_double_p, c_int64_p, c_int64_p]),
        "ad_delay_kernel_info": (C.c_int, [vp] + [C.POINTER(C.c_int)] * 4),
        "ad_delay_set_regime": (C.c_int, [vp, C.c_int]),
        "ad_flanger_derived": (C.c_int, [vp, c_int64_p, c_int64_p, c_int64_p, c_double_p]),
        "ad_flanger_kernel_info": (C.c_int, [vp] + [C.POINTER(C.c_int)] * 4),
        "ad_fx_graph_create_ext": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.POINTER(vp)]),
        "ad_phaser_set_range": (C.c_int, [vp, C.c_double, C.c_double]),
        "ad_phaser_kernel_info": (C.c_int, [vp] + [C.POINTER(C.c_int)] * 3),
        "ad_tremolo_kernel_info": (C.c_int, [vp] + [C.POINTER(C.c_int)] * 3),
        "ad_ringmod_kernel_info": (C.c_int, [vp, C.POINTER(C.c_int), C.POINTER(C.c_int), c_double_p]),
        "ad_fx_graph_create_cfg": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.POINTER(vp)]),
        "ad_distortion_set_weights": (C.c_int, [vp, c_double_p, C.c_int]),
        "ad_distortion_derived": (C.c_int, [vp] + [c_double_p] * 4 + [C.POINTER(C.c_int)]),
        "ad_distortion_kernel_info": (C.c_int, [vp] + [C.POINTER(C.c_int)] * 4),
        "ad_distortion_curve": (C.c_int, [vp, c_double_p, i64, c_double_p]),
        "ad_bitcrusher_derived": (C.c_int, [vp, C.c_int, c_double_p, C.POINTER(C.c_int), c_double_p]),
        "ad_bitcrusher_kernel_info": (C.c_int, [vp] + [C.POINTER(C.c_int)] * 3),
        "ad_transient_derived": (C.c_int, [C.POINTER(TransientConfig), c_double_p, c_double_p]),
        "ad_transient_kernel_info": (C.c_int, [vp] + [C.POINTER(C.c_int)] * 3),
        "ad_transient_get_state": (C.c_int, [vp, C.c_int, c_double_p]),
        "ad_transient_set_state": (C.c_int, [vp, C.c_int, C.c_double]),
        "ad_deesser_derived": (C.c_int, [C.POINTER(DeEsserConfig)] + [c_double_p] * 7),
        "ad_deesser_kernel_info": (C.c_int, [vp] + [C.POINTER(C.c_int)] * 4),
        "ad_deesser_get_state": (C.c_int, [vp, C.c_int, c_double_p, c_double_p, c_double_p]),
        "ad_deesser_set_state": (C.c_int, [vp, C.c_int, C.c_double, c_double_p, c_double_p]),
        "ad_deesser_metrics": (C.c_int, [vp, C.c_int, c_double_p, c_double_p]),
        "ad_deesser_reset_metrics": (C.c_int, [vp]),
        "ad_deesser_gain": (C.c_int, [vp, c_double_p, c_double_p, i64]),
        "ad_fx_chain_reset_compressor_metrics": (C.c_int, [vp]),
        "ad_lookahead_derived": (C.c_int, [C.POINTER(LookaheadConfig), c_double_p, c_double_p, c_double_p, c_int64_p]),
        "ad_lookahead_get_state": (C.c_int, [vp, C.c_int, c_double_p]),
        "ad_lookahead_gain": (C.c_int, [vp, c_double_p, c_double_p, i64]),
        "ad_lookahead_last_envelope": (C.c_int, [vp, c_double_p, i64]),
        "ad_lookahead_process": (C.c_int, [vp, c_double_p, c_double_p, i64, i64]),
        "ad_lookahead_process_device": (C.c_int, [vp, vp, i64, vp, i64, i64, i64, vp]),
        "ad_vocoder_derived": (C.c_int, [C.POINTER(VocoderConfig), C.POINTER(VocoderTables)]),
        "ad_vocoder_num_bands": (C.c_int, [vp, C.POINTER(C.c_int)]),
        "ad_vocoder_downsample_factors": (C.c_int, [vp, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int)]),
        "ad_vocoder_kernel_info": (C.c_int, [vp] + [C.POINTER(C.c_int)] * 3),
        "ad_vocoder_get_state": (C.c_int, [vp, C.c_int, c_double_p, C.POINTER(C.c_int)]),
        "ad_vocoder_process": (C.c_int, [vp, c_double_p, c_double_p, c_double_p, i64]),
        "ad_vocoder_process_device": (C.c_int, [vp, vp, i64, vp, i64, vp, i64, i64, vp]),
        "ad_xover_validate": (C.c_int, [c_double_p, C.c_int, C.c_int, C.c_double]),
        "ad_xover_sections": (C.c_int, [c_double_p, C.c_int, C.c_int, C.c_double, c_double_p, i64,
                                        C.POINTER(C.c_int)]),
        "ad_xover_create": (C.c_int, [c_double_p, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, C.POINTER(vp)]),
        "ad_xover_process": (C.c_int, [vp, c_double_p, c_double_p, i64]),
        "ad_xover_process_device": (C.c_int, [vp, vp, i64, vp, i64, i64, i64, vp]),
        "ad_xover_get_state": (C.c_int, [vp, C.c_int, c_double_p, i64]),
        "ad_xover_set_state": (C.c_int, [vp, C.c_int, c_double_p, i64]),
        "ad_xover_reset": (C.c_int, [vp]),
        "ad_xover_kernel_info": (C.c_int, [vp] + [C.POINTER(C.c_int)] * 3),
        "ad_xover_set_pipelined": (C.c_int, [vp, C.c_int]),
        "ad_xover_destroy": (None, [vp]),
        "ad_multiband_validate": (C.c_int, [c_double_p, C.c_int, C.c_int, C.c_double]),
        "ad_multiband_create": (C.c_int, [c_double_p, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, C.POINTER(vp)]),
        "ad_multiband_set_band": (C.c_int, [vp, C.c_int, C.POINTER(CompressorConfig)]),
        "ad_multiband_get_band": (C.c_int, [vp, C.c_int, C.POINTER(CompressorConfig)]),
        "ad_multiband_process": (C.c_int, [vp, c_double_p, i64]),
        "ad_multiband_process_device": (C.c_int, [vp, vp, i64, i64, vp]),
        "ad_multiband_process_multi": (C.c_int, [vp, c_double_p, c_double_p, i64]),
        "ad_multiband_process_multi_device": (C.c_int, [vp, vp, i64, vp, i64, i64, i64, vp]),
        "ad_multiband_metrics": (C.c_int, [vp, C.c_int, C.c_int, c_double_p, c_double_p, c_double_p]),
        "ad_multiband_reset_metrics": (C.c_int, [vp]),
        "ad_multiband_reset": (C.c_int, [vp]),
        "ad_multiband_xover_state": (C.c_int, [vp, C.c_int, c_double_p, i64]),
        "ad_multiband_set_chunk": (C.c_int, [vp, i64]),
        "ad_multiband_destroy": (None, [vp]),
        "ad_specfreeze_state": (C.c_int, [vp, c_double_p, c_double_p, C.POINTER(C.c_int)]),
        "ad_specfreeze_norm": (C.c_int, [vp, c_double_p, i64]),
        "ad_pitchspec_set_resample_taps": (C.c_int, [vp, c_double_p, i64]),
        "ad_pitchspec_effective_ratio": (C.c_int, [vp, c_double_p]),
        "ad_pitchspec_synthesis_hop": (C.c_int, [vp, C.POINTER(C.c_int)]),
        "ad_pitchspec_path": (C.c_int, [vp, C.POINTER(C.c_int)]),
        "ad_correlate_fft": (C.c_int, [c_double_p, i64, c_double_p, i64, c_double_p, C.c_int]),
        "ad_correlate_fft_device": (C.c_int, [vp, i64, vp, i64, vp, C.c_int, vp]),
        "ad_deconv_default_options": (DeconvOptionsC, []),
        "ad_deconvolve": (C.c_int, [c_double_p, i64, c_double_p, i64, C.POINTER(DeconvOptionsC), c_double_p, i64,
                                    c_int64_p, C.c_int]),
        "ad_inverse_filter": (C.c_int, [c_double_p, i64, i64, C.c_double, c_double_p, C.c_int]),
    }
    for kind in ("phaser", "tremolo", "ringmod"):
        sig[f"ad_{kind}_peek_lfo"] = (C.c_int, [vp, i64, c_double_p, c_double_p])
    for kind in ("specfreeze", "pitchspec"):
        sig[f"ad_{kind}_set_frame"] = (C.c_int, [vp, C.c_int, c_double_p])
        sig[f"ad_{kind}_set_window"] = (C.c_int, [vp, C.c_int, c_double_p])
        sig[f"ad_{kind}_profile"] = (C.c_int, [vp, C.c_int, c_double_p])
    for kind, cfg in _HANDLE_KINDS:
        for name, proto in _handle_prototypes(kind, cfg).items():
            sig.setdefault(name, proto)  # lookahead's and vocoder's own process / process_device above stand
    # an older build selected through ALGODSP_LIB (A/B runs against a parent
    # commit's library) may lack the entry points named in _NEWEST: those stay
    # unbound and raise AttributeError when called.  Any other missing symbol
    # is a stale build and fails here.
    older = "ALGODSP_LIB" in os.environ
    for name, (res, args) in sig.items():
        fn = getattr(L, name, None)
        if fn is None and older and name in _NEWEST:
            continue
        if fn is None:
            raise AttributeError(f"{L._name}: undefined symbol: {name}")
        fn.restype = res
        fn.argtypes = args


def check(rc: int) -> None:
    if rc == AD_OK:
        return
    msg = lib().ad_last_error().decode("utf-8", "replace")
    raise _BY_CODE.get(rc, ErrDevice if rc >= 100 else ADError)(rc, msg)


def f64(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64))


def ptr(a: np.ndarray):
    if a.size == 0:
        return C.cast(C.c_void_p(0), c_double_p)
    return a.ctypes.data_as(c_double_p)


def device_count() -> int:
    n = C.c_int(0)
    lib().ad_device_count(C.byref(n))
    return n.value


def exported_symbols() -> list[str]:
    """Every ad_* symbol declared in include/algodsp.h."""
    import re

    text = HEADER_PATH.read_text()
    return sorted(set(re.findall(r"\b(ad_[a-z0-9_]+)\s*\(", text)))
