"""The contract every effect handle's C ABI shares (csrc/fx_handle.hpp), for the
fourteen handle types, through ctypes.

Without a GPU: a valid config with device -1 reports AD_ERR_NO_DEVICE, the same
config with one field out of range reports AD_ERR_INVALID_ARGUMENT, so a config
is validated before any device call; bad arguments of create leave *out null;
every entry point takes a null handle as AD_ERR_INVALID_ARGUMENT and destroy
takes it silently.  The same holds on a machine with a GPU (no device has index
-1).

With a GPU: a call that fails after it was ordered against the handle's earlier
calls leaves the handle usable on another stream (the spectral pitch shifter's
missing resampling prototype is the one argument error a call can meet there).
"""
import ctypes as C

import numpy as np
import pytest

from algodsp import _lib

FS = 48000.0
FRAME = 256
WINDOW = np.ascontiguousarray(0.5 - 0.5 * np.cos(2 * np.pi * np.arange(FRAME) / FRAME))
DP = C.POINTER(C.c_double)


def _stft(cfg):
    cfg.frame_size = FRAME
    setattr(cfg, "hop_size" if hasattr(cfg, "hop_size") else "analysis_hop", FRAME // 4)
    cfg.window = WINDOW.ctypes.data_as(DP)


# name, config structure, what a valid config needs beyond the defaults, one (field, value) a validator rejects
FAMILIES = [
    ("phaser", _lib.PhaserConfig, None, ("stages", 0)),
    ("tremolo", _lib.TremoloConfig, None, ("depth", 2.0)),
    ("ringmod", _lib.RingModConfig, None, ("mix", -1.0)),
    ("transient", _lib.TransientConfig, None, ("attack_ms", 0.0)),
    ("deesser", _lib.DeEsserConfig, None, ("q", 0.0)),
    ("distortion", _lib.DistortionConfig, None, ("drive", 0.0)),
    ("bitcrusher", _lib.BitCrusherConfig, None, ("downsample", 0)),
    ("specfreeze", _lib.SpecFreezeConfig, _stft, ("hop_size", 0)),
    ("pitchspec", _lib.PitchSpecConfig, _stft, ("pitch_ratio", 8.0)),
    ("delay", _lib.DelayConfig, None, ("feedback", 1.5)),
    ("flanger", _lib.FlangerConfig, None, ("mix", 2.0)),
    ("fdn", _lib.FdnConfig, None, ("damp", 2.0)),
    ("lookahead", _lib.LookaheadConfig, None, ("release_ms", 0.0)),
    ("vocoder", _lib.VocoderConfig, None, ("synth_q", 0.0)),
]
IDS = [f[0] for f in FAMILIES]


def fn(name, what):
    return getattr(_lib.lib(), f"ad_{name}_{what}")


def valid_config(name, cls, fix):
    cfg = cls()
    fn(name, "default_config")(C.byref(cfg), FS)
    if fix:
        fix(cfg)
    assert fn(name, "validate")(C.byref(cfg)) == _lib.AD_OK, _lib.lib().ad_last_error()
    return cfg


def create(name, cfg, channels, device, out):
    return fn(name, "create")(C.byref(cfg) if cfg is not None else None, channels, device,
                              C.byref(out) if out is not None else None)


@pytest.mark.parametrize("name,cls,fix,bad", FAMILIES, ids=IDS)
def test_create_validates_before_any_device_call(name, cls, fix, bad):
    cfg = valid_config(name, cls, fix)
    h = C.c_void_p(1)
    assert create(name, cfg, 2, -1, h) == _lib.AD_ERR_NO_DEVICE
    assert not h.value
    setattr(cfg, *bad)
    assert fn(name, "validate")(C.byref(cfg)) == _lib.AD_ERR_INVALID_ARGUMENT
    h = C.c_void_p(1)
    assert create(name, cfg, 2, -1, h) == _lib.AD_ERR_INVALID_ARGUMENT
    assert not h.value


@pytest.mark.parametrize("name,cls,fix,bad", FAMILIES, ids=IDS)
def test_create_rejects_bad_arguments_and_nulls_out(name, cls, fix, bad):
    cfg = valid_config(name, cls, fix)
    h = C.c_void_p(1)
    assert create(name, cfg, 0, -1, h) == _lib.AD_ERR_INVALID_ARGUMENT
    assert not h.value
    h = C.c_void_p(1)
    assert create(name, None, 2, -1, h) == _lib.AD_ERR_INVALID_ARGUMENT
    assert not h.value
    assert create(name, cfg, 2, -1, None) == _lib.AD_ERR_INVALID_ARGUMENT


@pytest.mark.parametrize("name,cls,fix,bad", FAMILIES, ids=IDS)
def test_null_handle_is_an_argument_error(name, cls, fix, bad):
    bad_arg = _lib.AD_ERR_INVALID_ARGUMENT
    x = np.zeros(8)
    p = x.ctypes.data_as(DP)
    vp = C.c_void_p(x.ctypes.data)  # never read: the handle is checked first
    if name == "lookahead":
        assert fn(name, "process")(None, p, None, 0, 8) == bad_arg
        assert fn(name, "process_device")(None, vp, 8, None, 0, 0, 8, None) == bad_arg
    elif name == "vocoder":
        assert fn(name, "process")(None, p, p, p, 8) == bad_arg
        assert fn(name, "process_device")(None, vp, 8, vp, 8, vp, 8, 8, None) == bad_arg
    else:
        assert fn(name, "process")(None, p, 8) == bad_arg
        assert fn(name, "process_device")(None, vp, 8, 8, None) == bad_arg
    assert fn(name, "reset")(None) == bad_arg
    assert fn(name, "set_param")(None, 0, 1.0) == bad_arg
    assert fn(name, "get_config")(None, C.byref(cls())) == bad_arg
    assert fn(name, "destroy")(None) is None
    assert not np.any(x)


# ---- the error path of a call, on the device -------------------------------------
@pytest.mark.gpu
def test_failed_call_leaves_the_handle_usable_on_another_stream(gpu):
    """3 channels, frame 256, four frames of input.  A ratio outside the bin-shift range without a resampling
    prototype is an argument error of the call; the buffer keeps its bits, and the next call, on another stream
    with a ratio inside the range, gives what a fresh handle gives."""
    import torch

    channels, n, ratio = 3, 4 * FRAME, 1.1
    P_RATIO = 1  # AD_PITCHSPEC_RATIO
    x = np.random.default_rng(0xF8).standard_normal((channels, n))

    def make(r):
        cfg = valid_config("pitchspec", _lib.PitchSpecConfig, _stft)
        cfg.pitch_ratio = r
        h = C.c_void_p()
        _lib.check(fn("pitchspec", "create")(C.byref(cfg), channels, 0, C.byref(h)))
        return h

    def call(h, d, stream):
        return fn("pitchspec", "process_device")(h, d.data_ptr(), n, n, stream.cuda_stream)

    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    h, fresh = make(1.5), make(ratio)
    try:
        d = torch.from_numpy(x).to("cuda:0")
        torch.cuda.synchronize()
        assert call(h, d, s1) == _lib.AD_ERR_INVALID_ARGUMENT
        torch.cuda.synchronize()
        assert np.array_equal(d.cpu().numpy().view(np.int64), x.view(np.int64))
        _lib.check(fn("pitchspec", "set_param")(h, P_RATIO, ratio))
        _lib.check(call(h, d, s2))
        want = torch.from_numpy(x).to("cuda:0")
        torch.cuda.synchronize()
        _lib.check(call(fresh, want, s1))
        torch.cuda.synchronize()
        got, want = d.cpu().numpy(), want.cpu().numpy()
        assert not np.array_equal(got, x)
        assert np.array_equal(got.view(np.int64), want.view(np.int64))
    finally:
        fn("pitchspec", "destroy")(h)
        fn("pitchspec", "destroy")(fresh)
