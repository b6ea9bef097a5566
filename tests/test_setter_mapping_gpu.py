"""Every forwarding setter of algodsp.processors against the parameter it names:
one handle of one channel per class, no audio processed.

A row is (setter, arguments, {config field: value it must hold afterwards},
getter or None).  After the call every field of the row holds its value, the
row's first field differs from what it was (the value is not the default), the
getter returns the value, and no other field changed, apart from the class's
`derived` fields: the coefficients that the library recomputes from the times
and the sample rate (ad_*_set_param).  One rejected value per class raises
ErrInvalidArgument and leaves the configuration byte for byte as it was.  Values
that another test already uses are taken from there (test_fdn_gpu MIDSTREAM,
test_delayfx_gpu FL_MIDSTREAM, test_dynfx_gpu, test_lookahead_gpu,
test_vocoder_gpu, test_abi GOOD_COMPRESSOR_EDGES, reference_kats.json).
"""
import ctypes as C

import pytest

from algodsp import _lib
from algodsp import processors as P

pytestmark = pytest.mark.gpu

FS = 48000.0
TOGGLE = object()  # a boolean setter: the opposite of what the field holds


def _value(v):
    if isinstance(v, C.Array):
        return list(v)
    if isinstance(v, C._Pointer):
        return C.cast(v, C.c_void_p).value
    return v


def _fields(cfg):
    return {n: _value(getattr(cfg, n)) for n, _ in cfg._fields_}


def state(h):
    """(every field by name, the bytes of the configuration structures)."""
    if isinstance(h, P.MultibandCompressor):
        cfgs = [h._band(b) for b in range(h.NumBands())]
        return {(b, n): v for b, c in enumerate(cfgs) for n, v in _fields(c).items()}, b"".join(map(bytes, cfgs))
    if isinstance(h, P.Reverb):
        return {n: getattr(h, n) for n in ("wet", "dry", "room", "damp", "gain")}, b""
    if isinstance(h, P.Compressor):
        s = _fields(h.cfg)
        if isinstance(h, P.Expander):
            s.update(range_db=h.range_db, hold_ms=h.hold_ms)
        return s, bytes(h.cfg)
    return _fields(h.config()), bytes(h.config())


def _simple_delay():
    cfg = _lib.DelayConfig()
    _lib.lib().ad_delay_default_config(C.byref(cfg), FS)
    cfg.mode, cfg.delay_samples = 1, 10
    return P.Delay(FS, 1, config=cfg)


COMPRESSOR_ROWS = [
    ("SetThreshold", (-60.0,), {"threshold_db": -60.0}, None),
    ("SetRatio", (100.0,), {"ratio": 100.0}, None),
    ("SetKnee", (24.0,), {"knee_db": 24.0}, None),
    ("SetAttack", (1000.0,), {"attack_ms": 1000.0}, None),
    ("SetRelease", (5000.0,), {"release_ms": 5000.0}, None),
    ("SetRMSWindow", (1000.0,), {"rms_window_ms": 1000.0}, None),
    ("SetSidechainLowCut", (150.0,), {"sidechain_low_cut_hz": 150.0}, None),
    ("SetSidechainHighCut", (6000.0,), {"sidechain_high_cut_hz": 6000.0}, None),
    ("SetAutoMakeup", (TOGGLE,), {"auto_makeup": TOGGLE}, None),
    ("SetAutoMakeup", (TOGGLE,), {"auto_makeup": TOGGLE}, None),  # on again: SetMakeupGain turns it off
    ("SetMakeupGain", (6.0,), {"makeup_db": 6.0, "auto_makeup": 0}, None),  # core.go:201-210
    ("SetTopology", (1,), {"topology": 1}, None),
    ("SetDetectorMode", (1,), {"detector_mode": 1}, None),
    ("SetFeedbackRatioScale", (TOGGLE,), {"feedback_ratio_scale": TOGGLE}, None),
]

# MultibandCompressor's SetBand<suffix> / SetAllBands<suffix>:
# (suffix, value, {field: value}, BandView getter, has a SetAllBands form)
BAND_ROWS = [
    ("Threshold", -12.0, {"threshold_db": -12.0}, "Threshold", True),
    ("Ratio", 10.0, {"ratio": 10.0}, "Ratio", True),
    ("Knee", 9.0, {"knee_db": 9.0}, "Knee", True),
    ("Attack", 2.0, {"attack_ms": 2.0}, "Attack", True),
    ("Release", 30.0, {"release_ms": 30.0}, "Release", True),
    ("AutoMakeup", False, {"auto_makeup": 0}, "AutoMakeup", False),
    ("MakeupGain", 2.0, {"makeup_db": 2.0, "auto_makeup": 0}, "MakeupGain", False),
    ("Topology", 1, {"topology": 1}, "Topology", True),
    ("DetectorMode", 1, {"detector_mode": 1}, "DetectorMode", True),
    ("FeedbackRatioScale", False, {"feedback_ratio_scale": 0}, "FeedbackRatioScale", True),
    ("RMSWindow", 20.0, {"rms_window_ms": 20.0}, "RMSWindow", True),
    ("SidechainLowCut", 150.0, {"sidechain_low_cut_hz": 150.0}, "SidechainLowCut", False),
    ("SidechainHighCut", 6000.0, {"sidechain_high_cut_hz": 6000.0}, "SidechainHighCut", False),
]

# name: (constructor, derived fields, rows, (setter, arguments) that is rejected or None)
CASES = {
    "FDNReverb": (lambda: P.FDNReverb(44100.0, 1), (), [
        ("SetSampleRate", (11025.0,), {"sample_rate": 11025.0}, "SampleRate"),
        ("SetWet", (0.7,), {"wet": 0.7}, "Wet"),
        ("SetDry", (0.1,), {"dry": 0.1}, "Dry"),
        ("SetRT60", (0.9,), {"rt60_seconds": 0.9}, "RT60"),
        ("SetDamp", (0.8,), {"damp": 0.8}, "Damp"),
        ("SetPreDelay", (0.02,), {"pre_delay_seconds": 0.02}, "PreDelay"),
        ("SetModDepth", (0.004,), {"mod_depth_seconds": 0.004}, "ModDepth"),
        ("SetModRate", (0.5,), {"mod_rate_hz": 0.5}, "ModRate"),
    ], ("SetDamp", (1.5,))),
    "Delay": (lambda: P.Delay(FS, 1), ("smooth_coeff",), [
        ("SetSampleRate", (8000.0,), {"sample_rate": 8000.0}, "SampleRate"),
        ("SetTime", (0.1,), {"time_seconds": 0.1}, "Time"),
        ("SetTargetTime", (0.3,), {"time_seconds": 0.3}, "Time"),
        ("SetFeedback", (0.9,), {"feedback": 0.9}, "Feedback"),
        ("SetMix", (1.0,), {"mix": 1.0}, "Mix"),
        ("SetSmoothCoeff", (0.125,), {"smooth_coeff": 0.125}, None),
    ], ("SetFeedback", (1.0,))),
    "Delay mode 1": (_simple_delay, (), [
        ("SetDelaySamples", (25,), {"delay_samples": 25}, None),
    ], ("SetDelaySamples", (2.5,))),
    "Flanger": (lambda: P.Flanger(FS, 1), (), [
        ("SetSampleRate", (44100.0,), {"sample_rate": 44100.0}, "SampleRate"),
        ("SetRateHz", (2.0,), {"rate_hz": 2.0}, "RateHz"),
        ("SetDepthSeconds", (0.004,), {"depth_seconds": 0.004}, "DepthSeconds"),
        ("SetBaseDelaySeconds", (0.0003,), {"base_delay_seconds": 0.0003}, "BaseDelaySeconds"),
        ("SetFeedback", (-0.8,), {"feedback": -0.8}, "Feedback"),
        ("SetMix", (1.0,), {"mix": 1.0}, "Mix"),
    ], ("SetMix", (2.0,))),
    "Phaser": (lambda: P.Phaser(FS, 1), (), [
        ("SetSampleRate", (44100.0,), {"sample_rate": 44100.0}, "SampleRate"),
        ("SetRateHz", (1.5,), {"rate_hz": 1.5}, "RateHz"),
        ("SetStages", (4,), {"stages": 4}, "Stages"),
        ("SetFeedback", (-0.5,), {"feedback": -0.5}, "Feedback"),
        ("SetMix", (0.25,), {"mix": 0.25}, "Mix"),
    ], ("SetStages", (0,))),
    "Tremolo": (lambda: P.Tremolo(FS, 1), ("smoothing_coeff",), [
        ("SetSampleRate", (44100.0,), {"sample_rate": 44100.0}, "SampleRate"),
        ("SetRateHz", (7.0,), {"rate_hz": 7.0}, "RateHz"),
        ("SetDepth", (0.25,), {"depth": 0.25}, "Depth"),
        ("SetSmoothingMs", (2.0,), {"smoothing_ms": 2.0}, "SmoothingMs"),
        ("SetMix", (0.5,), {"mix": 0.5}, "Mix"),
        ("SetSmoothingCoeff", (0.125,), {"smoothing_coeff": 0.125}, None),
    ], ("SetDepth", (2.0,))),
    "RingModulator": (lambda: P.RingModulator(FS, 1), (), [
        ("SetSampleRate", (44100.0,), {"sample_rate": 44100.0}, "SampleRate"),
        ("SetCarrierHz", (1000.0,), {"carrier_hz": 1000.0}, "CarrierHz"),
        ("SetMix", (0.5,), {"mix": 0.5}, "Mix"),
    ], ("SetMix", (-1.0,))),
    "Distortion": (lambda: P.Distortion(FS, 1), (), [
        ("SetSampleRate", (44100.0,), {"sample_rate": 44100.0}, "SampleRate"),
        ("SetMode", (14,), {"mode": 14}, "Mode"),
        ("SetApproxMode", (1,), {"approx": 1}, None),
        ("SetDrive", (5.0,), {"drive": 5.0}, "Drive"),
        ("SetMix", (0.5,), {"mix": 0.5}, "Mix"),
        ("SetOutputLevel", (2.0,), {"output_level": 2.0}, "OutputLevel"),
        ("SetClipLevel", (0.5,), {"clip_level": 0.5}, "ClipLevel"),
        ("SetShape", (0.25,), {"shape": 0.25}, "Shape"),
        ("SetBias", (-0.5,), {"bias": -0.5}, "Bias"),
        ("SetChebyshevOrder", (5,), {"cheb_order": 5}, "ChebyshevOrder"),
        ("SetChebyshevHarmonicMode", (1,), {"cheb_harmonic": 1}, None),
        ("SetChebyshevInvert", (TOGGLE,), {"cheb_invert": TOGGLE}, None),
        ("SetChebyshevGainLevel", (2.0,), {"cheb_gain": 2.0}, None),
        ("SetChebyshevDCBypass", (TOGGLE,), {"cheb_dc_bypass": TOGGLE}, None),
    ], ("SetDrive", (0.0,))),
    "BitCrusher": (lambda: P.BitCrusher(FS, 1), (), [
        ("SetSampleRate", (44100.0,), {"sample_rate": 44100.0}, "SampleRate"),
        ("SetBitDepth", (12.0,), {"bit_depth": 12.0}, "BitDepth"),
        ("SetDownsample", (4,), {"downsample": 4}, "Downsample"),
        ("SetMix", (0.5,), {"mix": 0.5}, "Mix"),
    ], ("SetDownsample", (0,))),
    "TransientShaper": (lambda: P.TransientShaper(FS, 1), ("attack_coeff", "release_coeff"), [
        ("SetSampleRate", (44100.0,), {"sample_rate": 44100.0}, "SampleRate"),
        ("SetAttackAmount", (0.5,), {"attack_amount": 0.5}, "AttackAmount"),
        ("SetSustainAmount", (-0.5,), {"sustain_amount": -0.5}, "SustainAmount"),
        ("SetAttack", (2.0,), {"attack_ms": 2.0}, "Attack"),
        ("SetRelease", (30.0,), {"release_ms": 30.0}, "Release"),
        ("SetAttackCoeff", (0.125,), {"attack_coeff": 0.125}, None),
        ("SetReleaseCoeff", (0.0625,), {"release_coeff": 0.0625}, None),
    ], ("SetAttack", (0.05,))),
    "DeEsser": (lambda: P.DeEsser(FS, 1), ("attack_coeff", "release_coeff"), [
        ("SetSampleRate", (44100.0,), {"sample_rate": 44100.0}, "SampleRate"),
        ("SetFrequency", (7000.0,), {"freq_hz": 7000.0}, "Frequency"),
        ("SetQ", (3.0,), {"q": 3.0}, "Q"),
        ("SetThreshold", (-35.0,), {"threshold_db": -35.0}, "Threshold"),
        ("SetRatio", (10.0,), {"ratio": 10.0}, "Ratio"),
        ("SetKnee", (0.0,), {"knee_db": 0.0}, "Knee"),
        ("SetAttack", (2.0,), {"attack_ms": 2.0}, "Attack"),
        ("SetRelease", (5.0,), {"release_ms": 5.0}, "Release"),
        ("SetRange", (-6.0,), {"range_db": -6.0}, "Range"),
        ("SetMode", (1,), {"mode": 1}, "Mode"),
        ("SetDetector", (1,), {"detector": 1}, "Detector"),
        ("SetListen", (TOGGLE,), {"listen": TOGGLE}, "Listen"),
        ("SetFilterOrder", (4,), {"filter_order": 4}, "FilterOrder"),
        ("SetAttackCoeff", (0.125,), {"attack_coeff": 0.125}, None),
        ("SetReleaseCoeff", (0.0625,), {"release_coeff": 0.0625}, None),
    ], ("SetQ", (11.0,))),
    "Vocoder": (lambda: P.Vocoder(FS, 1), (), [
        ("SetSampleRate", (44100.0,), {"sample_rate": 44100.0}, "SampleRate"),
        ("SetAttack", (3.0,), {"attack_ms": 3.0}, "Attack"),
        ("SetRelease", (40.0,), {"release_ms": 40.0}, "Release"),
        ("SetInputLevel", (1.0,), {"input_level": 1.0}, "InputLevel"),
        ("SetSynthLevel", (0.5,), {"synth_level": 0.5}, "SynthLevel"),
        ("SetVocoderLevel", (10.0,), {"vocoder_level": 10.0}, "VocoderLevel"),
        ("SetDownsampling", (TOGGLE,), {"downsample": TOGGLE}, "Downsampling"),
    ], ("SetAttack", (0.005,))),
    "LookaheadLimiter": (lambda: P.LookaheadLimiter(FS, 1), (), [
        ("SetSampleRate", (44100.0,), {"sample_rate": 44100.0}, "SampleRate"),
        ("SetThreshold", (-20.0,), {"threshold_db": -20.0}, "Threshold"),
        ("SetRelease", (5.0,), {"release_ms": 5.0}, "Release"),
        ("SetLookahead", (1.0,), {"lookahead_ms": 1.0}, "Lookahead"),
    ], ("SetRelease", (0.5,))),
    "SpectralFreeze": (lambda: P.SpectralFreeze(FS, 1, frame_size=256, hop_size=64), (), [
        ("SetSampleRate", (44100.0,), {"sample_rate": 44100.0}, "SampleRate"),
        ("SetHopSize", (32,), {"hop_size": 32}, "HopSize"),
        ("SetMix", (0.5,), {"mix": 0.5}, "Mix"),
        ("SetPhaseMode", (P.SpectralFreeze.PhaseHold,), {"phase_mode": P.SpectralFreeze.PhaseHold}, "PhaseMode"),
    ], ("SetHopSize", (0,))),
    # the resampling prototype follows the ratio, the hop and the quality (_sync_taps)
    "SpectralPitchShifter": (lambda: P.SpectralPitchShifter(FS, 1, frame_size=256, analysis_hop=64),
                             ("resample_taps", "n_resample_taps"), [
        ("SetSampleRate", (44100.0,), {"sample_rate": 44100.0}, "SampleRate"),
        ("SetPitchRatio", (1.1,), {"pitch_ratio": 1.1}, "PitchRatio"),
        ("SetAnalysisHop", (32,), {"analysis_hop": 32}, "AnalysisHop"),
        ("SetResampleQuality", (0,), {"resample_quality": 0}, "ResampleQuality"),
    ], ("SetPitchRatio", (8.0,))),
    "Compressor": (lambda: P.Compressor(FS, 1), (), COMPRESSOR_ROWS, ("SetRatio", (0.5,))),
    "Expander": (lambda: P.Expander(FS, 1), (), COMPRESSOR_ROWS + [
        ("SetRange", (-30.0,), {"range_db": -30.0}, None),
    ], ("SetRelease", (0.5,))),
    "Gate": (lambda: P.Gate(FS, 1), (), COMPRESSOR_ROWS + [
        ("SetRange", (-20.0,), {"range_db": -20.0}, None),
        ("SetHold", (5000.0,), {"hold_ms": 5000.0}, None),
    ], ("SetHold", (-1.0,))),
    # the reference's Freeverb setters reject nothing (reverb.go:192-220), so there is no rejected row
    "Reverb": (lambda: P.Reverb(1), (), [
        ("SetWet", (0.5,), {"wet": 0.5}, None),
        ("SetDry", (0.25,), {"dry": 0.25}, None),
        ("SetRoomSize", (0.9,), {"room": 0.9}, None),
        ("SetDamp", (0.125,), {"damp": 0.125}, None),
        ("SetGain", (0.03,), {"gain": 0.03}, None),
    ], None),
}


def apply_row(h, derived, setter, args, want, getter, key=lambda f: f):
    before, _ = state(h)
    want = {key(f): (not bool(before[key(f)])) if v is TOGGLE else v for f, v in want.items()}
    args = tuple(next(iter(want.values())) if a is TOGGLE else a for a in args)
    getattr(h, setter)(*args)
    after, _ = state(h)
    for f, v in want.items():
        assert after[f] == v, (setter, f, after[f])
    changed = {f for f in after if after[f] != before[f]}
    assert next(iter(want)) in changed, (setter, "the value is the default")
    loose = {key(f) for f in derived}
    assert changed - loose <= set(want), (setter, sorted(changed, key=str))
    if getter:
        got = getter(h) if callable(getter) else getattr(h, getter)()
        assert got == next(iter(want.values())), (setter, getter, got)


@pytest.mark.parametrize("name", list(CASES))
def test_setters_reach_their_parameter(gpu, name):
    make, derived, rows, reject = CASES[name]
    h = make()
    try:
        for row in rows:
            apply_row(h, derived, *row)
        if reject:
            before = state(h)
            with pytest.raises(_lib.ErrInvalidArgument):
                getattr(h, reject[0])(*reject[1])
            assert state(h) == before
    finally:
        h.close()


def test_multiband_band_setters(gpu):
    """Two bands.  SetBandX(b, v) changes band b alone; SetAllBandsX(v) changes both; a value that only band 1
    rejects stops SetAllBandsX there with band 0 changed (multiband.go:331-437)."""
    h = P.MultibandCompressor((1000.0,), 4, FS, 1)
    try:
        for suffix, v, want, getter, _ in BAND_ROWS:
            for b in (1, 0):
                apply_row(h, (), "SetBand" + suffix, (b, v), want, lambda m: getattr(m.Band(b), getter)(),
                          key=lambda f: (b, f))
        before = state(h)
        with pytest.raises(_lib.ErrInvalidArgument):
            h.SetBandRatio(1, 0.5)
        with pytest.raises(_lib.ErrInvalidArgument):
            h.SetBandThreshold(2, -20.0)  # no such band
        assert state(h) == before
    finally:
        h.close()
    h = P.MultibandCompressor((1000.0,), 4, FS, 1)
    try:
        for suffix, v, want, getter, all_bands in BAND_ROWS:
            if not all_bands:
                assert not hasattr(h, "SetAllBands" + suffix)
                continue
            before, _ = state(h)
            getattr(h, "SetAllBands" + suffix)(v)
            after, _ = state(h)
            (field, value), = want.items()
            assert {f for f in after if after[f] != before[f]} == {(0, field), (1, field)}, suffix
            assert (after[(0, field)], after[(1, field)]) == (value, value)
        # band 1's detector high cut at 100 Hz makes a 150 Hz low cut invalid there alone; the attack of 0.01 ms
        # is invalid everywhere, so band 0 stops it
        h.SetBandSidechainHighCut(1, 100.0)
        before, _ = state(h)
        with pytest.raises(_lib.ErrInvalidArgument):
            h._all("SetBandSidechainLowCut", 150.0)
        after, _ = state(h)
        assert {f for f in after if after[f] != before[f]} == {(0, "sidechain_low_cut_hz")}
        assert after[(0, "sidechain_low_cut_hz")] == 150.0
        before = state(h)
        with pytest.raises(_lib.ErrInvalidArgument):
            h.SetAllBandsAttack(0.01)
        assert state(h) == before
    finally:
        h.close()
