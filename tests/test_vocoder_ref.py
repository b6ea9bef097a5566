"""The vocoder restatement (tests/vocoder_ref.py) against the reference's own
tests (dsp/effects/vocoder_test.go), restated, and the host tables of the GPU
runtime (ad_vocoder_derived, host only) against the restatement on bits.  No
GPU is needed."""
import cmath
import ctypes as C
import math

import numpy as np
import pytest

import vocoder_ref as R
from algodsp import _lib, processors as P

NAN, INF = float("nan"), float("inf")


def sine(freq, n, fs=48000.0, start=0):
    return [math.sin(2 * math.pi * freq * float(i) / fs) for i in range(start, start + n)]


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


@pytest.mark.parametrize("sr,kw", [
    (0, {}), (-1, {}), (NAN, {}), (INF, {}), (48000, dict(layout=99)), (48000, dict(attackMs=-1)),
    (48000, dict(attackMs=NAN)), (48000, dict(releaseMs=-1)), (48000, dict(releaseMs=NAN)),
    (48000, dict(inputLevel=-1)), (48000, dict(inputLevel=11)), (48000, dict(synthLevel=-1)),
    (48000, dict(vocoderLevel=-1)), (48000, dict(synthQ=0.01)), (48000, dict(synthQ=25))])
def test_new_vocoder_validation(sr, kw):  # TestNewVocoderValidation
    with pytest.raises(ValueError):
        R.Vocoder(sr, **kw)


def test_defaults():  # TestNewVocoderDefaults
    v = R.Vocoder(48000)
    assert (v.Layout(), v.SampleRate(), v.Attack(), v.Release()) == (R.THIRD_OCTAVE, 48000, 0.5, 2.0)
    assert (v.InputLevel(), v.SynthLevel(), v.VocoderLevel(), v.NumBands()) == (0, 0, 1, 32)
    assert v.SynthesisQ() == R.thirdOctaveQ and not v.Downsampling() and v.DownsampleFactors() is None


@pytest.mark.parametrize("fs,third,bark", [(48000, 32, 24), (44100, 31, 24), (8000, 24, 16)])
def test_band_counts(fs, third, bark):  # TestNewVocoderBandCountAtLowSampleRate, pinned from the tables
    assert R.Vocoder(fs).NumBands() == third
    assert R.Vocoder(fs, layout=R.BARK).NumBands() == bark


def test_band_counts_at_100_hz():
    assert R.Vocoder(100).NumBands() == 5
    with pytest.raises(ValueError, match="no usable Bark bands"):
        R.Vocoder(100, layout=R.BARK)


@pytest.mark.parametrize("layout", [R.THIRD_OCTAVE, R.BARK])
def test_silent_modulator_produces_silence(layout):  # TestVocoderSilentModulatorProducesSilence
    v = R.Vocoder(48000, layout=layout)
    assert max(abs(v.ProcessSample(0.0, c)) for c in sine(1000, 1000)) <= 1e-6


@pytest.mark.parametrize("layout", [R.THIRD_OCTAVE, R.BARK])
@pytest.mark.parametrize("downsample", [False, True])
def test_output_is_live_and_bounded(layout, downsample):  # TestVocoderNonSilentOutput, OutputBounded, DownsamplingProducesOutput
    v = R.Vocoder(48000, layout=layout, downsample=downsample)
    sig = [a + 0.5 * b for a, b in zip(sine(1000, 2000), sine(200, 2000))]
    out = [abs(v.ProcessSample(s, s)) for s in sig]
    assert all(math.isfinite(o) for o in out)
    assert sum(out) / len(out) >= 1e-6 and max(out) <= 10


def test_process_block_is_the_sample_loop_and_many_is_the_block():  # TestVocoderProcessBlock
    rng = np.random.default_rng(7)
    m, c = rng.standard_normal((3, 300)), rng.standard_normal((3, 300))
    for downsample in (False, True):
        kw = dict(downsample=downsample, inputLevel=0.3, synthLevel=0.2, layout=R.BARK)
        many = R.Vocoder(48000, channels=3, **kw).process_many(m, c)
        for ch in range(3):
            one = R.Vocoder(48000, **kw)
            want = [one.ProcessSample(float(a), float(b)) for a, b in zip(m[ch], c[ch])]
            assert np.array_equal(bits(many[ch]), bits(want))
            assert np.array_equal(bits(R.Vocoder(48000, **kw).ProcessBlock(m[ch], c[ch])), bits(want))
    with pytest.raises(ValueError):
        R.Vocoder(48000).ProcessBlock([0.0] * 3, [0.0] * 4)


@pytest.mark.parametrize("downsample", [False, True])
def test_reset(downsample):  # TestVocoderReset, TestVocoderDownsamplingResetClearsCounter
    v = R.Vocoder(48000, downsample=downsample)
    s = sine(1000, 137)
    first = [v.ProcessSample(x, x) for x in s]
    if downsample:
        assert v.downsampleCount == 137 % 128
    v.Reset()
    assert v.downsampleCount == 0 and not v.envelopes.any() and not v.synthesisFilters.any()
    assert [v.ProcessSample(x, x) for x in s] == first


def test_set_sample_rate():  # TestVocoderSetSampleRate, TestVocoderDownsamplingSetSampleRateRecomputes
    v = R.Vocoder(48000, downsample=True)
    for x in sine(1000, 50):
        v.ProcessSample(x, x)
    before = v.DownsampleFactors()
    v.SetSampleRate(8000)
    assert (v.SampleRate(), v.NumBands()) == (8000, 24)
    assert len(v.DownsampleFactors()) == 24 and v.DownsampleFactors() != before[:24]
    assert v.downsampleCount == 0 and not v.envelopes.any() and not v.analysisFilters.any()
    for bad in (0, -1, NAN, INF):
        with pytest.raises(ValueError):
            v.SetSampleRate(bad)
    assert v.SampleRate() == 8000
    # the reference would assign and then fail in buildFilterBanks; the runtime and this restatement refuse first
    b = R.Vocoder(48000, layout=R.BARK)
    with pytest.raises(ValueError, match="no usable Bark bands"):
        b.SetSampleRate(100)
    assert (b.SampleRate(), b.NumBands()) == (48000, 24)


def test_setters_roundtrip_and_validation():  # TestVocoderSetterGetterRoundtrip, TestVocoderSetterValidation
    v = R.Vocoder(48000)
    for name, getter, good, bad in [("SetAttack", "Attack", 5.0, [0.001, 101, NAN, INF]),
                                    ("SetRelease", "Release", 50.0, [0.001, 1001, NAN]),
                                    ("SetInputLevel", "InputLevel", 0.5, [-1, 11, NAN]),
                                    ("SetSynthLevel", "SynthLevel", 0.7, [-1, 11, INF]),
                                    ("SetVocoderLevel", "VocoderLevel", 2.0, [-1, 11, NAN])]:
        getattr(v, name)(good)
        assert getattr(v, getter)() == good
        for b in bad:
            with pytest.raises(ValueError):
                getattr(v, name)(b)
            assert getattr(v, getter)() == good
    assert v.attackCoeff == 1.0 - math.exp(-1.0 / (5.0 * 0.001 * 48000))
    assert v.releaseCoeff == math.exp(-1.0 / (50.0 * 0.001 * 48000))


def test_envelope_asymmetry():  # TestVocoderEnvelopeAsymmetry
    v = R.Vocoder(48000, attackMs=0.1, releaseMs=200)
    for s in sine(1000, 2000):
        v.ProcessSample(s, s)
    steady = math.sqrt(sum(v.ProcessSample(s, s) ** 2 for s in sine(1000, 500, start=2000)) / 500)
    decay = math.sqrt(sum(v.ProcessSample(0.0, s) ** 2 for s in sine(1000, 500, start=2500)) / 500)
    assert steady >= 1e-6 and decay / steady >= 0.2


def test_dry_mix():  # TestVocoderDryMix
    v = R.Vocoder(48000, vocoderLevel=0, inputLevel=1)
    for i in range(100):
        assert abs(v.ProcessSample(i * 0.01, i * 0.05) - i * 0.01) <= 1e-12


def test_bark_synthesis_q_defaults_and_override():  # TestVocoderBarkLayout, BarkSynthesisQDefaultsAndOverride
    v = R.Vocoder(48000, layout=R.BARK)
    assert v.Layout() == R.BARK and v.NumBands() == 24
    for i in range(24):
        assert v.synthesisCoeffs[i] == R.cpgBandpass(R.barkFrequencies[i], R.barkBandQ(i), 48000.0)
        assert v.synthesisCoeffs[i] == v.analysisCoeffs[i]
    o = R.Vocoder(48000, layout=R.BARK, synthQ=2.0)
    for i in range(24):
        assert o.synthesisCoeffs[i] == R.cpgBandpass(R.barkFrequencies[i], 2.0, 48000.0)
        assert o.analysisCoeffs[i] == v.analysisCoeffs[i]
    assert R.barkBandQ(0) == 100 / (150 - 50) and R.barkBandQ(23) == 15500 / (15500 * 1.25 - (12000 + 15500) / 2)


def test_downsampling_option_and_setter():  # TestVocoderDownsamplingDefault, Option, SetDownsampling
    assert not R.Vocoder(48000).Downsampling()
    v = R.Vocoder(48000, downsample=True)
    assert v.Downsampling() and len(v.DownsampleFactors()) == 32
    v.SetDownsampling(False)
    assert not v.Downsampling() and v.DownsampleFactors() is None and v.downsampleMax == 0
    v.SetDownsampling(True)
    assert v.Downsampling() and v.DownsampleFactors() is not None


def test_set_downsampling_keeps_envelopes_and_full_rate_sections():
    v = R.Vocoder(48000)
    for s in sine(1000, 100):
        v.ProcessSample(s, s)
    env, ana, syn = v.envelopes.copy(), v.analysisFilters.copy(), v.synthesisFilters.copy()
    v.SetDownsampling(True)
    assert np.array_equal(v.envelopes, env) and np.array_equal(v.analysisFilters, ana)
    assert np.array_equal(v.synthesisFilters, syn)
    for s in sine(1000, 77):
        v.ProcessSample(s, s)
    assert v.downsampleCount == 77 and v.downsampleAnalysisFilters.any() and v.downsampleGroupAAFilters.any()
    assert np.array_equal(v.analysisFilters, ana)  # the full-rate analysis sections rest while downsampling
    v.SetDownsampling(True)  # on again: rebuilt all the same
    assert v.downsampleCount == 0 and not v.downsampleAnalysisFilters.any() and not v.downsampleGroupAAFilters.any()
    assert v.envelopes.any()


def test_downsample_factors():  # TestVocoderDownsampleFactors
    v = R.Vocoder(44100, downsample=True)
    f = v.DownsampleFactors()
    assert len(f) == v.NumBands() == 31
    assert all(x >= 1 and x & (x - 1) == 0 for x in f)
    assert f[0] > f[-1] == 1
    w = R.Vocoder(48000, downsample=True)
    f = w.DownsampleFactors()
    assert (min(f), max(f), w.downsampleMax) == (1, 128, 128)
    assert w.downsampleGroupFactors == [1, 2, 4, 8, 16, 32, 64, 128]
    assert sorted(b for g in w.downsampleGroupBands for b in g) == list(range(32))


@pytest.mark.parametrize("layout", [R.THIRD_OCTAVE, R.BARK])
def test_retuned_multirate_analysis_sections(layout):  # ...BuildsRetunedMultirateAnalysisFilters
    v = R.Vocoder(48000.0, layout=layout, downsample=True)
    freqs = R.thirdOctaveFrequencies if layout == R.THIRD_OCTAVE else R.barkFrequencies
    assert len(v.downsampleAnalysisCoeffs) == v.NumBands()
    for i in range(v.NumBands()):
        factor = v.downsampleFactors[i]
        q = R.thirdOctaveQ if layout == R.THIRD_OCTAVE else R.barkBandQ(i)
        assert v.downsampleAnalysisCoeffs[i] == R.cpgBandpass(freqs[i], q, 48000.0 / float(factor))
        assert (factor > 1) == (v.downsampleAnalysisCoeffs[i] != v.analysisCoeffs[i])


def magnitude_squared(c, freq, fs):
    b0, b1, b2, a1, a2 = c
    z = cmath.exp(-1j * 2 * math.pi * freq / fs)
    return abs((b0 + b1 * z + b2 * z * z) / (1 + a1 * z + a2 * z * z)) ** 2


def test_anti_alias_sections():  # TestVocoderDownsamplingBuildsAntiAliasFilters
    v = R.Vocoder(48000.0, downsample=True)
    assert len(v.downsampleGroupAACoeffs) == len(v.downsampleGroupFactors) == v.downsampleGroupAAFilters.shape[1]
    for g, factor in enumerate(v.downsampleGroupFactors):
        c = v.downsampleGroupAACoeffs[g]
        if factor == 1:
            assert c == (1.0, 0.0, 0.0, 0.0, 0.0)
            continue
        nyq = 0.5 * 48000.0 / float(factor)
        assert magnitude_squared(c, 0.2 * nyq, 48000.0) >= 0.7
        assert magnitude_squared(c, nyq, 48000.0) <= 0.2


def test_envelope_coefficients_are_factor_aware():  # ...EnvelopeCoefficientsAreFactorAware
    v = R.Vocoder(48000.0, downsample=True, attackMs=12.0, releaseMs=80.0)
    f = v.DownsampleFactors()
    assert len(f) == len(v.downsampleAttackCoeffs) == len(v.downsampleReleaseCoeffs)
    for i, factor in enumerate(f):
        assert v.downsampleAttackCoeffs[i] == 1.0 - math.exp(-float(factor) / (12.0 * 0.001 * 48000.0))
        assert v.downsampleReleaseCoeffs[i] == math.exp(-float(factor) / (80.0 * 0.001 * 48000.0))
    v.SetAttack(3.0)
    assert v.downsampleAttackCoeffs[0] == 1.0 - math.exp(-128.0 / (3.0 * 0.001 * 48000.0))


def test_a_nan_level_takes_the_release_form():
    v = R.Vocoder(48000, channels=2)
    out = v.process_many(np.array([[NAN, 0.0, 0.0], [1.0, 0.5, 0.25]]), np.ones((2, 3)))
    one = R.Vocoder(48000)
    assert np.isnan(out[0]).all() and np.isnan(v.envelopes[0]).all()
    assert [one.ProcessSample(a, 1.0) for a in (1.0, 0.5, 0.25)] == list(out[1])


# ---- the GPU runtime's host tables: the same bits, without a device ----------
def config(fs, **kw):
    cfg = _lib.VocoderConfig()
    _lib.lib().ad_vocoder_default_config(C.byref(cfg), float(fs))
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


@pytest.mark.parametrize("downsample", [0, 1])
@pytest.mark.parametrize("fs,layout,q", [(fs, layout, q) for fs in (48000.0, 44100.0, 8000.0, 22050.0, 96000.0)
                                         for layout in (0, 1) for q in (None, 0.1, 20.0)] + [(100.0, 0, None)])
def test_host_tables_are_the_restatements(fs, layout, q, downsample):
    kw = {} if q is None else dict(synth_q=q, synth_q_set=1)
    d = P.vocoder_derived(config(fs, layout=layout, downsample=downsample, attack_ms=1.7, release_ms=33.0, **kw))
    r = R.Vocoder(fs, layout=layout, synthQ=q, downsample=bool(downsample), attackMs=1.7, releaseMs=33.0)
    assert d["num_bands"] == r.numBands
    assert np.array_equal(bits(d["analysis"]), bits(r.analysisCoeffs))
    assert np.array_equal(bits(d["synthesis"]), bits(r.synthesisCoeffs))
    assert bits([d["attack_coeff"], d["release_coeff"]]).tolist() == bits([r.attackCoeff, r.releaseCoeff]).tolist()
    if not downsample:
        assert d["factors"] is None and d["downsample_max"] == 0 and d["group_factors"] == []
        return
    assert d["factors"] == r.downsampleFactors and d["downsample_max"] == r.downsampleMax
    assert d["group_factors"] == r.downsampleGroupFactors
    assert [[b for b, g in enumerate(d["group_of_band"]) if g == k] for k in range(len(d["group_factors"]))] \
        == r.downsampleGroupBands
    assert np.array_equal(bits(d["decimated"]), bits(r.downsampleAnalysisCoeffs))
    assert np.array_equal(bits(d["antialias"]), bits(r.downsampleGroupAACoeffs))
    assert np.array_equal(bits(d["ds_attack"]), bits(r.downsampleAttackCoeffs))
    assert np.array_equal(bits(d["ds_release"]), bits(r.downsampleReleaseCoeffs))


def test_default_config_and_host_validation():
    cfg = config(48000.0)
    assert (cfg.synth_q, cfg.attack_ms, cfg.release_ms, cfg.input_level, cfg.synth_level, cfg.vocoder_level) \
        == (R.thirdOctaveQ, 0.5, 2.0, 0.0, 0.0, 1.0)
    assert (cfg.layout, cfg.synth_q_set, cfg.downsample) == (0, 0, 0)
    L = _lib.lib()
    assert L.ad_vocoder_validate(C.byref(cfg)) == _lib.AD_OK
    for kw in (dict(sample_rate=0.0), dict(sample_rate=NAN), dict(sample_rate=INF), dict(layout=2), dict(layout=-1),
               dict(synth_q=0.05), dict(synth_q=NAN), dict(attack_ms=0.005), dict(attack_ms=100.5),
               dict(release_ms=0.005), dict(release_ms=1000.5), dict(input_level=-0.5), dict(synth_level=10.5),
               dict(vocoder_level=NAN), dict(downsample=2), dict(synth_q_set=-1), dict(sample_rate=100.0, layout=1)):
        bad = config(48000.0, **kw)
        assert L.ad_vocoder_validate(C.byref(bad)) == _lib.AD_ERR_INVALID_ARGUMENT, kw
    assert b"no usable Bark bands" in L.ad_last_error()
    assert L.ad_vocoder_validate(None) == _lib.AD_ERR_INVALID_ARGUMENT
    for kw in (dict(attack_ms=0.01), dict(attack_ms=100.0), dict(release_ms=1000.0), dict(synth_q=0.1),
               dict(synth_q=20.0), dict(input_level=10.0), dict(sample_rate=100.0)):
        assert L.ad_vocoder_validate(C.byref(config(48000.0, **kw))) == _lib.AD_OK, kw
