"""The reference's own unit tests of the spectral freeze and the spectral
pitch shifter (dsp/effects/spectral_freeze_test.go,
dsp/effects/pitch/pitch_shift_spectral_test.go) restated against the GPU
processors, with their tolerances as written there.  The measuring transforms
(dominantFrequencyHz, measureSNR) are numpy's.
"""
import math

import numpy as np
import pytest

from algodsp import _lib, processors as P

pytestmark = pytest.mark.gpu

BAD = _lib.ErrInvalidArgument


def sine(freq, fs, amplitude, n):  # testutil.DeterministicSine signals.go:9-18
    step = 2 * math.pi * freq / fs
    return amplitude * np.sin(step * np.arange(n, dtype=np.float64))


# ---- spectral_freeze_test.go --------------------------------------------------
def test_new_spectral_freeze_rejects_invalid_sample_rate(gpu):  # :8-16
    for rate in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(BAD):
            P.SpectralFreeze(rate)


def test_spectral_freeze_mix_zero_passthrough(gpu):  # :18-46
    f = P.SpectralFreeze(48000)
    f.SetMix(0)
    f.Freeze()
    x = np.sin(2 * math.pi * 440 * np.arange(512, dtype=np.float64) / 48000)
    assert float(np.max(np.abs(f.Process(x) - x))) <= 1e-12


def test_spectral_freeze_in_place_matches_out_of_place(gpu):  # :48-95
    f1, f2 = P.SpectralFreeze(48000), P.SpectralFreeze(48000)
    for f in (f1, f2):
        f.SetPhaseMode(P.SpectralFreeze.PhaseAdvance)
        f.Freeze()
    i = np.arange(1024, dtype=np.float64)
    x = np.sin(2 * math.pi * 220 * i / 48000) + 0.2 * np.sin(2 * math.pi * 660 * i / 48000)
    want = f1.Process(x)
    got = x.copy()
    f2.ProcessInPlace(got)
    assert float(np.max(np.abs(got - want))) <= 1e-12


def test_spectral_freeze_reset_deterministic(gpu):  # :97-129
    f = P.SpectralFreeze(48000)
    f.Freeze()
    x = np.zeros(2048)
    x[:512] = np.sin(2 * math.pi * 330 * np.arange(512, dtype=np.float64) / 48000)
    out1 = f.Process(x)
    f.Reset()
    out2 = f.Process(x)
    assert float(np.max(np.abs(out1 - out2))) <= 1e-12


def test_spectral_freeze_sustains_energy_on_silence_tail(gpu):  # :131-172
    f = P.SpectralFreeze(48000)
    f.SetFrameSize(256)
    f.SetHopSize(64)
    f.SetPhaseMode(P.SpectralFreeze.PhaseAdvance)
    f.Freeze()
    x = np.zeros(4096)
    x[:256] = np.sin(2 * math.pi * 440 * np.arange(256, dtype=np.float64) / 48000)
    out = f.Process(x)
    assert float(np.sum(out[1024:] ** 2)) > 1e-3


# ---- pitch_shift_spectral_test.go -----------------------------------------------
@pytest.mark.parametrize("rate,ok", [(44100.0, True), (48000.0, True), (0.0, False), (-1.0, False),
                                     (float("nan"), False), (float("inf"), False)])
def test_new_spectral_pitch_shifter(gpu, rate, ok):  # :11-64
    if not ok:
        with pytest.raises(BAD):
            P.SpectralPitchShifter(rate)
        return
    s = P.SpectralPitchShifter(rate)
    assert s.SampleRate() == rate and s.PitchRatio() == 1.0 and s.FrameSize() == 1024
    assert s.AnalysisHop() == 256 and s.SynthesisHop() == 256 and s.EffectivePitchRatio() == 1


def test_spectral_pitch_shifter_setters_validate(gpu):  # :66-146
    s = P.SpectralPitchShifter(48000)
    for v in (0, 0.1, 6, float("nan"), float("inf")):
        with pytest.raises(BAD):
            s.SetPitchRatio(v)
    with pytest.raises(BAD):
        s.SetPitchSemitones(float("nan"))
    s.SetPitchSemitones(7)
    with pytest.raises(BAD):
        s.SetSampleRate(0)
    s.SetSampleRate(96000)
    for v in (1000, 32):
        with pytest.raises(BAD):
            s.SetFrameSize(v)
    s.SetFrameSize(2048)
    for v in (0, 2048):
        with pytest.raises(BAD):
            s.SetAnalysisHop(v)
    s.SetAnalysisHop(512)
    assert (s.SampleRate(), s.FrameSize(), s.AnalysisHop()) == (96000, 2048, 512)


def test_spectral_pitch_shifter_process_length_and_finite(gpu):  # :148-167
    s = P.SpectralPitchShifter(48000)
    s.SetPitchRatio(1.25)
    x = sine(220, 48000, 0.8, 4096)
    out = s.Process(x)
    assert out.shape == x.shape and np.all(np.isfinite(out))


def test_spectral_pitch_shifter_process_in_place_matches_process(gpu):  # :169-194
    s = P.SpectralPitchShifter(48000)
    s.SetPitchRatio(0.8)
    x = sine(330, 48000, 0.7, 4096)
    want = s.Process(x)
    got = x.copy()
    s.ProcessInPlace(got)
    assert float(np.max(np.abs(got - want))) <= 1e-9


def dominant_frequency_hz(signal, fs):  # :485-524
    mag = np.abs(np.fft.fft(signal)) ** 2
    k = 1 + int(np.argmax(mag[1:len(signal) // 2 + 1]))
    return fs * k / len(signal)


def test_spectral_pitch_shifter_identity_keeps_dominant_frequency(gpu):  # :196-223
    fs, n, b = 48000.0, 8192, 48
    freq = fs * b / n
    s = P.SpectralPitchShifter(fs)
    s.SetPitchRatio(1)
    out = s.Process(sine(freq, fs, 0.8, n))
    got = dominant_frequency_hz(out[n // 4:3 * n // 4], fs)
    assert abs(got - freq) / freq <= 0.04


@pytest.mark.parametrize("ratio", [1.5, 0.75], ids=["up", "down"])
def test_spectral_pitch_shifter_moves_dominant_frequency(gpu, ratio):  # :225-271
    fs, n, b = 48000.0, 8192, 40
    freq = fs * b / n
    s = P.SpectralPitchShifter(fs)
    s.SetPitchRatio(ratio)
    out = s.Process(sine(freq, fs, 0.8, n))
    got = dominant_frequency_hz(out[n // 4:3 * n // 4], fs)
    want = freq * s.EffectivePitchRatio()
    assert abs(got - want) / want <= 0.10


def measure_snr(out, target_freq, fs, fft_len):  # measureSNR :438-483
    mid = max(len(out) // 2 - fft_len // 2, 0)
    spec = np.fft.fft(out[mid:mid + fft_len])
    mag2 = spec.real ** 2 + spec.imag ** 2
    target = int(math.floor(target_freq * fft_len / fs + 0.5))
    k = np.arange(1, fft_len // 2 + 1)
    sig = (k >= target - 10) & (k <= target + 10)
    signal, noise = float(np.sum(mag2[k][sig])), float(np.sum(mag2[k][~sig]))
    return 100.0 if noise <= 1e-30 else 10 * math.log10(signal / noise)


def quality_input(ratio, fs=48000.0, n=32768, fft_len=16384):
    out_freq = 100.0 * fs / fft_len
    in_freq = out_freq / ratio
    return 0.8 * np.sin(2 * math.pi * in_freq * np.arange(n, dtype=np.float64) / fs), out_freq


@pytest.mark.parametrize("ratio", [0.5, 0.75, 1.5, 2.0], ids=["down_octave", "down_fourth", "up_fifth", "up_octave"])
def test_spectral_pitch_shifter_signal_quality(gpu, ratio):  # :273-364
    s = P.SpectralPitchShifter(48000.0)
    s.SetPitchRatio(ratio)
    x, out_freq = quality_input(ratio)
    snr = measure_snr(s.Process(x), out_freq, 48000.0, 16384)
    print(f"ratio {ratio}: SNR {snr:.1f} dB")
    assert snr >= 45


@pytest.mark.parametrize("frame,hop,min_snr", [(1024, 512, -5), (1024, 256, 15), (1024, 128, 45)],
                         ids=["2x_overlap", "4x_overlap", "8x_overlap"])
def test_spectral_pitch_shifter_signal_quality_overlap(gpu, frame, hop, min_snr):  # :366-434
    s = P.SpectralPitchShifter(48000.0)
    s.SetFrameSize(frame)
    s.SetAnalysisHop(hop)
    s.SetPitchRatio(1.1)
    x, out_freq = quality_input(1.1)
    snr = measure_snr(s.Process(x), out_freq, 48000.0, 16384)
    print(f"overlap {frame}/{hop}: SNR {snr:.1f} dB")
    assert snr >= min_snr
