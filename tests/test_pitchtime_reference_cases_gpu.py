"""The reference's own unit tests of the time-domain pitch shifter
(dsp/effects/pitch/pitch_shifter_test.go) restated against the GPU processor,
with their tolerances as written there.  The measuring transforms
(estimateFrequencyAutoCorrelation, measureTimeDomainSNR) are those of
tests/pitchtime_measure.py, numpy's.
"""
import math

import numpy as np
import pytest

from algodsp import _lib, pitch
from pitchtime_measure import bin_sine, estimate_frequency, sine, snr_db

pytestmark = pytest.mark.gpu

BAD = _lib.ErrInvalidArgument


@pytest.mark.parametrize("rate,ok", [(44100.0, True), (48000.0, True), (0.0, False), (-1.0, False),
                                     (float("nan"), False), (float("inf"), False)])
def test_new_pitch_shifter(gpu, rate, ok):  # :11-37
    if not ok:
        with pytest.raises(BAD):
            pitch.PitchShifter(rate)
        return
    p = pitch.PitchShifter(rate)
    assert p.SampleRate() == rate and p.PitchRatio() == 1.0
    assert (p.Sequence(), p.Overlap(), p.Search()) == (82.0, 10.0, 28.0)


def test_set_pitch_ratio(gpu):  # :39-72
    p = pitch.PitchShifter(48000)
    for ratio in (0.5, 1.0, 2.0):
        p.SetPitchRatio(ratio)
        assert p.PitchRatio() == ratio
    for ratio in (0, 0.1, 8.0, float("nan"), float("inf")):
        with pytest.raises(BAD):
            p.SetPitchRatio(ratio)
        assert p.PitchRatio() == 2.0


def test_set_overlap_rejects_overlap_above_sequence(gpu):  # :74-95
    p = pitch.PitchShifter(48000)
    p.SetSequence(20)
    old = p.Overlap()
    with pytest.raises(BAD):
        p.SetOverlap(30)
    assert p.Overlap() == old


def test_identity_is_exact_copy(gpu):  # :97-123
    p = pitch.PitchShifter(48000)
    x = sine(440, 48000, 0.8, 4096)
    out = p.Process(x)
    assert out is not x and np.array_equal(out, x)


def test_process_in_place_matches_process(gpu):  # :125-160
    p1, p2 = pitch.PitchShifter(48000, semitones=7), pitch.PitchShifter(48000, semitones=7)
    x = sine(330, 48000, 0.7, 4096)
    want = p1.Process(x)
    got = x.copy()
    p2.ProcessInPlace(got)
    assert float(np.max(np.abs(got - want))) <= 1e-12


def test_pitch_accuracy(gpu):  # :162-215
    fs, f0 = 48000.0, 220.0
    x = sine(f0, fs, 0.8, 60000)
    up = pitch.PitchShifter(fs)
    up.SetPitchSemitones(12.0)
    assert abs(estimate_frequency(up.Process(x)[8000:52000], fs, 300.0, 600.0) - 2 * f0) <= 10.0
    down = pitch.PitchShifter(fs)
    down.SetPitchSemitones(-12.0)
    assert abs(estimate_frequency(down.Process(x)[8000:52000], fs, 80.0, 180.0) - 0.5 * f0) <= 6.0


def test_short_buffer_produces_finite_values(gpu):  # :217-240
    p = pitch.PitchShifter(48000, pitch_ratio=1.7)
    out = p.Process(np.array([1, -0.25, 0.1, 0, -0.1, 0.2, -0.3, 0.4]))
    assert len(out) == 8 and np.all(np.isfinite(out))


def test_reset_deterministic(gpu):  # :242-264
    p = pitch.PitchShifter(48000, pitch_ratio=0.75)
    x = sine(330, 48000, 0.9, 8192)
    got1 = p.Process(x)
    p.Reset()
    assert float(np.max(np.abs(got1 - p.Process(x)))) <= 1e-12


def test_signal_quality(gpu):  # :328-380: the five ratios as five channels' worth of separate processors' inputs
    fs, fft_len = 48000.0, 16384
    out_freq = 100 * fs / fft_len
    for ratio in (0.5, 0.75, 1.5, 1.9, 2.0):
        p = pitch.PitchShifter(fs, pitch_ratio=ratio)
        assert snr_db(p.Process(bin_sine(out_freq, ratio)), [out_freq], fs, fft_len) >= 50, ratio


def test_signal_quality_wsola_params(gpu):  # :382-445
    fs, fft_len, ratio = 48000.0, 16384, 1.1
    out_freq = 100 * fs / fft_len
    for sequence_ms, overlap_ms in ((20, 5), (40, 10), (80, 20)):
        p = pitch.PitchShifter(fs)
        p.SetSequence(sequence_ms), p.SetOverlap(overlap_ms), p.SetPitchRatio(ratio)
        assert snr_db(p.Process(bin_sine(out_freq, ratio)), [out_freq], fs, fft_len) >= 45, sequence_ms


@pytest.mark.parametrize("first_bin,spacing", [(60, 2.0), (80, 1.2)])
def test_two_tone(gpu, first_bin, spacing):  # well separated :447-503, closely spaced :505-561
    fs, fft_len = 48000.0, 16384
    f1 = first_bin * fs / fft_len
    f2 = f1 * spacing
    for ratio in (0.75, 1.5, 1.9):
        p = pitch.PitchShifter(fs, pitch_ratio=ratio)
        out = p.Process(bin_sine(f1, ratio, amplitude=0.5) + bin_sine(f2, ratio, amplitude=0.5))
        assert np.all(np.isfinite(out))
        assert snr_db(out, [f1, f2], fs, fft_len) >= 45, ratio
