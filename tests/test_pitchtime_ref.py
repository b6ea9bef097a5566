"""tests/pitchtime_ref.py, the restatement the GPU pitch shifter is held to,
passes the reference's own unit tests (dsp/effects/pitch/pitch_shifter_test.go)
with the thresholds written there; the measuring transforms are numpy's.  Then
what of the feature needs no device: the node's parameter clamps, the order of
the constructor's errors, and the unchanged C surface.
"""
import json
import math
import pathlib
import re

import numpy as np
import pytest

import pitchtime_ref as R
from algodsp import _lib, effectchain as E, pitch
from pitchtime_measure import bin_sine, estimate_frequency, sine, snr_db

BAD = _lib.ErrInvalidArgument


# ---- pitch_shifter_test.go on the restatement ----------------------------------------
@pytest.mark.parametrize("rate,ok", [(44100.0, True), (48000.0, True), (0.0, False), (-1.0, False),
                                     (float("nan"), False), (float("inf"), False)])
def test_new_pitch_shifter(rate, ok):  # :11-37
    if ok:
        assert R.PitchShifter(rate).SampleRate() == rate
    else:
        with pytest.raises(ValueError):
            R.PitchShifter(rate)


def test_set_pitch_ratio():  # :39-72
    p = R.PitchShifter(48000)
    for ratio in (0.5, 1.0, 2.0):
        p.SetPitchRatio(ratio)
        assert p.PitchRatio() == ratio
    for ratio in (0, 0.1, 8.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            p.SetPitchRatio(ratio)
        assert p.PitchRatio() == 2.0


def test_setter_ranges():  # the setters' bounds :150-217
    p = R.PitchShifter(48000)
    for setter, lo, hi in ((p.SetSequence, 20, 120), (p.SetSearch, 2, 40)):
        setter(lo), setter(hi)
        for v in (lo - 0.5, hi + 0.5, float("nan"), float("inf")):
            with pytest.raises(ValueError):
                setter(v)
    p.SetOverlap(4), p.SetOverlap(60)
    for v in (3.5, 60.5, float("nan"), float("-inf")):
        with pytest.raises(ValueError):
            p.SetOverlap(v)
    for v in (float("nan"), float("inf"), 25, -25):
        with pytest.raises(ValueError):
            p.SetPitchSemitones(v)
    p.SetPitchSemitones(7)
    assert p.PitchRatio() == math.pow(2, 7 / 12.0) and abs(p.PitchSemitones() - 7) < 1e-12


def test_set_overlap_rejects_overlap_above_sequence():  # :74-95
    p = R.PitchShifter(48000)
    p.SetSequence(20)
    old = p.Overlap()
    with pytest.raises(ValueError):
        p.SetOverlap(30)
    assert p.Overlap() == old and p.overlapLen == 480 and p.sequenceLen == 960


def test_identity_is_exact_copy():  # :97-123
    p = R.PitchShifter(48000)
    x = sine(440, 48000, 0.8, 4096)
    out = p.Process(x)
    assert out is not x and np.array_equal(out, x)


def test_process_in_place_matches_process():  # :125-160
    p1, p2 = R.PitchShifter(48000), R.PitchShifter(48000)
    p1.SetPitchSemitones(7), p2.SetPitchSemitones(7)
    x = sine(330, 48000, 0.7, 4096)
    want = p1.Process(x)
    got = x.copy()
    p2.ProcessInPlace(got)
    assert float(np.max(np.abs(got - want))) <= 1e-12


def test_pitch_accuracy():  # :162-215
    fs, f0 = 48000.0, 220.0
    x = sine(f0, fs, 0.8, 60000)
    up = R.PitchShifter(fs)
    up.SetPitchSemitones(12.0)
    assert abs(estimate_frequency(up.Process(x)[8000:52000], fs, 300.0, 600.0) - 2 * f0) <= 10.0
    down = R.PitchShifter(fs)
    down.SetPitchSemitones(-12.0)
    assert abs(estimate_frequency(down.Process(x)[8000:52000], fs, 80.0, 180.0) - 0.5 * f0) <= 6.0


def test_short_buffer_produces_finite_values():  # :217-240
    p = R.PitchShifter(48000)
    p.SetPitchRatio(1.7)
    out = p.Process(np.array([1, -0.25, 0.1, 0, -0.1, 0.2, -0.3, 0.4]))
    assert len(out) == 8 and np.all(np.isfinite(out))


def test_reset_deterministic():  # :242-264
    p = R.PitchShifter(48000)
    p.SetPitchRatio(0.75)
    x = sine(330, 48000, 0.9, 8192)
    got1 = p.Process(x)
    p.Reset()
    assert float(np.max(np.abs(got1 - p.Process(x)))) <= 1e-12


@pytest.mark.parametrize("ratio", [0.5, 0.75, 1.5, 1.9, 2.0])
def test_signal_quality(ratio):  # :328-380
    fs, fft_len = 48000.0, 16384
    out_freq = 100 * fs / fft_len
    p = R.PitchShifter(fs)
    p.SetPitchRatio(ratio)
    assert snr_db(p.Process(bin_sine(out_freq, ratio)), [out_freq], fs, fft_len) >= 50


@pytest.mark.parametrize("sequence_ms,overlap_ms", [(20, 5), (40, 10), (80, 20)])
def test_signal_quality_wsola_params(sequence_ms, overlap_ms):  # :382-445
    fs, fft_len, ratio = 48000.0, 16384, 1.1
    out_freq = 100 * fs / fft_len
    p = R.PitchShifter(fs)
    p.SetSequence(sequence_ms), p.SetOverlap(overlap_ms), p.SetPitchRatio(ratio)
    assert snr_db(p.Process(bin_sine(out_freq, ratio)), [out_freq], fs, fft_len) >= 45


@pytest.mark.parametrize("ratio", [0.75, 1.5, 1.9])
@pytest.mark.parametrize("first_bin,spacing", [(60, 2.0), (80, 1.2)])
def test_two_tone(first_bin, spacing, ratio):  # well separated :447-503, closely spaced :505-561
    fs, fft_len = 48000.0, 16384
    f1 = first_bin * fs / fft_len
    f2 = f1 * spacing
    p = R.PitchShifter(fs)
    p.SetPitchRatio(ratio)
    out = p.Process(bin_sine(f1, ratio, amplitude=0.5) + bin_sine(f2, ratio, amplitude=0.5))
    assert np.all(np.isfinite(out))
    assert snr_db(out, [f1, f2], fs, fft_len) >= 45


# ---- the restatement's own corners ------------------------------------------------------
def test_selection_ties_and_nan_take_the_scan_s_winner():
    p = R.PitchShifter(8000)
    p.SetSequence(20), p.SetOverlap(4), p.SetSearch(2)
    p.SetPitchRatio(2.0)
    p.Process(np.zeros(1024))  # every score is 0: the lowest candidate of every frame
    nominal, predicted = p.stepOut / 2.0, []
    acc = nominal
    for _ in p.selections:
        predicted.append(int(R.go_round(acc)))
        acc += nominal
    assert p.selections == [q - p.searchLen for q in predicted]
    x = np.zeros(1024)
    x[:] = np.nan  # every score is NaN: nothing wins, best stays predicted
    p.Process(x)
    assert p.selections == predicted


def test_hermite4_is_interp_go_s():
    # interp.go:51-58 at t = 0.5 on (0, 1, 2, 4): c1 = 1, c2 = 0 - 2.5 + 4 - 2 = -0.5, c3 = 2 - 1.5 = 0.5
    assert R.hermite4(0.5, 0.0, 1.0, 2.0, 4.0) == ((0.5 * 0.5 - 0.5) * 0.5 + 1.0) * 0.5 + 1.0
    assert R.hermite4(0.0, 9.0, 3.0, 5.0, 7.0) == 3.0


# ---- the node's parameters and the processor's host side ------------------------------
def params(**num):
    return E.Params("n", "pitch-time", num=num)


def config_of(p, fs=48000.0):
    cfg, fade = E.time_pitch_params(p, fs)
    return cfg, fade


def test_time_pitch_params_defaults_and_clamps():  # runtime_filter_pitch_reverb.go:226-242
    cfg, fade = config_of(params())
    assert (cfg.sequence_ms, cfg.overlap_ms, cfg.search_ms, cfg.pitch_ratio) == (40.0, 10.0, 15.0, 1.0)
    assert cfg.fade_len == 480 == fade.size and np.array_equal(fade, R.fade_in_table(480))
    cfg, _ = config_of(params(sequence=500, overlap=1, search=100, semitones=30))
    assert (cfg.sequence_ms, cfg.overlap_ms, cfg.search_ms) == (120.0, 4.0, 40.0)
    assert cfg.pitch_ratio == math.pow(2, 24 / 12.0)
    cfg, _ = config_of(params(sequence=1, overlap=99, search=0, semitones=-30))
    assert (cfg.sequence_ms, cfg.overlap_ms, cfg.search_ms) == (20.0, 19.0, 2.0)  # ov >= seq -> seq - 1
    assert cfg.pitch_ratio == math.pow(2, -24 / 12.0)
    cfg, _ = config_of(params(sequence=30, overlap=30))
    assert (cfg.sequence_ms, cfg.overlap_ms) == (30.0, 29.0)
    with pytest.raises(BAD):
        config_of(params(), fs=float("nan"))


def test_frame_lengths_are_rebuild_s():  # :262-276
    assert pitch.frame_lengths(48000.0, 82.0, 10.0, 28.0) == (3936, 480, 1344, 3456)
    assert pitch.frame_lengths(8000.0, 20.0, 4.0, 2.0) == (160, 32, 16, 128)
    assert pitch.frame_lengths(100.0, 120.0, 4.0, 2.0) == (32, 8, 1, 24)  # the lower bounds 32 / 8 / 1
    assert pitch.frame_lengths(1000.5, 20.0, 4.0, 2.5)[2] == 3  # round(2.50125) and halves away from zero below
    assert pitch.go_round(2.5) == 3.0 and pitch.go_round(-2.5) == -3.0 and pitch.go_round(0.49999999999999994) == 0.0
    for ref_fs in (44100.0, 48000.0, 192000.0, 11025.0):
        r = R.PitchShifter(ref_fs)
        assert pitch.frame_lengths(ref_fs, 82.0, 10.0, 28.0) == (r.sequenceLen, r.overlapLen, r.searchLen, r.stepOut)


def test_constructor_errors_in_order():
    with pytest.raises(BAD):  # the arguments are refused before the device is looked for
        pitch.PitchShifter(48000.0, 2, device=-1, overlap_ms=90, sequence_ms=82)
    for bad in (dict(pitch_ratio=0.2), dict(pitch_ratio=4.5), dict(semitones=float("nan")), dict(sequence_ms=10),
                dict(search_ms=41), dict(overlap_ms=3), dict(sequence_ms=20, overlap_ms=20)):
        with pytest.raises(BAD):
            pitch.PitchShifter(48000.0, 2, device=-1, **bad)
    with pytest.raises(BAD):
        pitch.PitchShifter(float("inf"), 2, device=-1)
    with pytest.raises(TypeError):
        pitch.PitchShifter(48000.0, 2, device=-1, pitch=2)
    with pytest.raises(_lib.ErrDevice) as e:
        pitch.PitchShifter(48000.0, 2, device=-1)
    assert e.value.code == _lib.AD_ERR_NO_DEVICE


def test_c_surface_is_unchanged():
    header = _lib.HEADER_PATH.read_text()
    assert re.search(r"#define\s+AD_FXN_PITCHTIME\s+25\b", header) and pitch.FXN_PITCHTIME == E.FXN_PITCHTIME == 25
    assert "ad_pitchtime_config" in header
    symbols = _lib.exported_symbols()
    assert not [s for s in symbols if "pitchtime" in s]
    # every declared entry point is one the prototype snapshot of tests/test_processors_surface.py knew
    snapshot = json.loads((pathlib.Path(__file__).parent / "golden" / "lib_prototypes.json").read_text())
    assert set(symbols) <= set(snapshot["functions"])


def test_chain_refuses_pitch_time_without_the_keyword():
    graph = E._graph_json([{"id": "p", "type": "pitch-time", "params": {"semitones": 3}}],
                          [(E.INPUT_NODE_ID, "p"), ("p", E.OUTPUT_NODE_ID)])
    with pytest.raises(E.UnknownEffect):
        E.Chain(48000.0, 2).LoadGraph(graph)
