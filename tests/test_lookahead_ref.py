"""The lookahead limiter restatement (tests/lookahead_ref.py) against the
reference's own tests (dsp/effects/dynamics/lookahead_limiter_test.go),
restated, and the GPU runtime's host-side derivation (ad_lookahead_derived,
host only) against the restatement on bits.  No GPU is needed."""
import ctypes as C
import math

import numpy as np
import pytest

import lookahead_ref as R
from algodsp import _lib, processors as P

NAN, INF = float("nan"), float("inf")


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def sine(amp, freq, n, fs=48000.0):
    return [amp * math.sin(2 * math.pi * freq * float(i) / fs) for i in range(n)]


@pytest.mark.parametrize("sr,ok", [(48000, True), (44100, True), (0, False), (-1, False), (NAN, False), (INF, False)])
def test_new_lookahead_limiter(sr, ok):  # TestNewLookaheadLimiter
    if not ok:
        with pytest.raises(ValueError):
            R.LookaheadLimiter(sr)
        return
    l = R.LookaheadLimiter(sr)
    assert (l.SampleRate(), l.Threshold(), l.Release(), l.Lookahead()) == (sr, -0.1, 100.0, 3.0)
    assert l.delaySamples == round(3.0 * sr / 1000) and l.delayBuf.shape == (1, l.delaySamples + 1)


def test_parameter_validation():  # TestLookaheadLimiterParameterValidation, with the ranges' edges
    l = R.LookaheadLimiter(48000)
    for name, bad, good in [("SetThreshold", [-30, -24.5, 0.1, NAN, INF], [-24, 0]),
                            ("SetRelease", [0.5, 5000.5, NAN], [1, 5000]),
                            ("SetLookahead", [-1, 200.5, NAN, INF], [0, 200]),
                            ("SetSampleRate", [0, -1, NAN, INF], [8000])]:
        for v in good:
            getattr(l, name)(v)
        before = (l.Threshold(), l.Release(), l.Lookahead(), l.SampleRate(), l.delaySamples)
        for v in bad:
            with pytest.raises(ValueError):
                getattr(l, name)(v)
        assert before == (l.Threshold(), l.Release(), l.Lookahead(), l.SampleRate(), l.delaySamples)


def test_delay_behaviour():  # TestLookaheadLimiterDelayBehavior
    l = R.LookaheadLimiter(1000)
    l.SetThreshold(0)
    l.SetRelease(50)
    l.SetLookahead(2)
    out = [l.ProcessSample(x) for x in [1.0] + [0.0] * 7]
    assert abs(out[0]) <= 1e-12 and abs(out[1]) <= 1e-12 and out[2] > 0
    z = R.LookaheadLimiter(1000)
    z.SetLookahead(0)
    assert z.delayBuf.shape == (1, 1) and z.ProcessSample(0.25) == 0.25


def test_in_place_and_many_match_the_sample_path():  # TestLookaheadLimiterProcessInPlaceMatchesSamplePath
    def make(channels=1):
        l = R.LookaheadLimiter(48000, channels)
        l.SetThreshold(-3)
        l.SetRelease(80)
        l.SetLookahead(3)
        return l

    x = sine(0.9, 440, 256)
    one = make()
    want = [one.ProcessSample(v) for v in x]
    assert list(make().ProcessInPlace(list(x))) == want
    rows = np.array([x, [2 * v for v in x]])
    many = make(2)
    got = many.process_many(rows)
    assert np.array_equal(bits(got[0]), bits(want))
    two = make()
    assert np.array_equal(bits(got[1]), bits([two.ProcessSample(float(v)) for v in rows[1]]))
    env, gain, delayed = many.trace
    assert np.array_equal(delayed[0, 144:], rows[0, :256 - 144]) and not delayed[:, :144].any()
    assert env[0, -1] == many.envelope[0] and (gain <= 1).all() and (gain[1] < 1).any()


def test_sidechain_drives_gain_and_a_short_row_reads_as_zero():  # TestLookaheadLimiterSidechainDrivesGain
    neutral, side = R.LookaheadLimiter(48000), R.LookaheadLimiter(48000)
    for l in (neutral, side):
        l.SetThreshold(-12)
        l.SetLookahead(0)
    for _ in range(200):
        neutral.ProcessSample(0.08)
        side.ProcessSampleSidechain(0.08, 1.0)
    assert side.ProcessSampleSidechain(0.08, 1.0) < neutral.ProcessSample(0.08)
    # ProcessInPlaceSidechain :221-230 with a shorter detector row
    a, b = R.LookaheadLimiter(48000), R.LookaheadLimiter(48000, 1)
    prog, sc = [0.5] * 40, [1.0] * 10
    want = list(a.ProcessInPlaceSidechain(list(prog), sc))
    full = R.LookaheadLimiter(48000)
    assert want == list(full.ProcessInPlaceSidechain(list(prog), sc + [0.0] * 30))
    assert np.array_equal(bits(b.process_many(np.array([prog]), np.array([sc]))[0]), bits(want))


def test_reset_restores_deterministic_state():  # TestLookaheadLimiterResetRestoresDeterministicState
    l = R.LookaheadLimiter(48000)
    l.SetThreshold(-6)
    l.SetLookahead(4)
    x = sine(0.7, 220, 128 + 300)
    out1 = [l.ProcessSample(v) for v in x]
    l.Reset()
    assert [l.ProcessSample(v) for v in x] == out1


def test_setters_rebuild_the_ring_zeroed_and_keep_the_envelope():
    l = R.LookaheadLimiter(48000)
    for v in sine(0.9, 440, 300):
        l.ProcessSample(v)
    env = l.envelope.copy()
    assert l.delayBuf.any() and env[0] > 0
    l.SetLookahead(3.0)  # unchanged value: rebuilt all the same
    assert not l.delayBuf.any() and l.writePos == 0 and np.array_equal(l.envelope, env)
    for v in sine(0.9, 440, 300):
        l.ProcessSample(v)
    l.SetSampleRate(48000)
    assert not l.delayBuf.any() and l.envelope[0] > 0


@pytest.mark.parametrize("x,want", [(0.5, 1.0), (1.5, 2.0), (2.5, 3.0), (-0.5, -1.0), (-2.5, -3.0), (0.49999999999999994, 0.0),
                                    (2.4999999999999996, 2.0), (144.0, 144.0), (1e300, 1e300), (-0.2, -0.0)])
def test_go_round_rounds_halves_away_from_zero(x, want):
    assert R.go_round(x) == want


# (ms, fs) whose product over 1000 ends in .5: math.Round goes up where Python's round would go to even
HALVES = [(0.5, 1000.0, 1), (2.5, 1000.0, 3), (10.0, 44050.0, 441), (0.03125, 48000.0, 2), (4.5, 1000.0, 5),
          (62.5, 8.0, 1)]


@pytest.mark.parametrize("ms,fs,want", HALVES)
def test_delay_samples_at_halves(ms, fs, want):
    assert (ms * fs / 1000.0) % 1 == 0.5
    l = R.LookaheadLimiter(fs)
    l.SetLookahead(ms)
    assert l.delaySamples == want
    cfg = _lib.LookaheadConfig()
    _lib.lib().ad_lookahead_default_config(C.byref(cfg), fs)
    cfg.lookahead_ms = ms
    assert P.lookahead_derived(cfg)["delay_samples"] == want


@pytest.mark.parametrize("fs,th,rel,ms", [(48000.0, -0.1, 100.0, 3.0), (44100.0, -24.0, 1.0, 0.0),
                                          (96000.0, 0.0, 5000.0, 200.0), (8000.0, -6.5, 33.3, 7.7)])
def test_host_derivation_is_the_restatements(fs, th, rel, ms):
    cfg = _lib.LookaheadConfig(fs, th, rel, ms)
    d = P.lookahead_derived(cfg)
    l = R.LookaheadLimiter(fs)
    l.SetThreshold(th)
    l.SetRelease(rel)
    l.SetLookahead(ms)
    assert bits([d["attack_coeff"], d["release_coeff"], d["threshold_log2"]]).tolist() \
        == bits([l.attackCoeff, l.releaseCoeff, l.thresholdLog2]).tolist()
    assert d["delay_samples"] == l.delaySamples


def test_default_config_and_host_validation():
    cfg = _lib.LookaheadConfig()
    L = _lib.lib()
    L.ad_lookahead_default_config(C.byref(cfg), 48000.0)
    assert (cfg.sample_rate, cfg.threshold_db, cfg.release_ms, cfg.lookahead_ms) == (48000.0, -0.1, 100.0, 3.0)
    assert L.ad_lookahead_validate(C.byref(cfg)) == _lib.AD_OK
    for bad in [(0.0, -0.1, 100.0, 3.0), (NAN, -0.1, 100.0, 3.0), (48000.0, -24.5, 100.0, 3.0), (48000.0, 0.5, 100.0, 3.0),
                (48000.0, NAN, 100.0, 3.0), (48000.0, -1.0, 0.5, 3.0), (48000.0, -1.0, 5001.0, 3.0),
                (48000.0, -1.0, 100.0, -0.5), (48000.0, -1.0, 100.0, 200.5), (48000.0, -1.0, 100.0, INF)]:
        assert L.ad_lookahead_validate(C.byref(_lib.LookaheadConfig(*bad))) == _lib.AD_ERR_INVALID_ARGUMENT, bad
    assert L.ad_lookahead_validate(None) == _lib.AD_ERR_INVALID_ARGUMENT
