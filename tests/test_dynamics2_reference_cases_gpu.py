"""The reference's TransientShaper and DeEsser unit tests, restated against the
HIP engine.

Each test names the test it follows (dsp/effects/dynamics/
transient_shaper_test.go, deesser_test.go under github.com/cwbudde/algo-dsp)
and keeps its settings, inputs and thresholds.  A loop of reference
`ProcessSample` calls is one `ProcessInPlace` over the same samples (the sample
path and the block path are the same code there; here one test checks one-sample
calls against a block); a constructor or setter error is ErrInvalidArgument.
"""
import math

import numpy as np
import pytest

from algodsp import _lib, processors as P

pytestmark = pytest.mark.gpu
FS = 48000.0
NAN, INF = float("nan"), float("inf")


def sine(n, hz, amp, start=0):
    return np.array([amp * math.sin(2 * math.pi * hz * float(start + i) / FS) for i in range(n)])


def block(proc, xs):
    b = np.array(xs, dtype=np.float64)
    proc.ProcessInPlace(b)
    return b


def one_sample_calls(proc, xs):
    out = []
    for x in xs:
        b = np.array([x], dtype=np.float64)
        proc.ProcessInPlace(b)
        out.append(b[0])
    return np.array(out)


def apply(obj, setup):
    for name, v in setup:
        getattr(obj, name)(v)
    return obj


# ---- transient_shaper_test.go -----------------------------------------------
def test_new_transient_shaper(gpu):
    """TestNewTransientShaper :8-33."""
    P.TransientShaper(48000)
    for fs in (0, -1, NAN, INF):
        with pytest.raises(_lib.ErrInvalidArgument):
            P.TransientShaper(fs)


def test_transient_shaper_defaults_and_validation(gpu):
    """TestTransientShaperDefaults :35-56, TestTransientShaperParameterValidation :58-80."""
    ts = P.TransientShaper(48000)
    assert (ts.AttackAmount(), ts.SustainAmount(), ts.Attack(), ts.Release(), ts.SampleRate()) == (0, 0, 10, 120, 48000)
    for name, v in (("SetAttackAmount", -1.1), ("SetSustainAmount", 1.1), ("SetAttack", 0.05), ("SetRelease", 0.5)):
        with pytest.raises(_lib.ErrInvalidArgument):
            getattr(ts, name)(v)


def test_transient_shaper_process_in_place_matches_sample_path(gpu):
    """TestTransientShaperProcessInPlaceMatchesSamplePath :82-111: within 1e-12 (here: the same bits)."""
    setup = [("SetAttackAmount", 0.6), ("SetSustainAmount", -0.4)]
    x = sine(512, 220, 0.5)
    want = one_sample_calls(apply(P.TransientShaper(48000), setup), x)
    got = block(apply(P.TransientShaper(48000), setup), x)
    assert np.max(np.abs(got - want)) <= 1e-12
    np.testing.assert_array_equal(got.view(np.int64), want.view(np.int64))


def test_transient_shaper_attack_boosts_rising_edge(gpu):
    """TestTransientShaperAttackBoostsRisingEdge :113-131."""
    x = np.zeros(129)
    x[128] = 1.0
    neutral = block(P.TransientShaper(48000), x)
    boosted = block(apply(P.TransientShaper(48000), [("SetAttackAmount", 1.0)]), x)
    assert boosted[128] > neutral[128]


def test_transient_shaper_negative_sustain_reduces_decay_tail(gpu):
    """TestTransientShaperNegativeSustainReducesDecayTail :133-169."""
    x = np.array([0.8] * 300 + [0.15] * 300)
    neutral = block(P.TransientShaper(48000), x)
    shaped = block(apply(P.TransientShaper(48000), [("SetSustainAmount", -1.0), ("SetRelease", 40)]), x)
    assert np.mean(np.abs(shaped[300:])) < np.mean(np.abs(neutral[300:]))


def test_transient_shaper_reset_restores_deterministic_state(gpu):
    """TestTransientShaperResetRestoresDeterministicState :171-198."""
    ts = apply(P.TransientShaper(48000), [("SetAttackAmount", 0.7), ("SetSustainAmount", -0.2)])
    x = sine(256, 330, 0.6)
    out1 = block(ts, x)
    ts.Reset()
    assert np.max(np.abs(block(ts, x) - out1)) <= 1e-12


# ---- deesser_test.go --------------------------------------------------------
def test_new_deesser_and_defaults(gpu):
    """TestNewDeEsser :9-39, TestDeEsserDefaults :41-87."""
    for fs in (0, -1, NAN, INF):
        with pytest.raises(_lib.ErrInvalidArgument):
            P.DeEsser(fs)
    d = P.DeEsser(48000)
    assert (d.Frequency(), d.Q(), d.Threshold(), d.Ratio(), d.Knee(), d.Attack(), d.Release(), d.Range()) == \
        (6000, 1.5, -20, 4, 3, 0.5, 20, -24)
    assert (d.Mode(), d.Detector(), d.Listen(), d.FilterOrder(), d.SampleRate()) == (0, 0, False, 2, 48000)
    assert d.GetMetrics() == (0.0, 1.0)


def test_deesser_setter_validation_and_updates(gpu):
    """TestDeEsserSetterValidation :89-168, TestDeEsserSettersUpdate :170-290."""
    d = P.DeEsser(48000)
    bad = (("SetFrequency", (999, 20001, 24000, NAN, INF)), ("SetQ", (0.09, 10.1, NAN)), ("SetThreshold", (NAN, INF, -INF)),
           ("SetRatio", (0.9, 101, NAN)), ("SetKnee", (-1, 13, NAN)), ("SetAttack", (0.009, 51, NAN)),
           ("SetRelease", (0.9, 501, NAN)), ("SetRange", (-61, 1, NAN)), ("SetMode", (-1, 2)), ("SetDetector", (-1, 2)),
           ("SetFilterOrder", (0, 5)), ("SetSampleRate", (0, -1, NAN, INF, 12000)))
    for name, values in bad:
        for v in values:
            with pytest.raises(_lib.ErrInvalidArgument):
                getattr(d, name)(v)
    good = (("SetFrequency", "Frequency", 8000), ("SetQ", "Q", 2.5), ("SetThreshold", "Threshold", -30),
            ("SetRatio", "Ratio", 8), ("SetKnee", "Knee", 6), ("SetAttack", "Attack", 1), ("SetRelease", "Release", 50),
            ("SetRange", "Range", -12), ("SetMode", "Mode", 1), ("SetDetector", "Detector", 1),
            ("SetFilterOrder", "FilterOrder", 3), ("SetSampleRate", "SampleRate", 96000), ("SetListen", "Listen", True))
    for setter, getter, v in good:
        getattr(d, setter)(v)
        assert getattr(d, getter)() == v


def test_deesser_silence_produces_silence(gpu):
    """TestDeEsserSilenceProducesSilence :292-304."""
    assert not block(P.DeEsser(48000), np.zeros(1024)).any()


def test_deesser_low_frequency_transparent(gpu):
    """TestDeEsserLowFrequencyTransparent :308-352: 0.05."""
    d = apply(P.DeEsser(48000), [("SetThreshold", -60)])
    block(d, sine(4096, 200, 0.5))
    x = sine(4096, 200, 0.5, start=4096)
    assert np.max(np.abs(block(d, x) - x)) <= 0.05


def test_deesser_reduces_sibilance(gpu):
    """TestDeEsserReducesSibilance :356-404: below 0.9 of the amplitude."""
    d = apply(P.DeEsser(48000), [("SetThreshold", -40), ("SetRatio", 20)])
    block(d, sine(2048, 6000, 0.5))
    assert np.max(np.abs(block(d, sine(2048, 6000, 0.5, start=2048)))) < 0.5 * 0.9


def test_deesser_wideband_mode(gpu):
    """TestDeEsserWidebandMode :407-461."""
    d = apply(P.DeEsser(48000), [("SetMode", 1), ("SetThreshold", -40), ("SetRatio", 20)])
    block(d, sine(2048, 6000, 0.5))
    x = sine(2048, 6000, 0.5, start=2048) + sine(2048, 300, 0.3, start=2048)
    assert np.max(np.abs(block(d, x))) < (0.5 + 0.3) * 0.9


def test_deesser_listen_mode(gpu):
    """TestDeEsserListenMode :464-516."""
    d = P.DeEsser(48000)
    d.SetListen(True)
    block(d, sine(2048, 200, 0.5))
    low = np.max(np.abs(block(d, sine(2048, 200, 0.5, start=2048))))
    d.Reset()
    block(d, sine(2048, 6000, 0.5))
    high = np.max(np.abs(block(d, sine(2048, 6000, 0.5, start=2048))))
    assert low < high and high >= 0.01


def test_deesser_highpass_detector(gpu):
    """TestDeEsserHighpassDetector :519-564: an 8 kHz sine above the 6 kHz highpass, below 0.9 of the amplitude."""
    d = apply(P.DeEsser(48000), [("SetDetector", 1), ("SetThreshold", -40), ("SetRatio", 10)])
    block(d, sine(2048, 8000, 0.5))
    assert np.max(np.abs(block(d, sine(2048, 8000, 0.5, start=2048)))) < 0.5 * 0.9


def test_deesser_process_in_place_matches_sample(gpu):
    """TestDeEsserProcessInPlaceMatchesSample :567-599: within 1e-12 (here: the same bits)."""
    x = sine(256, 6000, 0.4)
    want = one_sample_calls(P.DeEsser(48000), x)
    got = block(P.DeEsser(48000), x)
    assert np.max(np.abs(got - want)) <= 1e-12
    np.testing.assert_array_equal(got.view(np.int64), want.view(np.int64))


def test_deesser_reset_restores_state(gpu):
    """TestDeEsserResetRestoresState :602-631."""
    d = P.DeEsser(48000)
    x = sine(512, 6000, 0.5)
    out1 = block(d, x)
    d.Reset()
    assert np.max(np.abs(block(d, x) - out1)) <= 1e-12


def test_deesser_metrics(gpu):
    """TestDeEsserMetrics :634-669."""
    d = apply(P.DeEsser(48000), [("SetThreshold", -30)])
    block(d, sine(2048, 6000, 0.8))
    level, reduction = d.GetMetrics()
    assert level > 0 and reduction < 1.0
    d.ResetMetrics()
    assert d.GetMetrics() == (0.0, 1.0)


def test_deesser_hard_knee(gpu):
    """TestDeEsserHardKnee :672-697."""
    d = apply(P.DeEsser(48000), [("SetKnee", 0), ("SetThreshold", -30)])
    block(d, sine(1024, 6000, 0.5))
    assert d.GetMetrics()[1] < 1.0


def test_deesser_filter_order_effect(gpu):
    """TestDeEsserFilterOrderEffect :701-748."""
    def peak(order):
        d = apply(P.DeEsser(48000), [("SetFilterOrder", order)])
        d.SetListen(True)
        block(d, sine(4096, 3000, 0.5))
        return np.max(np.abs(block(d, sine(4096, 3000, 0.5, start=4096))))

    assert peak(4) < peak(1)


def test_deesser_range_limit(gpu):
    """TestDeEsserRangeLimit :751-800."""
    d = apply(P.DeEsser(48000), [("SetThreshold", -60), ("SetRatio", 100), ("SetRange", -12), ("SetMode", 1),
                                 ("SetKnee", 0)])
    block(d, sine(8192, 6000, 0.9))
    assert d.GetMetrics()[1] >= math.pow(10, -12.0 / 20.0) * 0.95


def test_deesser_ratio_one_is_transparent(gpu):
    """TestDeEsserRatioOneIsTransparent :803-830: 1e-10."""
    d = apply(P.DeEsser(48000), [("SetRatio", 1), ("SetMode", 1)])
    x = sine(1024, 6000, 0.5)
    assert np.max(np.abs(block(d, x) - x)) <= 1e-10
