"""The reference's Phaser, Tremolo and RingModulator unit tests, restated
against the HIP engine.

Each test names the test it follows (dsp/effects/modulation/phaser_test.go,
tremolo_test.go, ring_modulator_test.go under github.com/cwbudde/algo-dsp) and
keeps its settings, inputs and tolerance.  A reference `Process` call is a
one-sample `ProcessInPlace` on the GPU; a constructor or setter error is
ErrInvalidArgument.
"""
import math

import numpy as np
import pytest

from algodsp import _lib, processors as P

pytestmark = pytest.mark.gpu
FS = 48000.0


def one_sample_calls(proc, xs):
    out = []
    for x in xs:
        b = np.array([x], dtype=np.float64)
        proc.ProcessInPlace(b)
        out.append(b[0])
    return np.array(out)


def block(proc, xs):
    b = np.array(xs, dtype=np.float64)
    proc.ProcessInPlace(b)
    return b


MAKERS = {"phaser": lambda: P.Phaser(FS), "tremolo": lambda: P.Tremolo(FS), "ringmod": lambda: P.RingModulator(FS)}


@pytest.mark.parametrize("kind", list(MAKERS))
def test_process_in_place_matches_process(gpu, kind):
    """TestPhaserProcessInPlaceMatchesProcess (phaser_test.go:8-44), TestTremolo... (tremolo_test.go:8-44),
    TestRingModulator... (ring_modulator_test.go:8-40): 128 samples of a sine, sample by sample and as one block,
    within 1e-12 (here: the same bits)."""
    x = np.sin(2 * math.pi * np.arange(128) / 29)
    a, b = one_sample_calls(MAKERS[kind](), x), block(MAKERS[kind](), x)
    assert np.max(np.abs(a - b)) <= 1e-12
    np.testing.assert_array_equal(a.view(np.int64), b.view(np.int64))


@pytest.mark.parametrize("kind", list(MAKERS))
def test_reset_restores_state(gpu, kind):
    """Test*ResetRestoresState (phaser_test.go:46-72: an impulse of 128 samples; tremolo_test.go:46-72 and
    ring_modulator_test.go:42-70, carrier 300 Hz: an impulse of 96): the output after Reset within 1e-12.  An
    impulse shows the first sample's gain only, so a sine follows."""
    p = P.RingModulator(FS, carrier_hz=300.0) if kind == "ringmod" else MAKERS[kind]()
    x = np.zeros(128 if kind == "phaser" else 96)
    x[0] = 1
    for sig in (x, np.sin(2 * math.pi * 440 * np.arange(96) / FS)):
        p.Reset()
        out1 = one_sample_calls(p, sig)
        p.Reset()
        out2 = one_sample_calls(p, sig)
        assert np.max(np.abs(out1 - out2)) <= 1e-12
    assert np.any(out1 != 0)


def test_tremolo_depth_zero_is_transparent(gpu):
    """TestTremoloDepthZeroIsTransparent (tremolo_test.go:74-91): depth 0, mix 1, 512 samples, within 1e-12."""
    t = P.Tremolo(FS, depth=0.0, mix=1.0)
    x = 0.5 * np.sin(2 * math.pi * 440 * np.arange(512) / FS)
    assert np.max(np.abs(one_sample_calls(t, x) - x)) <= 1e-12


def test_ring_modulator_mix_zero_is_transparent(gpu):
    """TestRingModulatorMixZeroIsTransparent (ring_modulator_test.go:72-89): carrier 1 kHz, mix 0, within 1e-12."""
    r = P.RingModulator(FS, carrier_hz=1000.0, mix=0.0)
    x = 0.5 * np.sin(2 * math.pi * 440 * np.arange(512) / FS)
    assert np.max(np.abs(one_sample_calls(r, x) - x)) <= 1e-12


def test_ring_modulator_dc_input_produces_sine(gpu):
    """TestRingModulatorDCInputProducesSine (:91-117): a constant 1.0 at carrier 100 Hz gives
    sin(2 pi 100 i / fs) over one carrier cycle of 480 samples, within 1e-9."""
    r = P.RingModulator(FS, carrier_hz=100.0, mix=1.0)
    got = one_sample_calls(r, np.ones(480))
    want = np.array([math.sin(2 * math.pi * 100.0 * i / FS) for i in range(480)])
    assert np.max(np.abs(got - want)) <= 1e-9


def test_ring_modulator_silence_produces_silence(gpu):
    """TestRingModulatorSilenceInputProducesSilence (:119-134): zeros in, exact zeros out."""
    r = P.RingModulator(FS, carrier_hz=1000.0, mix=1.0)
    assert not np.any(block(r, np.zeros(128)))


def test_ring_modulator_sum_difference_frequencies(gpu):
    """TestRingModulatorSumDifferenceFrequencies (:136-194): 400 Hz through a 100 Hz carrier has its
    energy at 300 and 500 Hz (magnitude >= 0.2) and none at 400 and 100 Hz (<= 0.01)."""
    n = 4800
    i = np.arange(n)
    out = block(P.RingModulator(FS, carrier_hz=100.0, mix=1.0), np.sin(2 * math.pi * 400.0 * i / FS))

    def mag(freq):
        angle = 2 * math.pi * freq * i / FS
        return math.hypot(float(np.sum(out * np.cos(angle))), float(np.sum(out * np.sin(angle)))) / n

    assert mag(500.0) >= 0.2 and mag(300.0) >= 0.2
    assert mag(400.0) <= 0.01 and mag(100.0) <= 0.01


def test_phaser_finite_output_under_feedback(gpu):
    """TestPhaserFiniteOutputUnderFeedback (phaser_test.go:96-114): feedback 0.85, mix 0.8, 8 stages,
    12000 samples of a 440 Hz sine at 0.3 stay finite."""
    p = P.Phaser(FS, feedback=0.85, mix=0.8, stages=8)
    y = block(p, 0.3 * np.sin(2 * math.pi * 440 * np.arange(12000) / FS))
    assert np.all(np.isfinite(y)) and np.any(y != 0)


def test_constructor_validation(gpu):
    """TestPhaserValidation (phaser_test.go:74-94), TestTremoloValidation (tremolo_test.go:93-108),
    TestRingModulatorValidation (ring_modulator_test.go:196-251)."""
    bad = [lambda: P.Phaser(0.0), lambda: P.Phaser(FS, stages=0), lambda: P.Phaser(FS, min_freq_hz=1000.0, max_freq_hz=800.0),
           lambda: P.Phaser(FS, min_freq_hz=1000.0, max_freq_hz=30000.0),
           lambda: P.Tremolo(0.0), lambda: P.Tremolo(FS, depth=1.2), lambda: P.Tremolo(FS, smoothing_ms=-1.0),
           lambda: P.RingModulator(0.0), lambda: P.RingModulator(-1.0), lambda: P.RingModulator(float("nan")),
           lambda: P.RingModulator(float("inf")), lambda: P.RingModulator(FS, carrier_hz=0.0),
           lambda: P.RingModulator(FS, carrier_hz=-100.0), lambda: P.RingModulator(FS, carrier_hz=float("nan")),
           lambda: P.RingModulator(FS, mix=-0.1), lambda: P.RingModulator(FS, mix=1.1),
           lambda: P.RingModulator(FS, mix=float("nan"))]
    for make in bad:
        with pytest.raises(_lib.ErrInvalidArgument):
            make()
    P.RingModulator(FS, carrier_hz=300.0, mix=0.5)  # "valid" (:240-250)


def test_ring_modulator_setter_validation_getters_and_state(gpu):
    """TestRingModulatorSetterValidation (:253-288), TestRingModulatorGetters (:290-310) and
    TestRingModulatorSettersUpdateState (:312-344)."""
    r = P.RingModulator(FS)
    for setter, v in ((r.SetSampleRate, 0.0), (r.SetSampleRate, float("nan")), (r.SetCarrierHz, 0.0),
                      (r.SetCarrierHz, -1.0), (r.SetMix, -0.1), (r.SetMix, 1.1)):
        with pytest.raises(_lib.ErrInvalidArgument):
            setter(v)
    g = P.RingModulator(FS, carrier_hz=300.0, mix=0.7)
    assert (g.SampleRate(), g.CarrierHz(), g.Mix()) == (48000.0, 300.0, 0.7)
    r.SetSampleRate(96000.0)
    assert r.SampleRate() == 96000.0
    r.SetCarrierHz(1000.0)
    assert r.CarrierHz() == 1000.0
    r.SetMix(0.5)
    assert r.Mix() == 0.5
    assert r.kernel_info()[2] == 2 * math.pi * 1000.0 / 96000.0  # updatePhaseIncrement
