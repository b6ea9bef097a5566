"""The behavioural tests of dsp/effects/dynamics/multiband_test.go and of
dsp/filter/crossover/crossover_test.go (TestMultiBand_*) run against the GPU
processors.  A ProcessSample loop of the reference is one ProcessInPlace call
here: the processors have no per-sample entry point.
"""
import math

import numpy as np
import pytest

from algodsp import _lib, processors as P

pytestmark = pytest.mark.gpu

FS = 48000.0


def impulse(n, a=1.0):
    x = np.zeros((1, n))
    x[0, 0] = a
    return x


def sine(n, f, a):
    return a * np.sin(2 * np.pi * f * np.arange(n) / FS)


def unity(mc):
    for i in range(mc.NumBands()):
        mc.SetBandRatio(i, 1.0)
        mc.SetBandAutoMakeup(i, False)
        mc.SetBandMakeupGain(i, 0)
    return mc


def run(mc, x):
    y = np.array(x, dtype=np.float64).reshape(1, -1).copy()
    mc.ProcessInPlace(y)
    return y[0]


def test_crossover_three_and_four_way(gpu):  # TestNewMultiBand_ThreeWay, TestMultiBand_FourWay
    assert P.MultiBandCrossover([500, 5000], 4, FS).NumBands() == 3
    mb = P.MultiBandCrossover([200, 2000, 10000], 4, FS)
    assert mb.NumBands() == 4 and np.isfinite(mb.ProcessBlock(impulse(1))).all()


def test_crossover_energy_preservation(gpu):  # TestMultiBand_ProcessSample_EnergyPreservation
    s = P.MultiBandCrossover([500, 5000], 4, FS).ProcessBlock(impulse(8192)).sum(axis=0)[0]
    assert abs(float(np.sum(s * s)) - 1.0) <= 0.01


def test_crossover_block_equals_samples_and_reset(gpu):  # TestMultiBand_ProcessBlock, TestMultiBand_Reset
    a, b = P.MultiBandCrossover([500, 5000], 4, FS), P.MultiBandCrossover([500, 5000], 4, FS)
    x = impulse(128)
    per_sample = np.concatenate([a.ProcessBlock(x[:, i:i + 1]) for i in range(128)], axis=2)
    assert np.max(np.abs(per_sample - b.ProcessBlock(x))) <= 1e-12
    a.Reset()
    fresh = P.MultiBandCrossover([500, 5000], 4, FS)
    assert np.max(np.abs(a.ProcessBlock(impulse(1)) - fresh.ProcessBlock(impulse(1)))) <= 1e-15


def test_compresses_loud_signal(gpu):  # TestMultibandCompressesLoudSignal
    mc = P.MultibandCompressor([1000], 4, FS)
    for i in range(mc.NumBands()):
        mc.SetBandThreshold(i, -20)
        mc.SetBandRatio(i, 10.0)
        mc.SetBandKnee(i, 0)
        mc.SetBandAttack(i, 0.1)
        mc.SetBandAutoMakeup(i, False)
        mc.SetBandMakeupGain(i, 0)
    assert abs(run(mc, np.full(5000, 0.8))[-1]) < 0.8


def test_band_independence(gpu):  # TestMultibandBandIndependence
    mc = P.MultibandCompressor([1000], 4, FS)
    mc.SetBandThreshold(0, -30)
    mc.SetBandRatio(0, 20.0)
    mc.SetBandAutoMakeup(0, False)
    mc.SetBandMakeupGain(0, 0)
    mc.SetBandRatio(1, 1.0)
    assert mc.Band(0).Ratio() == 20.0 and mc.Band(1).Ratio() == 1.0


@pytest.mark.parametrize("order", [2, 4, 8, 12])
def test_different_orders(gpu, order):  # TestMultibandDifferentOrders
    mc = P.MultibandCompressor([1000], order, FS)
    assert mc.CrossoverOrder() == order and math.isfinite(run(mc, [0.5])[0])


def test_energy_preservation(gpu):  # TestMultibandEnergyPreservation
    y = run(unity(P.MultibandCompressor([500, 5000], 4, FS)), impulse(8192))
    assert abs(float(np.sum(y * y)) - 1.0) <= 0.02


def test_recombination_consistency(gpu):  # TestMultibandRecombinationConsistency
    mc = unity(P.MultibandCompressor([300, 3000], 4, FS))
    x = sine(512, 220, 0.4) + sine(512, 2200, 0.2)
    per_band = mc.ProcessInPlaceMulti(x.copy())
    mc.Reset()
    assert np.max(np.abs(run(mc, x) - per_band.sum(axis=0)[0])) <= 1e-12


def test_phase_latency_sanity(gpu):  # TestMultibandPhaseLatencySanity
    y = run(unity(P.MultibandCompressor([500, 5000], 4, FS)), impulse(2048))
    e = y * y
    assert abs(y[0]) >= 1e-6 and e[:256].sum() / e.sum() >= 0.8


def test_process_stereo_in_place(gpu):  # TestMultibandProcessStereoInPlace, two channels
    mc = P.MultibandCompressor([500, 5000], 4, FS, channels=2)
    left, right = sine(128, 440, 0.3), sine(128, 880, 0.3)
    want = [run(P.MultibandCompressor([500, 5000], 4, FS), v) for v in (left, right)]
    mc.ProcessStereoInPlace(left, right)
    assert np.array_equal(left, want[0]) and np.array_equal(right, want[1])
    with pytest.raises(ValueError):
        mc.ProcessStereoInPlace(left, right[:64])


def test_empty_input(gpu):  # TestMultibandProcessInPlaceEmpty, ...MultiEmpty
    mc = P.MultibandCompressor([1000], 4, FS)
    mc.ProcessInPlace(np.zeros((1, 0)))
    assert mc.ProcessInPlaceMulti(np.zeros((1, 0))).shape == (2, 1, 0)
    assert P.MultiBandCrossover([1000], 4, FS).ProcessBlock(np.zeros((1, 0))).shape == (2, 1, 0)


def test_zero_in_zero_out_and_finite(gpu):  # TestMultibandProcessSampleZero, ...Finite, ...InPlaceMulti
    mc = P.MultibandCompressor([1000], 4, FS)
    mc.Reset()
    assert not run(mc, np.zeros(100)).any()
    mc = P.MultibandCompressor([500, 5000], 4, FS)
    assert np.isfinite(run(mc, impulse(1000, 0.5))).all()
    assert mc.ProcessInPlaceMulti(impulse(128, 0.5)).shape == (3, 1, 128)


def test_reset(gpu):  # TestMultibandReset
    mc, fresh = P.MultibandCompressor([1000], 4, FS), P.MultibandCompressor([1000], 4, FS)
    run(mc, np.full(100, 0.5))
    mc.Reset()
    assert abs(run(mc, [0.3])[0] - run(fresh, [0.3])[0]) <= 1e-15


def test_metrics(gpu):  # TestMultibandMetrics
    mc = P.MultibandCompressor([1000], 4, FS)
    mc.ResetMetrics()
    run(mc, np.full(500, 0.8))
    m = mc.GetMetrics()
    assert len(m) == 2 and any(b[0] > 0 for b in m)
    mc.ResetMetrics()
    assert all(b[0] == 0 and b[1] == 0 for b in mc.GetMetrics())


def test_constructor_table(gpu):  # TestNewMultibandCompressor, ...WithConfig
    mc = P.MultibandCompressor([100, 300, 1000, 3000, 8000, 16000], 4, FS)
    assert (mc.NumBands(), mc.CrossoverOrder(), mc.SampleRate()) == (7, 4, FS)
    for freqs, order, fs in (([], 4, FS), ([1000], 3, FS), ([1000], 26, FS), ([1000], 4, 0.0), ([24000], 4, FS),
                             ([10], 4, FS), ([5000, 500], 4, FS), ([float("nan")], 4, FS)):
        with pytest.raises(_lib.ErrInvalidArgument):
            P.MultibandCompressor(freqs, order, fs)
    configs = [
        {"ThresholdDB": -30, "Ratio": 2.0, "KneeDB": 6.0, "AttackMs": 20, "ReleaseMs": 200, "AutoMakeup": True},
        {"ThresholdDB": -20, "Ratio": 4.0, "KneeDB": 3.0, "AttackMs": 10, "ReleaseMs": 100},
        {"ThresholdDB": -15, "Ratio": 6.0, "KneeDB": 0.0, "AttackMs": 5, "ReleaseMs": 50},
    ]
    mc = P.MultibandCompressor([500, 5000], 4, FS, configs=configs)
    assert (mc.Band(0).Threshold(), mc.Band(1).Ratio(), mc.Band(2).Attack(), mc.Band(2).Knee()) == (-30, 4.0, 5.0, 0.0)
    with pytest.raises(_lib.ErrInvalidArgument):
        P.MultibandCompressor([1000], 4, FS, configs=[{"Ratio": 0.5}, {}])
