"""The restatement in tests/multiband_ref.py held to the reference's own tests
(filter/crossover/crossover_test.go TestNewMultiBand_*, TestMultiBand_*;
effects/dynamics/multiband_test.go), and the host-only part of the ad_xover /
ad_multiband ABI: the validation tables, the section designer against
design.crossover on bits, ad_multiband_set_band's checks.  No GPU.
"""
import ctypes as C
import math

import numpy as np
import pytest

import multiband_ref as R
from algodsp import _lib, design, processors as P

FS = 48000.0
NAN = float("nan")


def impulse(n, a=1.0):
    x = np.zeros(n)
    x[0] = a
    return x


def sine(n, f, a, fs=FS):
    return a * np.sin(2 * np.pi * f * np.arange(n) / fs)


# ---- crossover_test.go ------------------------------------------------------
def test_new_multiband_three_way():  # TestNewMultiBand_ThreeWay
    mb = R.MultiBand([500, 5000], 4, FS)
    assert mb.NumBands() == 3 and len(mb.stages) == 2


XOVER_ERRORS = {  # TestNewMultiBand_Errors
    "empty freqs": ([], 4, 48000.0),
    "non-ascending": ([5000, 500], 4, 48000.0),
    "duplicate": ([1000, 1000], 4, 48000.0),
    "odd order": ([1000], 3, 48000.0),
    "freq at nyquist": ([24000], 4, 48000.0),
}
XOVER_OK = {
    "three-way": ([500, 5000], 4, 48000.0),
    "four-way": ([200, 2000, 10000], 4, 48000.0),
    "LR2": ([1000], 2, 48000.0),
    "LR24 seven stages": ([60, 150, 400, 1000, 2500, 6000, 12000], 24, 48000.0),
    "below the compressor's 20 Hz": ([10], 4, 48000.0),
}
# the kernel's limits on top of the reference's rules
XOVER_LIMITS = {
    "order 26": ([1000], 26, 48000.0),
    "eight stages": ([100, 200, 400, 800, 1600, 3200, 6400, 12800], 4, 48000.0),
    "zero order": ([1000], 0, 48000.0),
    "zero sample rate": ([1000], 4, 0.0),
    "NaN freq": ([NAN], 4, 48000.0),
}


@pytest.mark.parametrize("name", list(XOVER_ERRORS))
def test_new_multiband_errors(name):
    freqs, order, fs = XOVER_ERRORS[name]
    with pytest.raises(ValueError):
        R.MultiBand(freqs, order, fs)


def test_multiband_energy_preservation():  # TestMultiBand_ProcessSample_EnergyPreservation
    mb = R.MultiBand([500, 5000], 4, FS)
    s = mb.ProcessBlock(impulse(8192)).sum(axis=0)
    assert abs(float(np.sum(s * s)) - 1.0) <= 0.01


def test_multiband_process_block_equals_samples():  # TestMultiBand_ProcessBlock
    a, b = R.MultiBand([500, 5000], 4, FS), R.MultiBand([500, 5000], 4, FS)
    x = impulse(128)
    per_sample = np.array([a.ProcessSample(v) for v in x]).T
    np.testing.assert_array_equal(per_sample, b.ProcessBlock(x))


def test_multiband_reset():  # TestMultiBand_Reset
    mb, fresh = R.MultiBand([500, 5000], 4, FS), R.MultiBand([500, 5000], 4, FS)
    mb.ProcessSample(1.0)
    mb.ProcessSample(0.5)
    mb.Reset()
    np.testing.assert_array_equal(mb.ProcessSample(1.0), fresh.ProcessSample(1.0))


def test_multiband_four_way():  # TestMultiBand_FourWay
    mb = R.MultiBand([200, 2000, 10000], 4, FS)
    assert mb.NumBands() == 4 and np.isfinite(mb.ProcessSample(1.0)).all()


# ---- multiband_test.go: constructor and validation ---------------------------
NEW_OK = {  # TestNewMultibandCompressor
    "2-band LR4": ([1000], 4, 48000.0),
    "3-band LR4": ([500, 5000], 4, 48000.0),
    "4-band LR8": ([200, 2000, 10000], 8, 48000.0),
    "2-band LR2": ([1000], 2, 48000.0),
    "2-band LR12": ([1000], 12, 48000.0),
    "7-band max": ([100, 300, 1000, 3000, 8000, 16000], 4, 48000.0),
    "8 bands": ([60, 150, 400, 1000, 2500, 6000, 12000], 24, 48000.0),
}
NEW_ERRORS = {
    "no freqs": ([], 4, 48000.0),
    "odd order": ([1000], 3, 48000.0),
    "zero order": ([1000], 0, 48000.0),
    "negative order": ([1000], -2, 48000.0),
    "order too high": ([1000], 26, 48000.0),
    "zero sample rate": ([1000], 4, 0.0),
    "negative sample rate": ([1000], 4, -44100.0),
    "NaN sample rate": ([1000], 4, NAN),
    "freq at nyquist": ([24000], 4, 48000.0),
    "freq above nyquist": ([25000], 4, 48000.0),
    "freq below min": ([10], 4, 48000.0),
    "non-ascending freqs": ([5000, 500], 4, 48000.0),
    "duplicate freqs": ([1000, 1000], 4, 48000.0),
    "NaN freq": ([NAN], 4, 48000.0),
    "too many bands": ([100, 200, 400, 800, 1600, 3200, 6400, 12800], 4, 48000.0),
}


@pytest.mark.parametrize("name", list(NEW_OK))
def test_new_multiband_compressor(name):
    freqs, order, fs = NEW_OK[name]
    mc = R.MultibandCompressor(freqs, order, fs)
    assert (mc.NumBands(), mc.CrossoverOrder(), mc.SampleRate()) == (len(freqs) + 1, order, fs)


@pytest.mark.parametrize("name", list(NEW_ERRORS))
def test_new_multiband_compressor_errors(name):
    with pytest.raises(ValueError):
        R.MultibandCompressor(*NEW_ERRORS[name])


def test_new_with_config():  # TestNewMultibandCompressorWithConfig
    configs = [
        {"ThresholdDB": -30, "Ratio": 2.0, "KneeDB": 6.0, "AttackMs": 20, "ReleaseMs": 200, "AutoMakeup": True},
        {"ThresholdDB": -20, "Ratio": 4.0, "KneeDB": 3.0, "AttackMs": 10, "ReleaseMs": 100},
        {"ThresholdDB": -15, "Ratio": 6.0, "KneeDB": 0.0, "AttackMs": 5, "ReleaseMs": 50},
    ]
    mc = R.MultibandCompressor([500, 5000], 4, FS, configs)
    assert mc.Band(0)["threshold_db"] == -30 and mc.Band(1)["ratio"] == 4.0 and mc.Band(2)["attack_ms"] == 5.0
    assert mc.Band(2)["knee_db"] == 0.0  # a hard knee is applied, not skipped
    with pytest.raises(ValueError):
        R.MultibandCompressor([500, 5000], 4, FS, [{}, {}])
    with pytest.raises(ValueError):
        R.MultibandCompressor([1000], 4, FS, [{"Ratio": 0.5}, {}])


def test_accessors():  # TestMultibandAccessors
    mc = R.MultibandCompressor([500, 5000], 4, FS)
    got = mc.CrossoverFreqs()
    assert got == [500, 5000]
    got[0] = 999
    assert mc.CrossoverFreqs()[0] == 500


# ---- setters ----------------------------------------------------------------
def test_set_band_params():  # TestMultibandSetBandParams
    mc = R.MultibandCompressor([1000], 4, FS)
    mc.SetBandThreshold(0, -30)
    mc.SetBandRatio(1, 8.0)
    mc.SetBandKnee(0, 12.0)
    mc.SetBandAttack(0, 5.0)
    mc.SetBandRelease(1, 200.0)
    mc.SetBandMakeupGain(0, 3.0)
    b0, b1 = mc.Band(0), mc.Band(1)
    assert (b0["threshold_db"], b1["ratio"], b0["knee_db"], b0["attack_ms"], b1["release_ms"]) == (-30, 8, 12, 5, 200)
    assert b0["makeup_db"] == 3.0 and not b0["auto_makeup"]
    mc.SetBandAutoMakeup(0, True)
    mc.SetBandTopology(0, 1)
    mc.SetBandDetectorMode(0, 1)
    mc.SetBandFeedbackRatioScale(0, False)
    mc.SetBandRMSWindow(0, 25)
    mc.SetBandSidechainLowCut(0, 300)
    mc.SetBandSidechainHighCut(0, 5000)
    b0 = mc.Band(0)
    assert b0["auto_makeup"] and b0["topology"] == 1 and b0["detector_mode"] == 1 and not b0["feedback_ratio_scale"]
    assert (b0["rms_window_ms"], b0["sidechain_low_cut_hz"], b0["sidechain_high_cut_hz"]) == (25, 300, 5000)
    for call in (lambda: mc.SetBandThreshold(-1, -20), lambda: mc.SetBandThreshold(2, -20),
                 lambda: mc.SetBandRatio(-1, 2.0), lambda: mc.SetBandKnee(5, 6.0), lambda: mc.SetBandAttack(5, 10.0),
                 lambda: mc.SetBandRelease(5, 100.0), lambda: mc.SetBandMakeupGain(5, 3.0),
                 lambda: mc.SetBandAutoMakeup(5, True), lambda: mc.SetBandTopology(5, 1),
                 lambda: mc.SetBandDetectorMode(5, 1), lambda: mc.SetBandFeedbackRatioScale(5, True),
                 lambda: mc.SetBandRMSWindow(5, 20), lambda: mc.SetBandSidechainLowCut(5, 100),
                 lambda: mc.SetBandSidechainHighCut(5, 1000), lambda: mc.SetBandConfig(5, {})):
        with pytest.raises(IndexError):
            call()
    before = mc.Band(0)
    with pytest.raises(ValueError):
        mc.SetBandRatio(0, 0.5)
    with pytest.raises(ValueError):
        mc.SetBandThreshold(0, NAN)
    assert mc.Band(0) == before  # a rejected value changes nothing


def test_set_all_bands():  # TestMultibandSetAllBands
    mc = R.MultibandCompressor([500, 5000], 4, FS)
    mc.SetAllBandsThreshold(-15)
    mc.SetAllBandsRatio(3.0)
    mc.SetAllBandsKnee(10.0)
    mc.SetAllBandsAttack(15.0)
    mc.SetAllBandsRelease(250.0)
    mc.SetAllBandsTopology(1)
    mc.SetAllBandsDetectorMode(1)
    mc.SetAllBandsFeedbackRatioScale(False)
    mc.SetAllBandsRMSWindow(30)
    for i in range(mc.NumBands()):
        b = mc.Band(i)
        assert (b["threshold_db"], b["ratio"], b["knee_db"], b["attack_ms"], b["release_ms"]) == (-15, 3, 10, 15, 250)
        assert b["topology"] == 1 and b["detector_mode"] == 1 and not b["feedback_ratio_scale"]
        assert b["rms_window_ms"] == 30


def test_set_all_bands_invalid():  # TestMultibandSetAllBandsInvalid
    mc = R.MultibandCompressor([1000], 4, FS)
    for call in (lambda: mc.SetAllBandsRatio(0.5), lambda: mc.SetAllBandsThreshold(NAN), lambda: mc.SetAllBandsKnee(-1),
                 lambda: mc.SetAllBandsAttack(0.01), lambda: mc.SetAllBandsRelease(0.1),
                 lambda: mc.SetAllBandsRMSWindow(0.5)):
        with pytest.raises(ValueError):
            call()


def test_set_all_bands_stops_at_the_first_rejection():
    """SetAllBands* applies band by band (:331-437): bands before the one that rejects stay changed."""
    mc = R.MultibandCompressor([500, 5000], 4, FS)
    mc.SetBandSidechainHighCut(1, 100.0)
    with pytest.raises(ValueError):
        mc._all("SetBandSidechainLowCut", 200.0)  # band 1: low >= high
    assert [mc.Band(i)["sidechain_low_cut_hz"] for i in range(3)] == [200.0, 0.0, 0.0]


def test_set_band_config():  # TestSetBandConfig
    mc = R.MultibandCompressor([1000], 4, FS)
    mc.SetBandConfig(0, {"ThresholdDB": -25, "Ratio": 6.0, "KneeDB": 8.0, "AttackMs": 15.0, "ReleaseMs": 150.0,
                         "MakeupGainDB": 5.0, "AutoMakeup": False, "Topology": 1, "DetectorMode": 1,
                         "FeedbackRatioScale": False, "RMSWindowMs": 20.0, "SidechainLowCutHz": 200.0,
                         "SidechainHighCutHz": 6000.0})
    b = mc.Band(0)
    assert (b["threshold_db"], b["ratio"], b["knee_db"], b["attack_ms"], b["release_ms"]) == (-25, 6, 8, 15, 150)
    assert not b["auto_makeup"] and b["topology"] == 1 and b["detector_mode"] == 1 and not b["feedback_ratio_scale"]
    assert b["rms_window_ms"] == 20.0
    keep = mc.Band(1)
    mc.SetBandConfig(1, {"Ratio": 0, "AttackMs": 0, "ReleaseMs": 0, "ThresholdDB": None})  # all "keep"
    assert mc.Band(1) == keep


# ---- processing -------------------------------------------------------------
def test_zero_in_zero_out():  # TestMultibandProcessSampleZero
    mc = R.MultibandCompressor([1000], 4, FS)
    mc.Reset()
    assert all(mc.ProcessSample(0.0) == 0 for _ in range(100))


def test_finite_outputs():  # TestMultibandProcessSampleFinite, ...SampleMulti, ...InPlaceMulti(Empty)
    mc = R.MultibandCompressor([500, 5000], 4, FS)
    assert np.isfinite(mc.ProcessInPlace(impulse(1000, 0.5))).all()
    assert mc.ProcessSampleMulti(0.5).shape == (3,)
    assert mc.ProcessInPlaceMulti(impulse(128, 0.5)).shape == (3, 128)
    assert R.MultibandCompressor([1000], 4, FS).ProcessInPlaceMulti([]).shape == (2, 0)
    assert R.MultibandCompressor([1000], 4, FS).ProcessInPlace([]).shape == (0,)


def test_process_in_place_equals_sample_loop():  # TestMultibandProcessInPlace
    a, b = R.MultibandCompressor([1000], 4, FS), R.MultibandCompressor([1000], 4, FS)
    for mc in (a, b):
        for i in range(mc.NumBands()):
            mc.SetBandAutoMakeup(i, False)
            mc.SetBandMakeupGain(i, 0)
    x = sine(256, 440, 0.3)
    want = np.array([a.ProcessSample(v) for v in x])
    assert np.max(np.abs(b.ProcessInPlace(x) - want)) <= 1e-10


def test_compresses_loud_signal():  # TestMultibandCompressesLoudSignal
    mc = R.MultibandCompressor([1000], 4, FS)
    for i in range(mc.NumBands()):
        mc.SetBandThreshold(i, -20)
        mc.SetBandRatio(i, 10.0)
        mc.SetBandKnee(i, 0)
        mc.SetBandAttack(i, 0.1)
        mc.SetBandAutoMakeup(i, False)
        mc.SetBandMakeupGain(i, 0)
    assert abs(mc.ProcessInPlace(np.full(5000, 0.8))[-1]) < 0.8


def test_band_independence():  # TestMultibandBandIndependence
    mc = R.MultibandCompressor([1000], 4, FS)
    mc.SetBandThreshold(0, -30)
    mc.SetBandRatio(0, 20.0)
    mc.SetBandAutoMakeup(0, False)
    mc.SetBandMakeupGain(0, 0)
    mc.SetBandRatio(1, 1.0)
    assert mc.Band(0)["ratio"] == 20.0 and mc.Band(1)["ratio"] == 1.0


def test_reset_determinism():  # TestMultibandReset
    mc, fresh = R.MultibandCompressor([1000], 4, FS), R.MultibandCompressor([1000], 4, FS)
    mc.ProcessInPlace(np.full(100, 0.5))
    mc.Reset()
    assert mc.ProcessSample(0.3) == fresh.ProcessSample(0.3)


def test_metrics():  # TestMultibandMetrics
    mc = R.MultibandCompressor([1000], 4, FS)
    mc.ProcessInPlace(np.full(500, 0.8))
    m = mc.GetMetrics()
    assert len(m) == 2 and any(b[0] > 0 for b in m)


@pytest.mark.parametrize("order", [2, 4, 8, 12])
def test_different_orders(order):  # TestMultibandDifferentOrders
    mc = R.MultibandCompressor([1000], order, FS)
    assert mc.CrossoverOrder() == order and math.isfinite(mc.ProcessSample(0.5))


def unity(mc):
    for i in range(mc.NumBands()):
        mc.SetBandRatio(i, 1.0)
        mc.SetBandAutoMakeup(i, False)
        mc.SetBandMakeupGain(i, 0)
    return mc


def test_energy_preservation():  # TestMultibandEnergyPreservation
    y = unity(R.MultibandCompressor([500, 5000], 4, FS)).ProcessInPlace(impulse(8192))
    assert abs(float(np.sum(y * y)) - 1.0) <= 0.02


def test_recombination_consistency():  # TestMultibandRecombinationConsistency
    mc = unity(R.MultibandCompressor([300, 3000], 4, FS))
    x = sine(512, 220, 0.4) + sine(512, 2200, 0.2)
    per_band = mc.ProcessInPlaceMulti(x)
    mc.Reset()
    assert np.max(np.abs(mc.ProcessInPlace(x) - per_band.sum(axis=0))) <= 1e-12


def test_phase_latency_sanity():  # TestMultibandPhaseLatencySanity
    y = unity(R.MultibandCompressor([500, 5000], 4, FS)).ProcessInPlace(impulse(2048))
    e = y * y
    assert abs(y[0]) >= 1e-6 and e[:256].sum() / e.sum() >= 0.8


# ---- the host-only ABI ------------------------------------------------------
def _validate(fn, freqs, order, fs):
    f = _lib.f64(freqs)
    return fn(_lib.ptr(f), int(f.size), int(order), float(fs))


@pytest.mark.parametrize("name", list(XOVER_OK) + list(XOVER_ERRORS) + list(XOVER_LIMITS))
def test_ad_xover_validate(name):
    ok = name in XOVER_OK
    args = (XOVER_OK if ok else XOVER_ERRORS if name in XOVER_ERRORS else XOVER_LIMITS)[name]
    rc = _validate(_lib.lib().ad_xover_validate, *args)
    assert rc == (_lib.AD_OK if ok else _lib.AD_ERR_INVALID_ARGUMENT), name
    if name not in XOVER_LIMITS:  # the restatement applies the reference's rules alone
        try:
            R.MultiBand(*args)
            assert ok
        except ValueError:
            assert not ok


@pytest.mark.parametrize("name", list(NEW_OK) + list(NEW_ERRORS))
def test_ad_multiband_validate(name):
    ok = name in NEW_OK
    rc = _validate(_lib.lib().ad_multiband_validate, *(NEW_OK if ok else NEW_ERRORS)[name])
    assert rc == (_lib.AD_OK if ok else _lib.AD_ERR_INVALID_ARGUMENT), name


def sections_of(order):
    """Sections per side: the halved-order Butterworth prototype twice, a first-order section for an odd half."""
    half = order // 2
    return 2 * (half // 2 + half % 2)


@pytest.mark.parametrize("order", list(range(2, 26, 2)))
def test_ad_xover_sections_equal_design_on_bits(order):
    """Every even order ad_xover_create accepts: 2 / 2 / 4 / 4 / 12 sections for orders 2 / 4 / 6 / 8 / 24."""
    want = sections_of(order)
    assert [sections_of(o) for o in (2, 4, 6, 8, 24)] == [2, 2, 4, 4, 12]
    freqs = [60.0, 150.0, 400.0, 1000.0, 2500.0, 6000.0, 12000.0]
    tab = P.crossover_sections(freqs, order, FS)
    assert tab.shape == (7, 2, want, 5)
    ref = np.array([design.crossover(f, order, FS) for f in freqs])
    assert ref.shape == tab.shape
    assert np.array_equal(tab.view(np.int64), ref.view(np.int64)), np.argwhere(tab.view(np.int64) != ref.view(np.int64))[:4]
    # the edge frequencies of the GPU cases, and another sample rate
    for fr, fs in (([20.0, 23999.0], 48000.0), ([1000.0], 44100.0)):
        tab = P.crossover_sections(fr, order, fs)
        ref = np.array([design.crossover(f, order, fs) for f in fr])
        assert np.array_equal(tab.view(np.int64), ref.view(np.int64))
    assert np.array_equal(R.MultiBand(freqs, order, FS).sections().view(np.int64), ref_bits(freqs, order))


def ref_bits(freqs, order):
    return P.crossover_sections(freqs, order, FS).view(np.int64)


def test_ad_xover_sections_buffer_rules():
    L = _lib.lib()
    f = _lib.f64([1000.0])
    s = C.c_int()
    assert L.ad_xover_sections(_lib.ptr(f), 1, 4, FS, None, 0, C.byref(s)) == _lib.AD_OK and s.value == 2
    small = np.zeros(19)
    assert L.ad_xover_sections(_lib.ptr(f), 1, 4, FS, _lib.ptr(small), 19, C.byref(s)) == _lib.AD_ERR_LENGTH_MISMATCH
    assert L.ad_xover_sections(_lib.ptr(f), 1, 3, FS, None, 0, C.byref(s)) == _lib.AD_ERR_INVALID_ARGUMENT


def test_ad_multiband_set_band_host_checks():
    """ad_multiband_set_band has no host-only path past its handle check: a handle needs a device, so all
    this test can show of set_band itself is that a null handle is an argument error and not a crash.  That
    set_band rejects a bad config or band index and changes nothing is shown on a device handle
    (test_multiband_gpu.py::test_multiband_setter_semantics).  Covered here besides: the check set_band runs,
    ad_compressor_validate, agrees with the restatement's rules on the default config and on a bad ratio."""
    L = _lib.lib()
    cfg = _lib.CompressorConfig()
    L.ad_compressor_default_config(C.byref(cfg), FS)
    assert L.ad_compressor_validate(C.byref(cfg)) == _lib.AD_OK
    R.validate_compressor({n: getattr(cfg, n) for n, _ in _lib.CompressorConfig._fields_})
    assert L.ad_multiband_set_band(None, 0, C.byref(cfg)) == _lib.AD_ERR_INVALID_ARGUMENT
    assert L.ad_multiband_get_band(None, 0, C.byref(cfg)) == _lib.AD_ERR_INVALID_ARGUMENT
    assert L.ad_fx_chain_reset_compressor_metrics(None) == _lib.AD_ERR_INVALID_ARGUMENT
    cfg.ratio = 0.5
    assert L.ad_compressor_validate(C.byref(cfg)) == _lib.AD_ERR_INVALID_ARGUMENT
    with pytest.raises(ValueError):
        R.validate_compressor({n: getattr(cfg, n) for n, _ in _lib.CompressorConfig._fields_})
