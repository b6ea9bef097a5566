"""Host side of algodsp.resample: validation before any device use, the ratio
approximation, the prototype designer's properties, and the restated reference
(resample_ref) held to itself and to the reference's own quality bounds.
None of this needs a GPU."""
import math

import numpy as np
import pytest

import resample_ref as RR
from algodsp import resample as R

PROFILES = [R.QualityFast, R.QualityBalanced, R.QualityBest]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def same(a, b):
    a, b = bits(a), bits(b)
    return a.shape == b.shape and np.array_equal(a, b)


def test_invalid_ratio_precedes_device_use():
    """resample.go:154-156"""
    for up, down in [(0, 1), (1, 0), (-3, 2), (2, -3)]:
        with pytest.raises(R.ErrInvalidRatio):
            R.NewRational(up, down)
    with pytest.raises(R.ErrInvalidRatio):
        R.Resample(np.ones(4), 0, 1)


def test_invalid_rate_precedes_device_use():
    """resample.go:191-193"""
    for a, b in [(0.0, 48000.0), (48000.0, 0.0), (-1.0, 48000.0), (48000.0, -44100.0),
                 (float("nan"), 48000.0), (48000.0, float("nan"))]:
        with pytest.raises(R.ErrInvalidRate):
            R.NewForRates(a, b)


def test_abi_create_validates_before_any_device():
    """ad_resampler_create: ratio, channel count and prototype are checked
    first, so these fail the same way with and without a GPU."""
    import ctypes as C

    from algodsp import _lib

    L = _lib.lib()
    good = np.ones(320)

    def create(up, down, taps, n_taps, channels):
        h = C.c_void_p()
        rc = L.ad_resampler_create(up, down, None if taps is None else _lib.ptr(taps), n_taps, channels, 0,
                                   C.byref(h))
        assert not h.value or rc == _lib.AD_OK
        if h.value:
            L.ad_resampler_destroy(h)
        return rc

    bad_tap = good.copy()
    bad_tap[7] = np.nan
    inf_tap = good.copy()
    inf_tap[319] = -np.inf
    for args in [(0, 1, good, 320, 1), (1, 0, good, 320, 1), (-2, 3, good, 320, 1), (160, 147, good, 320, 0),
                 (160, 147, good, 319, 1), (160, 147, good, 0, 1), (160, 147, None, 320, 1),
                 (320, 294, good[:240], 240, 1),  # 240 is no multiple of the reduced up, 160
                 (160, 147, bad_tap, 320, 1), (160, 147, inf_tap, 320, 1),
                 ((1 << 30) + 1, 1, good, 320, 1), (1, (1 << 30) + 1, good, 320, 1)]:
        assert create(*args) == _lib.AD_ERR_INVALID_ARGUMENT, args[:2] + args[3:]
    if _lib.device_count() == 0:
        assert create(160, 147, good, 320, 1) == _lib.AD_ERR_NO_DEVICE  # no CPU fallback
    assert L.ad_resampler_reset(None) == _lib.AD_ERR_INVALID_ARGUMENT
    assert L.ad_resampler_taps_per_phase(None) == 0
    L.ad_resampler_destroy(None)


def test_approximate_ratio():
    """resample_design.go:71-114"""
    assert R.approximate_ratio(48000 / 44100) == (160, 147)
    assert R.approximate_ratio(96000 / 48000) == (2, 1)
    assert R.approximate_ratio(44100 / 48000) == (147, 160)
    assert R.approximate_ratio(1.0) == (1, 1)
    for bad in (0.0, -2.0, float("nan"), float("inf")):
        assert R.approximate_ratio(bad) == (1, 1)
    # the denominator cap stops the continued fraction (pi: 3, 22/7, 333/106, 355/113)
    assert R.approximate_ratio(math.pi, 10) == (22, 7)
    assert R.approximate_ratio(math.pi, 112) == (333, 106)
    assert R.approximate_ratio(math.pi, 0) == R.approximate_ratio(math.pi, 4096)


def test_quality_profiles():
    """resample.go:36-45"""
    assert R.QualityProfile(R.QualityFast)[:3] == (16, 0.88, 5.0)
    assert R.QualityProfile(R.QualityBalanced)[:3] == (32, 0.92, 7.5)
    assert R.QualityProfile(R.QualityBest)[:3] == (64, 0.96, 9.0)
    assert R.QualityProfile(17) == R.QualityProfile(R.QualityBalanced)


def test_option_acceptance_rules():
    """resample.go:58-132: an out-of-range option is ignored, not an error."""
    prof = R.QualityProfile(R.QualityFast)
    base = R._config(R.QualityFast, None, None, None, None)
    assert base == (R.QualityFast, prof.TapsPerPhase, prof.CutoffScale, prof.KaiserBeta, 4096)
    assert R._config(R.QualityFast, 0, 0.0, 0.0, 0) == base
    assert R._config(R.QualityFast, -4, 1.5, -1.0, -7) == base
    assert R._config(R.QualityFast, 24, 1.0, 3.0, 100) == (R.QualityFast, 24, 1.0, 3.0, 100)
    assert R._config(None, None, None, None, None)[0] == R.QualityBalanced


@pytest.mark.parametrize("q", PROFILES)
@pytest.mark.parametrize("up,down", [(1, 2), (2, 1), (3, 2), (160, 147)])
def test_designer_properties(q, up, down):
    """designPolyphaseFIR (resample_design.go:9-50): T*up taps that sum to up,
    symmetric about the centre."""
    p = R.QualityProfile(q)
    h = R.design_polyphase_fir(up, down, p.TapsPerPhase, p.CutoffScale, p.KaiserBeta)
    assert h.dtype == np.float64 and h.shape == (p.TapsPerPhase * up,)
    assert abs(math.fsum(h) - up) <= 1e-12 * up
    assert np.max(np.abs(h - h[::-1])) <= 1e-14 * np.max(np.abs(h))
    assert np.all(np.isfinite(h))


def test_designer_rejects_what_the_reference_rejects():
    """resample_design.go:10-27"""
    with pytest.raises(R.ErrInvalidRatio):
        R.design_polyphase_fir(0, 1, 16, 0.9, 5.0)
    with pytest.raises(ValueError):
        R.design_polyphase_fir(1, 1, 0, 0.9, 5.0)
    with pytest.raises(ValueError):
        R.design_polyphase_fir(1, 1, 16, 1.5, 5.0)
    with pytest.raises(ValueError):
        R.design_polyphase_fir(1, 1, 16, 1.0, 5.0)  # fc = 0.5
    # beta 0: a rectangular window (kaiserWindow returns 1)
    h = R.design_polyphase_fir(1, 2, 4, 1.0, 0.0)
    assert h.shape == (4,) and abs(h.sum() - 1) < 1e-15


@pytest.mark.parametrize("up,down,T", RR.SHAPES + RR.MORE_SHAPES)
def test_reference_loop_and_vector_forms_agree(up, down, T):
    """The literal loop and the vectorised form give the same bits and leave
    the same state, whole and chunked, on the GPU test shapes."""
    taps = RR.random_taps(up, T, 7 * up + down)
    for n in RR.N_IN:
        x = RR.random_input(1, n, n + up)[0]
        a, b = RR.Ref(up, down, taps), RR.Ref(up, down, taps)
        assert a.predict_output_len(n) == b.predict_output_len(n)
        ya, yb = a.process(x), b.process_vec(x)
        assert same(ya, yb)
        assert (a.phase, a.input_index, a.total_in) == (b.phase, b.input_index, b.total_in)
        assert same(a.history, b.history)
    x = RR.random_input(1, 1500, 99)[0]
    whole = RR.Ref(up, down, taps).process_vec(x)
    for chunk, vec in [(257, False), (3, True), (1, True)]:
        got, lens = RR.resample(up, down, taps, x[:1500 if chunk > 1 else 300], chunks=chunk, vec=vec)
        assert same(got[0], whole[:got.shape[1]]), chunk
        # a call of `chunk` samples yields at least floor(chunk*up/down) outputs
        assert (0 in lens) == (chunk * up < down)


def test_reference_predict_matches_closed_form():
    """PredictOutputLen's counting loop (resample.go:295-313) against
    ceil((L*up - phase) / down), L = totalIn + n - inputIndex."""
    for up, down, T in RR.SHAPES:
        r = RR.Ref(up, down, RR.random_taps(up, T, 1))
        for n in (1, 2, 5, 64, 300, 7, 1, 1, 1, 1000, 3):
            L = r.total_in + n - r.input_index
            want = 0 if L <= 0 else -((-(L * r.up - r.phase)) // r.down)
            assert r.predict_output_len(n) == want
            assert len(r.process_vec(np.zeros(n))) == want


def _sine(freq, fs, n):
    return np.array([math.sin(2 * math.pi * freq * float(i) / fs) for i in range(n)])


def _rms(x):
    return math.sqrt(float(np.sum(x * x)) / len(x))


@pytest.mark.parametrize("q,max_pass_db,min_stop_db", [(R.QualityFast, 0.7, 20.0), (R.QualityBalanced, 0.35, 35.0),
                                                       (R.QualityBest, 0.2, 50.0)])
def test_quality_modes_passband_and_stopband(q, max_pass_db, min_stop_db):
    """The reference's TestQualityModes_PassbandAndStopband
    (resample_design_test.go:20-65) with this designer's prototype through the
    restated Process: ratio 1/2, 2 kHz and 17 kHz sines at 48 kHz."""
    p = R.QualityProfile(q)
    h = R.design_polyphase_fir(1, 2, p.TapsPerPhase, p.CutoffScale, p.KaiserBeta)
    in_pass, in_stop = _sine(2000, 48000, 32768), _sine(17000, 48000, 32768)
    out_pass = RR.Ref(1, 2, h).process_vec(in_pass)
    out_stop = RR.Ref(1, 2, h).process_vec(in_stop)
    droop = abs(20 * math.log10(_rms(out_pass[2048:]) / _rms(in_pass[4096:])))
    atten = -20 * math.log10(_rms(out_stop[2048:]) / _rms(in_stop[4096:]))
    print(f"quality {q}: droop {droop:.4f} dB, attenuation {atten:.1f} dB")
    assert droop <= max_pass_db
    assert atten >= min_stop_db
