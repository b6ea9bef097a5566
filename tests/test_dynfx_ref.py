"""The restated transient shaper and de-esser (tests/dynfx_ref.py) against the
reference's own test cases and their own invariants, the host-only C ABI
functions against the restatement, and the graph compiler's node parameters:
everything that needs no device."""
import ctypes as C
import math

import numpy as np
import pytest

import dynfx_ref as R
from algodsp import _lib, design, effectchain as E, processors as P, signals

NAN, INF = float("nan"), float("inf")
FS = 48000.0


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def sine(n, hz, amp, fs=FS, start=0):
    return [amp * math.sin(2 * math.pi * hz * float(start + i) / fs) for i in range(n)]


def refused(fn, v):
    try:
        fn(v)
    except ValueError:
        return True
    return False


# the setters' ranges: (restatement setter, config field, lowest, highest); transient_shaper.go:14-19, deesser.go:57-72
TRANSIENT_RANGES = (("SetAttackAmount", "attack_amount", -1.0, 1.0), ("SetSustainAmount", "sustain_amount", -1.0, 1.0),
                    ("SetAttack", "attack_ms", 0.1, 200.0), ("SetRelease", "release_ms", 1.0, 2000.0))
DEESSER_RANGES = (("SetFrequency", "freq_hz", 1000.0, 20000.0), ("SetQ", "q", 0.1, 10.0), ("SetRatio", "ratio", 1.0, 100.0),
                  ("SetKnee", "knee_db", 0.0, 12.0), ("SetAttack", "attack_ms", 0.01, 50.0),
                  ("SetRelease", "release_ms", 1.0, 500.0), ("SetRange", "range_db", -60.0, 0.0))


def edges(lo, hi):
    """Just inside and just outside both ends, and the values no range holds."""
    return (lo, hi, math.nextafter(lo, INF), math.nextafter(hi, -INF), math.nextafter(lo, -INF),
            math.nextafter(hi, INF), NAN, INF, -INF)


def cfg_of(kind, fs=FS, **kv):
    c = {"transient": _lib.TransientConfig, "deesser": _lib.DeEsserConfig}[kind]()
    getattr(_lib.lib(), f"ad_{kind}_default_config")(C.byref(c), fs)
    for k, v in kv.items():
        setattr(c, k, v)
    return c


def validate(kind, cfg):
    return getattr(_lib.lib(), f"ad_{kind}_validate")(C.byref(cfg) if cfg is not None else None)


# ---- the reference's cases on the restatement -------------------------------
def test_transient_defaults_and_setter_edges():
    """TestTransientShaperDefaults, TestTransientShaperParameterValidation transient_shaper_test.go:35-80."""
    ts = R.TransientShaper(FS)
    assert (ts.attackAmount, ts.sustainAmount, ts.attackMs, ts.releaseMs) == (0.0, 0.0, 10.0, 120.0)
    for v in (-1.1, ):
        assert refused(ts.SetAttackAmount, v)
    assert refused(ts.SetSustainAmount, 1.1) and refused(ts.SetAttack, 0.05) and refused(ts.SetRelease, 0.5)
    for name, _field, lo, hi in TRANSIENT_RANGES:
        for v in edges(lo, hi):
            assert refused(getattr(ts, name), v) == (not lo <= v <= hi), (name, v)
    for fs in (0.0, -1.0, NAN, INF):
        with pytest.raises(ValueError):
            R.TransientShaper(fs)
        assert refused(ts.SetSampleRate, fs)
    # a refused value changes nothing: the last accepted one (just inside the upper end) stands
    assert (ts.attackAmount, ts.attackMs, ts.releaseMs) == tuple(math.nextafter(v, -INF) for v in (1.0, 200.0, 2000.0))


def test_transient_attack_boost_and_sustain_tail():
    """TestTransientShaperAttackBoostsRisingEdge, ...NegativeSustainReducesDecayTail :113-169."""
    neutral, boosted = R.TransientShaper(FS), R.TransientShaper(FS)
    boosted.SetAttackAmount(1.0)
    for _ in range(128):
        neutral.ProcessSample(0.0)
        boosted.ProcessSample(0.0)
    assert boosted.ProcessSample(1.0) > neutral.ProcessSample(1.0)
    neutral, shaped = R.TransientShaper(FS), R.TransientShaper(FS)
    shaped.SetSustainAmount(-1.0)
    shaped.SetRelease(40)
    tails = [0.0, 0.0]
    for i in range(600):
        x = 0.8 if i < 300 else 0.15
        a, b = neutral.ProcessSample(x), shaped.ProcessSample(x)
        if i >= 300:
            tails[0] += abs(a)
            tails[1] += abs(b)
    assert tails[1] < tails[0]


def test_transient_silence_neutral_and_reset():
    """Silence stays silence, amounts 0 are the identity, Reset restores a deterministic state (:171-198)."""
    ts = R.TransientShaper(FS)
    assert all(bits(ts.ProcessSample(0.0)) == 0 for _ in range(64))
    x = sine(256, 330, 0.6)
    assert [ts.ProcessSample(v) for v in x] == x
    ts.SetAttackAmount(0.7)
    ts.SetSustainAmount(-0.2)
    ts.Reset()
    out1 = [ts.ProcessSample(v) for v in x]
    assert ts.envelope != 0.0
    ts.Reset()
    assert ts.envelope == 0.0 and np.array_equal(bits(out1), bits([ts.ProcessSample(v) for v in x]))


def test_deesser_defaults_and_setter_edges():
    """TestDeEsserDefaults, TestDeEsserSetterValidation deesser_test.go:41-168."""
    d = R.DeEsser(FS)
    assert (d.freqHz, d.q, d.thresholdDB, d.ratio, d.kneeDB, d.attackMs, d.releaseMs, d.rangeDB) == \
        (6000.0, 1.5, -20.0, 4.0, 3.0, 0.5, 20.0, -24.0)
    assert (d.mode, d.detector, d.listen, d.filterOrder) == (R.SPLIT_BAND, R.DETECT_BANDPASS, False, 2)
    assert d.GetMetrics() == (0.0, 1.0)
    d = R.DeEsser(96000.0)  # 20 kHz is below this Nyquist
    for name, _field, lo, hi in DEESSER_RANGES:
        for v in edges(lo, hi):
            assert refused(getattr(d, name), v) == (not lo <= v <= hi), (name, v)
    for v in (-1e300, 1e300, 0.0):
        assert not refused(d.SetThreshold, v)  # any finite value
    for v in (NAN, INF, -INF):
        assert refused(d.SetThreshold, v)
    for v in (-1, 2):
        assert refused(d.SetMode, v) and refused(d.SetDetector, v)
    for v in (0, 5):
        assert refused(d.SetFilterOrder, v)
    d30 = R.DeEsser(30000.0)  # :235: below Nyquist
    assert refused(d30.SetFrequency, 15000.0) and not refused(d30.SetFrequency, math.nextafter(15000.0, 0))
    d48 = R.DeEsser(FS)
    assert refused(d48.SetSampleRate, 2 * d48.freqHz) and d48.sampleRate == FS  # frequency >= fs / 2
    for fs in (0.0, -1.0, NAN, INF):
        with pytest.raises(ValueError):
            R.DeEsser(fs)
        assert refused(d48.SetSampleRate, fs)


def test_deesser_silence_ratio_one_range_floor_and_hard_knee():
    """:292-306, :803-830, :751-800, :672-697."""
    d = R.DeEsser(FS)
    assert all(d.ProcessSample(0.0) == 0.0 for _ in range(1024))
    d = R.DeEsser(FS)
    d.SetRatio(1)
    d.SetMode(R.WIDEBAND)
    for v in sine(1024, 6000, 0.5):
        assert abs(d.ProcessSample(v) - v) <= 1e-10
    d = R.DeEsser(FS)
    d.SetThreshold(-60)
    d.SetRatio(100)
    d.SetRange(-12)
    d.SetMode(R.WIDEBAND)
    d.SetKnee(0)
    for v in sine(8192, 6000, 0.9):
        d.ProcessSample(v)
    floor = math.pow(10, -12.0 / 20.0)
    assert d.GetMetrics()[1] >= floor * 0.95 and d.GetMetrics()[1] == d.rangeLin == floor
    d = R.DeEsser(FS)
    d.SetKnee(0)
    d.SetThreshold(-30)
    for v in sine(1024, 6000, 0.5):
        d.ProcessSample(v)
    assert d.GetMetrics()[1] < 1.0
    assert d.calculateGain(0.0) == 1.0 and d.calculateGain(-1.0) == 1.0
    assert d.calculateGain(2.0 ** d.thresholdLog2 * 0.999) == 1.0 and d.calculateGain(1.0) < 1.0


def test_deesser_listen_is_the_bare_cascade_and_reset_and_metrics():
    """:464-517 (listen), :602-631 (Reset), :634-669 (metrics)."""
    x = sine(512, 6000, 0.5)
    d = R.DeEsser(FS)
    d.SetListen(True)
    bare = [R.Section(design.bandpass(6000.0, 1.5, FS)) for _ in range(2)]
    for v in x:
        want = v
        for s in bare:
            want = s.ProcessSample(want)
        assert bits(d.ProcessSample(v)) == bits(want)
    assert d.envLevel == 0.0 and d.GetMetrics() == (0.0, 1.0)  # listen touches nothing else
    d = R.DeEsser(FS)
    d.SetThreshold(-30)
    out1 = [d.ProcessSample(v) for v in x]
    assert d.GetMetrics()[0] > 0 and d.GetMetrics()[1] < 1.0
    d.ResetMetrics()
    assert d.GetMetrics() == (0.0, 1.0) and d.envLevel > 0
    d.Reset()
    assert d.envLevel == 0.0 and d.GetMetrics() == (0.0, 1.0) and not np.any(d.states()[0]) and not np.any(d.states()[1])
    assert np.array_equal(bits(out1), bits([d.ProcessSample(v) for v in x]))


# ---- the restatement's own invariants ---------------------------------------
@pytest.mark.parametrize("detector", [R.DETECT_BANDPASS, R.DETECT_HIGHPASS])
def test_band_equals_detected_until_listen_or_wideband_has_run(detector):
    """Equal sections, equal input, equal states: one cascade stands for both.  A call that advances
    detectFilters alone (listen :422-424, wideband :448-449) ends that."""
    x = 2.0 * signals.white_noise(600, 0xD7)
    for breaker in ("listen", "wideband"):
        d = R.DeEsser(FS)
        d.SetDetector(detector)
        d.ProcessInPlace(x[:200].copy())
        det, band = d.states()
        assert np.array_equal(bits(det), bits(band)) and np.any(det)
        if breaker == "listen":
            d.SetListen(True)
        else:
            d.SetMode(R.WIDEBAND)
        d.ProcessInPlace(x[200:400].copy())
        d.SetListen(False)
        d.SetMode(R.SPLIT_BAND)
        det, band = d.states()
        assert not np.array_equal(bits(det), bits(band))
        d.ProcessInPlace(x[400:416].copy())  # (both are stable and see the same input: the difference dies out later)
        det, band = d.states()
        assert not np.array_equal(bits(det), bits(band))


def test_rebuild_setters_zero_the_cascades_and_keep_the_envelope():
    x = 2.0 * signals.white_noise(300, 0xD8)
    for name, v in (("SetFrequency", 7000.0), ("SetQ", 2.0), ("SetDetector", R.DETECT_HIGHPASS), ("SetFilterOrder", 3),
                    ("SetSampleRate", 44100.0), ("SetDetector", R.DETECT_BANDPASS)):
        d = R.DeEsser(FS)
        d.ProcessInPlace(x.copy())
        env, met = d.envLevel, d.GetMetrics()
        assert env > 0 and np.any(d.states()[0])
        getattr(d, name)(v)
        assert not np.any(d.states()[0]) and not np.any(d.states()[1])
        assert d.envLevel == env and d.GetMetrics() == met
    for name, v in (("SetThreshold", -30.0), ("SetRatio", 8.0), ("SetKnee", 0.0), ("SetAttack", 1.0), ("SetRelease", 50.0),
                    ("SetRange", -12.0), ("SetMode", R.WIDEBAND), ("SetListen", True)):
        d = R.DeEsser(FS)
        d.ProcessInPlace(x.copy())
        before = d.states()
        getattr(d, name)(v)
        assert np.array_equal(bits(before[0]), bits(d.states()[0])) and np.array_equal(bits(before[1]), bits(d.states()[1]))


# ---- the host-only C ABI ----------------------------------------------------
def test_struct_sizes_and_symbols():
    assert C.sizeof(_lib.TransientConfig) == 7 * 8 and C.sizeof(_lib.DeEsserConfig) == 11 * 8 + 4 * 4
    L = _lib.lib()
    names = [f"ad_{k}_{f}" for k in ("transient", "deesser")
             for f in ("default_config", "validate", "derived", "create", "set_param", "get_config", "kernel_info",
                       "get_state", "set_state", "process", "process_device", "reset", "destroy")]
    names += ["ad_deesser_metrics", "ad_deesser_reset_metrics", "ad_deesser_gain"]
    declared = set(_lib.exported_symbols())
    for n in names:
        assert hasattr(L, n) and n in declared, n
    text = _lib.HEADER_PATH.read_text()
    for i, n in enumerate(("SAMPLE_RATE", "ATTACK_AMOUNT", "SUSTAIN_AMOUNT", "ATTACK", "RELEASE", "ATTACK_COEFF",
                           "RELEASE_COEFF")):
        assert f"#define AD_TRANSIENT_{n} {i} " in text and getattr(P.TransientShaper, f"P_{n}") == i
    for i, n in enumerate(("SAMPLE_RATE", "FREQ", "Q", "THRESHOLD", "RATIO", "KNEE", "ATTACK", "RELEASE", "RANGE",
                           "ATTACK_COEFF", "RELEASE_COEFF", "MODE", "DETECTOR", "LISTEN", "FILTER_ORDER")):
        assert f"#define AD_DEESSER_{n} {i} " in text and getattr(P.DeEsser, f"P_{n}") == i
    assert "#define AD_FXN_DEESSER 18 " in text and "#define AD_FXN_TRANSIENT 19 " in text
    assert (E.FXN_DEESSER, E.FXN_TRANSIENT) == (18, 19)


def test_validate_agrees_with_the_restatement_at_every_edge():
    assert validate("transient", None) == validate("deesser", None) == _lib.AD_ERR_INVALID_ARGUMENT
    assert validate("transient", cfg_of("transient")) == validate("deesser", cfg_of("deesser")) == _lib.AD_OK
    for kind, ranges, make in (("transient", TRANSIENT_RANGES, lambda: R.TransientShaper(96000.0)),
                               ("deesser", DEESSER_RANGES, lambda: R.DeEsser(96000.0))):
        for name, field, lo, hi in ranges:
            for v in edges(lo, hi):
                want = _lib.AD_ERR_INVALID_ARGUMENT if refused(getattr(make(), name), v) else _lib.AD_OK
                assert validate(kind, cfg_of(kind, 96000.0, **{field: v})) == want, (field, v)
        for fs in (0.0, -1.0, NAN, INF, -INF):
            assert validate(kind, cfg_of(kind, fs)) == _lib.AD_ERR_INVALID_ARGUMENT
        for f in ("attack_coeff", "release_coeff"):
            for v, want in ((0.0, _lib.AD_OK), (1.0, _lib.AD_OK), (0.5, _lib.AD_OK), (-1e-9, _lib.AD_ERR_INVALID_ARGUMENT),
                            (math.nextafter(1.0, 2.0), _lib.AD_ERR_INVALID_ARGUMENT), (NAN, _lib.AD_ERR_INVALID_ARGUMENT)):
                assert validate(kind, cfg_of(kind, **{f: v})) == want
    for v in (-1e300, 1e300):
        assert validate("deesser", cfg_of("deesser", threshold_db=v)) == _lib.AD_OK
    for v in (NAN, INF, -INF):
        assert validate("deesser", cfg_of("deesser", threshold_db=v)) == _lib.AD_ERR_INVALID_ARGUMENT
    for f, bad in (("mode", (-1, 2)), ("detector", (-1, 2)), ("listen", (-1, 2)), ("filter_order", (0, 5))):
        for v in bad:
            assert validate("deesser", cfg_of("deesser", **{f: v})) == _lib.AD_ERR_INVALID_ARGUMENT
    for v in (1, 2, 3, 4):
        assert validate("deesser", cfg_of("deesser", filter_order=v)) == _lib.AD_OK
    # the Nyquist rule of SetFrequency :235 and SetSampleRate :399
    assert validate("deesser", cfg_of("deesser", 30000.0, freq_hz=15000.0)) == _lib.AD_ERR_INVALID_ARGUMENT
    assert validate("deesser", cfg_of("deesser", 30000.0, freq_hz=math.nextafter(15000.0, 0))) == _lib.AD_OK
    assert validate("deesser", cfg_of("deesser", 12000.0)) == _lib.AD_ERR_INVALID_ARGUMENT
    assert validate("deesser", cfg_of("deesser", math.nextafter(12000.0, INF))) == _lib.AD_OK


@pytest.mark.parametrize("fs", [44100.0, 48000.0, 96000.0])
def test_derived_gives_the_restatements_bits(fs):
    for detector in (0, 1):
        for order in (1, 2, 3, 4):
            for freq, q, thr, knee, rng, att, rel in ((6000.0, 1.5, -20.0, 3.0, -24.0, 0.5, 20.0),
                                                      (1000.0, 0.1, -37.5, 0.0, -60.0, 0.01, 1.0),
                                                      (20000.0, 10.0, 0.0, 12.0, 0.0, 50.0, 500.0),
                                                      (7350.0, 0.7071, -3.3, 5.5, -13.7, 3.3, 77.0)):
                d = R.DeEsser(fs)
                d.SetFrequency(freq)
                d.SetQ(q)
                d.SetThreshold(thr)
                d.SetKnee(knee)
                d.SetRange(rng)
                d.SetAttack(att)
                d.SetRelease(rel)
                d.SetDetector(detector)
                d.SetFilterOrder(order)
                got = P.deesser_derived(cfg_of("deesser", fs, freq_hz=freq, q=q, threshold_db=thr, knee_db=knee,
                                               range_db=rng, attack_ms=att, release_ms=rel, detector=detector,
                                               filter_order=order))
                assert np.array_equal(bits(got["section"]), bits(d.section())), (fs, detector, freq, q)
                want = (d.bandNorm, d.thresholdLog2, d.kneeWidthLog2, d.rangeLin, d.attackCoeff, d.releaseCoeff)
                have = tuple(got[k] for k in ("band_norm", "threshold_log2", "knee_width_log2", "range_lin",
                                              "attack_coeff", "release_coeff"))
                assert np.array_equal(bits(have), bits(want)), (fs, detector, order, freq)
    for att, rel in ((10.0, 120.0), (0.1, 1.0), (200.0, 2000.0), (0.1, 2000.0), (200.0, 1.0)):
        ts = R.TransientShaper(fs)
        ts.SetAttack(att)
        ts.SetRelease(rel)
        got = P.transient_derived(cfg_of("transient", fs, attack_ms=att, release_ms=rel))
        assert np.array_equal(bits(got), bits((ts.attackCoeff, ts.releaseCoeff)))
    # a caller's own coefficient is the one in use
    assert P.transient_derived(cfg_of("transient", fs, attack_coeff=0.25)) [0] == 0.25
    assert P.deesser_derived(cfg_of("deesser", 96000.0, release_coeff=0.75))["release_coeff"] == 0.75
    assert _lib.lib().ad_deesser_derived(None, *([None] * 7)) == _lib.AD_ERR_INVALID_ARGUMENT
    assert _lib.lib().ad_transient_derived(None, None, None) == _lib.AD_ERR_INVALID_ARGUMENT
    assert _lib.lib().ad_deesser_derived(C.byref(cfg_of("deesser", q=11.0)), *([None] * 7)) == _lib.AD_ERR_INVALID_ARGUMENT


@pytest.mark.parametrize("kind", ["transient", "deesser"])
def test_create_validates_before_the_device(kind):
    L = _lib.lib()
    h = C.c_void_p()
    create, destroy = getattr(L, f"ad_{kind}_create"), getattr(L, f"ad_{kind}_destroy")
    assert create(C.byref(cfg_of(kind, attack_ms=1e9)), 2, 0, C.byref(h)) == _lib.AD_ERR_INVALID_ARGUMENT and not h.value
    assert create(C.byref(cfg_of(kind)), 0, 0, C.byref(h)) == _lib.AD_ERR_INVALID_ARGUMENT
    assert create(None, 1, 0, C.byref(h)) == _lib.AD_ERR_INVALID_ARGUMENT
    rc = create(C.byref(cfg_of(kind)), 2, 0, C.byref(h))
    if _lib.device_count() == 0:
        assert rc == _lib.AD_ERR_NO_DEVICE and not h.value  # no CPU path
    else:
        assert rc == _lib.AD_OK
        destroy(h)
    assert getattr(L, f"ad_{kind}_process")(None, None, 0) == _lib.AD_ERR_INVALID_ARGUMENT
    assert getattr(L, f"ad_{kind}_reset")(None) == _lib.AD_ERR_INVALID_ARGUMENT
    assert getattr(L, f"ad_{kind}_process_device")(None, None, 0, 0, None) == _lib.AD_ERR_INVALID_ARGUMENT
    assert getattr(L, f"ad_{kind}_set_param")(None, 0, 1.0) == _lib.AD_ERR_INVALID_ARGUMENT
    assert getattr(L, f"ad_{kind}_get_config")(None, None) == _lib.AD_ERR_INVALID_ARGUMENT
    assert L.ad_deesser_gain(None, None, None, 0) == _lib.AD_ERR_INVALID_ARGUMENT
    assert L.ad_deesser_metrics(None, 0, None, None) == _lib.AD_ERR_INVALID_ARGUMENT
    assert L.ad_deesser_reset_metrics(None) == _lib.AD_ERR_INVALID_ARGUMENT


# ---- the graph compiler -----------------------------------------------------
def params(num=None, st=None, t="dyn-deesser"):
    return E.Params("n", t, False, num or {}, st or {})


def test_deesser_params_defaults_clamps_rounding_and_strings():
    """deesserRuntime.Configure runtime_dynamics.go:244-310, normalize.go:207-227."""
    c = E.deesser_params(params(), FS)
    assert E._config_dict(c) == E._config_dict(cfg_of("deesser"))
    lo = E.deesser_params(params(dict(freqHz=10, q=0, thresholdDB=-200, ratio=0, kneeDB=-1, attackMs=0, releaseMs=0,
                                      rangeDB=-100, filterOrder=-3, listen=0.49)), FS)
    assert (lo.freq_hz, lo.q, lo.threshold_db, lo.ratio, lo.knee_db, lo.attack_ms, lo.release_ms, lo.range_db,
            lo.filter_order, lo.listen) == (1000.0, 0.1, -80.0, 1.0, 0.0, 0.01, 1.0, -60.0, 1, 0)
    hi = E.deesser_params(params(dict(freqHz=1e6, q=99, thresholdDB=5, ratio=1e3, kneeDB=40, attackMs=1e3, releaseMs=1e4,
                                      rangeDB=3, filterOrder=9, listen=0.5)), FS)
    assert (hi.freq_hz, hi.q, hi.threshold_db, hi.ratio, hi.knee_db, hi.attack_ms, hi.release_ms, hi.range_db,
            hi.filter_order, hi.listen) == (FS * 0.49, 10.0, 0.0, 100.0, 12.0, 50.0, 500.0, 0.0, 4, 1)
    # Configure clamps freqHz to 0.49 fs, and SetFrequency then refuses what is above 20 kHz (:229): so does validate
    assert validate("deesser", lo) == _lib.AD_OK and validate("deesser", hi) == _lib.AD_ERR_INVALID_ARGUMENT
    hi.freq_hz = 20000.0
    assert validate("deesser", hi) == _lib.AD_OK
    assert E.deesser_params(params(dict(freqHz=1e6)), 40000.0).freq_hz == 40000.0 * 0.49
    for raw, want in ((2.5, 3), (3.5, 4), (1.49, 1), (2.4999, 2), (NAN, 2), (INF, 2)):  # math.Round; GetNum drops non-finite
        assert E.deesser_params(params(dict(filterOrder=raw)), FS).filter_order == want, raw
    for mode, want in (("wideband", 1), ("splitband", 0), ("Wideband", 0), ("", 0), ("other", 0)):
        assert E.deesser_params(params(st=dict(mode=mode)), FS).mode == want
    for det, want in (("highpass", 1), ("bandpass", 0), ("HP", 0), ("", 0)):
        assert E.deesser_params(params(st=dict(detector=det)), FS).detector == want


def test_transient_params_defaults_and_clamps():
    """transientShaperRuntime.Configure runtime_dynamics.go:320-347."""
    c = E.transient_params(params(t="dyn-transient"), FS)
    assert E._config_dict(c) == E._config_dict(cfg_of("transient"))
    lo = E.transient_params(params(dict(attack=-2, sustain=-2, attackMs=0, releaseMs=0)), FS)
    hi = E.transient_params(params(dict(attack=2, sustain=2, attackMs=1e4, releaseMs=1e5)), FS)
    assert (lo.attack_amount, lo.sustain_amount, lo.attack_ms, lo.release_ms) == (-1.0, -1.0, 0.1, 1.0)
    assert (hi.attack_amount, hi.sustain_amount, hi.attack_ms, hi.release_ms) == (1.0, 1.0, 200.0, 2000.0)
    nan = E.transient_params(params(dict(attack=NAN, attackMs=INF)), FS)
    assert (nan.attack_amount, nan.attack_ms) == (0.0, 10.0)
    assert validate("transient", lo) == validate("transient", hi) == _lib.AD_OK


def _graph(node_type, p=None):
    return E._graph_json([{"id": "n", "type": node_type, "params": p or {}}], [(E.INPUT_NODE_ID, "n"), ("n", E.OUTPUT_NODE_ID)])


@pytest.mark.parametrize("node_type", ["dyn-deesser", "dyn-transient"])
def test_graph_compiler_knows_the_two_nodes(node_type):
    """They compile; without a device they fail at the device, not as an unknown effect."""
    ch = E.Chain(FS, 2)
    if _lib.device_count() == 0:
        with pytest.raises(_lib.ADError) as e:
            ch.LoadGraph(_graph(node_type))
        assert e.value.code == _lib.AD_ERR_NO_DEVICE
    else:
        ch.LoadGraph(_graph(node_type, {"attackMs": 2.0}))
        kind = "deesser" if node_type == "dyn-deesser" else "transient"
        assert ch.spec[1]["type"] == kind and ch.spec[1][kind]["attack_ms"] == 2.0
    with pytest.raises(E.UnknownEffect):
        E.Chain(FS, 2).LoadGraph(_graph("dyn-multiband"))


def test_sample_rate_at_12k_is_refused_before_freq_is_read():
    """NewDeEsser(fs) carries 6000 Hz when Configure's SetSampleRate runs (deesser.go:399)."""
    for fs in (12000.0, 8000.0):
        with pytest.raises(_lib.ErrInvalidArgument):
            E.Chain(fs, 2).LoadGraph(_graph("dyn-deesser", {"freqHz": 1000}))
    assert validate("deesser", E.deesser_params(params(dict(freqHz=1000)), 12000.0)) == _lib.AD_OK  # the node's own is fine


def _three(node_type):
    par, par2 = (C.c_int32 * 1)(0), (C.c_int32 * 1)(1)
    nodes = (E._Node * 3)()
    nodes[0].type = E.FXN_INPUT
    nodes[1].type, nodes[1].n_parents, nodes[1].parents = node_type, 1, C.cast(par, C.POINTER(C.c_int32))
    nodes[2].type, nodes[2].n_parents, nodes[2].parents = E.FXN_OUTPUT, 1, C.cast(par2, C.POINTER(C.c_int32))
    return nodes, (par, par2)


def test_the_two_node_types_without_a_valid_config_are_refused():
    """Types 18 and 19 without their configuration, with another byte count or with a configuration validate
    refuses, through all three entry points (the device is picked first, so without one the error is
    AD_ERR_NO_DEVICE, as for the types before them)."""
    L = _lib.lib()
    want = _lib.AD_ERR_NO_DEVICE if _lib.device_count() == 0 else _lib.AD_ERR_INVALID_ARGUMENT
    for t, kind in ((E.FXN_DEESSER, "deesser"), (E.FXN_TRANSIENT, "transient")):
        nodes, _keep = _three(t)
        cfgs = (_lib.FxNodeCfg * 3)()
        h = C.c_void_p()
        np_ = C.cast(nodes, C.c_void_p)
        assert L.ad_fx_graph_create(np_, 3, 2, 0, C.byref(h)) == want and not h.value
        assert L.ad_fx_graph_create_ext(np_, None, 3, 2, 0, C.byref(h)) == want and not h.value
        assert L.ad_fx_graph_create_cfg(np_, None, None, 3, 2, 0, C.byref(h)) == want
        assert L.ad_fx_graph_create_cfg(np_, None, C.cast(cfgs, C.c_void_p), 3, 2, 0, C.byref(h)) == want
        good = cfg_of(kind)
        for nbytes in (C.sizeof(good) - 4, C.sizeof(good) + 8, 0):
            cfgs[1].config, cfgs[1].bytes = C.addressof(good), nbytes
            assert L.ad_fx_graph_create_cfg(np_, None, C.cast(cfgs, C.c_void_p), 3, 2, 0, C.byref(h)) == want
        bad = cfg_of(kind, release_ms=0.0)
        cfgs[1].config, cfgs[1].bytes = C.addressof(bad), C.sizeof(bad)
        assert L.ad_fx_graph_create_cfg(np_, None, C.cast(cfgs, C.c_void_p), 3, 2, 0, C.byref(h)) == want
        assert not h.value
    if _lib.device_count():  # 14 and 17 stay unknown next to them
        for t in (14, 17, 20):
            nodes, _keep = _three(t)
            h = C.c_void_p()
            assert L.ad_fx_graph_create(C.cast(nodes, C.c_void_p), 3, 2, 0, C.byref(h)) == 10 and not h.value  # UNKNOWN_EFFECT
