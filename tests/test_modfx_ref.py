"""Phaser, tremolo and ring modulator checks that need no GPU: the reference
restatement (tests/modfx_ref.py) against phaser_test.go, tremolo_test.go and
ring_modulator_test.go, the host-only part of the C ABI (defaults, validation,
create without a device), the graph compiler's parameter clamps and its two
phaser failures, and how far a last-place change of every sine (and, for the
phaser, every tangent) moves the output of the cases the GPU tests compare."""
import ctypes as C
import math

import numpy as np
import pytest

import modfx_ref as R
from algodsp import _lib, effectchain as E, signals

NAN, INF = float("nan"), float("inf")
RMS_BAR, ABS_BAR = 1e-12, 1e-10  # the GPU tests' bars (tests/test_modfx_gpu.py)


def noise(n, seed=0x30DF):
    return signals.white_noise(n, seed) * R.AMPLITUDE


def rel_rms(a, b):
    return float(np.sqrt(np.mean((a - b) ** 2)) / np.sqrt(np.mean(b ** 2)))


def impulse(n):
    x = np.zeros(n)
    x[0] = 1
    return x


# ---- the reference's unit tests, on the restatement -------------------------
@pytest.mark.parametrize("make", [lambda: R.Phaser(48000.0), lambda: R.Tremolo(48000.0),
                                  lambda: R.RingModulator(48000.0, carrier_hz=300.0)])
def test_process_in_place_matches_process_and_reset_restores_state(make):
    """Test*ProcessInPlaceMatchesProcess and Test*ResetRestoresState (phaser_test.go:8-72,
    tremolo_test.go:8-72, ring_modulator_test.go:8-70)."""
    x = np.sin(2 * math.pi * np.arange(128) / 29)
    a, b = make(), make()
    want = np.array([a.Process(float(v)) for v in x])
    assert np.max(np.abs(b.process(x) - want)) <= 1e-12
    p = make()
    x = impulse(128) if isinstance(p, R.Phaser) else np.full(128, 0.5)
    out1 = p.process(x)
    assert (p.phase if isinstance(p, R.RingModulator) else p.lfoPhase) > 0
    p.Reset()
    assert np.max(np.abs(p.process(x) - out1)) <= 1e-12


def test_tremolo_depth_zero_and_ringmod_mix_zero_are_transparent():
    """TestTremoloDepthZeroIsTransparent (tremolo_test.go:74-91), TestRingModulatorMixZeroIsTransparent (:72-89)."""
    x = noise(300)
    np.testing.assert_array_equal(R.Tremolo(48000.0, depth=0.0, mix=1.0).process(x), x)
    np.testing.assert_array_equal(R.RingModulator(48000.0, carrier_hz=1000.0, mix=0.0).process(x), x)


def test_ringmod_dc_input_gives_the_sine_and_silence_stays_silent():
    """TestRingModulatorDCInputProducesSine (:91-117), ...SilenceInputProducesSilence (:119-134)."""
    r = R.RingModulator(48000.0, carrier_hz=100.0, mix=1.0)
    got = r.process(np.ones(480))
    want = np.sin(2 * math.pi * 100.0 * np.arange(480) / 48000.0)
    assert np.max(np.abs(got - want)) <= 1e-9
    assert not np.any(R.RingModulator(48000.0, carrier_hz=1000.0).process(np.zeros(100)))


@pytest.mark.parametrize("feedback", [0.85, 0.99, -0.99])
def test_phaser_stays_finite_under_feedback(feedback):
    """TestPhaserFiniteOutputUnderFeedback (phaser_test.go:96-114: 0.85, mix 0.8, 8 stages), and the
    setters' extremes with 12 stages."""
    p = R.Phaser(48000.0, feedback=feedback, mix=0.8, stages=8 if feedback == 0.85 else 12)
    y = p.process(0.3 * np.sin(2 * math.pi * 440 * np.arange(12000) / 48000))
    assert np.all(np.isfinite(y))


def test_set_stages_zeroes_the_stages_only():
    p = R.Phaser(48000.0)
    p.process(noise(50))
    state = ([list(s) for s in p.stages], p.feedbackSample, p.lfoPhase)
    p.SetStages(6)
    assert ([list(s) for s in p.stages], p.feedbackSample, p.lfoPhase) == state
    p.SetStages(4)
    assert p.stages == [[0.0, 0.0]] * 4 and (p.feedbackSample, p.lfoPhase) == state[1:] and state[1] != 0


def test_tremolo_coefficient():
    t = R.Tremolo(48000.0)
    assert t.smoothingCoef == 1 - math.exp(-1 / (0.005 * 48000.0)) and t.currentMod == 1.0
    t.SetSmoothingMs(0.0)
    assert t.smoothingCoef == 1.0
    t.SetSmoothingMs(5.0), t.SetSampleRate(8000.0)
    assert t.smoothingCoef == 1 - math.exp(-1 / (0.005 * 8000.0))
    assert R.smoothing_coefficient(1e-9, 48000.0) == 1.0 and R.smoothing_coefficient(1e300, 48000.0) == 0.0


# ---- the host-only C ABI ----------------------------------------------------
CONFIGS = {"phaser": _lib.PhaserConfig, "tremolo": _lib.TremoloConfig, "ringmod": _lib.RingModConfig}


def cfg_of(kind, fs=48000.0, **kv):
    cfg = CONFIGS[kind]()
    getattr(_lib.lib(), f"ad_{kind}_default_config")(C.byref(cfg), fs)
    for k, v in kv.items():
        setattr(cfg, k, v)
    return cfg


def validate(kind, cfg):
    return getattr(_lib.lib(), f"ad_{kind}_validate")(C.byref(cfg))


def _fields(c):
    return [getattr(c, f) for f, _ in c._fields_]


def as_fields(field, value):
    return dict(min_freq_hz=value[0], max_freq_hz=value[1]) if field == "range" else {field: value}


@pytest.mark.parametrize("kind,field,value", R.REJECTED)
def test_rejected_values_fail_the_restatement_and_validation(kind, field, value):
    with pytest.raises(ValueError):
        R.set_on(R.KINDS[kind](48000.0), field, value)
    assert validate(kind, cfg_of(kind, **as_fields(field, value))) == _lib.AD_ERR_INVALID_ARGUMENT
    # with a device, tests/test_modfx_gpu.py::test_rejected_setter_changes_nothing runs the same list through ad_*_set_param
    assert getattr(_lib.lib(), f"ad_{kind}_set_param")(None, 0, 1.0) == _lib.AD_ERR_INVALID_ARGUMENT


@pytest.mark.parametrize("kind,field,value", R.ACCEPTED)
def test_validation_accepts_range_edges(kind, field, value):
    R.set_on(R.KINDS[kind](48000.0), field, value)
    assert validate(kind, cfg_of(kind, **as_fields(field, value))) == _lib.AD_OK


def test_default_configs_are_the_constructors():
    assert _fields(cfg_of("phaser", 12345.0)) == [12345.0, 0.4, 300.0, 1600.0, 0.2, 0.5, 6]
    p = R.Phaser(12345.0)
    assert (p.rateHz, p.minFreqHz, p.maxFreqHz, p.feedback, p.mix, len(p.stages)) == (0.4, 300.0, 1600.0, 0.2, 0.5, 6)
    assert _fields(cfg_of("tremolo", 12345.0)) == [12345.0, 4.0, 0.6, 5.0, 1.0, 0.0]
    t = R.Tremolo(12345.0)
    assert (t.rateHz, t.depth, t.smoothing, t.mix) == (4.0, 0.6, 5.0, 1.0)
    assert _fields(cfg_of("ringmod", 12345.0)) == [12345.0, 440.0, 1.0]
    r = R.RingModulator(12345.0)
    assert (r.carrierHz, r.mix, r.phaseInc) == (440.0, 1.0, 2 * math.pi * 440.0 / 12345.0)


def test_tremolo_coefficient_field():
    for k in (0.0, 0.25, 1.0):
        assert validate("tremolo", cfg_of("tremolo", smoothing_coeff=k)) == _lib.AD_OK
    for k in (-0.1, 1.5, NAN):
        assert validate("tremolo", cfg_of("tremolo", smoothing_coeff=k)) == _lib.AD_ERR_INVALID_ARGUMENT


def test_create_validates_before_the_device():
    L = _lib.lib()
    h = C.c_void_p()
    for kind, bad in (("phaser", dict(max_freq_hz=30000.0)), ("tremolo", dict(depth=1.2)), ("ringmod", dict(mix=1.1))):
        create, destroy = getattr(L, f"ad_{kind}_create"), getattr(L, f"ad_{kind}_destroy")
        assert create(C.byref(cfg_of(kind, **bad)), 2, 0, C.byref(h)) == _lib.AD_ERR_INVALID_ARGUMENT and not h.value
        assert create(C.byref(cfg_of(kind)), 0, 0, C.byref(h)) == _lib.AD_ERR_INVALID_ARGUMENT
        assert create(None, 1, 0, C.byref(h)) == _lib.AD_ERR_INVALID_ARGUMENT
        assert validate(kind, cfg_of(kind)) == _lib.AD_OK and getattr(L, f"ad_{kind}_validate")(None) == _lib.AD_ERR_INVALID_ARGUMENT
        rc = create(C.byref(cfg_of(kind)), 2, 0, C.byref(h))
        if _lib.device_count() == 0:
            assert rc == _lib.AD_ERR_NO_DEVICE and not h.value  # no CPU path
        else:
            assert rc == _lib.AD_OK
            destroy(h)
        assert getattr(L, f"ad_{kind}_process_device")(None, None, 0, 0, None) == _lib.AD_ERR_INVALID_ARGUMENT
        assert getattr(L, f"ad_{kind}_peek_lfo")(None, 0, None, None) == _lib.AD_ERR_INVALID_ARGUMENT
        assert getattr(L, f"ad_{kind}_reset")(None) == _lib.AD_ERR_INVALID_ARGUMENT
    assert L.ad_phaser_set_range(None, 300.0, 1600.0) == _lib.AD_ERR_INVALID_ARGUMENT


# ---- the graph compiler -----------------------------------------------------
def test_phaser_params_defaults_and_clamps():
    fs = 44100.0
    assert _fields(E.phaser_params(E.Params("p", "phaser"), 48000.0)) == [48000.0, 0.4, 300, 1600, 0.2, 0.5, 6]
    hi = E.phaser_params(E.Params("p", "phaser", num=dict(minFreqHz=1e9, maxFreqHz=1e9, stages=99, rateHz=99, feedback=9,
                                                            mix=9)), fs)
    assert _fields(hi) == [fs, 5, fs * 0.45, fs * 0.49, 0.99, 1, 12]
    assert validate("phaser", hi) == _lib.AD_ERR_INVALID_ARGUMENT  # the clamp's own upper end fails validateParams
    lo = E.phaser_params(E.Params("p", "phaser", num=dict(minFreqHz=0, maxFreqHz=0, stages=-3, rateHz=0, feedback=-9,
                                                            mix=-1)), fs)
    assert _fields(lo) == [fs, 0.05, 20, 21, -0.99, 0, 1]
    assert validate("phaser", lo) == _lib.AD_OK
    nan = E.phaser_params(E.Params("p", "phaser", num=dict(minFreqHz=NAN, maxFreqHz=INF, stages=NAN, rateHz=INF,
                                                             feedback=NAN, mix=INF)), fs)
    assert _fields(nan) == [fs, 0.4, 300, 1600, 0.2, 0.5, 6]
    for v, want in ((6.5, 7), (2.5, 3), (2.4999, 2), (0.5, 1), (12.4, 12)):  # math.Round: halves away from zero
        assert E.phaser_params(E.Params("p", "phaser", num=dict(stages=v)), fs).stages == want


def test_tremolo_params_defaults_and_clamps():
    fs = 44100.0
    assert _fields(E.tremolo_params(E.Params("t", "tremolo"), 48000.0)) == [48000.0, 4, 0.6, 5, 1, 0.0]
    hi = E.tremolo_params(E.Params("t", "tremolo", num=dict(rateHz=99, depth=9, smoothingMs=999, mix=9)), fs)
    assert _fields(hi) == [fs, 20, 1, 200, 1, 0.0]
    lo = E.tremolo_params(E.Params("t", "tremolo", num=dict(rateHz=0, depth=-1, smoothingMs=-1, mix=-1)), fs)
    assert _fields(lo) == [fs, 0.05, 0, 0, 0, 0.0]
    nan = E.tremolo_params(E.Params("t", "tremolo", num=dict(rateHz=NAN, depth=INF, smoothingMs=NAN, mix=INF)), fs)
    assert _fields(nan) == [fs, 4, 0.6, 5, 1, 0.0]
    for c in (hi, lo):
        assert validate("tremolo", c) == _lib.AD_OK


def test_ringmod_params_defaults_and_clamps():
    fs = 44100.0
    assert _fields(E.ringmod_params(E.Params("r", "ringmod"), 48000.0)) == [48000.0, 440, 1]
    hi = E.ringmod_params(E.Params("r", "ringmod", num=dict(carrierHz=1e9, mix=9)), fs)
    assert _fields(hi) == [fs, fs * 0.49, 1]
    lo = E.ringmod_params(E.Params("r", "ringmod", num=dict(carrierHz=0, mix=-1)), fs)
    assert _fields(lo) == [fs, 1, 0]
    nan = E.ringmod_params(E.Params("r", "ringmod", num=dict(carrierHz=NAN, mix=INF)), fs)
    assert _fields(nan) == [fs, 440, 1]
    for c in (hi, lo):
        assert validate("ringmod", c) == _lib.AD_OK


def _graph(node):
    return E._graph_json([node], [(E.INPUT_NODE_ID, node["id"]), (node["id"], E.OUTPUT_NODE_ID)])


@pytest.mark.parametrize("fs,params", [(48000.0, {"maxFreqHz": 0.49 * 48000.0}), (48000.0, {"maxFreqHz": 1e9}),
                                       (3000.0, {"minFreqHz": 100, "maxFreqHz": 1000})])
def test_phaser_node_that_fails_to_configure(fs, params):
    """A maxFreqHz that clamps to 0.49 fs fails SetFrequencyRangeHz's validateParams; at fs = 3000 the factory's
    NewPhaser(fs) fails on its own default range (1600 >= 1470) although the node's range would fit."""
    if fs == 3000.0:
        cfg = E.phaser_params(E.Params("p", "phaser", num=params), fs)
        assert validate("phaser", cfg) == _lib.AD_OK
        with pytest.raises(ValueError):
            R.Phaser(fs)
    else:
        with pytest.raises(ValueError):
            R.Phaser(fs).SetFrequencyRangeHz(300.0, fs * 0.49)
    with pytest.raises(_lib.ErrInvalidArgument):
        E.Chain(fs, 2).LoadGraph(_graph({"id": "p", "type": "phaser", "params": params}))


@pytest.mark.parametrize("kind", ["phaser", "tremolo", "ringmod"])
def test_graph_compiler_knows_the_modulation_nodes(kind):
    """They compile; without a device they fail at the device, not as an unknown effect."""
    ch = E.Chain(48000.0, 2)
    if _lib.device_count() == 0:
        with pytest.raises(_lib.ADError) as e:
            ch.LoadGraph(_graph({"id": "n", "type": kind}))
        assert e.value.code == _lib.AD_ERR_NO_DEVICE
    else:
        ch.LoadGraph(_graph({"id": "n", "type": kind}))
        assert ch.spec[1]["type"] == kind


def test_fx_node_layout_is_unchanged_and_the_new_types_follow():
    names = [f for f, _ in E._Node._fields_]
    assert names[-3:] == ["fdn", "delay", "flanger"] and names[0] == "type" and len(names) == 22
    assert (E.FXN_PHASER, E.FXN_TREMOLO, E.FXN_RINGMOD) == (11, 12, 13)
    assert [f for f, _ in E._NodeExt._fields_] == ["phaser", "tremolo", "ringmod"]
    assert C.sizeof(E._NodeExt) == 3 * C.sizeof(C.c_void_p)


def test_new_node_types_without_config_are_refused():
    """Types 11 to 13 without a config are refused through both entry points
    (the device is picked first, so without one the error is AD_ERR_NO_DEVICE)."""
    par, par2 = (C.c_int32 * 1)(0), (C.c_int32 * 1)(1)
    want = _lib.AD_ERR_NO_DEVICE if _lib.device_count() == 0 else _lib.AD_ERR_INVALID_ARGUMENT
    for t in (E.FXN_PHASER, E.FXN_TREMOLO, E.FXN_RINGMOD):
        nodes = (E._Node * 3)()
        nodes[0].type = E.FXN_INPUT
        nodes[1].type, nodes[1].n_parents, nodes[1].parents = t, 1, C.cast(par, C.POINTER(C.c_int32))
        nodes[2].type, nodes[2].n_parents, nodes[2].parents = E.FXN_OUTPUT, 1, C.cast(par2, C.POINTER(C.c_int32))
        ext = (E._NodeExt * 3)()
        h = C.c_void_p()
        L = _lib.lib()
        assert L.ad_fx_graph_create(C.cast(nodes, C.c_void_p), 3, 2, 0, C.byref(h)) == want and not h.value
        assert L.ad_fx_graph_create_ext(C.cast(nodes, C.c_void_p), None, 3, 2, 0, C.byref(h)) == want and not h.value
        assert L.ad_fx_graph_create_ext(C.cast(nodes, C.c_void_p), C.cast(ext, C.c_void_p), 3, 2, 0, C.byref(h)) == want


# ---- the sine (and tangent) spread ------------------------------------------
@pytest.mark.parametrize("kind,fs,options,n", R.CASES)
def test_sine_spread(kind, fs, options, n):
    """Every sine, and for the phaser every tangent, moved by a random -1 / 0 /
    +1 ulp moves the output by at most a quarter of the GPU tests' bars: 2.5e-13
    relative RMS and 2.5e-11 absolute.  Measured: the phaser at fs 8000, rate 5,
    20 .. 3900 Hz, 12 stages, feedback +-0.99, mix 1 moves by 1.1e-14 relative
    RMS and 5.3e-14 absolute at an output peak of 3.9; the defaults by 4.7e-16
    and 2.5e-16; the tremolo and the ring modulator by at most 1.3e-16.  The
    200 ms smoothing (a coefficient of 6e-4) rounds a last-place change of its
    target away altogether."""
    x = noise(n)
    plain = R.KINDS[kind](fs, **options)
    extra = dict(tan=R.nudged(math.tan, 0x7A9)) if kind == "phaser" else {}
    moved = R.KINDS[kind](fs, sin=R.nudged(math.sin, 0xF1A, -1.0, 1.0), **extra, **options)
    a, b = plain.process(x), moved.process(x)
    spread, mx = rel_rms(b, a), float(np.max(np.abs(a - b)))
    print(f"{kind} {fs} {options}: spread rel rms {spread:.3g}, max abs {mx:.3g}, output peak {np.max(np.abs(a)):.3g}")
    assert np.any(a != b) or options.get("smoothing_ms") == 200.0
    assert spread <= RMS_BAR / 4 and mx <= ABS_BAR / 4
