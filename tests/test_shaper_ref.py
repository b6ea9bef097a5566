"""The restated distortion and bit crusher (tests/shaper_ref.py) against the
reference's own known answers, the host formulas the GPU runtime uses in place
of the reference's per-sample counting, the graph compiler's node parameters,
and the C ABI's validation: everything that needs no device."""
import ctypes as C
import math

import numpy as np
import pytest

import shaper_ref as R
from algodsp import _lib, effectchain as E

NAN, INF = float("nan"), float("inf")


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


# ---- the reference's known answers ------------------------------------------
def test_hard_clip_curve_at_half():
    """TestDistortionHardClipTransferCurve distortion_test.go:62-92."""
    d = R.Distortion(48000.0, mode=R.MODES.index("hardclip"), drive=1, clip_level=0.5, mix=1)
    for x, want in ((-2, -1), (-0.5, -1), (-0.25, -0.5), (0, 0), (0.25, 0.5), (0.5, 1), (2, 1)):
        assert abs(float(d.ProcessSample(x)) - want) <= 1e-12
    xs = np.array([-2, -0.5, -0.25, 0, 0.25, 0.5, 2.0])
    assert np.array_equal(d.process_many(xs[None, :])[0], [-1, -1, -0.5, 0, 0.5, 1, 1])


def test_one_bit_quantisation_table():
    """TestBitCrusherQuantization bit_crusher_test.go:117-151: Round(0.5) is 1, halves go away from zero."""
    bc = R.BitCrusher(48000.0, bit_depth=1, downsample=1, mix=1)
    assert bc.quantLevels == 1.0
    for x, want in ((0.0, 0.0), (0.3, 0.0), (0.5, 1.0), (0.6, 1.0), (1.0, 1.0), (-0.3, 0.0), (-0.6, -1.0), (-1.0, -1.0),
                    (-0.5, -1.0), (1.5, 2.0), (2.5, 3.0)):
        bc.Reset()
        assert float(bc.ProcessSample(x)) == want, x
    assert bits(R.go_round(-0.3)) == bits(-0.0)  # math.Round keeps the sign of zero
    assert float(R.go_round(0.49999999999999994)) == 0.0  # floor(x + 0.5) would give 1
    assert float(R.go_round(2.0 ** 52 + 1)) == 2.0 ** 52 + 1


def test_downsample_hold_trace():
    """TestBitCrusherDownsampleHold :153-202: three leading zeros, then the quantised fourth sample held."""
    bc = R.BitCrusher(48000.0, bit_depth=32, downsample=4, mix=1)
    x = np.array([0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8])
    out = [float(bc.ProcessSample(v)) for v in x]
    q4, q8 = float(bc.quantize(0.4)), float(bc.quantize(0.8))
    assert out == [0, 0, 0, q4, q4, q4, q4, q8] and q4 != q8
    assert abs(q4 - 0.4) <= 2.0 ** -32 and bc.holdCounter == 0
    bc.Reset()
    assert np.array_equal(bc.process_many(np.stack([x, -x])), np.stack([out, [-v for v in out]]))


def test_zero_weights_are_the_plain_tn_path():
    """TestChebyshevWeightsDefaultIsLegacyTN :280-301, TestChebyshevWeightsZeroAfterSet :407-450; weights past
    the order do not count (:690-695)."""
    d = R.Distortion(48000.0, mode=R.CHEBYSHEV, cheb_order=3)
    assert abs(float(d.ProcessSample(0.5)) - -1.0) <= 1e-10 and not d.has_weights()
    d.SetChebyshevWeights([1, 0, 0])
    assert d.has_weights() and abs(float(d.ProcessSample(0.5)) - 0.5) <= 1e-10
    d.SetChebyshevWeights([0, 0, 0])
    assert abs(float(d.ProcessSample(0.5)) - -1.0) <= 1e-10
    d.SetChebyshevWeights([0, 0, 0, 0.7])
    assert not d.has_weights()
    x = np.linspace(-1.2, 1.2, 101)
    plain = R.Distortion(48000.0, mode=R.CHEBYSHEV, cheb_order=3)
    assert np.array_equal(bits(d.ProcessSample(x)), bits(plain.ProcessSample(x)))


def test_additive_weight_blend():
    """TestChebyshevWeightsAdditiveBlend :303-344."""
    x = 0.3
    for w, want in (([1, 0, 0], x), ([0, 1, 0], 2 * x * x - 1), ([0, 0, 1], 4 * x * x * x - 3 * x)):
        d = R.Distortion(48000.0, mode=R.CHEBYSHEV, cheb_order=3, cheb_weights=w)
        assert abs(float(d.ProcessSample(x)) - max(-1.0, min(1.0, want))) <= 1e-10
    d = R.Distortion(48000.0, mode=R.CHEBYSHEV, cheb_order=3, cheb_weights=[0.5, 0.25, 0.125], cheb_gain=2.0)
    want = (0.5 * x + 0.25 * (2 * x * x - 1) + 0.125 * (4 * x ** 3 - 3 * x)) * 2.0
    assert abs(float(d.ProcessSample(x)) - want) <= 1e-12


def test_dc_bypass_reduces_the_mean():
    """TestDistortionChebyshevDCBypassReducesDC :200-239."""
    x = np.cos(2 * math.pi * np.arange(4000) / 128)[None, :]
    plain = R.Distortion(48000.0, mode=R.CHEBYSHEV, cheb_order=2, cheb_harmonic=R.EVEN)
    dc = R.Distortion(48000.0, mode=R.CHEBYSHEV, cheb_order=2, cheb_harmonic=R.EVEN, cheb_dc_bypass=True)
    a, b = plain.process_many(x).mean(), dc.process_many(x).mean()
    assert abs(b) < abs(a) * 0.2
    dc.Reset()
    assert float(dc.dcPrevIn) == 0.0 and float(dc.dcPrevOut) == 0.0


def test_vector_and_scalar_walks_agree():
    """process_many (a column of channels per step) is the per-sample walk of each row."""
    rng = np.random.default_rng(7)
    x = rng.standard_normal((3, 200))
    for kw in (dict(mode=R.CHEBYSHEV, cheb_order=5, cheb_dc_bypass=True, cheb_weights=[0.3, 0, -0.2], mix=0.7),
               dict(mode=R.MODES.index("waveshaper3"), drive=2.0, bias=0.1)):
        many = R.Distortion(48000.0, **kw).process_many(x)
        for c in range(3):
            one = R.Distortion(48000.0, **kw)
            assert np.array_equal(bits([float(one.ProcessSample(v)) for v in x[c]]), bits(many[c]))
    many = R.BitCrusher(48000.0, bit_depth=5, downsample=3, mix=0.5).process_many(x)
    for c in range(3):
        one = R.BitCrusher(48000.0, bit_depth=5, downsample=3, mix=0.5)
        assert np.array_equal(bits([float(one.ProcessSample(v)) for v in x[c]]), bits(many[c]))


def test_a_nan_passes_the_clamps_and_is_zeroed():
    for m in range(len(R.MODES)):
        for approx in (R.EXACT, R.POLYNOMIAL):
            d = R.Distortion(48000.0, mode=m, approx=approx, mix=0.5)
            x = np.array([NAN, INF, -INF, 0.25])
            wet = d.curve(x)  # the finite check: 0 for a NaN (softClip gives copysign(1, NaN) instead), never a NaN
            assert np.all(np.isfinite(wet)) and np.all(np.abs(wet) <= 1.0)
            assert wet[0] == 0.0 or R.MODES[m] in ("softclip", "saturate2")
            out = d.ProcessSample(x)  # the dry part keeps the NaN and the infinities
            assert math.isnan(out[0]) and out[1] == INF and out[2] == -INF and abs(out[3]) <= 1.0


# ---- the counter formula ----------------------------------------------------
@pytest.mark.parametrize("downsample", [1, 2, 3, 4, 255, 256])
def test_counter_formula_against_the_literal_loop(downsample):
    """first_update and counter_after against holdCounter++ / >= downsample, for every counter a call can start
    with: 0 .. 259 includes values at and above the factor, as after SetDownsample lowers it."""
    for c0 in range(260):
        for n in (0, 1, 2, 255, 256, 257, 700):
            c, updates = c0, []
            for t in range(n):
                c += 1
                if c >= downsample:
                    c = 0
                    updates.append(t)
            t0 = R.first_update(downsample, c0)
            assert R.counter_after(downsample, c0, n) == c, (downsample, c0, n)
            assert updates == list(range(t0, n, downsample)), (downsample, c0, n)


# ---- node parameters --------------------------------------------------------
def _cfg(c):
    return E._config_dict(c)


def P(type_, num=None, str_=None):
    return E.Params("n", type_, num=num or {}, str_=str_ or {})


def test_distortion_params_defaults_and_clamps():
    fs = 44100.0
    d = _cfg(E.distortion_params(P("distortion"), fs))
    assert d == dict(sample_rate=fs, drive=1.8, mix=1.0, output_level=1.0, clip_level=1.0, shape=0.5, bias=0.0,
                     cheb_gain=1.0, cheb_weights=[0.0] * 16, mode=0, approx=0, cheb_order=3, cheb_harmonic=0,
                     cheb_invert=0, cheb_dc_bypass=0)
    assert d == R.config_of(R.distortion_node({}, {}, fs))
    hi = dict(drive=99, mix=9, output=9, clip=9, shape=9, bias=9, order=9, gain=9, invert=1, dcBypass=1, w1=0.5)
    lo = dict(drive=0, mix=-1, output=-1, clip=0, shape=-1, bias=-9)
    nan = dict(drive=NAN, mix=INF, output=NAN, clip=-INF, shape=NAN, bias=INF)
    for num, want in ((hi, (20, 1, 4, 1, 1, 1)), (lo, (0.01, 0, 0, 0.05, 0, -1)), (nan, (1.8, 1, 1, 1, 0.5, 0))):
        c = E.distortion_params(P("distortion", num, dict(mode="hardclip", approx="polynomial", harmonic="even")), fs)
        assert (c.drive, c.mix, c.output_level, c.clip_level, c.shape, c.bias) == want
        # the node fixes order 3, every harmonic, no inversion, gain 1, no DC bypass, and reads no weights
        assert (c.mode, c.approx, c.cheb_order, c.cheb_harmonic, c.cheb_invert, c.cheb_gain, c.cheb_dc_bypass) == \
            (1, 1, 3, 0, 0, 1.0, 0) and list(c.cheb_weights) == [0.0] * 16
        assert _lib.lib().ad_distortion_validate(C.byref(c)) == _lib.AD_OK
        assert _cfg(c) == R.config_of(R.distortion_node(num, dict(mode="hardclip", approx="polynomial"), fs))
    for i, name in enumerate(R.MODES):
        assert E.distortion_params(P("distortion", str_=dict(mode=name)), fs).mode == i
    for raw in ("", "SoftClip", "fuzz", "tanh "):  # an unknown mode string is softclip, an unknown approximation exact
        c = E.distortion_params(P("distortion", str_=dict(mode=raw, approx=raw)), fs)
        assert (c.mode, c.approx) == (0, 0)


def test_dist_cheb_params_defaults_clamps_and_order_adjustment():
    fs = 48000.0
    d = _cfg(E.dist_cheb_params(P("dist-cheb"), fs))
    assert d == dict(sample_rate=fs, drive=1.0, mix=1.0, output_level=1.0, clip_level=1.0, shape=0.5, bias=0.0,
                     cheb_gain=1.0, cheb_weights=[0.0] * 16, mode=14, approx=0, cheb_order=3, cheb_harmonic=0,
                     cheb_invert=0, cheb_dc_bypass=0)
    num = dict(drive=99, mix=9, output=9, clip=0.2, shape=0.9, bias=0.5, order=99, gain=9, invert=0.5, dcBypass=0.49,
               w1=0.25, w16=-3.0, w17=9.0, w3=NAN)
    c = E.dist_cheb_params(P("dist-cheb", num, dict(mode="tanh", approx="polynomial", harmonic="all")), fs)
    assert (c.drive, c.mix, c.output_level, c.clip_level, c.shape, c.bias, c.cheb_gain) == (20, 1, 4, 1.0, 0.5, 0.0, 4)
    assert (c.mode, c.approx, c.cheb_order, c.cheb_harmonic, c.cheb_invert, c.cheb_dc_bypass) == (14, 1, 16, 0, 1, 0)
    assert list(c.cheb_weights) == [0.25] + [0.0] * 14 + [-3.0]
    assert _cfg(c) == R.config_of(R.dist_cheb_node(num, dict(approx="polynomial", harmonic="all"), fs))
    lo = E.dist_cheb_params(P("dist-cheb", dict(drive=0, order=-4, gain=-1)), fs)
    assert (lo.drive, lo.cheb_order, lo.cheb_gain) == (0.01, 1, 0)
    # configureDistortion configure.go:131-153
    for harmonic, order, want in (("odd", 4, 5), ("even", 3, 4), ("odd", 16, 15), ("even", 1, 2), ("odd", 3, 3),
                                  ("even", 16, 16), ("all", 4, 4), ("sometimes", 7, 7), ("even", 15, 16), ("odd", 1, 1)):
        c = E.dist_cheb_params(P("dist-cheb", dict(order=order), dict(harmonic=harmonic)), fs)
        assert c.cheb_order == want and c.cheb_harmonic == {"odd": 1, "even": 2}.get(harmonic, 0)
        assert R.adjust_order(order, c.cheb_harmonic) == want
        assert _lib.lib().ad_distortion_validate(C.byref(c)) == _lib.AD_OK
    for v, want in ((2.5, 3), (2.4999, 2), (0.4, 1), (15.5, 16)):  # math.Round: halves away from zero
        assert E.dist_cheb_params(P("dist-cheb", dict(order=v)), fs).cheb_order == want


def test_bitcrusher_params_defaults_and_clamps():
    fs = 44100.0
    assert _cfg(E.bitcrusher_params(P("bitcrusher"), fs)) == dict(sample_rate=fs, bit_depth=8, mix=1, downsample=4)
    for num, want in ((dict(bitDepth=99, downsample=999, mix=9), (32, 1, 256)), (dict(bitDepth=0, downsample=-3, mix=-1), (1, 0, 1)),
                      (dict(bitDepth=NAN, downsample=INF, mix=NAN), (8, 1, 4)), (dict(bitDepth=7.5, downsample=2.5, mix=0.5), (7.5, 0.5, 3)),
                      (dict(downsample=0.4), (8, 1, 1))):
        c = E.bitcrusher_params(P("bitcrusher", num), fs)
        assert (c.bit_depth, c.mix, c.downsample) == want
        assert _lib.lib().ad_bitcrusher_validate(C.byref(c)) == _lib.AD_OK
        assert _cfg(c) == R.config_of(R.bitcrusher_node(num, {}, fs))


# ---- validate ---------------------------------------------------------------
def cfg_of(kind, **kv):
    c = (_lib.DistortionConfig if kind == "distortion" else _lib.BitCrusherConfig)()
    getattr(_lib.lib(), f"ad_{kind}_default_config")(C.byref(c), 48000.0)
    for k, v in kv.items():
        setattr(c, k, v)
    return c


def validate(kind, c):
    return getattr(_lib.lib(), f"ad_{kind}_validate")(C.byref(c))


def test_struct_sizes_and_defaults():
    assert C.sizeof(_lib.DistortionConfig) == 24 * 8 + 6 * 4 == 216
    assert C.sizeof(_lib.BitCrusherConfig) == 3 * 8 + 8 == 32
    assert C.sizeof(_lib.FxNodeCfg) == 16 and [f for f, _ in _lib.FxNodeCfg._fields_] == ["config", "bytes"]
    assert [f for f, _ in _lib.DistortionConfig._fields_][:9] == ["sample_rate", "drive", "mix", "output_level", "clip_level",
                                                                  "shape", "bias", "cheb_gain", "cheb_weights"]
    assert E._config_dict(cfg_of("distortion")) == R.config_of(R.Distortion(48000.0))
    assert E._config_dict(cfg_of("bitcrusher")) == R.config_of(R.BitCrusher(48000.0))
    assert (E.FXN_DISTORTION, E.FXN_BITCRUSHER) == (15, 16)


@pytest.mark.parametrize("kind", ["distortion", "bitcrusher"])
def test_validate_accepts_every_range_edge_and_refuses_just_outside(kind):
    assert validate(kind, cfg_of(kind)) == _lib.AD_OK
    ref = R.Distortion if kind == "distortion" else R.BitCrusher
    ok, bad = R.accepted(kind), R.rejected(kind)
    assert len(ok) >= 8 and len(bad) >= 20
    for field, value in ok:
        assert validate(kind, cfg_of(kind, **{field: value})) == _lib.AD_OK, (field, value)
        ref(**{field: value})
    for field, value in bad:
        assert validate(kind, cfg_of(kind, **{field: value})) == _lib.AD_ERR_INVALID_ARGUMENT, (field, value)
        with pytest.raises(R.Invalid):
            ref(**{field: value})
    assert getattr(_lib.lib(), f"ad_{kind}_validate")(None) == _lib.AD_ERR_INVALID_ARGUMENT


def test_validate_chebyshev_parity_weights_and_flags():
    """TestDistortionValidation distortion_test.go:25-41, TestSetChebyshevWeightsValidation :359-405."""
    assert validate("distortion", cfg_of("distortion", mode=14, cheb_order=4, cheb_harmonic=1)) == _lib.AD_ERR_INVALID_ARGUMENT
    assert validate("distortion", cfg_of("distortion", cheb_order=4, cheb_harmonic=2)) == _lib.AD_OK
    assert validate("distortion", cfg_of("distortion", cheb_order=4, cheb_harmonic=0)) == _lib.AD_OK
    for v in (NAN, INF, -INF):
        c = cfg_of("distortion")
        c.cheb_weights[15] = v
        assert validate("distortion", c) == _lib.AD_ERR_INVALID_ARGUMENT
    c = cfg_of("distortion")
    c.cheb_weights[15] = -1e300
    assert validate("distortion", c) == _lib.AD_OK
    for f in ("cheb_invert", "cheb_dc_bypass"):
        assert validate("distortion", cfg_of("distortion", **{f: 2})) == _lib.AD_ERR_INVALID_ARGUMENT
        assert validate("distortion", cfg_of("distortion", **{f: -1})) == _lib.AD_ERR_INVALID_ARGUMENT


@pytest.mark.parametrize("kind", ["distortion", "bitcrusher"])
def test_create_validates_before_the_device(kind):
    L = _lib.lib()
    h = C.c_void_p()
    create, destroy = getattr(L, f"ad_{kind}_create"), getattr(L, f"ad_{kind}_destroy")
    assert create(C.byref(cfg_of(kind, mix=1.5)), 2, 0, C.byref(h)) == _lib.AD_ERR_INVALID_ARGUMENT and not h.value
    assert create(C.byref(cfg_of(kind)), 0, 0, C.byref(h)) == _lib.AD_ERR_INVALID_ARGUMENT
    assert create(None, 1, 0, C.byref(h)) == _lib.AD_ERR_INVALID_ARGUMENT
    rc = create(C.byref(cfg_of(kind)), 2, 0, C.byref(h))
    if _lib.device_count() == 0:
        assert rc == _lib.AD_ERR_NO_DEVICE and not h.value  # no CPU path
    else:
        assert rc == _lib.AD_OK
        destroy(h)
    for fn in ("process", "reset"):
        assert getattr(L, f"ad_{kind}_{fn}")(*([None, None, 0] if fn == "process" else [None])) == _lib.AD_ERR_INVALID_ARGUMENT
    assert getattr(L, f"ad_{kind}_process_device")(None, None, 0, 0, None) == _lib.AD_ERR_INVALID_ARGUMENT
    assert getattr(L, f"ad_{kind}_set_param")(None, 0, 1.0) == _lib.AD_ERR_INVALID_ARGUMENT
    assert L.ad_distortion_curve(None, None, 0, None) == _lib.AD_ERR_INVALID_ARGUMENT
    assert L.ad_distortion_set_weights(None, None, 0) == _lib.AD_ERR_INVALID_ARGUMENT


# ---- the graph's configuration transport ------------------------------------
def _three(node_type):
    par, par2 = (C.c_int32 * 1)(0), (C.c_int32 * 1)(1)
    nodes = (E._Node * 3)()
    nodes[0].type = E.FXN_INPUT
    nodes[1].type, nodes[1].n_parents, nodes[1].parents = node_type, 1, C.cast(par, C.POINTER(C.c_int32))
    nodes[2].type, nodes[2].n_parents, nodes[2].parents = E.FXN_OUTPUT, 1, C.cast(par2, C.POINTER(C.c_int32))
    return nodes, (par, par2)


def test_create_cfg_refusals_that_need_no_device():
    L = _lib.lib()
    h = C.c_void_p()
    nodes, _keep = _three(E.FXN_DISTORTION)
    cfgs = (_lib.FxNodeCfg * 3)()
    assert L.ad_fx_graph_create_cfg(None, None, None, 3, 2, 0, C.byref(h)) == _lib.AD_ERR_INVALID_ARGUMENT
    assert L.ad_fx_graph_create_cfg(C.cast(nodes, C.c_void_p), None, C.cast(cfgs, C.c_void_p), 0, 2, 0, C.byref(h)) \
        == _lib.AD_ERR_INVALID_ARGUMENT
    assert L.ad_fx_graph_create_cfg(C.cast(nodes, C.c_void_p), None, C.cast(cfgs, C.c_void_p), 3, 0, 0, C.byref(h)) \
        == _lib.AD_ERR_INVALID_ARGUMENT
    assert not h.value


def test_new_node_types_without_config_are_refused():
    """Types 15 and 16 without their configuration are refused through all three entry points (the device is
    picked first, so without one the error is AD_ERR_NO_DEVICE, as for the types before them)."""
    L = _lib.lib()
    want = _lib.AD_ERR_NO_DEVICE if _lib.device_count() == 0 else _lib.AD_ERR_INVALID_ARGUMENT
    for t in (E.FXN_DISTORTION, E.FXN_BITCRUSHER):
        nodes, _keep = _three(t)
        cfgs = (_lib.FxNodeCfg * 3)()
        h = C.c_void_p()
        assert L.ad_fx_graph_create(C.cast(nodes, C.c_void_p), 3, 2, 0, C.byref(h)) == want and not h.value
        assert L.ad_fx_graph_create_ext(C.cast(nodes, C.c_void_p), None, 3, 2, 0, C.byref(h)) == want and not h.value
        assert L.ad_fx_graph_create_cfg(C.cast(nodes, C.c_void_p), None, None, 3, 2, 0, C.byref(h)) == want
        assert L.ad_fx_graph_create_cfg(C.cast(nodes, C.c_void_p), None, C.cast(cfgs, C.c_void_p), 3, 2, 0, C.byref(h)) == want
        assert not h.value


@pytest.mark.parametrize("node_type", ["distortion", "dist-cheb", "bitcrusher"])
def test_graph_compiler_knows_the_waveshaping_nodes(node_type):
    """They compile; without a device they fail at the device, not as an unknown effect."""
    graph = E._graph_json([{"id": "n", "type": node_type}], [(E.INPUT_NODE_ID, "n"), ("n", E.OUTPUT_NODE_ID)])
    ch = E.Chain(48000.0, 2)
    if _lib.device_count() == 0:
        with pytest.raises(_lib.ADError) as e:
            ch.LoadGraph(graph)
        assert e.value.code == _lib.AD_ERR_NO_DEVICE
    else:
        ch.LoadGraph(graph)
        assert ch.spec[1]["type"] == ("bitcrusher" if node_type == "bitcrusher" else "distortion")
    for still_unknown in ("transformer", "widener", "bass", "chorus"):
        with pytest.raises(E.UnknownEffect):
            E.Chain(48000.0, 2).LoadGraph(E._graph_json([{"id": "n", "type": still_unknown}],
                                                        [(E.INPUT_NODE_ID, "n"), ("n", E.OUTPUT_NODE_ID)]))
