"""The reference's Distortion and BitCrusher unit tests, restated against the HIP
engine.

Each test names the test it follows (dsp/effects/distortion_test.go,
bit_crusher_test.go under github.com/cwbudde/algo-dsp) and keeps its settings,
inputs and tolerance.  A reference `ProcessSample` call is a one-sample
`ProcessInPlace` on the GPU; a constructor or setter error is
ErrInvalidArgument.
"""
import ctypes as C
import math

import numpy as np
import pytest

import shaper_ref as R
from algodsp import _lib, processors as P

pytestmark = pytest.mark.gpu
FS = 48000.0
M = {name: i for i, name in enumerate(R.MODES)}


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


# ---- distortion_test.go -----------------------------------------------------
def test_distortion_validation(gpu):
    """TestDistortionValidation :9-42."""
    with pytest.raises(_lib.ErrInvalidArgument):
        P.Distortion(0.0)
    with pytest.raises(_lib.ErrInvalidArgument):
        P.Distortion(FS, drive=100.0)
    with pytest.raises(_lib.ErrInvalidArgument):
        P.Distortion(FS, mode=999)
    with pytest.raises(_lib.ErrInvalidArgument):
        P.Distortion(FS, mode=M["chebyshev"], cheb_order=4, cheb_harmonic=R.ODD)
    d = P.Distortion(FS)
    with pytest.raises(_lib.ErrInvalidArgument):
        d.SetChebyshevHarmonicMode(R.EVEN)  # the default order 3 is odd
    assert d.config().cheb_harmonic == R.ALL  # and this handle does not keep the rejected mode


def test_distortion_mix_zero_passthrough(gpu):
    """TestDistortionMixZeroPassthrough :44-60."""
    d = P.Distortion(FS, mode=M["hardclip"], drive=10.0, mix=0.0)
    x = np.array([-1.2, -0.5, 0, 0.4, 1.3])
    assert np.max(np.abs(one_sample_calls(d, x) - x)) <= 1e-12


def test_distortion_hard_clip_transfer_curve(gpu):
    """TestDistortionHardClipTransferCurve :62-92."""
    d = P.Distortion(FS, mode=M["hardclip"], drive=1.0, clip_level=0.5, mix=1.0)
    x = np.array([-2, -0.5, -0.25, 0, 0.25, 0.5, 2.0])
    want = np.array([-1, -1, -0.5, 0, 0.5, 1, 1.0])
    assert np.max(np.abs(one_sample_calls(d, x) - want)) <= 1e-12
    assert np.max(np.abs(d.curve(x) - want)) <= 1e-12


def test_distortion_all_formula_modes_finite_and_bounded(gpu):
    """TestDistortionAllFormulaModesFiniteAndBounded :94-131: drive 4, shape 0.7, mix 1."""
    for name in ("waveshaper1", "waveshaper2", "waveshaper3", "waveshaper4", "waveshaper5", "waveshaper6", "waveshaper7",
                 "waveshaper8", "saturate", "saturate2", "softsat"):
        d = P.Distortion(FS, mode=M[name], drive=4.0, shape=0.7, mix=1.0)
        out = one_sample_calls(d, [-2, -1, -0.2, 0, 0.2, 1, 2])
        assert np.all(np.isfinite(out)) and np.max(np.abs(out)) <= 1.0000001, name


def test_distortion_tanh_approx_close_to_exact(gpu):
    """TestDistortionTanhApproxCloseToExact :133-163: drive 2.5, in = i / 50 for i in -100 .. 100, within 0.05."""
    x = np.arange(-100, 101) / 50.0
    exact = block(P.Distortion(FS, mode=M["tanh"], approx=R.EXACT, drive=2.5, mix=1.0), x)
    approx = block(P.Distortion(FS, mode=M["tanh"], approx=R.POLYNOMIAL, drive=2.5, mix=1.0), x)
    assert np.max(np.abs(exact - approx)) <= 0.05
    assert np.max(np.abs(exact - np.tanh(2.5 * x))) <= 1e-12


def _harmonic(x, k):  # harmonicAmplitude :452-463
    ph = 2 * math.pi * k * np.arange(len(x)) / len(x)
    return 2 * math.hypot(float(np.sum(x * np.cos(ph))), float(-np.sum(x * np.sin(ph)))) / len(x)


def test_distortion_chebyshev_harmonic_balance(gpu):
    """TestDistortionChebyshevHarmonicBalance :165-198: T_3 of a cosine is its third harmonic."""
    d = P.Distortion(FS, mode=M["chebyshev"], cheb_order=3, cheb_harmonic=R.ODD, drive=1.0, mix=1.0)
    out = block(d, np.cos(2 * math.pi * np.arange(4096) / 4096))
    a1, a2, a3 = (_harmonic(out, k) for k in (1, 2, 3))
    assert a3 > a1 and a2 <= a3 * 0.1


def test_distortion_chebyshev_dc_bypass_reduces_dc(gpu):
    """TestDistortionChebyshevDCBypassReducesDC :200-239: order 2, even, 4000 samples of a cosine of period 128."""
    x = np.cos(2 * math.pi * np.arange(4000) / 128)
    make = lambda dc: P.Distortion(FS, mode=M["chebyshev"], cheb_order=2, cheb_harmonic=R.EVEN, cheb_dc_bypass=dc, mix=1.0)
    mean_no, mean_dc = block(make(0), x).mean(), block(make(1), x).mean()
    assert abs(mean_dc) < abs(mean_no) * 0.2


def test_distortion_process_in_place(gpu):
    """TestDistortionProcessInPlace :241-278: SoftSat, drive 3, 256 samples of a sine, sample by sample and as one
    block, within 1e-12 (here: the same bits); and the stateful path, Chebyshev with DC bypass."""
    x = np.sin(2 * math.pi * np.arange(256) / 53)
    for kw in (dict(mode=M["softsat"], drive=3.0, mix=1.0), dict(mode=M["chebyshev"], cheb_dc_bypass=1)):
        a, b = one_sample_calls(P.Distortion(FS, **kw), x), block(P.Distortion(FS, **kw), x)
        assert np.max(np.abs(a - b)) <= 1e-12
        np.testing.assert_array_equal(a.view(np.int64), b.view(np.int64))


def test_chebyshev_weights(gpu):
    """TestChebyshevWeightsDefaultIsLegacyTN :280-301, ...AdditiveBlend :303-344, TestSetChebyshevWeightsValidation
    :359-405, TestChebyshevWeightsZeroAfterSet :407-450."""
    base = dict(mode=M["chebyshev"], cheb_order=3, drive=1.0, mix=1.0, output_level=1.0, cheb_gain=1.0)
    d = P.Distortion(FS, **base)
    assert abs(one_sample_calls(d, [0.5])[0] - -1.0) <= 1e-10
    x = 0.3
    for w, want in (([1, 0, 0], x), ([0, 1, 0], 2 * x * x - 1), ([0, 0, 1], max(-1.0, min(1.0, 4 * x * x * x - 3 * x)))):
        assert abs(one_sample_calls(P.Distortion(FS, cheb_weights=w, **base), [x])[0] - want) <= 1e-10
    for bad in ([0.0] * 17, [float("nan")], [float("inf")]):
        with pytest.raises(_lib.ErrInvalidArgument):
            d.SetChebyshevWeights(bad)
    d.SetChebyshevWeights([1, 0, 0])
    assert abs(one_sample_calls(d, [0.4])[0] - 0.4) <= 1e-10 and d.derived()["weights_active"]
    assert abs(one_sample_calls(d, [0.5])[0] - 0.5) <= 1e-10
    d.SetChebyshevWeights([0, 0, 0])
    assert abs(one_sample_calls(d, [0.5])[0] - -1.0) <= 1e-10 and not d.derived()["weights_active"]
    d.SetChebyshevWeights([0.25, 0.5])  # a shorter list clears the other slots
    assert list(d.config().cheb_weights) == [0.25, 0.5] + [0.0] * 14
    d.SetChebyshevWeights([])
    assert list(d.config().cheb_weights) == [0.0] * 16


# ---- bit_crusher_test.go ----------------------------------------------------
def test_bitcrusher_process_in_place_matches_sample(gpu):
    """TestBitCrusherProcessInPlaceMatchesSample :8-40, and with a hold that spans the one-sample calls."""
    x = np.sin(2 * math.pi * np.arange(128) / 31)
    for kw in (dict(), dict(bit_depth=4.0, downsample=4)):
        a, b = one_sample_calls(P.BitCrusher(FS, **kw), x), block(P.BitCrusher(FS, **kw), x)
        assert np.max(np.abs(a - b)) <= 1e-12
        np.testing.assert_array_equal(a.view(np.int64), b.view(np.int64))


def test_bitcrusher_reset_restores_state(gpu):
    """TestBitCrusherResetRestoresState :42-73: depth 4, downsample 4, 96 samples of a sine."""
    bc = P.BitCrusher(FS, bit_depth=4.0, downsample=4)
    x = np.sin(2 * math.pi * np.arange(96) / 17)
    out1 = one_sample_calls(bc, x)
    bc.Reset()
    out2 = one_sample_calls(bc, x)
    assert np.max(np.abs(out1 - out2)) <= 1e-12 and np.any(out1 != 0)


def test_bitcrusher_mix_zero_is_transparent(gpu):
    """TestBitCrusherMixZeroIsTransparent :75-93."""
    x = 0.5 * np.sin(2 * math.pi * 440 * np.arange(512) / FS)
    assert np.max(np.abs(block(P.BitCrusher(FS, bit_depth=2.0, downsample=8, mix=0.0), x) - x)) <= 1e-12


def test_bitcrusher_high_bit_depth_is_transparent(gpu):
    """TestBitCrusherHighBitDepthIsTransparent :95-115: depth 32, downsample 1, within 1e-9."""
    x = 0.75 * np.sin(2 * math.pi * 440 * np.arange(512) / FS)
    assert np.max(np.abs(block(P.BitCrusher(FS, bit_depth=32.0, downsample=1, mix=1.0), x) - x)) <= 1e-9


def test_bitcrusher_quantization(gpu):
    """TestBitCrusherQuantization :117-151: one bit is round(x), halves away from zero."""
    bc = P.BitCrusher(FS, bit_depth=1.0, downsample=1, mix=1.0)
    for x, want in ((0.0, 0.0), (0.3, 0.0), (0.5, 1.0), (0.6, 1.0), (1.0, 1.0), (-0.3, 0.0), (-0.6, -1.0), (-1.0, -1.0)):
        bc.Reset()
        assert one_sample_calls(bc, [x])[0] == want, x


def test_bitcrusher_downsample_hold(gpu):
    """TestBitCrusherDownsampleHold :153-202."""
    bc = P.BitCrusher(FS, bit_depth=32.0, downsample=4, mix=1.0)
    out = one_sample_calls(bc, [0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8])
    assert np.all(out[:3] == 0) and np.all(out[3:7] == out[3]) and out[7] != out[3]
    assert abs(out[3] - 0.4) <= 1e-9 and abs(out[7] - 0.8) <= 1e-9


def test_bitcrusher_silence_produces_silence(gpu):
    """TestBitCrusherSilenceProducesSilence :204-220, and the distortion's modes on silence."""
    assert np.all(one_sample_calls(P.BitCrusher(FS, bit_depth=4.0, downsample=2, mix=1.0), np.zeros(256)) == 0)
    assert np.all(block(P.BitCrusher(FS, bit_depth=4.0, downsample=2, mix=1.0), np.zeros(256)) == 0)
    for m in range(len(R.MODES)):
        if m == M["chebyshev"]:
            continue  # T_N(0) is not 0 for even N; order 3 below
        assert np.all(block(P.Distortion(FS, mode=m), np.zeros(64)) == 0), R.MODES[m]
    assert np.all(block(P.Distortion(FS, mode=M["chebyshev"], cheb_order=3, cheb_dc_bypass=1), np.zeros(64)) == 0)


def test_bitcrusher_quantization_error(gpu):
    """TestBitCrusherQuantizationError :419-447: the error is at most half a step."""
    x = 2.0 * np.arange(1000) / 999.0 - 1.0
    for depth in (2.0, 4.0, 8.0, 16.0):
        out = block(P.BitCrusher(FS, bit_depth=depth, downsample=1, mix=1.0), x)
        assert np.max(np.abs(out - x)) <= 0.5 / 2.0 ** (depth - 1) + 1e-12


def test_bitcrusher_getters_and_setters(gpu):
    """TestBitCrusherGetters :338-363, TestBitCrusherSettersUpdateState :365-406, TestBitCrusherNilOption :408-417."""
    bc = P.BitCrusher(FS, bit_depth=12.0, downsample=3, mix=0.8)
    assert (bc.SampleRate(), bc.BitDepth(), bc.Downsample(), bc.Mix()) == (48000.0, 12.0, 3, 0.8)
    bc = P.BitCrusher(FS)
    assert (bc.BitDepth(), bc.Downsample(), bc.Mix()) == (8.0, 1, 1.0)
    bc.SetSampleRate(96000.0), bc.SetBitDepth(16.0), bc.SetDownsample(8), bc.SetMix(0.5)
    assert (bc.SampleRate(), bc.BitDepth(), bc.Downsample(), bc.Mix()) == (96000.0, 16.0, 8, 0.5)
    assert bc.derived()["quant_levels"] == 32768.0


# ---- the validation tables --------------------------------------------------
@pytest.mark.parametrize("kind", ["distortion", "bitcrusher"])
def test_validation_tables(gpu, kind):
    """TestBitCrusherValidation :222-289, TestBitCrusherSetterValidation :291-336 and the distortion's options
    and setters (distortion.go:135-269, 364-529): every value against validate, the constructor and set_param."""
    make = P.Distortion if kind == "distortion" else P.BitCrusher
    cfg_t = _lib.DistortionConfig if kind == "distortion" else _lib.BitCrusherConfig
    L = _lib.lib()

    def cfg(**kv):
        c = cfg_t()
        getattr(L, f"ad_{kind}_default_config")(C.byref(c), FS)
        for k, v in kv.items():
            setattr(c, k, v)
        return c

    validate = getattr(L, f"ad_{kind}_validate")
    for field, value in R.rejected(kind):
        assert validate(C.byref(cfg(**{field: value}))) == _lib.AD_ERR_INVALID_ARGUMENT, (field, value)
        with pytest.raises(_lib.ErrInvalidArgument):
            make(config=cfg(**{field: value}))
        h = make(FS)
        with pytest.raises(_lib.ErrInvalidArgument):
            R.set_on(h, field, value)
        assert getattr(h.config(), field) == getattr(cfg(), field)
    for field, value in R.accepted(kind):
        assert validate(C.byref(cfg(**{field: value}))) == _lib.AD_OK, (field, value)
        assert getattr(make(config=cfg(**{field: value})).config(), field) == value
        h = make(FS)
        R.set_on(h, field, value)
        assert getattr(h.config(), field) == value
