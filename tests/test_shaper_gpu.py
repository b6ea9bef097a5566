"""effects.Distortion and effects.BitCrusher on the GPU (processors.Distortion /
BitCrusher, the effect graph's distortion, dist-cheb and bitcrusher nodes)
against the restated reference (tests/shaper_ref.py), with distinct noise per
channel.

Bars.  Outputs are compared on the float64 bits, the sign of zero included; a
NaN is compared by position only.  The modes made of + - * / (and the
polynomial approximations) are compared with the pure restatement.  The modes
that call tanh, atan or exp are compared on the bits given ad_distortion_curve
of the same arguments (out = in (1 - mix) + curve mix), and the curve itself is
held to the project's bars for device-library functions, relative RMS <= 1e-12
and max abs <= 1e-10, as tests/test_delayfx_gpu.py and test_modfx_gpu.py hold
the sine.  The bit crusher is compared on the bits given quantLevels as
derived() reports it (exp2 of the C library; exactly 2^(depth - 1) for whole
depths).

Worst ulp distance of curve() against numpy's tanh / arctan / exp on this
machine's libm, over the sweep of test_transcendental_curve (noise and 200001
even steps of x in [-8, 8], drive and bias left out).  Measured on the MI355X
by this test, which prints it; nothing is asserted on it:

    mode         shape   worst ulp distance   max abs    relative RMS
    tanh         -       1                    1.1e-16    5.1e-17
    waveshaper5  0.5     2                    2.2e-16    2.0e-17
    waveshaper7  0.5     1                    1.1e-16    3.9e-17
    waveshaper8  0.5     256                  1.1e-16    7.2e-18
    softsat      -       2                    2.2e-16    4.0e-17

waveshaper8's 256 is at 1 - exp(-a |x|) near x = 0, where the subtraction cancels a last-place difference of
exp into the low bits of a small result.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import layout_lib as LL
import shaper_ref as R
from algodsp import _lib, design, effectchain as E, processors as P, signals

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
RMS_BAR, ABS_BAR = 1e-12, 1e-10
FS = 48000.0
N, CUTS = 1501, [700, 1, 800]
CHANNELS = [1, 3, 65]  # one past a wave, and no multiple of 64
NAN, INF = float("nan"), float("inf")
M = {name: i for i, name in enumerate(R.MODES)}


def noise(n, channels=3, seed=0x5A7, amplitude=2.0):
    return np.stack([signals.white_noise(n, seed + c) for c in range(channels)]) * amplitude


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def same_bits(got, want, what=""):
    """Bit patterns, the sign of zero included; a NaN by position only."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, what
    gn, wn = np.isnan(got), np.isnan(want)
    np.testing.assert_array_equal(gn, wn, err_msg=f"{what}: NaN positions")
    bad = np.flatnonzero((bits(got) != bits(want)).reshape(-1) & ~gn.reshape(-1))
    if bad.size:
        i = int(bad[0])
        raise AssertionError(f"{what}: {bad.size} of {got.size} differ, first at flat index {i}: "
                             f"got {got.reshape(-1)[i]!r}, want {want.reshape(-1)[i]!r}")


def gpu_run(h, x, cuts=None):
    y = x.copy()
    pos = 0
    for m in cuts or [x.shape[1]]:
        blk = y[:, pos:pos + m].copy()
        h.ProcessInPlace(blk)
        y[:, pos:pos + m] = blk
        pos += m
    assert pos == x.shape[1]
    return y


def distortion_pair(channels, **options):
    h, ref = P.Distortion(FS, channels, **options), R.Distortion(FS, **options)
    d = h.derived()
    # the host's constants are the restatement's: the same C library, the same rounded operations
    assert d["atan_scale"] == math.atan(1 + 4 * ref.shape) and d["scale6"] == 1 + 6 * ref.shape
    assert d["scale2"] == 1 + 2 * ref.shape and d["one_minus_mix"] == 1 - ref.mix
    assert d["weights_active"] == ref.has_weights()
    ref.atanScale = d["atan_scale"]
    return h, ref


def crusher_pair(channels, **options):
    h, ref = P.BitCrusher(FS, channels, **options), R.BitCrusher(FS, **options)
    sync_q(h, ref)
    return h, ref


def sync_q(h, ref):
    q = h.derived()["quant_levels"]
    if ref.bitDepth == int(ref.bitDepth):
        assert q == 2.0 ** (int(ref.bitDepth) - 1)  # exact for whole depths
    assert math.nextafter(ref.quantLevels, 0.0) <= q <= math.nextafter(ref.quantLevels, INF)
    ref.quantLevels = q


# ---- the algebraic modes: bit-exact against the restatement ------------------
W16 = [0.5, -0.25, 0.125, 0.3, -0.2, 0.1, 0.05, -0.05, 0.02, 0.01, -0.01, 0.03, 0.002, -0.004, 0.001, 0.0005]
ALGEBRAIC = [
    ("softclip", dict(mode=M["softclip"])),
    ("hardclip", dict(mode=M["hardclip"], clip_level=0.5)),
    ("waveshaper1", dict(mode=M["waveshaper1"], shape=0.7)),
    ("waveshaper2", dict(mode=M["waveshaper2"], shape=0.7)),
    ("waveshaper3", dict(mode=M["waveshaper3"], shape=0.7)),
    ("waveshaper4", dict(mode=M["waveshaper4"])),
    ("waveshaper6", dict(mode=M["waveshaper6"], shape=0.3)),
    ("saturate", dict(mode=M["saturate"])),
    ("saturate2", dict(mode=M["saturate2"], shape=0.7)),
    ("tanh polynomial", dict(mode=M["tanh"], approx=R.POLYNOMIAL)),
    ("waveshaper7 polynomial", dict(mode=M["waveshaper7"], approx=R.POLYNOMIAL, shape=0.1)),
    ("softsat polynomial", dict(mode=M["softsat"], approx=R.POLYNOMIAL)),
    ("chebyshev 1", dict(mode=M["chebyshev"], cheb_order=1)),
    ("chebyshev 3", dict(mode=M["chebyshev"], cheb_order=3, cheb_harmonic=R.ODD)),
    ("chebyshev 16", dict(mode=M["chebyshev"], cheb_order=16, cheb_harmonic=R.EVEN, cheb_gain=0.8)),
    ("chebyshev 1 weights", dict(mode=M["chebyshev"], cheb_order=1, cheb_weights=[0.7])),
    ("chebyshev 3 weights", dict(mode=M["chebyshev"], cheb_order=3, cheb_weights=[0.5, -0.25, 0.125])),
    ("chebyshev 16 weights", dict(mode=M["chebyshev"], cheb_order=16, cheb_weights=W16, cheb_gain=1.5)),
    ("chebyshev 3, weights past the order", dict(mode=M["chebyshev"], cheb_order=3, cheb_weights=[0, 0, 0, 0.9])),
    ("chebyshev 5 inverted", dict(mode=M["chebyshev"], cheb_order=5, cheb_invert=1)),
    ("chebyshev 4 weights inverted", dict(mode=M["chebyshev"], cheb_order=4, cheb_invert=1, cheb_weights=[0.1, 0.9, 0, -0.3])),
    ("chebyshev 3 DC bypass", dict(mode=M["chebyshev"], cheb_order=3, cheb_dc_bypass=1)),
    ("chebyshev 16 weights DC bypass", dict(mode=M["chebyshev"], cheb_order=16, cheb_weights=W16, cheb_dc_bypass=1)),
    ("chebyshev 2 inverted DC bypass", dict(mode=M["chebyshev"], cheb_order=2, cheb_invert=1, cheb_dc_bypass=1,
                                          cheb_harmonic=R.EVEN)),
]


def branch_points(clip):
    """x on every branch boundary and on both sides of it, and the values arithmetic treats specially."""
    pts = []
    for b in (1.0, 3.0, clip):
        pts += [b, -b, math.nextafter(b, 0.0), math.nextafter(b, INF), -math.nextafter(b, 0.0), -math.nextafter(b, INF)]
    return pts + [0.0, -0.0, 5e-324, -5e-324, 1e-310, 2.2250738585072014e-308]


def points_input(channels, clip, nonfinite_row):
    """Noise with x = in * 2 (bias 0, drive 2: exact) on the branch points; +-Inf and NaN go to one row only."""
    x = noise(N, channels)
    pts = branch_points(clip)
    for c in range(channels):
        for k, p in enumerate(pts):
            x[c, 10 + 37 * k + c] = p / 2.0
    if nonfinite_row is not None:
        for k, p in enumerate((INF, -INF, NAN)):
            x[nonfinite_row, 900 + 101 * k] = p
    return x


@pytest.mark.parametrize("channels", CHANNELS)
@pytest.mark.parametrize("name,options", ALGEBRAIC, ids=[a[0] for a in ALGEBRAIC])
def test_algebraic_modes_are_bit_exact(gpu, name, options, channels):
    clip = options.get("clip_level", 1.0)
    row = channels // 2
    # x = 2 in on the branch points, finite everywhere
    h, ref = distortion_pair(channels, drive=2.0, **options)
    x = points_input(channels, clip, None)
    got = gpu_run(h, x, CUTS)
    same_bits(got, ref.process_many(x), f"{name}, {channels} ch, branch points")
    # +-Inf and NaN in one row: that row as the restatement says (with DC bypass, poisoned from there on
    # exactly as it says), the other rows' bits as without them
    h, ref = distortion_pair(channels, drive=2.0, **options)
    bad = points_input(channels, clip, row)
    got_bad = gpu_run(h, bad, CUTS)
    same_bits(got_bad, ref.process_many(bad), f"{name}, {channels} ch, non-finite samples in row {row}")
    for c in range(channels):
        if c != row:
            same_bits(got_bad[c], got[c], f"{name}: row {c} next to the non-finite row")
    if options.get("cheb_dc_bypass"):
        assert float(np.asarray(ref.dcPrevOut).reshape(-1)[row]) != 0.0
        tail_bad, tail = got_bad[row, 1200:], got[row, 1200:]
        print(f"{name}: after the non-finite samples row {row} differs in {int(np.sum(bits(tail_bad) != bits(tail)))} of 301")
    # bias, a drive that is no power of two, a mix and an output level
    h, ref = distortion_pair(channels, drive=3.3, bias=0.1, mix=0.7, output_level=1.5, **options)
    x = noise(N, channels, seed=0x77, amplitude=0.6)
    same_bits(gpu_run(h, x, CUTS), ref.process_many(x), f"{name}, {channels} ch, drive 3.3, bias 0.1, mix 0.7")
    same_bits(gpu_run(P.Distortion(FS, channels, drive=3.3, bias=0.1, mix=0.7, output_level=1.5, **options), x),
              ref_once(x, drive=3.3, bias=0.1, mix=0.7, output_level=1.5, **options), f"{name}: one call")


def ref_once(x, **options):
    return R.Distortion(FS, **options).process_many(x)


def test_dc_bypass_keeps_a_non_finite_state(gpu):
    """A non-finite y stays in dcPrevOut (the finite check comes after the filter and repairs nothing): the
    output of that row is 0 * mix from there on, the restatement's, and Reset clears it."""
    opts = dict(mode=M["chebyshev"], cheb_order=3, cheb_dc_bypass=1, output_level=4.0, mix=1.0)
    h, ref = distortion_pair(3, **opts)
    x = noise(400, 3, amplitude=0.9)
    # no input makes chebyshevShape non-finite (it clamps first), so poison the state the way a caller can: a
    # NaN input is clamped through (comparisons false), T_3(NaN) is NaN, y is NaN and stays
    x[1, 100] = NAN
    got = gpu_run(h, x, [150, 250])
    want = ref.process_many(x)
    same_bits(got, want, "DC bypass with a NaN at row 1, sample 100")
    assert np.all(got[1, 101:] == 0.0) and np.any(got[0, 101:] != 0.0) and np.isnan(ref.dcPrevOut[1])
    h.Reset(), ref.Reset()
    x[1, 100] = 0.5
    same_bits(gpu_run(h, x), ref.process_many(x), "after Reset")


# ---- the transcendental modes -------------------------------------------------
TRANSCENDENTAL = [("tanh", dict(mode=M["tanh"])), ("waveshaper5", dict(mode=M["waveshaper5"], shape=0.5)),
                  ("waveshaper7", dict(mode=M["waveshaper7"], shape=0.5)), ("waveshaper8", dict(mode=M["waveshaper8"], shape=0.5)),
                  ("softsat", dict(mode=M["softsat"]))]


def ulps(a, b):
    return int(np.max(np.abs(bits(a) - bits(b)))) if len(a) else 0


@pytest.mark.parametrize("channels", CHANNELS)
@pytest.mark.parametrize("name,options", TRANSCENDENTAL, ids=[a[0] for a in TRANSCENDENTAL])
def test_transcendental_process_is_bit_exact_given_the_curve(gpu, name, options, channels):
    h, ref = distortion_pair(channels, drive=3.3, bias=0.1, mix=0.7, output_level=1.5, **options)
    x = points_input(channels, 1.0, channels // 2)
    curve = h.curve(ref.argument(x))
    same_bits(h.curve(ref.argument(x)), curve, "a curve advances nothing")
    same_bits(gpu_run(h, x, CUTS), ref.process_many(x, curve), f"{name}, {channels} ch, given the curve")
    assert not np.isnan(curve).any() and not np.isinf(curve).any()  # the finite check is in the curve


@pytest.mark.parametrize("name,options", TRANSCENDENTAL, ids=[a[0] for a in TRANSCENDENTAL])
def test_transcendental_curve(gpu, name, options):
    """curve() against the restatement with numpy's tanh, arctan and exp: the project's bars for device-library
    functions.  The worst ulp distance is printed for the table above, not asserted."""
    h, ref = distortion_pair(1, **options)
    x = np.concatenate([noise(20000, 1, amplitude=4.0)[0], np.linspace(-8.0, 8.0, 200001), branch_points(1.0)])
    got, want = h.curve(x), ref.curve(x)
    err = float(np.sqrt(np.mean((got - want) ** 2)) / np.sqrt(np.mean(want ** 2)))
    mx = float(np.max(np.abs(got - want)))
    print(f"curve {name}: rel rms {err:.3g}, max abs {mx:.3g}, worst ulp distance {ulps(got, want)}, "
          f"differing {int(np.sum(got != want))} of {x.size}")
    assert err <= RMS_BAR and mx <= ABS_BAR
    h2, ref2 = distortion_pair(1, output_level=2.5, **options)
    same_bits(h2.curve(np.array([NAN, INF, -INF])), ref2.curve(np.array([NAN, INF, -INF])), f"{name}: non-finite arguments")


def test_algebraic_curve_is_the_restatements(gpu):
    x = np.concatenate([noise(3000, 1, amplitude=4.0)[0], branch_points(0.5), [INF, -INF, NAN]])
    for name, options in ALGEBRAIC:
        h, ref = distortion_pair(1, output_level=1.7, **options)
        same_bits(h.curve(x), ref.curve(x), f"curve {name}")
    assert h.curve(np.empty(0)).size == 0
    assert h.curve(x.reshape(3, -1)).shape == (3, x.size // 3)


# ---- the bit crusher --------------------------------------------------------
CALLS = [1, 2, 3, 255, 257, 1500, 64]
CRUSH_COMBOS = [dict(mix=1.0, bit_depth=8.0, channels=3), dict(mix=0.5, bit_depth=7.5, channels=65),
                dict(mix=0.0, bit_depth=32.0, channels=1), dict(mix=1.0, bit_depth=1.0, channels=3)]


def crush_calls(h, ref, x, calls, what):
    """The handle and the restatement over the same calls; after each the counter and every row's hold value."""
    pos = 0
    out = x.copy()
    for m in calls:
        blk = x[:, pos:pos + m].copy()
        c0 = ref.holdCounter
        want = ref.process_many(blk)
        h.ProcessInPlace(blk)
        same_bits(blk, want, f"{what} [{pos}, {pos + m}) from counter {c0}")
        assert ref.holdCounter == R.counter_after(ref.downsample, c0, m)
        for c in range(x.shape[0]):
            d = h.derived(c)
            assert d["counter"] == ref.holdCounter, f"{what}: counter after [{pos}, {pos + m})"
            assert bits(d["hold_value"]) == bits(ref.holdValue[c]), f"{what}: hold value of row {c} after [{pos}, {pos + m})"
        out[:, pos:pos + m] = blk
        pos += m
    return out


@pytest.mark.parametrize("combo", CRUSH_COMBOS, ids=lambda c: f"mix{c['mix']}-depth{c['bit_depth']}-{c['channels']}ch")
@pytest.mark.parametrize("downsample", [1, 2, 3, 4, 255, 256])
def test_bitcrusher_is_bit_exact(gpu, downsample, combo):
    ch = combo["channels"]
    h, ref = crusher_pair(ch, downsample=downsample, mix=combo["mix"], bit_depth=combo["bit_depth"])
    n = sum(CALLS) + 300 + 90
    x = noise(n, ch, amplitude=1.2)
    x[:, 5] = [0.5 / ref.quantLevels * (1 if c % 2 else -1) for c in range(ch)]  # a half: away from zero
    x[0, 7], x[0, 8] = -0.0, -0.2 / ref.quantLevels  # rounds to -0
    what = f"downsample {downsample}, {combo}"
    crush_calls(h, ref, x[:, :sum(CALLS)], CALLS, what)
    # the factor rises: calls without an update carry the counter up; then it drops below the counter, and
    # the next call's first sample is an update (t0 = max(downsample - 1 - c0, 0))
    for o in (h, ref):
        o.SetDownsample(256)
    crush_calls(h, ref, x[:, sum(CALLS):sum(CALLS) + 300], [100, 1, 199], what + " -> 256")
    assert ref.holdCounter >= 2
    for o in (h, ref):
        o.SetDownsample(2)
    assert R.first_update(2, ref.holdCounter) == 0
    crush_calls(h, ref, x[:, sum(CALLS) + 300:], [1, 89], what + " -> 256 -> 2")


@pytest.mark.parametrize("downsample", [2, 3, 255, 256])
def test_bitcrusher_rows_longer_than_a_span(gpu, downsample):
    """Several span workgroups a row: spans of whole hold periods, the last one cut mid-period, the call's last
    update in any of them; a carried counter moves the first span's start."""
    h, ref = crusher_pair(3, downsample=downsample, bit_depth=6.0, mix=0.8)
    span = h.kernel_info()[1]
    assert span % downsample == 0 and 2048 - downsample < span <= 2048
    x = noise(3 * 2048 + 4500 + 77, 3)
    crush_calls(h, ref, x, [77, 4500, span, 3 * 2048 - span], f"downsample {downsample}")


def test_bitcrusher_a_non_finite_sample_stays_in_its_row(gpu):
    x = noise(600, 3)
    bad = x.copy()
    bad[1, 100], bad[1, 301] = INF, NAN
    for ds in (1, 4):
        h, ref = crusher_pair(3, downsample=ds, mix=0.5)
        got = crush_calls(h, ref, bad, [250, 350], f"downsample {ds}, non-finite samples")
        clean = gpu_run(P.BitCrusher(FS, 3, downsample=ds, mix=0.5), x, [250, 350])
        for c in (0, 2):
            same_bits(got[c], clean[c], f"row {c} next to the non-finite row")


# ---- the device-buffer layout contract, streams -----------------------------
MAKERS = {"shape": lambda: P.Distortion(FS, 3, mode=M["waveshaper3"], drive=2.0, shape=0.7, mix=0.8),
          "dc bypass": lambda: P.Distortion(FS, 3, mode=M["chebyshev"], cheb_order=4, cheb_dc_bypass=1, cheb_weights=[0.2, 0.5, 0, 0.3]),
          "crush 1": lambda: P.BitCrusher(FS, 3, bit_depth=5.0, downsample=1, mix=0.6),
          "crush 3": lambda: P.BitCrusher(FS, 3, bit_depth=5.0, downsample=3, mix=0.6)}


@pytest.mark.parametrize("kind", list(MAKERS))
def test_process_device_layouts(gpu, kind):
    """Row strides greater than n and rows 8 bytes off 16-byte alignment give the bits of the aligned
    contiguous placement, and touch nothing around the rows."""
    n = 1501
    x = noise(n, amplitude=0.9)

    def run(layout):
        h = MAKERS[kind]()
        b = LL.place(x, layout, DEV)
        torch.cuda.synchronize()
        h.process_device(b.ptr, b.stride, 1000)  # a first call that leaves the last 501 columns alone
        h.process_device(b.ptr + 8 * 1000, b.stride, 501)
        torch.cuda.synchronize()
        LL.check_guards(b)
        return LL.payload(b)

    want = run(LL.LA(n))
    for layout in LL.variants(n):
        same_bits(run(layout), want, f"{kind} {layout}")
    h = MAKERS[kind]()
    same_bits(gpu_run(h, x, [1000, 501]), want, "host-buffer calls")
    b = LL.place(x, LL.L1, DEV)
    torch.cuda.synchronize()
    with pytest.raises(_lib.ErrInvalidArgument):
        h.process_device(b.ptr, n - 1, n)
    with pytest.raises(_lib.ErrInvalidArgument):
        h.process_device(0, b.stride, n)
    with pytest.raises(_lib.ErrInvalidArgument):
        h.process_device(b.ptr, b.stride, -1)
    h.process_device(b.ptr, b.stride, 0)
    torch.cuda.synchronize()
    LL.check_unchanged(b, x)


@pytest.mark.parametrize("n", [1, 2, 3])
@pytest.mark.parametrize("kind", list(MAKERS))
def test_shortest_rows(gpu, kind, n):
    """One, two and three samples a row, aligned and 8 bytes off: the lead sample, one pair and the odd one at the end."""
    x = noise(n, amplitude=0.9)
    want = gpu_run(MAKERS[kind](), x)
    for layout in [LL.LA(n)] + LL.variants(n):
        b = LL.place(x, layout, DEV)
        torch.cuda.synchronize()
        MAKERS[kind]().process_device(b.ptr, b.stride, n)
        torch.cuda.synchronize()
        LL.check_guards(b)
        same_bits(LL.payload(b), want, f"{kind}, {n} samples {layout}")


@pytest.mark.parametrize("kind", list(MAKERS))
def test_two_streams_alternate_on_one_handle(gpu, kind):
    """Calls alternate between the NULL stream and a side stream (and one host-buffer call): the state is
    shared, every call waits for the one before, so the result is one sequential processor's."""
    C_, n = 3, 4000
    x = noise(n, C_, amplitude=0.9)
    want = gpu_run(MAKERS[kind](), x)
    h = MAKERS[kind]()
    d = torch.from_numpy(x).to(DEV)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    host = None
    for i, t0 in enumerate(range(0, n, 500)):
        if i == 5:
            torch.cuda.synchronize()
            host = d[:, t0:t0 + 500].cpu().numpy().copy()
            h.ProcessInPlace(host)
            continue
        h.process_device(d.data_ptr() + 8 * t0, n, 500, side.cuda_stream if i % 2 else 0)
    torch.cuda.synchronize()
    got = d.cpu().numpy()
    got[:, 2500:3000] = host
    same_bits(got, want, f"{kind} on two streams")
    h.process_device(d.data_ptr(), n, 700, side.cuda_stream)
    h.Reset()  # ordered after the side stream's call
    torch.cuda.synchronize()


# ---- handles ----------------------------------------------------------------
@pytest.mark.parametrize("kind", ["dc bypass", "crush 3"])
def test_reset_restores_the_first_output(gpu, kind):
    x = noise(700, amplitude=0.9)
    h = MAKERS[kind]()
    first = gpu_run(h, x, [699, 1])
    assert np.any(gpu_run(h, x) != first)  # the DC states, the counter and the hold values carry over
    h.Reset()
    same_bits(gpu_run(h, x), first, f"{kind} after Reset")
    if kind == "crush 3":
        h.Reset()
        assert h.derived(2) == dict(quant_levels=16.0, counter=0, hold_value=0.0)


def fields(cfg):
    return E._config_dict(cfg)


@pytest.mark.parametrize("kind", ["distortion", "bitcrusher"])
def test_rejected_setter_changes_nothing(gpu, kind):
    x = noise(600, amplitude=0.9)
    make = (lambda: P.Distortion(FS, 3, mode=M["chebyshev"], cheb_dc_bypass=1, cheb_weights=[0.5, 0.2])) \
        if kind == "distortion" else (lambda: P.BitCrusher(FS, 3, downsample=5, bit_depth=6.0))
    h, twin = make(), make()
    gpu_run(h, x[:, :300]), gpu_run(twin, x[:, :300])
    before, derived = fields(h.config()), h.derived()
    tried = 0
    for field, value in R.rejected(kind):
        if kind == "distortion" and (field, value) == ("cheb_harmonic", R.EVEN):
            continue  # below, with the order it needs
        with pytest.raises(_lib.ErrInvalidArgument):
            R.set_on(h, field, value)
        assert fields(h.config()) == before and h.derived() == derived, (field, value)
        tried += 1
    assert tried >= 20
    with pytest.raises(_lib.ErrInvalidArgument):
        h._set(99, 1.0)
    if kind == "distortion":
        # the parity rule (validateChebyshevParity): order 3 refuses the even mode, the odd mode refuses order 4;
        # whole numbers only; weights: at most 16, all finite
        for field, value in (("cheb_harmonic", R.EVEN), ("cheb_order", 2.5), ("mode", 1.5), ("cheb_invert", 2), ("cheb_dc_bypass", 0.5)):
            with pytest.raises(_lib.ErrInvalidArgument):
                R.set_on(h, field, value)
        h.SetChebyshevHarmonicMode(R.ODD)
        with pytest.raises(_lib.ErrInvalidArgument):
            h.SetChebyshevOrder(4)
        assert h.ChebyshevOrder() == 3
        h.SetChebyshevHarmonicMode(R.ALL)
        for w in ([0.0] * 17, [NAN], [0.1, INF]):
            with pytest.raises(_lib.ErrInvalidArgument):
                h.SetChebyshevWeights(w)
    else:
        with pytest.raises(_lib.ErrInvalidArgument):
            R.set_on(h, "downsample", 2.5)
        with pytest.raises(_lib.ErrInvalidArgument):
            h.derived(3)
    assert fields(h.config()) == before and h.derived() == derived
    same_bits(gpu_run(h, x[:, 300:]), gpu_run(twin, x[:, 300:]), f"{kind} after the rejected values")


def test_accepted_setters_take_effect_without_clearing_state(gpu):
    x = noise(900, amplitude=0.9)
    h, ref = distortion_pair(3, mode=M["chebyshev"], cheb_order=3, cheb_dc_bypass=1)
    same_bits(gpu_run(h, x[:, :300]), ref.process_many(x[:, :300]), "before")
    for field, value in (("drive", 2.5), ("mix", 0.6), ("output_level", 1.2), ("cheb_gain", 0.9), ("cheb_order", 6),
                         ("cheb_invert", 1), ("bias", -0.1), ("sample_rate", 96000.0)):
        R.set_on(h, field, value), R.set_on(ref, field, value)
    h.SetChebyshevWeights([0.3, 0.0, -0.4]), ref.SetChebyshevWeights([0.3, 0.0, -0.4])
    assert h.derived()["weights_active"] and fields(h.config()) == R.config_of(ref)
    assert np.any(np.asarray(ref.dcPrevOut) != 0)
    same_bits(gpu_run(h, x[:, 300:600]), ref.process_many(x[:, 300:600]), "after the setters: the DC states carried over")
    for field, value in (("mode", M["waveshaper2"]), ("shape", 0.9), ("clip_level", 0.3)):
        R.set_on(h, field, value), R.set_on(ref, field, value)
    same_bits(gpu_run(h, x[:, 600:750]), ref.process_many(x[:, 600:750]), "another mode")
    for field, value in (("mode", M["chebyshev"]),):  # back: the DC states are where the last Chebyshev call left them
        R.set_on(h, field, value), R.set_on(ref, field, value)
    same_bits(gpu_run(h, x[:, 750:]), ref.process_many(x[:, 750:]), "Chebyshev again")
    assert (h.Mode(), h.Drive(), h.Mix(), h.OutputLevel(), h.ClipLevel(), h.Shape(), h.Bias(), h.ChebyshevOrder(),
            h.SampleRate()) == (14, 2.5, 0.6, 1.2, 0.3, 0.9, -0.1, 6, 96000.0)
    assert h.kernel_info() == (2048, 64, 32, 3 * 64 * 33 * 8)
    for field, value in R.accepted("distortion"):
        k, kref = distortion_pair(1)
        R.set_on(k, field, value), R.set_on(kref, field, value)
        assert fields(k.config()) == R.config_of(kref), (field, value)

    b, bref = crusher_pair(3, downsample=4, bit_depth=6.0)
    crush_calls(b, bref, x[:, :301], [301], "before")
    for field, value in (("bit_depth", 3.5), ("mix", 0.25), ("sample_rate", 8000.0), ("downsample", 7)):
        R.set_on(b, field, value), R.set_on(bref, field, value)
    sync_q(b, bref)
    assert fields(b.config()) == R.config_of(bref) and bref.holdCounter == 1
    crush_calls(b, bref, x[:, 301:], [599], "after the setters: the counter and the hold values carried over")
    assert (b.BitDepth(), b.Downsample(), b.Mix(), b.SampleRate()) == (3.5, 7, 0.25, 8000.0)
    assert b.kernel_info() == (2044, 2044, 2048 * 8)
    b.SetDownsample(1)
    assert b.kernel_info() == (2048, 0, 0)
    for field, value in R.accepted("bitcrusher"):
        k, kref = crusher_pair(1)
        R.set_on(k, field, value), R.set_on(kref, field, value)
        assert fields(k.config()) == R.config_of(kref), (field, value)


# ---- the effect graph -------------------------------------------------------
GFS = 8000.0
DIST_NODE = {"id": "d", "type": "distortion", "params": {"mode": "waveshaper3", "drive": 2.5, "shape": 0.8, "mix": 0.9, "bias": 0.05}}
CHEB_NODE = {"id": "c", "type": "dist-cheb", "params": {"order": 4, "harmonic": "odd", "gain": 0.7, "dcBypass": 1, "w1": 0.5,
                                                        "w3": 0.4, "w5": 0.2, "invert": 1, "drive": 1.5}}
CRUSH_NODE = {"id": "b", "type": "bitcrusher", "params": {"bitDepth": 5.5, "downsample": 3, "mix": 0.75}}
FILTER_NODE = {"id": "f", "type": "filter-lowpass", "params": {"freq": 1500, "q": 0.9}}
TREMOLO_NODE = {"id": "t", "type": "tremolo", "params": {"rateHz": 9.0, "depth": 0.9, "smoothingMs": 2.0}}


def _graph(nodes, dry_edge=False):
    ids = [E.INPUT_NODE_ID] + [n["id"] for n in nodes] + [E.OUTPUT_NODE_ID]
    edges = list(zip(ids[:-1], ids[1:]))
    if dry_edge:
        edges.append((E.INPUT_NODE_ID, E.OUTPUT_NODE_ID))
    return E._graph_json(nodes, edges)


def _chain_run(graph, x, channels=3, designer=None):
    ch = E.Chain(GFS, channels, designer=designer)
    ch.LoadGraph(graph)
    y = x.copy()
    assert ch.Process(y)
    return ch, y


def _params(node):
    raw = node.get("params", {})
    return E.Params(node["id"], node["type"], num={k: float(v) for k, v in raw.items() if not isinstance(v, str)},
                    str_={k: v for k, v in raw.items() if isinstance(v, str)})


def _processor(node):
    p = _params(node)
    if node["type"] == "distortion":
        return P.Distortion(channels=3, config=E.distortion_params(p, GFS))
    if node["type"] == "dist-cheb":
        return P.Distortion(channels=3, config=E.dist_cheb_params(p, GFS))
    if node["type"] == "bitcrusher":
        return P.BitCrusher(channels=3, config=E.bitcrusher_params(p, GFS))
    if node["type"] == "tremolo":
        return P.Tremolo(channels=3, config=E.tremolo_params(p, GFS))
    raise AssertionError(node["type"])


@pytest.mark.parametrize("node", [DIST_NODE, CHEB_NODE, CRUSH_NODE, {"id": "d", "type": "distortion"},
                                  {"id": "c", "type": "dist-cheb"}, {"id": "b", "type": "bitcrusher"}],
                         ids=["distortion", "dist-cheb", "bitcrusher", "distortion defaults", "dist-cheb defaults",
                              "bitcrusher defaults"])
def test_graph_node_is_the_processor(gpu, node):
    x = noise(1500, amplitude=0.9)
    ch, y = _chain_run(_graph([node]), x)
    kind = "bitcrusher" if node["type"] == "bitcrusher" else "distortion"
    assert ch.spec[1]["type"] == kind and ch.op_count()[0] == 1
    proc = _processor(node)
    assert ch.spec[1][kind] == fields(proc.config())
    same_bits(y, gpu_run(proc, x), node["type"])
    # and the restated node runtime, for the nodes that are bit-exact against it on their own
    p = _params(node)
    ref = R.NODES[node["type"]](p.Num, p.Str, GFS)
    assert fields(proc.config()) == R.config_of(ref)
    if isinstance(ref, R.BitCrusher):
        sync_q(proc, ref)
    same_bits(y, ref.process_many(x), f"{node['type']} against the restated node runtime")
    stateful = node["type"] == "bitcrusher" or bool(node.get("params", {}).get("dcBypass"))
    y2 = x.copy()
    assert ch.Process(y2)
    assert np.any(y2 != y) == stateful  # the counter, the hold values and the DC states carry over calls
    ch.Reset()
    y3 = x.copy()
    assert ch.Process(y3)
    same_bits(y3, y, f"{node['type']} after Chain.Reset")


def test_graph_chain_with_dry_edge_bypass_and_reset(gpu):
    """filter -> distortion -> bitcrusher -> tremolo with a dry edge to _output, each node bypassed in turn, Reset."""
    x = noise(2000, amplitude=0.9)
    nodes = [FILTER_NODE, DIST_NODE, CRUSH_NODE, TREMOLO_NODE]
    designer = design.RBJDesigner()
    ch, y = _chain_run(_graph(nodes, dry_edge=True), x, designer=designer)
    assert [s["type"] for s in ch.spec] == ["input", "biquad", "distortion", "bitcrusher", "tremolo", "output"]
    assert ch.spec[2]["distortion"]["mode"] == M["waveshaper3"] and ch.spec[3]["bitcrusher"]["downsample"] == 3
    secs, gain = ch.spec[1]["sections"]  # the filter node's designed chain, on a biquad.Chain of its own
    assert len(secs) >= 1

    def in_turn(ns, v):
        for nd in ns:
            if nd["type"].startswith("filter"):
                v = v.copy()
                P.Chain(np.asarray(secs), gain, channels=3).ProcessBlock(v)
            else:
                v = gpu_run(_processor(nd), v)
        return v

    want = (in_turn(nodes, x) + x) * 0.5  # edge order: tremolo, _input
    same_bits(y, want, "filter -> distortion -> bitcrusher -> tremolo, averaged with the dry edge")
    y2 = x.copy()
    assert ch.Process(y2) and np.any(y2 != y)
    ch.Reset()  # every node: the same output again
    y3 = x.copy()
    assert ch.Process(y3)
    same_bits(y3, y, "after Chain.Reset")
    for skip in range(len(nodes)):  # a bypassed node mixes only
        ns = [dict(nd, bypassed=(i == skip)) for i, nd in enumerate(nodes)]
        ch, y = _chain_run(_graph(ns), x, designer=designer)
        same_bits(y, in_turn([nd for i, nd in enumerate(nodes) if i != skip], x), f"bypassed {nodes[skip]['type']}")
    ch, y = _chain_run(_graph([dict(nd, bypassed=True) for nd in nodes]), x, designer=designer)
    same_bits(y, x, "everything bypassed")


def _three(node_type):
    par, par2 = (C.c_int32 * 1)(0), (C.c_int32 * 1)(1)
    nodes = (E._Node * 3)()
    nodes[0].type = E.FXN_INPUT
    nodes[1].type, nodes[1].n_parents, nodes[1].parents = node_type, 1, C.cast(par, C.POINTER(C.c_int32))
    nodes[2].type, nodes[2].n_parents, nodes[2].parents = E.FXN_OUTPUT, 1, C.cast(par2, C.POINTER(C.c_int32))
    return nodes, (par, par2)


def test_graph_node_without_config_is_refused(gpu):
    L = _lib.lib()
    BAD = _lib.AD_ERR_INVALID_ARGUMENT
    for t, kind, cfg_t, other_t in ((E.FXN_DISTORTION, "distortion", _lib.DistortionConfig, _lib.BitCrusherConfig),
                                    (E.FXN_BITCRUSHER, "bitcrusher", _lib.BitCrusherConfig, _lib.DistortionConfig)):
        nodes, _keep = _three(t)
        np_, h = C.cast(nodes, C.c_void_p), C.c_void_p()
        ext = (E._NodeExt * 3)()
        cfgs = (_lib.FxNodeCfg * 3)()
        cp = C.cast(cfgs, C.c_void_p)
        # no configuration at all, through the three entry points
        assert L.ad_fx_graph_create(np_, 3, 2, 0, C.byref(h)) == BAD and not h.value
        for e in (None, C.cast(ext, C.c_void_p)):
            assert L.ad_fx_graph_create_ext(np_, e, 3, 2, 0, C.byref(h)) == BAD and not h.value
            assert L.ad_fx_graph_create_cfg(np_, e, None, 3, 2, 0, C.byref(h)) == BAD and not h.value
            assert L.ad_fx_graph_create_cfg(np_, e, cp, 3, 2, 0, C.byref(h)) == BAD and not h.value
        good = cfg_t()
        getattr(L, f"ad_{kind}_default_config")(C.byref(good), 48000.0)
        # the wrong size: one byte off either way, 0, and the other node type's structure
        for nbytes in (C.sizeof(good) - 1, C.sizeof(good) + 1, 0, C.sizeof(other_t)):
            cfgs[1].config, cfgs[1].bytes = C.addressof(good), nbytes
            assert L.ad_fx_graph_create_cfg(np_, None, cp, 3, 2, 0, C.byref(h)) == BAD and not h.value
        cfgs[1].config, cfgs[1].bytes = None, C.sizeof(good)
        assert L.ad_fx_graph_create_cfg(np_, None, cp, 3, 2, 0, C.byref(h)) == BAD and not h.value
        # another node's slot does not serve
        cfgs[2].config, cfgs[2].bytes = C.addressof(good), C.sizeof(good)
        assert L.ad_fx_graph_create_cfg(np_, None, cp, 3, 2, 0, C.byref(h)) == BAD and not h.value
        # a configuration that fails validate, also on a bypassed node
        bad = cfg_t()
        C.memmove(C.byref(bad), C.byref(good), C.sizeof(good))
        bad.mix = 1.5
        cfgs[1].config, cfgs[1].bytes = C.addressof(bad), C.sizeof(bad)
        assert L.ad_fx_graph_create_cfg(np_, None, cp, 3, 2, 0, C.byref(h)) == BAD and not h.value
        nodes[1].bypassed = 1
        assert L.ad_fx_graph_create_cfg(np_, None, cp, 3, 2, 0, C.byref(h)) == BAD and not h.value
        nodes[1].bypassed = 0
        cfgs[1].config, cfgs[1].bytes = C.addressof(good), C.sizeof(good)
        assert L.ad_fx_graph_create_cfg(np_, None, cp, 3, 2, 0, C.byref(h)) == _lib.AD_OK and h.value
        L.ad_fx_graph_destroy(h)
    # 14 is still nobody's; with cfg NULL the new entry point is ad_fx_graph_create_ext
    nodes, _keep = _three(14)
    h = C.c_void_p()
    for rc in (L.ad_fx_graph_create(C.cast(nodes, C.c_void_p), 3, 2, 0, C.byref(h)),
               L.ad_fx_graph_create_ext(C.cast(nodes, C.c_void_p), None, 3, 2, 0, C.byref(h)),
               L.ad_fx_graph_create_cfg(C.cast(nodes, C.c_void_p), None, None, 3, 2, 0, C.byref(h)),
               L.ad_fx_graph_create_cfg(C.cast(nodes, C.c_void_p), None, cp, 3, 2, 0, C.byref(h))):
        assert rc == 10 and not h.value  # AD_ERR_UNKNOWN_EFFECT
    nodes, _keep = _three(17)
    assert L.ad_fx_graph_create_cfg(C.cast(nodes, C.c_void_p), None, cp, 3, 2, 0, C.byref(h)) == 10
    nodes, _keep = _three(E.FXN_PASS)
    assert L.ad_fx_graph_create_cfg(C.cast(nodes, C.c_void_p), None, None, 3, 2, 0, C.byref(h)) == _lib.AD_OK
    L.ad_fx_graph_destroy(h)


def test_unknown_effects_stay_unknown(gpu):
    for t in ("transformer", "widener", "bass", "chorus"):
        with pytest.raises(E.UnknownEffect):
            E.Chain(48000.0, 2).LoadGraph(_graph([{"id": "n", "type": t}]))
