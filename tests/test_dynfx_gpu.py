"""The GPU transient shaper and de-esser against the restatement in
tests/dynfx_ref.py.

The transient shaper, the de-esser's listen output and every envelope are
compared on float64 bits.  The de-esser's gain goes through the device math
library's log and exp2: the curve (ad_deesser_gain) is held to the bars for
device-library functions, and with that curve substituted into the restatement
the output and the metrics are compared on bits again.  End to end against the
pure restatement the output meets the same two bars, no sample excluded.

Shapes: N = 1501 in calls of [700, 1, 800] (the walk's tiles of 32 and 16
samples both end inside a call, a call of one sample, more than one pointwise
workgroup is covered by the denormal-tail row), channels 1, 3 and 65 (one past
a wave), distinct noise per channel at amplitude 2, 48 kHz.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import dynfx_ref as R
import layout_lib as LL
from algodsp import _lib, design, effectchain as E, processors as P, signals

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
RMS_BAR, ABS_BAR = 1e-12, 1e-10
FS = 48000.0
N, CUTS = 1501, [700, 1, 800]
CHANNELS = [1, 3, 65]
NAN, INF = float("nan"), float("inf")


def noise(n=N, channels=3, seed=0xDE5, amplitude=2.0):
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


def within_bars(got, want, what=""):
    err = np.asarray(got) - np.asarray(want)
    rms = math.sqrt(float(np.mean(err ** 2))) / max(math.sqrt(float(np.mean(np.asarray(want) ** 2))), 1e-300)
    worst = float(np.max(np.abs(err)))
    print(f"{what}: relative rms {rms:.3e}, max abs {worst:.3e}")
    assert rms <= RMS_BAR and worst <= ABS_BAR, (what, rms, worst)


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


def apply(obj, setup):
    for name, v in setup:
        getattr(obj, name)(v)
    return obj


# ---- transient shaper -------------------------------------------------------
def transient_case(x, setup, cuts=CUTS, what=""):
    """Output and the envelope after every call, every channel, on bits."""
    C_ = x.shape[0]
    refs = [apply(R.TransientShaper(FS), setup) for _ in range(C_)]
    h = apply(P.TransientShaper(FS, C_), setup)
    a, r = h.derived()
    same_bits([a, r], [refs[0].attackCoeff, refs[0].releaseCoeff], f"{what}: coefficients")
    got, want = x.copy(), x.copy()
    pos = 0
    for m in cuts:
        blk = got[:, pos:pos + m].copy()
        h.ProcessInPlace(blk)
        got[:, pos:pos + m] = blk
        for c in range(C_):
            want[c, pos:pos + m] = refs[c].ProcessInPlace(want[c, pos:pos + m].copy())
        same_bits([h.get_state(c) for c in range(C_)], [p.envelope for p in refs], f"{what}: envelope after {pos + m}")
        pos += m
    same_bits(got, want, what)
    return h, refs, got


TRANSIENT_SETUPS = {
    "defaults": [],
    "amounts +1": [("SetAttackAmount", 1.0), ("SetSustainAmount", 1.0)],
    "amounts -1": [("SetAttackAmount", -1.0), ("SetSustainAmount", -1.0)],
    "attack +1 sustain -1": [("SetAttackAmount", 1.0), ("SetSustainAmount", -1.0)],
    "times 0.1 / 1": [("SetAttackAmount", 0.6), ("SetSustainAmount", -0.4), ("SetAttack", 0.1), ("SetRelease", 1.0)],
    "times 0.1 / 2000": [("SetAttackAmount", 0.6), ("SetSustainAmount", -0.4), ("SetAttack", 0.1), ("SetRelease", 2000.0)],
    "times 200 / 1": [("SetAttackAmount", 0.6), ("SetSustainAmount", -0.4), ("SetAttack", 200.0), ("SetRelease", 1.0)],
    "times 200 / 2000": [("SetAttackAmount", 0.6), ("SetSustainAmount", -0.4), ("SetAttack", 200.0),
                         ("SetRelease", 2000.0)],
}


@pytest.mark.parametrize("channels", CHANNELS)
@pytest.mark.parametrize("name", list(TRANSIENT_SETUPS))
def test_transient_is_bit_exact(gpu, name, channels):
    if channels == 65 and name not in ("defaults", "times 0.1 / 1"):
        channels = 2  # the wide case once per kernel path; the other settings change constants only
    transient_case(noise(channels=channels), TRANSIENT_SETUPS[name], what=f"transient {name}, {channels} ch")


def edge_rows(channels=3):
    """Row 0 carries -0, 1e-320, +inf, -inf and NaN among its noise; the other rows must not notice."""
    x = noise(channels=channels)
    x[0, 5], x[0, 6], x[0, 40], x[0, 41] = -0.0, 1e-320, -0.0, 1e-320
    x[0, 720], x[0, 900], x[0, 1200] = INF, -INF, NAN
    return x


def test_transient_edge_inputs(gpu):
    h, refs, got = transient_case(edge_rows(), TRANSIENT_SETUPS["attack +1 sustain -1"], what="transient edge inputs")
    assert math.isnan(refs[0].envelope) and np.isnan(got[0, 1200:]).all() and np.isfinite(got[1:]).all()
    z = np.zeros((1, 64))
    z[0, ::2] = -0.0
    transient_case(z, TRANSIENT_SETUPS["amounts +1"], cuts=[64], what="signed zeros")


def test_transient_denormal_tail(gpu):
    """A burst, then 65536 zeros at the shortest release: the envelope decays down into the subnormals."""
    x = np.zeros((1, 64 + 65536))
    x[0, :64] = signals.white_noise(64, 0xB0) * 1.5
    h, refs, got = transient_case(x, [("SetSustainAmount", -1.0), ("SetAttackAmount", 1.0), ("SetRelease", 1.0)],
                                  cuts=[x.shape[1]], what="denormal tail")
    env = []
    p = apply(R.TransientShaper(FS), [("SetRelease", 1.0)])
    for v in x[0]:
        p.ProcessSample(float(v))
        env.append(p.envelope)
    env = np.asarray(env)
    # it did go down into them; it stalls at the subnormal where coeff * env rounds to nothing
    assert np.count_nonzero((env > 0) & (env < 2.2250738585072014e-308)) > 1000 and env[-1] == env[-2] < 1e-300


def test_transient_reset_and_state_round_trip(gpu):
    x = noise()
    setup = TRANSIENT_SETUPS["attack +1 sustain -1"]
    h = apply(P.TransientShaper(FS, 3), setup)
    first = gpu_run(h, x)
    assert h.get_state(1) > 0
    h.Reset()
    assert [h.get_state(c) for c in range(3)] == [0.0, 0.0, 0.0]
    same_bits(gpu_run(h, x), first, "after Reset")
    # a stream migrates: the envelope of one handle continues on another
    a, b = apply(P.TransientShaper(FS, 3), setup), apply(P.TransientShaper(FS, 3), setup)
    head = gpu_run(a, x[:, :700])
    for c in range(3):
        b.set_state(c, a.get_state(c))
    tail = gpu_run(b, x[:, 700:])
    same_bits(np.concatenate([head, tail], axis=1), first, "state moved to a second handle")
    for bad in (-1, 3):
        with pytest.raises(_lib.ErrInvalidArgument):
            h.get_state(bad)
    assert h.kernel_info() == (64, 32, 2 * 64 * 33 * 8)


def test_transient_setters(gpu):
    """A refused value changes nothing; an accepted one takes effect and keeps the envelope."""
    x = noise()
    h = P.TransientShaper(FS, 3)
    gpu_run(h, x[:, :700])
    env = h.get_state(2)
    before = bytes(h.config())
    for name, v in (("SetAttackAmount", 1.5), ("SetSustainAmount", NAN), ("SetAttack", 0.05), ("SetRelease", 2001.0),
                    ("SetSampleRate", 0.0), ("SetAttackCoeff", 0.0), ("SetReleaseCoeff", 1.5)):
        with pytest.raises(_lib.ErrInvalidArgument):
            getattr(h, name)(v)
    assert bytes(h.config()) == before and h.get_state(2) == env
    ref = R.TransientShaper(FS)
    for obj in (h, ref):
        apply(obj, [("SetAttackAmount", 0.5), ("SetSustainAmount", -0.5), ("SetAttack", 2.0), ("SetRelease", 30.0),
                    ("SetSampleRate", 44100.0)])
    assert h.get_state(2) == env
    same_bits(h.derived(), [ref.attackCoeff, ref.releaseCoeff], "coefficients after the setters")
    ref.envelope = env
    same_bits(gpu_run(h, x[:, 700:])[2], ref.ProcessInPlace(x[2, 700:].copy()), "after the setters")
    h.SetAttackCoeff(0.25)  # a caller's own coefficient is used as it is ...
    assert h.derived()[0] == 0.25 and h.config().attack_coeff == 0.25
    h.SetAttack(2.0)  # ... until a setter derives both again
    same_bits(h.derived(), [ref.attackCoeff, ref.releaseCoeff], "derived again")


# ---- de-esser ---------------------------------------------------------------
def deesser_case(x, setup, cuts=CUTS, actions=None, what="", check_clamp=False):
    """Runs the pure restatement, the restatement with the device's curve substituted, and the GPU handle in
    lockstep over the calls; `actions[i]` (setter list) is applied to all three before call i.  Checks the
    envelope, the cascade states and the metrics after every call and the output on bits given the curve;
    returns (got, pure, handle, curve restatements)."""
    C_ = x.shape[0]
    actions = actions or {}
    pure = [apply(R.DeEsser(FS), setup) for _ in range(C_)]
    curve = [apply(R.DeEsser(FS), setup) for _ in range(C_)]
    h = apply(P.DeEsser(FS, C_), setup)
    got, want_pure, want_curve = x.copy(), x.copy(), x.copy()
    pos = 0
    for i, m in enumerate(cuts):
        for obj in pure + curve + [h]:
            apply(obj, actions.get(i, []))
        levels = []
        for c in range(C_):
            pure[c].trace = []
            want_pure[c, pos:pos + m] = pure[c].ProcessInPlace(want_pure[c, pos:pos + m].copy())
            levels.append(np.asarray(pure[c].trace, dtype=np.float64))
        gains = h.gain(np.concatenate(levels)) if sum(v.size for v in levels) else np.zeros(0)
        at = 0
        for c in range(C_):
            it = iter(gains[at:at + levels[c].size].tolist())
            at += levels[c].size
            curve[c].gain_fn = lambda env, it=it: next(it)
            want_curve[c, pos:pos + m] = curve[c].ProcessInPlace(want_curve[c, pos:pos + m].copy())
        blk = got[:, pos:pos + m].copy()
        h.ProcessInPlace(blk)
        got[:, pos:pos + m] = blk
        for c in range(C_):
            env, det, band = h.get_state(c)
            where = f"{what}: channel {c} after {pos + m}"
            same_bits(env, curve[c].envLevel, f"{where}: envelope")
            same_bits(env, pure[c].envLevel, f"{where}: envelope (pure)")
            rd, rb = curve[c].states()
            same_bits(det, rd, f"{where}: detect states")
            same_bits(band, rb, f"{where}: band states")
            same_bits(h.GetMetrics(c), curve[c].GetMetrics(), f"{where}: metrics")
        pos += m
    same_bits(got, want_curve, f"{what}: given the curve")
    if check_clamp:
        kept, replaced = (sum(p.clamped[k] for p in curve) for k in (0, 1))
        assert kept > 0 and replaced > 0, (what, kept, replaced)  # both sides of the clamp :467 were taken
    return got, want_pure, h, curve


def test_deesser_listen_is_the_bare_cascade(gpu):
    for channels in CHANNELS:
        for detector in (0, 1):
            for order in (1, 2, 3, 4):
                if channels == 65 and (detector, order) not in ((0, 2), (1, 4)):
                    continue
                x = noise(channels=channels)
                setup = [("SetDetector", detector), ("SetFilterOrder", order), ("SetListen", True)]
                got, pure, h, refs = deesser_case(x, setup, what=f"listen det {detector} order {order} {channels} ch")
                same_bits(got, pure, "listen: the pure restatement, no curve involved")
                assert h.GetMetrics(0) == (0.0, 1.0) and h.get_state(0)[0] == 0.0  # nothing else is touched


MODES = {"split": R.SPLIT_BAND, "wide": R.WIDEBAND}


@pytest.mark.parametrize("channels", CHANNELS)
@pytest.mark.parametrize("mode", list(MODES))
def test_deesser_defaults(gpu, mode, channels):
    x = noise(channels=channels)
    got, pure, h, refs = deesser_case(x, [("SetMode", MODES[mode])], what=f"{mode} defaults {channels} ch",
                                      check_clamp=mode == "split")
    within_bars(got, pure, f"{mode} defaults {channels} ch, end to end")
    assert h.kernel_info()[3] == 1


@pytest.mark.parametrize("q", [0.1, 10.0])
@pytest.mark.parametrize("order", [1, 2, 3, 4])
@pytest.mark.parametrize("detector", [0, 1])
def test_deesser_detectors_orders_and_q(gpu, detector, order, q):
    x = noise(channels=3)
    # a bandpass section at q 0.1 passes a tenth of the level: the threshold goes down with it, so that the gain moves
    threshold = -30.0 - 20.0 * order if (detector == 0 and q < 1) else -30.0
    setup = [("SetDetector", detector), ("SetFilterOrder", order), ("SetQ", q), ("SetThreshold", threshold)]
    for mode in MODES:
        got, pure, h, refs = deesser_case(x, setup + [("SetMode", MODES[mode])],
                                          what=f"{mode} det {detector} order {order} q {q}", check_clamp=mode == "split")
        within_bars(got, pure, f"{mode} det {detector} order {order} q {q}, end to end")


GAIN_SETUPS = {
    "soft knee": [],
    "hard knee": [("SetKnee", 0.0)],
    "ratio 1": [("SetRatio", 1.0)],
    "ratio 100": [("SetRatio", 100.0), ("SetKnee", 12.0)],
    "range 0": [("SetRange", 0.0)],
    "range -60": [("SetRange", -60.0), ("SetRatio", 100.0), ("SetThreshold", -60.0)],
}


@pytest.mark.parametrize("name", list(GAIN_SETUPS))
def test_deesser_gain_curve(gpu, name):
    """ad_deesser_gain against the restatement's calculateGain: noise-derived levels and 20001 levels from 1e-6 to 4."""
    ref = apply(R.DeEsser(FS), GAIN_SETUPS[name])
    h = apply(P.DeEsser(FS, 1), GAIN_SETUPS[name])
    ref.trace = []
    ref.ProcessInPlace(noise(channels=1)[0])
    levels = np.concatenate([np.asarray(ref.trace), np.geomspace(1e-6, 4.0, 20001),
                             [0.0, -0.0, -1.0, 2.0 ** ref.thresholdLog2, 5e-324, 1e308]])
    want = np.asarray([ref.calculateGain(float(v)) for v in levels])
    got = h.gain(levels)
    within_bars(got, want, f"gain curve, {name}")
    assert np.all(got <= 1.0) and np.all(got >= ref.rangeLin)
    # +inf gives the floor, except at ratio 1 where -inf * 0 is NaN in the reference too
    same_bits(h.gain([NAN, INF, 0.0]), [ref.calculateGain(v) for v in (NAN, INF, 0.0)], "NaN, +inf and 0")
    assert math.isnan(ref.calculateGain(INF)) == (name == "ratio 1")
    if name == "ratio 1":
        assert np.all(got == 1.0)
    if name == "range -60":
        assert got.min() == ref.rangeLin == 0.001


def test_deesser_divergent_cascades(gpu):
    """Listen for one call, then off: detectFilters moved alone, so the split-band calls after it walk both
    cascades, and are still the reference's.  The same after a wideband call."""
    x = noise(channels=3)
    for breaker, back in (([("SetListen", True)], [("SetListen", False)]),
                          ([("SetMode", R.WIDEBAND)], [("SetMode", R.SPLIT_BAND)])):
        cuts = [300, 16, 1, 384, 800]
        h = P.DeEsser(FS, 3)
        assert h.kernel_info() == (64, 16, 2 * 2 * 64 * 17 * 8, 1)
        got, pure, h, refs = deesser_case(x, [], cuts=cuts, actions={1: breaker, 2: back},
                                          what=f"divergent after {breaker[0][0]}", check_clamp=True)
        assert h.kernel_info()[3] == 2
        det, band = refs[0].states()
        within_bars(got, pure, "divergent, end to end")
        # in the restatement the band cascade really was elsewhere after the lone call
        twin = R.DeEsser(FS)
        twin.ProcessInPlace(x[0, :300].copy())
        apply(twin, breaker)
        twin.ProcessInPlace(x[0, 300:316].copy())
        d2, b2 = twin.states()
        assert not np.array_equal(bits(d2), bits(b2))
        h.SetQ(1.5)  # a rebuild makes them equal again
        assert h.kernel_info()[3] == 1
        h.SetListen(True)
        assert h.kernel_info()[2:] == (2 * 64 * 33 * 8, 1)


def test_deesser_rebuild_setters_between_calls(gpu):
    """States zeroed, envelope and metrics kept (checked inside deesser_case after every call)."""
    x = noise(channels=3)
    actions = {1: [("SetFrequency", 7000.0)], 2: [("SetQ", 3.0)], 3: [("SetDetector", 1)], 4: [("SetFilterOrder", 4)],
               5: [("SetDetector", 1)], 6: [("SetThreshold", -35.0), ("SetRatio", 10.0), ("SetKnee", 0.0)],
               7: [("SetAttack", 2.0), ("SetRelease", 5.0), ("SetRange", -6.0)], 8: [("SetFilterOrder", 1)]}
    got, pure, h, refs = deesser_case(x, [], cuts=[200, 100, 150, 151, 100, 200, 200, 200, 200], actions=actions,
                                      what="rebuild setters")
    within_bars(got, pure, "rebuild setters, end to end")
    env = h.get_state(1)[0]
    met = h.GetMetrics(1)
    h.SetSampleRate(44100.0)
    e2, det, band = h.get_state(1)
    assert e2 == env and not det.any() and not band.any() and h.GetMetrics(1) == met
    before = bytes(h.config())
    for name, v in (("SetSampleRate", 12000.0), ("SetFrequency", 22050.0), ("SetFrequency", 999.0), ("SetQ", 11.0),
                    ("SetThreshold", NAN), ("SetRatio", 0.5), ("SetKnee", 13.0), ("SetAttack", 0.001),
                    ("SetRelease", 501.0), ("SetRange", 1.0), ("SetMode", 2), ("SetDetector", -1), ("SetFilterOrder", 5),
                    ("SetFilterOrder", 2.5), ("SetAttackCoeff", 0.0)):
        with pytest.raises(_lib.ErrInvalidArgument):
            getattr(h, name)(v)
    assert bytes(h.config()) == before


def test_deesser_metrics_reset_and_state_round_trip(gpu):
    x = noise(channels=3)
    got, pure, h, refs = deesser_case(x, [("SetThreshold", -30.0)], what="metrics")
    assert h.GetMetrics(2)[0] > 0 and h.GetMetrics(2)[1] < 1.0
    env = h.get_state(2)[0]
    h.ResetMetrics()
    assert [h.GetMetrics(c) for c in range(3)] == [(0.0, 1.0)] * 3 and h.get_state(2)[0] == env
    # a stream migrates to a second handle
    a, b = apply(P.DeEsser(FS, 3), [("SetThreshold", -30.0)]), apply(P.DeEsser(FS, 3), [("SetThreshold", -30.0)])
    head = gpu_run(a, x[:, :700])
    for c in range(3):
        b.set_state(c, *a.get_state(c))
    assert b.kernel_info()[3] == 1  # equal cascades came in
    same_bits(np.concatenate([head, gpu_run(b, x[:, 700:])], axis=1), got, "state moved to a second handle")
    e, det, band = b.get_state(0)
    b.set_state(0, e, det, band * 0.5)
    assert b.kernel_info()[3] == 2
    h.Reset()
    for c in range(3):
        e, det, band = h.get_state(c)
        assert e == 0.0 and not det.any() and not band.any() and h.GetMetrics(c) == (0.0, 1.0)
    same_bits(gpu_run(h, x, CUTS), got, "after Reset")


def test_deesser_edge_inputs(gpu):
    for mode in MODES:
        got, pure, h, refs = deesser_case(edge_rows(), [("SetMode", MODES[mode])], what=f"{mode} edge inputs")
        assert np.isnan(got[0, 1201:]).all() and np.isfinite(got[1:]).all()
        within_bars(got[1:], pure[1:], f"{mode}: the rows next to the non-finite one")
    got, pure, h, refs = deesser_case(edge_rows(), [("SetListen", True)], what="listen edge inputs")
    same_bits(got, pure, "listen edge inputs")
    # a NaN gain while GainReduction is still exactly 1 (:442): it becomes NaN and stays
    x = np.zeros((2, 40))
    x[0, 20] = NAN
    x[1, 20] = 1.0
    got, pure, h, refs = deesser_case(x, [], cuts=[30, 10], what="NaN into fresh metrics")
    assert math.isnan(h.GetMetrics(0)[1]) and not math.isnan(h.GetMetrics(1)[1])


# ---- layouts and streams ----------------------------------------------------
MAKERS = {
    "transient": lambda: apply(P.TransientShaper(FS, 3), TRANSIENT_SETUPS["attack +1 sustain -1"]),
    "deesser split": lambda: P.DeEsser(FS, 3),
    "deesser wide": lambda: apply(P.DeEsser(FS, 3), [("SetMode", R.WIDEBAND), ("SetFilterOrder", 4)]),
    "deesser listen": lambda: apply(P.DeEsser(FS, 3), [("SetListen", True), ("SetDetector", 1)]),
}


@pytest.mark.parametrize("kind", list(MAKERS))
def test_process_device_layouts(gpu, kind):
    """Row strides greater than n and rows 8 bytes off 16-byte alignment give the bits of the aligned
    contiguous placement, and touch nothing around the rows."""
    n = N
    x = noise(n)

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
    x = noise(n)
    want = gpu_run(MAKERS[kind](), x)
    for layout in [LL.LA(n)] + LL.variants(n):
        b = LL.place(x, layout, DEV)
        torch.cuda.synchronize()
        MAKERS[kind]().process_device(b.ptr, b.stride, n)
        torch.cuda.synchronize()
        LL.check_guards(b)
        same_bits(LL.payload(b), want, f"{kind}, {n} samples {layout}")


@pytest.mark.parametrize("kind", list(MAKERS))
def test_two_streams_alternate_with_a_second_handle(gpu, kind):
    """Calls alternate between the NULL stream and a side stream (and one host-buffer call) while a second
    handle works on its own buffer on the same streams: the state of each is its own and every call of a handle
    waits for the one before, so each result is one sequential processor's."""
    C_, n = 3, 4000
    x, x2 = noise(n, C_), noise(n, C_, seed=0xABC)
    want, want2 = gpu_run(MAKERS[kind](), x), gpu_run(MAKERS[kind](), x2)
    h, h2 = MAKERS[kind](), MAKERS[kind]()
    d, d2 = torch.from_numpy(x).to(DEV), torch.from_numpy(x2).to(DEV)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    host = None
    for i, t0 in enumerate(range(0, n, 500)):
        if i == 5:
            torch.cuda.synchronize()
            host = d[:, t0:t0 + 500].cpu().numpy().copy()
            h.ProcessInPlace(host)
        else:
            h.process_device(d.data_ptr() + 8 * t0, n, 500, side.cuda_stream if i % 2 else 0)
        h2.process_device(d2.data_ptr() + 8 * t0, n, 500, 0 if i % 2 else side.cuda_stream)
    torch.cuda.synchronize()
    got = d.cpu().numpy()
    got[:, 2500:3000] = host
    same_bits(got, want, f"{kind} on two streams")
    same_bits(d2.cpu().numpy(), want2, f"{kind}: the second handle")
    h.process_device(d.data_ptr(), n, 700, side.cuda_stream)
    h.Reset()  # ordered after the side stream's call
    torch.cuda.synchronize()


WIDE_MAKERS = {
    "transient": (32768, lambda c: apply(P.TransientShaper(FS, c), TRANSIENT_SETUPS["attack +1 sustain -1"])),
    "deesser split": (16384, lambda c: P.DeEsser(FS, c)),
    "deesser wide": (16384, lambda c: apply(P.DeEsser(FS, c), [("SetMode", R.WIDEBAND)])),
}


@pytest.mark.parametrize("kind", list(WIDE_MAKERS))
def test_calls_longer_than_one_scratch_pass(gpu, kind):
    """The scratch rows of one pass are bounded (256 MiB), so at this many channels a call of 1501 samples is
    cut along time into passes of 1024 and 477 samples.  Three distinct rows repeat down the channels (the
    buffer stays on the device); every row must carry the bits a 3-channel handle gives in one pass."""
    channels, make = WIDE_MAKERS[kind]
    x3 = noise(N, 3)
    small = make(3)
    want = torch.from_numpy(gpu_run(small, x3)).to(DEV)
    reps = channels // 3 + 1
    d = torch.from_numpy(x3).to(DEV).repeat(reps, 1)[:channels].contiguous()
    h = make(channels)
    torch.cuda.synchronize()
    h.process_device(d.data_ptr(), N, N)
    torch.cuda.synchronize()
    assert torch.equal(d.view(torch.int64), want.repeat(reps, 1)[:channels].view(torch.int64))
    for c in (0, 4097, channels - 1):
        if kind == "transient":
            same_bits(h.get_state(c), small.get_state(c % 3), f"{kind}: envelope of channel {c}")
        else:
            same_bits(h.get_state(c)[0], small.get_state(c % 3)[0], f"{kind}: envelope of channel {c}")
            same_bits(h.GetMetrics(c), small.GetMetrics(c % 3), f"{kind}: metrics of channel {c}")
    h.close()
    del d, want
    torch.cuda.empty_cache()


# ---- graph ------------------------------------------------------------------
DEESS_NODE ={"id": "de", "type": "dyn-deesser", "params": {"threshold": -20.0, "freq": 6000.0, "ratio": 4.0,
                                                            "mode": "splitband", "detector": "bandpass"}}
TRANS_NODE = {"id": "tr", "type": "dyn-transient", "params": {"attack": 0.5, "sustain": 0.5}}  # integration_test.go:40-41
FILTER_NODE = {"id": "eq", "type": "filter-peak", "params": {"freq": 5000, "gain": 4, "q": 2}}
COMP_NODE = {"id": "co", "type": "dyn-compressor", "params": {"thresholdDB": -20, "ratio": 4}}
DEESS_WIDE = {"id": "dw", "type": "dyn-deesser", "params": {"thresholdDB": -30, "freqHz": 7000, "mode": "wideband",
                                                            "detector": "highpass", "filterOrder": 3.4}}


def _graph(nodes, dry_edge=False):
    ids = [E.INPUT_NODE_ID] + [n["id"] for n in nodes] + [E.OUTPUT_NODE_ID]
    edges = list(zip(ids[:-1], ids[1:]))
    if dry_edge:
        edges.append((E.INPUT_NODE_ID, E.OUTPUT_NODE_ID))
    return E._graph_json(nodes, edges)


def _chain_run(graph, x, designer=None):
    ch = E.Chain(FS, x.shape[0], designer=designer)
    ch.LoadGraph(graph)
    y = x.copy()
    assert ch.Process(y)
    return ch, y


def _params(node):
    raw = node.get("params", {})
    return E.Params(node["id"], node["type"], num={k: float(v) for k, v in raw.items() if not isinstance(v, str)},
                    str_={k: v for k, v in raw.items() if isinstance(v, str)})


def _processor(node, channels=3):
    if node["type"] == "dyn-deesser":
        return P.DeEsser(channels=channels, config=E.deesser_params(_params(node), FS))
    return P.TransientShaper(channels=channels, config=E.transient_params(_params(node), FS))


def fields(cfg):
    return {f: getattr(cfg, f) for f, _ in cfg._fields_}


@pytest.mark.parametrize("node", [DEESS_NODE, TRANS_NODE, DEESS_WIDE], ids=["dyn-deesser", "dyn-transient", "wideband"])
def test_graph_node_is_the_processor(gpu, node):
    x = noise()
    ch, y = _chain_run(_graph([node]), x)
    kind = "deesser" if node["type"] == "dyn-deesser" else "transient"
    assert ch.spec[1]["type"] == kind and ch.op_count()[0] == 1
    proc = _processor(node)
    spec = dict(ch.spec[1][kind])
    have = fields(proc.config())
    for f in ("attack_coeff", "release_coeff"):  # the spec carries 0 (derive), the handle the derived ones
        assert spec.pop(f) == 0.0 and have.pop(f) > 0
    assert spec == have
    if node is DEESS_WIDE:
        assert (have["mode"], have["detector"], have["filter_order"], have["freq_hz"]) == (1, 1, 3, 7000.0)
    same_bits(y, gpu_run(proc, x), node["type"])
    y2 = x.copy()
    assert ch.Process(y2) and np.any(y2 != y)  # the envelope carries over
    ch.Reset()
    y3 = x.copy()
    assert ch.Process(y3)
    same_bits(y3, y, f"{node['type']} after Chain.Reset")


def test_graph_vocal_chain_split_and_bypass(gpu):
    """filter -> dyn-deesser -> dyn-compressor; the two nodes on parallel branches; bypassed nodes; Reset."""
    x = noise()
    designer = design.RBJDesigner()
    nodes = [FILTER_NODE, DEESS_NODE, COMP_NODE]
    ch, y = _chain_run(_graph(nodes), x, designer=designer)
    assert [s["type"] for s in ch.spec] == ["input", "biquad", "deesser", "comp", "output"]
    secs, gain = ch.spec[1]["sections"]
    comp = {k: v for k, v in ch.spec[3]["comp"].items() if k != "sample_rate"}

    def in_turn(ns, v):
        for nd in ns:
            v = v.copy()
            if nd["type"].startswith("filter"):
                P.Chain(np.asarray(secs), gain, channels=3).ProcessBlock(v)
            elif nd["type"] == "dyn-compressor":
                P.Compressor(FS, 3, **comp).ProcessInPlace(v)
            else:
                v = gpu_run(_processor(nd), v)
        return v

    same_bits(y, in_turn(nodes, x), "filter -> dyn-deesser -> dyn-compressor")
    ch.Reset()
    y2 = x.copy()
    assert ch.Process(y2)
    same_bits(y2, y, "after Chain.Reset")
    for skip in range(len(nodes)):
        ns = [dict(nd, bypassed=(i == skip)) for i, nd in enumerate(nodes)]
        _c, yb = _chain_run(_graph(ns), x, designer=designer)
        rest = [nd for i, nd in enumerate(nodes) if i != skip]
        if nodes[skip] is DEESS_NODE:
            # filter -> compressor then fuse into one launch, whose engine is not the lone compressor's to the
            # bit: a bypassed node only mixes, so the graph without it is the reference
            _c, want = _chain_run(_graph(rest), x, designer=designer)
        else:
            want = in_turn(rest, x)
        same_bits(yb, want, f"bypassed {nodes[skip]['type']}")
    # a split: the two nodes on parallel branches, averaged at the output in edge order
    graph = E._graph_json([DEESS_NODE, TRANS_NODE],
                          [(E.INPUT_NODE_ID, "de"), (E.INPUT_NODE_ID, "tr"), ("de", E.OUTPUT_NODE_ID),
                           ("tr", E.OUTPUT_NODE_ID)])
    ch, y = _chain_run(graph, x)
    want = (gpu_run(_processor(DEESS_NODE), x) + gpu_run(_processor(TRANS_NODE), x)) * 0.5
    same_bits(y, want, "de-esser and transient shaper on parallel branches")
    assert ch.op_count()[2] >= 2  # they run on streams of their own
    _c, yb = _chain_run(_graph([dict(DEESS_NODE, bypassed=True), dict(TRANS_NODE, bypassed=True)]), x)
    same_bits(yb, x, "both bypassed")


def test_graph_refusals_on_the_device(gpu):
    L = _lib.lib()
    for t, make in ((E.FXN_DEESSER, _lib.DeEsserConfig), (E.FXN_TRANSIENT, _lib.TransientConfig)):
        par, par2 = (C.c_int32 * 1)(0), (C.c_int32 * 1)(1)
        nodes = (E._Node * 3)()
        nodes[0].type = E.FXN_INPUT
        nodes[1].type, nodes[1].n_parents, nodes[1].parents = t, 1, C.cast(par, C.POINTER(C.c_int32))
        nodes[2].type, nodes[2].n_parents, nodes[2].parents = E.FXN_OUTPUT, 1, C.cast(par2, C.POINTER(C.c_int32))
        np_ = C.cast(nodes, C.c_void_p)
        cfgs = (_lib.FxNodeCfg * 3)()
        cp = C.cast(cfgs, C.c_void_p)
        h = C.c_void_p()
        bad = _lib.AD_ERR_INVALID_ARGUMENT
        assert L.ad_fx_graph_create(np_, 3, 2, 0, C.byref(h)) == bad and not h.value
        assert L.ad_fx_graph_create_ext(np_, None, 3, 2, 0, C.byref(h)) == bad and not h.value
        assert L.ad_fx_graph_create_cfg(np_, None, None, 3, 2, 0, C.byref(h)) == bad and not h.value
        assert L.ad_fx_graph_create_cfg(np_, None, cp, 3, 2, 0, C.byref(h)) == bad and not h.value
        cfg = make()
        getattr(L, "ad_deesser_default_config" if t == E.FXN_DEESSER else "ad_transient_default_config")(C.byref(cfg), FS)
        cfgs[1].config, cfgs[1].bytes = C.addressof(cfg), C.sizeof(cfg) - 4
        assert L.ad_fx_graph_create_cfg(np_, None, cp, 3, 2, 0, C.byref(h)) == bad and not h.value
        cfgs[1].bytes = C.sizeof(cfg)
        cfg.release_ms = 0.0
        assert L.ad_fx_graph_create_cfg(np_, None, cp, 3, 2, 0, C.byref(h)) == bad and not h.value
        cfg.release_ms = 20.0
        assert L.ad_fx_graph_create_cfg(np_, None, cp, 3, 2, 0, C.byref(h)) == _lib.AD_OK and h.value
        L.ad_fx_graph_destroy(h)
    with pytest.raises(_lib.ErrInvalidArgument):  # NewDeEsser(12 kHz) carries 6000 Hz when SetSampleRate runs
        E.Chain(12000.0, 2).LoadGraph(_graph([dict(DEESS_NODE, params={"freqHz": 1000})]))
    with pytest.raises(E.UnknownEffect):
        E.Chain(FS, 2).LoadGraph(_graph([{"id": "m", "type": "dyn-multiband"}]))
