"""effects.Delay, the graph's delay-simple and modulation.Flanger on the GPU
(processors.Delay / Flanger, the effect graph's delay, delay-simple and flanger
nodes) against the restated reference (tests/delayfx_ref.py), per channel, with
distinct noise per channel.

Bars.  The delay, delay-simple and the flanger with depth 0 (the modulation
term is exactly 0) are compared on the float64 bits.  The modulated flanger
differs from the oracle by the device math library's sine only: relative RMS
<= 1e-12 and max abs <= 1e-10, the FDN reverb's bars for the same cause.
test_delayfx_ref.py::test_flanger_sine_spread measured, on the CPU, what a
last-place change of every sine does to these very cases: 3.0e-15 relative RMS
and 2.8e-14 absolute at the defaults, 5.5e-14 and 3.7e-13 at rate 5 Hz, depth
0.0089, feedback 0.7; four times that is inside the bars, so the feedback of
that case was not lowered."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import delayfx_ref as R
import layout_lib as LL
from algodsp import _lib, effectchain as E, processors as P, signals

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
RMS_BAR, ABS_BAR = 1e-12, 1e-10


def noise(n, channels=3, seed=0xDE1A):
    return np.stack([signals.white_noise(n, seed + c) for c in range(channels)])


def compare(got, want, exact=True, what=""):
    with np.errstate(all="ignore"):  # the delay-simple inputs carry inf and NaN
        err = float(np.sqrt(np.mean((got - want) ** 2)) / max(np.sqrt(np.mean(want ** 2)), 1e-300))
        mx = float(np.max(np.abs(got - want))) if got.size else 0.0
    print(f"{what}: rel rms {err:.3g}, max abs {mx:.3g}, differing samples {int(np.sum(got != want))}")
    if exact:
        np.testing.assert_array_equal(np.ascontiguousarray(got).view(np.int64), np.ascontiguousarray(want).view(np.int64))
    else:
        assert err <= RMS_BAR and mx <= ABS_BAR


def cut(n, cuts):
    """`cuts`, then the rest of n."""
    assert sum(cuts) < n
    return list(cuts) + [n - sum(cuts)]


def run_cuts(h, refs, x, cuts, exact=True, what="", after_call=None):
    """The GPU handle and the oracles over the same calls; `after_call` compares their state after each."""
    pos = 0
    for m in cuts:
        blk = np.ascontiguousarray(x[:, pos:pos + m])
        want = np.stack([r.process(blk[c]) for c, r in enumerate(refs)]) if m else blk.copy()
        h.ProcessInPlace(blk)
        for c in range(len(refs) if m else 0):  # an empty call has nothing to compare
            compare(blk[c], want[c], exact, f"{what} [{pos}, {pos + m}) channel {c}")
        if after_call:
            after_call()
        pos += m
    assert pos == x.shape[1]


def gpu_run(h, x, cuts=None):
    y = x.copy()
    pos = 0
    for m in cuts or [x.shape[1]]:
        blk = np.ascontiguousarray(y[:, pos:pos + m])
        h.ProcessInPlace(blk)
        y[:, pos:pos + m] = blk
        pos += m
    return y


# ---- the delay --------------------------------------------------------------
def sync_coeff(h, refs):
    """The handle derives the coefficient with the C library's exp, Python with the same one."""
    k = h.config().smooth_coeff
    for r in refs:
        assert math.nextafter(r.smoothCoeff, 0.0) <= k <= math.nextafter(r.smoothCoeff, 1.0)
        r.smoothCoeff = k


def dapply(h, refs, name, value=None):
    for o in [h] + list(refs):
        getattr(o, name)(*(() if value is None else (value,)))
    sync_coeff(h, refs)


def dpair(fs, channels=3, sets=(), regime=0):
    h = P.Delay(fs, channels)
    h.set_regime(regime)
    refs = [R.Delay(fs) for _ in range(channels)]
    sync_coeff(h, refs)
    for name, v in sets:
        dapply(h, refs, name, v)
    return h, refs


def dstate(h, refs):
    def check():
        cur, tgt, ln, wp = h.derived()
        for r in refs:
            assert (cur, tgt, ln, wp) == (r.currentSamples, r.targetSamples, len(r.buffer), r.write)
    return check


# (sample rate, time, feedback, mix, n): c = round(time * fs) = 0, 1, 2, 8 (blocks of 1 and 7), 48, 130
# (crosses a wave, no multiple of 64) at rings of 801 and 2001 samples, which n wraps more than twice
STATIC = [(400.0, 0.001, 0.35, 0.25, 2000), (1000.0, 0.001, 0.99, 1.0, 4500), (1000.0, 0.002, 0.0, 0.25, 4500),
          (1000.0, 0.008, 0.35, 0.0, 4500), (1000.0, 0.048, 0.99, 0.25, 4500), (1000.0, 0.130, 0.35, 1.0, 4500),
          (1000.0, 2.0, 0.99, 0.25, 4500)]


@pytest.mark.parametrize("regime", [1, 2])
@pytest.mark.parametrize("fs,time,feedback,mix,n", STATIC)
def test_delay_static_is_bit_exact(gpu, fs, time, feedback, mix, n, regime):
    h, refs = dpair(fs, 3, [("SetTime", time), ("SetFeedback", feedback), ("SetMix", mix)], regime)
    c = refs[0].currentSamples
    assert c == R.go_round(time * fs) and h.kernel_info()[0] == refs[0].block_bounds()[1]
    run_cuts(h, refs, noise(n), cut(n, [1, 63, 64, 65, 1031]), True, f"c {c} regime {regime}", dstate(h, refs))
    assert h.kernel_info()[2] == regime


def test_delay_default_ring_wraps_twice(gpu):
    """fs 8000: c = 2000, a ring of 16001, 40000 samples; the library picks regime 1 (block 1999)."""
    h, refs = dpair(8000.0, 3)
    assert h.derived() == (2000.0, 2000.0, 16001, 0) and h.kernel_info()[:2] == (1999, 64)
    n = 40000
    run_cuts(h, refs, noise(n), cut(n, [1, 63, 64, 65, 4097]), True, "default", dstate(h, refs))
    assert h.kernel_info()[2:] == (1, 18)  # the last call: 35710 samples in blocks of 1999
    assert h.derived()[3] == 40000 % 16001


def test_delay_picks_the_regime_from_block_and_length(gpu):
    h, refs = dpair(8000.0, 1, [("SetTime", 0.01)])
    x = noise(400, 1)
    run_cuts(h, refs, x, [79, 80, 241])  # block 79: one launch, then the persistent kernel
    assert h.kernel_info() == (79, 64, 2, 1)
    h2, _ = dpair(8000.0, 1, [("SetTime", 0.01)])
    h2.ProcessInPlace(x[:, :79].copy())
    assert h2.kernel_info()[2:] == (1, 1)


@pytest.mark.parametrize("channels", [1, 70])
@pytest.mark.parametrize("regime", [1, 2])
def test_delay_channel_counts(gpu, channels, regime):
    """70 channels: more than one workgroup in regime 2 at 8 samples x 8 channels per wave (c = 10, block 9)."""
    h, refs = dpair(1000.0, channels, [("SetTime", 0.01), ("SetFeedback", 0.99)], regime)
    assert h.kernel_info()[:2] == (9, 8)
    n = 2500
    run_cuts(h, refs, noise(n, channels), cut(n, [65, 1000]), True, f"{channels} channels")


@pytest.mark.parametrize("regime", [0, 1])
@pytest.mark.parametrize("t0,t1", [(0.25, 0.01), (0.01, 0.25)])
def test_delay_ramp_is_the_reference_sequence(gpu, t0, t1, regime):
    """SetTargetTime at 8 kHz, through the ramp's fixed point (about 2600
    steps) and 1000 samples past it, cut inside the ramp, with a second
    SetTargetTime on the way; currentSamples is the oracle's after every call."""
    h, refs = dpair(8000.0, 3, [("SetTime", t0), ("SetTargetTime", t1), ("SetFeedback", 0.9)], regime)
    x = noise(8000)
    check = dstate(h, refs)
    run_cuts(h, refs, x[:, :500], [1, 99, 400], True, "ramp", check)
    assert refs[0].currentSamples not in (refs[0].targetSamples, R.go_round(t0 * 8000.0))
    dapply(h, refs, "SetTargetTime", 0.05)
    run_cuts(h, refs, x[:, 500:1500], [1000], True, "second target", check)
    dapply(h, refs, "SetTargetTime", t1)
    run_cuts(h, refs, x[:, 1500:], [3000, 2500, 1000], True, "to the fixed point", check)
    r = refs[0]
    at = r.currentSamples
    assert r.ramp_step() == at  # the oracle sits at its fixed point
    # one call gives the same bits as the cut ones
    h2, _ = dpair(8000.0, 3, [("SetTime", t0), ("SetTargetTime", t1), ("SetFeedback", 0.9)], regime)
    whole = gpu_run(h2, x[:, :500])
    h3, _ = dpair(8000.0, 3, [("SetTime", t0), ("SetTargetTime", t1), ("SetFeedback", 0.9)], regime)
    compare(gpu_run(h3, x[:, :500], [1, 0, 99, 400]), whole, True, "cut against whole")


def test_delay_set_sample_rate_keeps_history(gpu):
    h, refs = dpair(8000.0, 3, [("SetFeedback", 0.9)])
    x = noise(9000)
    check = dstate(h, refs)
    run_cuts(h, refs, x[:, :3000], [3000], True, "8000", check)
    dapply(h, refs, "SetSampleRate", 11025.0)
    check()
    run_cuts(h, refs, x[:, 3000:6000], [3000], True, "11025", check)
    dapply(h, refs, "SetSampleRate", 8000.0)
    check()
    run_cuts(h, refs, x[:, 6000:], [3000], True, "8000 again", check)


def test_delay_reset_keeps_current_samples(gpu):
    h, refs = dpair(8000.0, 3, [("SetTargetTime", 0.01)])
    x = noise(1200)
    run_cuts(h, refs, x[:, :600], [600])
    cur = h.CurrentDelaySamples()
    assert 80 < cur < 2000
    dapply(h, refs, "Reset")
    assert h.derived() == (cur, 80.0, 16001, 0)
    run_cuts(h, refs, x[:, 600:], [600], True, "after Reset", dstate(h, refs))


@pytest.mark.parametrize("name,value", [("SetTime", 0.1), ("SetTargetTime", 0.3), ("SetFeedback", 0.0),
                                        ("SetMix", 1.0), ("SetSampleRate", 8000.0), ("Reset", None)])
def test_delay_setter_mid_stream(gpu, name, value):
    h, refs = dpair(8000.0, 3)
    x = noise(1600)
    run_cuts(h, refs, x[:, :800], [800], True, "before")
    dapply(h, refs, name, value)
    run_cuts(h, refs, x[:, 800:], [800], True, f"after {name}({value})", dstate(h, refs))


@pytest.mark.parametrize("name,value", [("SetTime", 2.5), ("SetTargetTime", 0.0005), ("SetFeedback", 1.0),
                                        ("SetMix", float("nan")), ("SetSampleRate", 0.0)])
def test_delay_rejected_setter_changes_nothing(gpu, name, value):
    h, _ = dpair(8000.0, 3, [("SetTargetTime", 0.01)])
    twin, _ = dpair(8000.0, 3, [("SetTargetTime", 0.01)])
    x = noise(1000)
    compare(gpu_run(h, x[:, :500]), gpu_run(twin, x[:, :500]))
    before = ([getattr(h.config(), f) for f, _ in _lib.DelayConfig._fields_], h.derived())
    with pytest.raises(_lib.ErrInvalidArgument):
        getattr(h, name)(value)
    assert ([getattr(h.config(), f) for f, _ in _lib.DelayConfig._fields_], h.derived()) == before
    compare(gpu_run(h, x[:, 500:]), gpu_run(twin, x[:, 500:]))


def test_delay_getters(gpu):
    h = P.Delay(48000.0, 2)
    assert (h.SampleRate(), h.Time(), h.Feedback(), h.Mix(), h.CurrentDelaySamples()) == (48000.0, 0.25, 0.35, 0.25, 12000.0)
    assert h.derived() == (12000.0, 12000.0, 96001, 0) and h.kernel_info() == (11999, 64, 0, 0)
    h.SetTargetTime(0.5), h.SetMix(0.75)
    assert (h.Time(), h.Mix(), h.derived()[:2]) == (0.5, 0.75, (12000.0, 24000.0))
    h.SetSmoothCoeff(0.125)
    assert h.config().smooth_coeff == 0.125
    for bad in (0.0, 1.5, float("nan")):
        with pytest.raises(_lib.ErrInvalidArgument):
            h.SetSmoothCoeff(bad)
    h.SetSampleRate(48000.0)  # derives it anew
    assert h.config().smooth_coeff == 1 - math.exp(-1 / (48000.0 * 0.010)) and h.derived()[:2] == (24000.0, 24000.0)
    with pytest.raises(_lib.ErrInvalidArgument):
        h.SetDelaySamples(3)  # mode 1 only
    with pytest.raises(_lib.ErrInvalidArgument):
        h.set_regime(3)
    h.close()


# ---- delay-simple -----------------------------------------------------------
def simple_pair(d, channels=2):
    h = P.Delay(channels=channels, config=_lib.DelayConfig(sample_rate=48000.0, mode=1, delay_samples=d))
    refs = []
    for _ in range(channels):
        s = R.SimpleDelay()
        s.delaySamples, s.buf = d, [0.0] * (d + 1)
        refs.append(s)
    return h, refs


@pytest.mark.parametrize("regime", [1, 2])
@pytest.mark.parametrize("d,cuts", [(0, [10, 90]), (1, [1, 3, 96]), (63, [10, 64, 126]), (64, [63, 65, 72]),
                                    (65, [64, 66, 70]), (24000, [5000, 25000])])
def test_delay_simple_copies_bits(gpu, d, cuts, regime):
    """Calls shorter and longer than D; -0.0, inf and a NaN payload come out as they went in."""
    if d == 24000 and regime == 2:
        regime = 0  # one block covers each call: the library takes one launch anyway
    n = sum(cuts)
    x = noise(n, 2)
    x[0, 3], x[1, 5], x[0, n // 3] = -0.0, float("inf"), -float("inf")
    x[1, 7:9].view(np.int64)[:] = [0x7FF8000000000123, -0x0007FFFFFFFFFFFF]
    h, refs = simple_pair(d)
    h.set_regime(regime)
    run_cuts(h, refs, x, cuts, True, f"D {d}")
    if d:
        y = gpu_run(simple_pair(d)[0], x)
        compare(y[:, d:], x[:, :n - d], True, "shifted input")
        assert not np.any(y[:, :d].view(np.int64))
        assert h.derived()[:3] == (float(d), float(d), d)
    else:
        assert h.kernel_info()[2] == 0  # nothing ran


def test_delay_simple_resize_and_reset(gpu):
    h, refs = simple_pair(100)
    x = noise(600, 2)
    run_cuts(h, refs, x[:, :300], [300])
    h.SetDelaySamples(100)  # the same size: state kept
    run_cuts(h, refs, x[:, 300:400], [100])
    h.SetDelaySamples(40)  # another size: a zeroed ring
    for s in refs:
        s.delaySamples, s.buf, s.write = 40, [0.0] * 41, 0
    run_cuts(h, refs, x[:, 400:500], [100])
    h.Reset()
    for s in refs:
        s.buf, s.write = [0.0] * 41, 0
    run_cuts(h, refs, x[:, 500:], [100])
    for bad in (-1.0, 2.5, float("nan"), 2.0 ** 28):
        with pytest.raises(_lib.ErrInvalidArgument):
            h.SetDelaySamples(bad)
    with pytest.raises(_lib.ErrInvalidArgument):
        h.SetMix(0.5)


# ---- the flanger ------------------------------------------------------------
def fpair(fs=48000.0, channels=3, **options):
    return P.Flanger(fs, channels, **options), [R.Flanger(fs, **options) for _ in range(channels)]


def fapply(h, refs, name, value=None):
    for o in [h] + list(refs):
        getattr(o, name)(*(() if value is None else (value,)))


def fstate(h, refs):
    def check():
        ln, md, wp, ph = h.derived()
        for r in refs:
            assert (ln, md, wp) == (len(r.delayLine), r.maxDelay, r.write)
            assert ph == r.lfoPhase  # the phase word, bitwise (both are finite)
    return check


@pytest.mark.parametrize("feedback", [0.99, -0.99])
@pytest.mark.parametrize("base,block,sub", [(0.0001, 3, 2), (0.001, 47, 32), (0.01, 479, 64)])
def test_flanger_depth_zero_is_bit_exact(gpu, base, block, sub, feedback):
    h, refs = fpair(base_delay_seconds=base, depth_seconds=0.0, feedback=feedback)
    assert h.kernel_info()[:2] == (block, sub) and refs[0].block_bound() == block
    n = 5000
    run_cuts(h, refs, noise(n), cut(n, [1, 63, 64, 65, 0, 1031]), True, f"base {base}", fstate(h, refs))


@pytest.mark.parametrize("channels", [1, 70])
@pytest.mark.parametrize("base", [0.0001, 0.001])
def test_flanger_channel_counts(gpu, channels, base):
    h, refs = fpair(channels=channels, base_delay_seconds=base, depth_seconds=0.0, feedback=-0.99, mix=1.0)
    n = 1500
    run_cuts(h, refs, noise(n, channels), cut(n, [129, 700]), True, f"{channels} channels", fstate(h, refs))


@pytest.mark.parametrize("fs,options", [(192000.0, dict(base_delay_seconds=0.0001, depth_seconds=0.0)),
                                        (8000.0, dict(base_delay_seconds=0.0001, depth_seconds=0.0)),
                                        (192000.0, dict(base_delay_seconds=0.0098, depth_seconds=0.0))])
def test_flanger_other_rates(gpu, fs, options):
    """192 kHz at the longest ring (1885 samples: two channels per workgroup) and
    at the shortest; 8 kHz at the minimum base delay, where the delay clamps to one sample."""
    h, refs = fpair(fs, 3, feedback=0.9, **options)
    n = 4500
    run_cuts(h, refs, noise(n), cut(n, [513, 1]), True, f"{fs} Hz {options}", fstate(h, refs))


MODULATED = [dict(), dict(rate_hz=5.0, base_delay_seconds=0.001, depth_seconds=0.0099 - 0.001, feedback=0.7)]


@pytest.mark.parametrize("options", MODULATED)
def test_flanger_modulated(gpu, options):
    h, refs = fpair(**options)
    n = 6000
    run_cuts(h, refs, noise(n), cut(n, [1, 500, 2049]), False, f"modulated {options}", fstate(h, refs))


def test_flanger_lfo_phase_wraps_as_the_reference(gpu):
    n = 30011
    want, wraps = 0.0, 0
    for _ in range(n):
        nxt = R.lfo_step(want, 5.0, 8000.0)
        wraps += nxt < want
        want = nxt
    assert wraps == 18
    h = P.Flanger(8000.0, 1, rate_hz=5.0)
    gpu_run(h, np.zeros((1, n)), [1, 7, 10000, n - 10008])
    assert h.derived()[3] == want
    h.Reset()
    assert h.derived()[2:] == (0, 0.0)


FL_MIDSTREAM = [("SetDepthSeconds", 0.004), ("SetDepthSeconds", 0.0), ("SetBaseDelaySeconds", 0.0003),
                ("SetBaseDelaySeconds", 0.005), ("SetSampleRate", 44100.0), ("SetRateHz", 2.0), ("SetFeedback", -0.8),
                ("SetMix", 1.0), ("Reset", None)]


@pytest.mark.parametrize("name,value", FL_MIDSTREAM)
def test_flanger_setter_mid_stream(gpu, name, value):
    """Depth, base delay and sample rate resize the line and keep its newest samples."""
    h, refs = fpair(rate_hz=3.0)
    x = noise(2000)
    check = fstate(h, refs)
    run_cuts(h, refs, x[:, :1000], [1000], False, "before", check)
    fapply(h, refs, name, value)
    check()
    run_cuts(h, refs, x[:, 1000:], [1000], False, f"after {name}({value})", check)


@pytest.mark.parametrize("options,name,bad,good", [
    (dict(base_delay_seconds=0.0087, depth_seconds=0.0012), "SetDepthSeconds", 0.0014, 0.0011),
    (dict(base_delay_seconds=0.004, depth_seconds=0.004), "SetBaseDelaySeconds", 0.007, 0.0055),
    (dict(), "SetMix", 2.0, 0.5), (dict(), "SetRateHz", 0.0, 1.0), (dict(), "SetFeedback", 1.0, 0.5),
    (dict(), "SetSampleRate", float("inf"), 48000.0)])
def test_flanger_rejected_setter_changes_nothing(gpu, options, name, bad, good):
    """flanger_test.go:125-186 (the two rollbacks) and the plain range checks."""
    h, refs = fpair(**options)
    x = noise(1500)
    check = fstate(h, refs)
    run_cuts(h, refs, x[:, :500], [500], False, "before", check)
    before = [getattr(h.config(), f) for f, _ in _lib.FlangerConfig._fields_]
    with pytest.raises(_lib.ErrInvalidArgument):
        getattr(h, name)(bad)
    assert [getattr(h.config(), f) for f, _ in _lib.FlangerConfig._fields_] == before
    check()
    run_cuts(h, refs, x[:, 500:1000], [500], False, "after the rejected value", check)
    fapply(h, refs, name, good)
    run_cuts(h, refs, x[:, 1000:], [500], False, "after the accepted one", check)


def test_flanger_getters_and_options(gpu):
    h = P.Flanger(48000.0, 2)
    assert (h.SampleRate(), h.RateHz(), h.DepthSeconds(), h.BaseDelaySeconds(), h.Feedback(), h.Mix()) == \
        (48000.0, 0.25, 0.0015, 0.001, 0.25, 0.5)
    assert h.derived() == (123, 120, 0, 0.0)
    block, sub, group, lds = h.kernel_info()
    assert (block, sub) == (47, 32) and group >= 2 and 0 < lds <= 65536
    h.SetRateHz(0.5), h.SetFeedback(-0.5)
    assert (h.RateHz(), h.Feedback()) == (0.5, -0.5)
    with pytest.raises(_lib.ErrInvalidArgument):
        P.Flanger(48000.0, 1, base_delay_seconds=0.009, depth_seconds=0.002)
    with pytest.raises(TypeError):
        P.Flanger(48000.0, 1, wobble=1.0)
    h.close()


# ---- the device-buffer layout contract, streams -----------------------------
def _delay_ramping():
    h = P.Delay(8000.0, 3)
    h.SetTargetTime(0.01)
    return h


def _delay_ramping_regime1():
    h = _delay_ramping()
    h.set_regime(1)
    return h


MAKERS = {"delay": _delay_ramping,
          "delay regime 1": _delay_ramping_regime1,
          "delay-simple": lambda: simple_pair(100, 3)[0],
          "flanger": lambda: P.Flanger(48000.0, 3, rate_hz=3.0)}


@pytest.mark.parametrize("kind", list(MAKERS))
def test_process_device_layouts(gpu, kind):
    """Row strides greater than n and rows 8 bytes off 16-byte alignment give
    the bits of the aligned contiguous placement, and touch nothing around the rows."""
    n = 1500
    x = noise(n)

    def run(layout):
        h = MAKERS[kind]()
        b = LL.place(x, layout, DEV)
        torch.cuda.synchronize()
        h.process_device(b.ptr, b.stride, 1000)  # a first call that leaves the last 500 columns alone
        h.process_device(b.ptr + 8 * 1000, b.stride, 500)
        torch.cuda.synchronize()
        LL.check_guards(b)
        return LL.payload(b)

    want = run(LL.LA(n))
    for layout in LL.variants(n):
        compare(run(layout), want, True, f"{kind} {layout}")
    h = MAKERS[kind]()
    compare(gpu_run(h, x, [1000, 500]), want, True, "host-buffer calls")
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


@pytest.mark.parametrize("kind", ["delay", "flanger"])
def test_two_streams_alternate_on_one_handle(gpu, kind):
    """Calls alternate between the NULL stream and a side stream (and one
    host-buffer call): the state is shared, every call waits for the one
    before, so the result is one sequential processor's."""
    C_, n = 3, 4000
    x = noise(n, C_)
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
    compare(got, want, True, f"{kind} on two streams")
    h.process_device(d.data_ptr(), n, 700, side.cuda_stream)
    h.Reset()  # ordered after the side stream's call


# ---- the effect graph -------------------------------------------------------
FS = 8000.0


def _graph(nodes, dry_edge=False):
    ids = [E.INPUT_NODE_ID] + [n["id"] for n in nodes] + [E.OUTPUT_NODE_ID]
    edges = list(zip(ids[:-1], ids[1:]))
    if dry_edge:
        edges.append((E.INPUT_NODE_ID, E.OUTPUT_NODE_ID))
    return E._graph_json(nodes, edges)


def _chain_run(graph, x, channels=3):
    ch = E.Chain(FS, channels)
    ch.LoadGraph(graph)
    y = x.copy()
    assert ch.Process(y)
    return ch, y


DELAY_NODE = {"id": "d", "type": "delay", "params": {"time": 0.02, "feedback": 0.6, "mix": 0.5}}
FLANGER_NODE = {"id": "f", "type": "flanger", "params": {"rateHz": 2.0, "depth": 0.002, "feedback": -0.5}}
SIMPLE_NODE = {"id": "s", "type": "delay-simple", "params": {"delayMs": 12.5}}


def _processor(node):
    p = E.Params(node["id"], node["type"], num=node.get("params", {}))
    if node["type"] == "delay":
        return P.Delay(channels=3, config=E.delay_params(p, FS))
    if node["type"] == "flanger":
        return P.Flanger(channels=3, config=E.flanger_params(p, FS))
    return simple_pair(E.simple_delay_samples(p, FS), 3)[0]


@pytest.mark.parametrize("node", [DELAY_NODE, FLANGER_NODE, SIMPLE_NODE, {"id": "d", "type": "delay"},
                                  {"id": "f", "type": "flanger"}])
def test_graph_node_is_the_processor(gpu, node):
    x = noise(1500)
    ch, y = _chain_run(_graph([node]), x)
    kind = "flanger" if node["type"] == "flanger" else "delay"
    assert ch.spec[1]["type"] == kind and ch.op_count()[0] == 1
    compare(y, gpu_run(_processor(node), x), True, node["type"])
    y2 = x.copy()
    assert ch.Process(y2)
    assert np.any(y2 != y)  # state carries over calls
    ch.Reset()


def test_graph_delay_node_starts_at_a_quarter_second_and_ramps(gpu):
    """configureDelay: SetSampleRate snaps to 0.25 s, SetTargetTime(0.02) ramps from there."""
    n = 4000
    x = noise(n)
    ch, y = _chain_run(_graph([DELAY_NODE]), x)
    refs = []
    coeff = _processor(DELAY_NODE).config().smooth_coeff
    for c in range(3):
        r = R.Delay(FS)
        r.SetSampleRate(FS), r.SetTargetTime(0.02), r.SetFeedback(0.6), r.SetMix(0.5)
        assert math.nextafter(r.smoothCoeff, 0.0) <= coeff <= math.nextafter(r.smoothCoeff, 1.0)
        r.smoothCoeff = coeff
        assert (r.currentSamples, r.targetSamples) == (2000.0, 160.0)
        compare(y[c], r.process(x[c]), True, f"delay node channel {c}")
        refs.append(r)
    snapped = R.Delay(FS)  # without the ramp the output is another one
    snapped.SetTime(0.02), snapped.SetFeedback(0.6), snapped.SetMix(0.5)
    assert np.any(snapped.process(x[0]) != y[0])
    # ad_fx_graph_reset is Reset: the rings are cleared, the ramp stays where it is
    ch.Reset()
    y2 = x.copy()
    assert ch.Process(y2)
    for c, r in enumerate(refs):
        r.Reset()
        compare(y2[c], r.process(x[c]), True, f"after Reset channel {c}")


def test_graph_delay_simple_zero_is_a_pass(gpu):
    x = noise(300)
    ch, y = _chain_run(_graph([{"id": "s", "type": "delay-simple", "params": {"delayMs": 0.05}}]), x)
    assert ch.spec[1]["type"] == "pass"
    compare(y, x, True, "delay-simple of 0 samples")


def test_graph_delay_into_flanger_with_dry_edge_and_bypass(gpu):
    x = noise(2000)
    ch, y = _chain_run(_graph([DELAY_NODE, FLANGER_NODE], dry_edge=True), x)
    assert [s["type"] for s in ch.spec] == ["input", "delay", "flanger", "output"]
    assert ch.spec[1]["delay"]["time_seconds"] == 0.02 and ch.spec[2]["flanger"]["rate_hz"] == 2.0
    wet = gpu_run(_processor(FLANGER_NODE), gpu_run(_processor(DELAY_NODE), x))
    compare(y, (wet + x) * 0.5, True, "delay -> flanger, averaged with the dry edge")  # edge order: flanger, _input
    ch.Reset()
    ch, y = _chain_run(_graph([dict(DELAY_NODE, bypassed=True), FLANGER_NODE]), x)
    compare(y, gpu_run(_processor(FLANGER_NODE), x), True, "bypassed delay")
    ch, y = _chain_run(_graph([dict(DELAY_NODE, bypassed=True), dict(SIMPLE_NODE, bypassed=True)]), x)
    compare(y, x, True, "everything bypassed")


def test_graph_node_without_config_is_refused(gpu):
    par = (C.c_int32 * 1)(0)
    par2 = (C.c_int32 * 1)(1)
    for t in (E.FXN_DELAY, E.FXN_FLANGER):
        nodes = (E._Node * 3)()
        nodes[0].type = E.FXN_INPUT
        nodes[1].type, nodes[1].n_parents, nodes[1].parents = t, 1, C.cast(par, C.POINTER(C.c_int32))
        nodes[2].type, nodes[2].n_parents, nodes[2].parents = E.FXN_OUTPUT, 1, C.cast(par2, C.POINTER(C.c_int32))
        h = C.c_void_p()
        rc = _lib.lib().ad_fx_graph_create(C.cast(nodes, C.c_void_p), 3, 2, 0, C.byref(h))
        assert rc == _lib.AD_ERR_INVALID_ARGUMENT and not h.value


@pytest.mark.parametrize("t", ["chorus", "dyn-lookahead", "filter-moog", "vocoder"])
def test_unknown_effect_still_raises(gpu, t):
    with pytest.raises(E.UnknownEffect):
        E.Chain(48000.0, 2).LoadGraph(_graph([{"id": "n", "type": t}]))
