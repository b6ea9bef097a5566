"""modulation.Phaser, Tremolo and RingModulator on the GPU (processors.Phaser /
Tremolo / RingModulator, the effect graph's phaser, tremolo and ringmod nodes)
against the restated reference (tests/modfx_ref.py), with distinct noise per
channel.

Bars.  The phase is compared on the float64 bits.  Given the per-sample table a
call took from the phase on the device (peek_lfo: the phaser's coefficient, the
tremolo's gain, the ring modulator's carrier) the output is compared on the
bits too.  The tables themselves differ from Python's by the device math
library's sin and tan: the sine and the tremolo's gain within 1e-15 absolute,
the phaser's coefficient within 1e-13 (near 0.49 fs, g = tan(pi f / fs) is about
32 and amplifies its last place).  End to end against the pure restatement:
relative RMS <= 1e-12 and max abs <= 1e-10, the flanger's and the FDN reverb's
bars for the same cause; test_modfx_ref.py::test_sine_spread measured, on the
CPU, what a last-place change of every sine and tangent does to these very
cases: at most 1.1e-14 relative RMS and 5.3e-14 absolute, inside a quarter of
the bars."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import layout_lib as LL
import modfx_ref as R
from algodsp import _lib, effectchain as E, processors as P, signals

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
RMS_BAR, ABS_BAR = 1e-12, 1e-10
HANDLES = {"phaser": P.Phaser, "tremolo": P.Tremolo, "ringmod": P.RingModulator}
CUTS = [1, 63, 64, 65, 1031]


def noise(n, channels=3, seed=0x30DF):
    return np.stack([signals.white_noise(n, seed + c) for c in range(channels)]) * R.AMPLITUDE


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def compare(got, want, exact=True, what=""):
    if not got.size:  # an empty call has nothing to compare
        assert got.shape == want.shape
        return
    with np.errstate(all="ignore"):
        err = float(np.sqrt(np.mean((got - want) ** 2)) / max(np.sqrt(np.mean(want ** 2)), 1e-300))
        mx = float(np.max(np.abs(got - want))) if got.size else 0.0
    print(f"{what}: rel rms {err:.3g}, max abs {mx:.3g}, differing samples {int(np.sum(got != want))}")
    if exact:
        np.testing.assert_array_equal(bits(got), bits(want))
    else:
        assert err <= RMS_BAR and mx <= ABS_BAR


def cut(n, cuts):
    """`cuts`, then the rest of n."""
    assert sum(cuts) < n
    return list(cuts) + [n - sum(cuts)]


def ref_phase(ref):
    return ref.phase if isinstance(ref, R.RingModulator) else ref.lfoPhase


def sync_coeff(h, ref):
    """The handle derives the tremolo's coefficient with the C library's exp, Python with the same one."""
    if isinstance(ref, R.Tremolo):
        k = h.config().smoothing_coeff
        assert math.nextafter(ref.smoothingCoef, 0.0) <= k <= math.nextafter(ref.smoothingCoef, 1.0)
        ref.smoothingCoef = k


def pair(kind, fs, channels=3, **options):
    h, ref = HANDLES[kind](fs, channels, **options), R.KINDS[kind](fs, **options)
    sync_coeff(h, ref)
    return h, ref


def apply(h, ref, name, *args):
    for o in (h, ref):
        getattr(o, name)(*args)
    sync_coeff(h, ref)


def run_cuts(h, ref, x, cuts, what="", tables=True):
    """The GPU handle and the oracle over the same calls.  Before each call the
    next phases are compared on the bits; with `tables` the oracle takes the
    device's per-sample table and the outputs are compared on the bits,
    without them it runs on its own and the bars apply.  Returns the output."""
    y = x.copy()
    pos = 0
    for m in cuts:
        blk = x[:, pos:pos + m].copy()  # a one-channel slice is contiguous as it is: never the caller's array
        ph, tab = h.peek_lfo(m)
        want_ph, _ = R.phases(ref_phase(ref), ref.inc(), m)
        np.testing.assert_array_equal(bits(ph), bits(want_ph), err_msg=f"{what}: phases of [{pos}, {pos + m})")
        ph2, tab2 = h.peek_lfo(m)  # a peek advances nothing
        np.testing.assert_array_equal(bits(ph2), bits(ph))
        np.testing.assert_array_equal(bits(tab2), bits(tab))
        want = R.process_many(ref, blk, tab if tables else None) if m else blk.copy()
        h.ProcessInPlace(blk)
        compare(blk, want, tables, f"{what} [{pos}, {pos + m})")
        assert bits(h.peek_lfo(1)[0])[0] == bits([ref_phase(ref)])[0], f"{what}: phase after [{pos}, {pos + m})"
        y[:, pos:pos + m] = blk
        pos += m
    assert pos == x.shape[1]
    return y


def gpu_run(h, x, cuts=None):
    y = x.copy()
    pos = 0
    for m in cuts or [x.shape[1]]:
        blk = y[:, pos:pos + m].copy()
        h.ProcessInPlace(blk)
        y[:, pos:pos + m] = blk
        pos += m
    return y


# ---- the phase --------------------------------------------------------------
@pytest.mark.parametrize("kind,fs,options", [
    ("phaser", 8000.0, dict(rate_hz=5.0)), ("tremolo", 8000.0, dict(rate_hz=5.0)),
    ("ringmod", 8000.0, dict(carrier_hz=0.49 * 8000.0)), ("ringmod", 8000.0, dict(carrier_hz=5.0)),
    ("tremolo", 48000.0, dict(rate_hz=20.0)), ("phaser", 44100.0, dict())])
def test_phase_is_the_reference_sequence(gpu, kind, fs, options):
    """peek_lfo's phases and the state after every call are the restated
    rounded additions and wraps, bit for bit: across the cuts, an empty call,
    and calls that start on the wrapped sample and on the one after it.  fs 8000
    with 5 Hz wraps every 1600 samples, the carrier at 0.49 fs about every
    second sample."""
    n = 4500
    h, ref = pair(kind, fs, 2, **options)
    seq, _ = R.phases(0.0, ref.inc(), n)
    wraps = [i for i in range(1, n) if seq[i] < seq[i - 1]]
    cuts = list(CUTS)
    later = [w for w in wraps if w > sum(cuts) + 1 and w + 2 < n]
    if later:  # calls that begin at the wrapped sample and at the one after it
        cuts += [later[0] - sum(cuts), 1]
        assert seq[sum(cuts) - 1] < seq[sum(cuts) - 2]
    print(f"{kind} {fs} {options}: {len(wraps)} wraps, cuts {cuts}")
    assert wraps or fs != 8000.0
    run_cuts(h, ref, noise(n, 2), cut(n, cuts + [0]), f"{kind} {options}")
    assert h.peek_lfo(0)[0].size == 0


# ---- bit-exact given the device's tables ------------------------------------
CHANNELS = [1, 3, 65, 130]  # one past a wave, and no multiple of 64
N = 4500


def _both_ways(kind, fs, channels, what, **options):
    """The cut calls against the oracle, and one call over everything against the cut calls."""
    x = noise(N, channels)
    h, ref = pair(kind, fs, channels, **options)
    y = run_cuts(h, ref, x, cut(N, CUTS), what)
    compare(gpu_run(HANDLES[kind](fs, channels, **options), x), y, True, f"{what}: one call")


PHASER_GRID = [(c, s, (0.0, 0.99, -0.99)[(i + j) % 3], (0.0, 0.5, 1.0)[(i + 2 * j) % 3])
               for i, c in enumerate(CHANNELS) for j, s in enumerate((1, 6, 12))]
PHASER_GRID += [(3, 6, 0.99, 1.0), (3, 12, -0.99, 0.5), (3, 1, 0.0, 0.0), (65, 12, 0.0, 0.5), (1, 1, -0.99, 1.0)]


@pytest.mark.parametrize("channels,stages,feedback,mix", PHASER_GRID)
def test_phaser_is_bit_exact_given_the_coefficients(gpu, channels, stages, feedback, mix):
    _both_ways("phaser", 8000.0, channels, f"phaser {channels} ch, {stages} stages, fb {feedback}, mix {mix}",
               rate_hz=5.0, min_freq_hz=20.0, max_freq_hz=3900.0, stages=stages, feedback=feedback, mix=mix)


@pytest.mark.parametrize("depth", [0.0, 1.0])
@pytest.mark.parametrize("smoothing_ms", [0.0, 5.0, 200.0])
@pytest.mark.parametrize("channels", CHANNELS)
def test_tremolo_is_bit_exact_given_the_gain(gpu, channels, smoothing_ms, depth):
    mix = (0.0, 0.5, 1.0)[(CHANNELS.index(channels) + int(smoothing_ms)) % 3]
    _both_ways("tremolo", 8000.0, channels, f"tremolo {channels} ch, {smoothing_ms} ms, depth {depth}, mix {mix}",
               rate_hz=5.0, depth=depth, smoothing_ms=smoothing_ms, mix=mix)


@pytest.mark.parametrize("mix", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("channels", CHANNELS)
def test_ringmod_is_bit_exact_given_the_carrier(gpu, channels, mix):
    _both_ways("ringmod", 8000.0, channels, f"ringmod {channels} ch, mix {mix}", carrier_hz=440.0, mix=mix)


# ---- the tables against the reference's math --------------------------------
def ulps(a, b):
    return int(np.max(np.abs(bits(a) - bits(b)))) if len(a) else 0


def test_device_sine_and_gain_against_python(gpu):
    """The carrier (the device's sine of the phase) and the tremolo's gain
    sequence are within 1e-15 absolute of Python's."""
    n = 6000
    for fs, carrier in ((48000.0, 440.0), (8000.0, 0.49 * 8000.0), (8000.0, 5.0)):
        h = P.RingModulator(fs, 1, carrier_hz=carrier)
        ph, tab = h.peek_lfo(n)
        want = np.array([math.sin(v) for v in ph])
        print(f"carrier {carrier} at {fs}: max abs {np.max(np.abs(tab - want)):.3g}, worst ulp distance {ulps(tab, want)}")
        assert np.max(np.abs(tab - want)) <= 1e-15
    for smoothing, depth, rate in ((0.0, 1.0, 20.0), (5.0, 1.0, 20.0), (200.0, 1.0, 20.0), (5.0, 0.6, 4.0)):
        h, ref = pair("tremolo", 8000.0, 1, rate_hz=rate, depth=depth, smoothing_ms=smoothing)
        for m in (1000, 0, 1, 4999):  # the gain carries over calls
            _, tab = h.peek_lfo(m)
            want = []
            for _ in range(m):
                ref.Process(0.0)
                want.append(ref.currentMod)
            h.ProcessInPlace(np.zeros((1, m)))
            err = float(np.max(np.abs(tab - np.array(want)))) if m else 0.0
            print(f"gain, smoothing {smoothing} ms, depth {depth}, {m} samples: max abs {err:.3g}")
            assert err <= 1e-15


def test_device_coefficient_against_python(gpu):
    """The phaser's coefficient is within 1e-13 absolute of Python's; the range
    20 .. 3900 Hz at 8 kHz reaches g = tan(pi f / fs) = 25, and a range that
    ends just under 0.49 fs reaches 32."""
    for fs, lo, hi, rate in ((8000.0, 20.0, 3900.0, 5.0), (8000.0, 20.0, math.nextafter(0.49 * 8000.0, 0.0), 5.0),
                             (48000.0, 300.0, 1600.0, 0.4), (48000.0, 5e-324, 1.0, 5.0)):
        h, ref = pair("phaser", fs, 1, rate_hz=rate, min_freq_hz=lo, max_freq_hz=hi)
        ph, tab = h.peek_lfo(6000)
        want = []
        for v in ph:
            ref.lfoPhase = float(v)
            want.append(ref.coefficient())
        want = np.array(want)
        print(f"coefficient {lo} .. {hi} Hz at {fs}: max abs {np.max(np.abs(tab - want)):.3g}, "
              f"worst ulp distance {ulps(tab, want)}, coefficients in [{tab.min():.6g}, {tab.max():.6g}]")
        assert np.max(np.abs(tab - want)) <= 1e-13


# ---- end to end against the pure restatement --------------------------------
@pytest.mark.parametrize("kind,fs,options,n", R.CASES)
def test_end_to_end_against_the_restatement(gpu, kind, fs, options, n):
    h, ref = pair(kind, fs, 3, **options)
    run_cuts(h, ref, noise(n), cut(n, CUTS), f"{kind} {fs} {options}", tables=False)


def test_tremolo_depth_zero_and_ringmod_mix_zero_are_bit_exact(gpu):
    """Nothing depends on the sine: (1 - 0) + 0 * lfo is 1, and a mix of 0 multiplies the wet part by 0."""
    x = noise(3000)
    for smoothing in (0.0, 5.0):
        h, ref = pair("tremolo", 48000.0, 3, depth=0.0, smoothing_ms=smoothing, mix=0.7)
        run_cuts(h, ref, x, cut(3000, CUTS), f"tremolo depth 0, {smoothing} ms", tables=False)
        ref2 = R.Tremolo(48000.0, depth=0.0, smoothing_ms=smoothing, mix=0.7)
        sync_coeff(h, ref2)
        compare(gpu_run(P.Tremolo(48000.0, 3, depth=0.0, smoothing_ms=smoothing, mix=0.7), x),
                R.process_many(ref2, x), True, "against the pure restatement")
    h, ref = pair("ringmod", 48000.0, 3, carrier_hz=1000.0, mix=0.0)
    compare(gpu_run(h, x), R.process_many(ref, x), True, "ringmod mix 0")
    compare(gpu_run(P.RingModulator(48000.0, 3, carrier_hz=1000.0, mix=0.0), x), x, True, "ringmod mix 0 is transparent")


# ---- state ------------------------------------------------------------------
def test_phaser_set_stages(gpu):
    """The same count keeps every state; another one zeroes the stages and keeps the feedback sample and the phase."""
    x = noise(1500)
    h, ref = pair("phaser", 8000.0, 3, rate_hz=5.0, feedback=0.9, mix=1.0)
    run_cuts(h, ref, x[:, :500], [500], "before")
    apply(h, ref, "SetStages", 6)
    assert h.Stages() == 6
    y = run_cuts(h, ref, x[:, 500:1000], [500], "SetStages(6) again")
    apply(h, ref, "SetStages", 4)
    assert h.Stages() == 4 and np.any(ref.feedbackSample != 0) and ref.lfoPhase != 0
    run_cuts(h, ref, x[:, 1000:], [500], "SetStages(4)")
    # a handle whose stage states were kept gives another output
    k, kref = pair("phaser", 8000.0, 3, rate_hz=5.0, feedback=0.9, mix=1.0)
    gpu_run(k, x[:, :500])
    assert np.all(gpu_run(k, x[:, 500:1000]) == y)
    apply(h, ref, "SetStages", 12)
    run_cuts(h, ref, x[:, :500], [500], "SetStages(12)")


@pytest.mark.parametrize("kind,options", [("phaser", dict(feedback=0.9)), ("tremolo", dict()), ("tremolo", dict(smoothing_ms=0.0)),
                                          ("ringmod", dict())])
def test_reset_restores_the_first_output(gpu, kind, options):
    """Test*ResetRestoresState on the GPU: the same bits again, the phase at 0, against the oracle after its Reset."""
    x = noise(700)
    h, ref = pair(kind, 8000.0, 3, **options)
    first = run_cuts(h, ref, x, [700], "first")
    assert h.peek_lfo(1)[0][0] > 0
    apply(h, ref, "Reset")
    assert h.peek_lfo(1)[0][0] == 0.0
    compare(run_cuts(h, ref, x, [700], "after Reset"), first, True, f"{kind} after Reset")


@pytest.mark.parametrize("kind", ["phaser", "tremolo", "ringmod"])
def test_rejected_setter_changes_nothing(gpu, kind):
    """Every value the reference's setters reject is refused by ad_*_set_param
    (ad_phaser_set_range), and leaves the configuration and the next output as they were."""
    x = noise(600)
    h, twin = HANDLES[kind](48000.0, 3), HANDLES[kind](48000.0, 3)
    gpu_run(h, x[:, :300]), gpu_run(twin, x[:, :300])
    before = [getattr(h.config(), f) for f, _ in h.config()._fields_]
    tried = 0
    for k, field, value in R.REJECTED:
        if k != kind:
            continue
        with pytest.raises(_lib.ErrInvalidArgument):
            R.set_on(h, field, value)
        assert [getattr(h.config(), f) for f, _ in h.config()._fields_] == before, (field, value)
        tried += 1
    assert tried >= 10
    with pytest.raises(_lib.ErrInvalidArgument):
        h._set(99, 1.0)
    if kind == "phaser":
        for which, v in ((h.P_MIN_FREQ, 1600.0), (h.P_MAX_FREQ, 300.0), (h.P_MAX_FREQ, 0.49 * 48000.0), (h.P_STAGES, 6.5)):
            with pytest.raises(_lib.ErrInvalidArgument):
                h._set(which, v)
    if kind == "tremolo":
        for v in (0.0, -0.5, 1.5, float("nan")):
            with pytest.raises(_lib.ErrInvalidArgument):
                h.SetSmoothingCoeff(v)
    assert [getattr(h.config(), f) for f, _ in h.config()._fields_] == before
    compare(gpu_run(h, x[:, 300:]), gpu_run(twin, x[:, 300:]), True, f"{kind} after the rejected values")


def test_accepted_setters_and_getters(gpu):
    for kind, field, value in R.ACCEPTED:
        h, ref = pair(kind, 48000.0, 1)
        R.set_on(h, field, value), R.set_on(ref, field, value)
    p = P.Phaser(48000.0, 2)
    p.SetFrequencyRangeHz(200.0, 5000.0), p.SetRateHz(2.0), p.SetFeedback(-0.5), p.SetMix(0.25), p.SetStages(3)
    assert (p.MinFrequencyHz(), p.MaxFrequencyHz(), p.RateHz(), p.Feedback(), p.Mix(), p.Stages(), p.SampleRate()) == \
        (200.0, 5000.0, 2.0, -0.5, 0.25, 3, 48000.0)
    p._set(p.P_MIN_FREQ, 100.0), p._set(p.P_MAX_FREQ, 6000.0)
    assert (p.MinFrequencyHz(), p.MaxFrequencyHz()) == (100.0, 6000.0)
    assert p.kernel_info() == (64, 32, (2 * 64 * 33 + 32) * 8)
    t = P.Tremolo(48000.0, 2)
    t.SetRateHz(2.0), t.SetDepth(0.25), t.SetSmoothingMs(0.0), t.SetMix(0.5)
    assert (t.RateHz(), t.Depth(), t.SmoothingMs(), t.Mix(), t.config().smoothing_coeff) == (2.0, 0.25, 0.0, 0.5, 1.0)
    assert t.kernel_info()[2] == 0
    t.SetSmoothingCoeff(0.125)
    assert t.config().smoothing_coeff == 0.125 and t.kernel_info()[2] == 1
    r = P.RingModulator(48000.0, 2)
    r.SetCarrierHz(300.0), r.SetMix(0.7)
    assert (r.CarrierHz(), r.Mix(), r.SampleRate()) == (300.0, 0.7, 48000.0)


def test_set_sample_rate_recomputes_increment_and_coefficient(gpu):
    """TestRingModulatorSettersUpdateState (:312-344), and the tremolo's updateSmoothingCoefficient."""
    x = noise(900)
    h, ref = pair("ringmod", 48000.0, 3)
    assert h.kernel_info()[2] == ref.phaseInc == 2 * math.pi * 440.0 / 48000.0
    run_cuts(h, ref, x[:, :300], [300], "ringmod at 48 kHz")
    apply(h, ref, "SetSampleRate", 96000.0)
    assert h.kernel_info()[2] == ref.phaseInc == 2 * math.pi * 440.0 / 96000.0
    apply(h, ref, "SetCarrierHz", 1000.0)
    assert h.kernel_info()[2] == ref.phaseInc == 2 * math.pi * 1000.0 / 96000.0
    run_cuts(h, ref, x[:, 300:], [600], "ringmod at 96 kHz, 1 kHz")
    h, ref = pair("tremolo", 48000.0, 3, depth=1.0)
    run_cuts(h, ref, x[:, :300], [300], "tremolo at 48 kHz")
    k48 = h.config().smoothing_coeff
    apply(h, ref, "SetSampleRate", 8000.0)
    assert h.config().smoothing_coeff == ref.smoothingCoef != k48
    run_cuts(h, ref, x[:, 300:600], [300], "tremolo at 8 kHz")
    apply(h, ref, "SetSmoothingMs", 0.0)  # from the smoothed gain to the target itself
    assert h.config().smoothing_coeff == 1.0
    run_cuts(h, ref, x[:, 600:750], [150], "tremolo unsmoothed")
    apply(h, ref, "SetSmoothingMs", 50.0)  # and back: the gain starts from the last target
    run_cuts(h, ref, x[:, 750:], [150], "tremolo smoothed again")
    h, ref = pair("phaser", 48000.0, 3)
    run_cuts(h, ref, x[:, :300], [300], "phaser at 48 kHz")
    apply(h, ref, "SetSampleRate", 8000.0)
    run_cuts(h, ref, x[:, 300:], [600], "phaser at 8 kHz")


@pytest.mark.parametrize("kind,options", [("phaser", dict(feedback=0.9, stages=12)), ("tremolo", dict()), ("ringmod", dict())])
def test_an_inf_sample_stays_in_its_channel(gpu, kind, options):
    x = noise(1000, 5)
    bad = x.copy()
    bad[2, 100] = float("inf")
    want = gpu_run(HANDLES[kind](8000.0, 5, **options), x)
    got = gpu_run(HANDLES[kind](8000.0, 5, **options), bad)
    for c in (0, 1, 3, 4):
        compare(got[c], want[c], True, f"{kind} channel {c} next to an inf")
    assert not np.all(np.isfinite(got[2]))


# ---- the device-buffer layout contract, streams -----------------------------
MAKERS = {"phaser": lambda: P.Phaser(8000.0, 3, rate_hz=5.0, feedback=0.7),
          "tremolo": lambda: P.Tremolo(8000.0, 3, rate_hz=5.0),
          "tremolo unsmoothed": lambda: P.Tremolo(8000.0, 3, rate_hz=5.0, smoothing_ms=0.0),
          "ringmod": lambda: P.RingModulator(8000.0, 3)}


@pytest.mark.parametrize("kind", list(MAKERS))
def test_process_device_layouts(gpu, kind):
    """Row strides greater than n and rows 8 bytes off 16-byte alignment give
    the bits of the aligned contiguous placement, and touch nothing around the rows."""
    n = 1501
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
        compare(run(layout), want, True, f"{kind} {layout}")
    h = MAKERS[kind]()
    compare(gpu_run(h, x, [1000, 501]), want, True, "host-buffer calls")
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
def test_apply_kernel_shortest_rows(gpu, n):
    """One, two and three samples a row, aligned and 8 bytes off: the lead sample, one pair and the odd one at the end."""
    x = noise(n)
    want = gpu_run(MAKERS["ringmod"](), x)
    for layout in [LL.LA(n)] + LL.variants(n):
        b = LL.place(x, layout, DEV)
        torch.cuda.synchronize()
        MAKERS["ringmod"]().process_device(b.ptr, b.stride, n)
        torch.cuda.synchronize()
        LL.check_guards(b)
        compare(LL.payload(b), want, True, f"{n} samples {layout}")


@pytest.mark.parametrize("kind", list(MAKERS))
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
    torch.cuda.synchronize()


# ---- the effect graph -------------------------------------------------------
FS = 8000.0
PHASER_NODE = {"id": "p", "type": "phaser", "params": {"rateHz": 5.0, "minFreqHz": 100, "maxFreqHz": 3000, "stages": 4,
                                                       "feedback": -0.6, "mix": 0.8}}
TREMOLO_NODE = {"id": "t", "type": "tremolo", "params": {"rateHz": 9.0, "depth": 0.9, "smoothingMs": 2.0}}
RINGMOD_NODE = {"id": "r", "type": "ringmod", "params": {"carrierHz": 700.0, "mix": 0.5}}


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


def _processor(node):
    p = E.Params(node["id"], node["type"], num=node.get("params", {}))
    if node["type"] == "phaser":
        return P.Phaser(channels=3, config=E.phaser_params(p, FS))
    if node["type"] == "tremolo":
        return P.Tremolo(channels=3, config=E.tremolo_params(p, FS))
    return P.RingModulator(channels=3, config=E.ringmod_params(p, FS))


@pytest.mark.parametrize("node", [PHASER_NODE, TREMOLO_NODE, RINGMOD_NODE, {"id": "p", "type": "phaser"},
                                  {"id": "t", "type": "tremolo"}, {"id": "r", "type": "ringmod"}])
def test_graph_node_is_the_processor(gpu, node):
    x = noise(1500)
    ch, y = _chain_run(_graph([node]), x)
    assert ch.spec[1]["type"] == node["type"] and ch.op_count()[0] == 1
    compare(y, gpu_run(_processor(node), x), True, node["type"])
    y2 = x.copy()
    assert ch.Process(y2)
    assert np.any(y2 != y)  # state carries over calls
    ch.Reset()
    y3 = x.copy()
    assert ch.Process(y3)
    compare(y3, y, True, f"{node['type']} after Chain.Reset")


def test_graph_chain_with_dry_edge_bypass_and_reset(gpu):
    x = noise(2000)
    nodes = [PHASER_NODE, TREMOLO_NODE, RINGMOD_NODE]
    ch, y = _chain_run(_graph(nodes, dry_edge=True), x)
    assert [s["type"] for s in ch.spec] == ["input", "phaser", "tremolo", "ringmod", "output"]
    assert ch.spec[1]["phaser"]["stages"] == 4 and ch.spec[2]["tremolo"]["rate_hz"] == 9.0
    assert ch.spec[3]["ringmod"]["carrier_hz"] == 700.0

    def in_turn(ns, v):
        for nd in ns:
            v = gpu_run(_processor(nd), v)
        return v

    want = (in_turn(nodes, x) + x) * 0.5  # edge order: ringmod, _input
    compare(y, want, True, "phaser -> tremolo -> ringmod, averaged with the dry edge")
    y2 = x.copy()
    assert ch.Process(y2) and np.any(y2 != y)
    ch.Reset()  # every node: the same output again
    y3 = x.copy()
    assert ch.Process(y3)
    compare(y3, y, True, "after Chain.Reset")
    for skip in range(3):  # a bypassed node mixes only
        ns = [dict(nd, bypassed=(i == skip)) for i, nd in enumerate(nodes)]
        ch, y = _chain_run(_graph(ns), x)
        compare(y, in_turn([nd for i, nd in enumerate(nodes) if i != skip], x), True, f"bypassed {nodes[skip]['type']}")
    ch, y = _chain_run(_graph([dict(nd, bypassed=True) for nd in nodes]), x)
    compare(y, x, True, "everything bypassed")


def test_graph_node_without_config_is_refused(gpu):
    L = _lib.lib()
    par = (C.c_int32 * 1)(0)
    par2 = (C.c_int32 * 1)(1)
    for t, field, cfg in ((E.FXN_PHASER, "phaser", _lib.PhaserConfig), (E.FXN_TREMOLO, "tremolo", _lib.TremoloConfig),
                          (E.FXN_RINGMOD, "ringmod", _lib.RingModConfig)):
        nodes = (E._Node * 3)()
        nodes[0].type = E.FXN_INPUT
        nodes[1].type, nodes[1].n_parents, nodes[1].parents = t, 1, C.cast(par, C.POINTER(C.c_int32))
        nodes[2].type, nodes[2].n_parents, nodes[2].parents = E.FXN_OUTPUT, 1, C.cast(par2, C.POINTER(C.c_int32))
        ext = (E._NodeExt * 3)()
        h = C.c_void_p()
        rc = L.ad_fx_graph_create(C.cast(nodes, C.c_void_p), 3, 2, 0, C.byref(h))
        assert rc == _lib.AD_ERR_INVALID_ARGUMENT and not h.value
        for e in (None, C.cast(ext, C.c_void_p)):
            rc = L.ad_fx_graph_create_ext(C.cast(nodes, C.c_void_p), e, 3, 2, 0, C.byref(h))
            assert rc == _lib.AD_ERR_INVALID_ARGUMENT and not h.value
        # another node's config does not serve
        other = _lib.RingModConfig() if field != "ringmod" else _lib.TremoloConfig()
        setattr(ext[1], "tremolo" if field == "ringmod" else "ringmod", C.pointer(other))
        rc = L.ad_fx_graph_create_ext(C.cast(nodes, C.c_void_p), C.cast(ext, C.c_void_p), 3, 2, 0, C.byref(h))
        assert rc == _lib.AD_ERR_INVALID_ARGUMENT and not h.value
        good = cfg()
        getattr(L, f"ad_{field}_default_config")(C.byref(good), 48000.0)
        setattr(ext[1], field, C.pointer(good))
        rc = L.ad_fx_graph_create_ext(C.cast(nodes, C.c_void_p), C.cast(ext, C.c_void_p), 3, 2, 0, C.byref(h))
        assert rc == _lib.AD_OK and h.value
        L.ad_fx_graph_destroy(h)
    nodes[1].type = 14
    assert L.ad_fx_graph_create_ext(C.cast(nodes, C.c_void_p), None, 3, 2, 0, C.byref(h)) == 10  # AD_ERR_UNKNOWN_EFFECT


@pytest.mark.parametrize("fs,params", [(48000.0, {"maxFreqHz": 0.49 * 48000.0}), (3000.0, {"minFreqHz": 100, "maxFreqHz": 1000})])
def test_graph_phaser_that_fails_to_configure(gpu, fs, params):
    with pytest.raises(_lib.ErrInvalidArgument):
        E.Chain(fs, 2).LoadGraph(_graph([{"id": "p", "type": "phaser", "params": params}]))


def test_chorus_still_raises_unknown_effect(gpu):
    with pytest.raises(E.UnknownEffect):
        E.Chain(48000.0, 2).LoadGraph(_graph([{"id": "n", "type": "chorus"}]))
