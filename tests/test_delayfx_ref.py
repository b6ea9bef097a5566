"""Delay, flanger and delay-simple checks that need no GPU: the reference
restatement (tests/delayfx_ref.py) against delay_test.go and flanger_test.go,
the dependency bounds the GPU kernels' blocks rest on, the ramp's fixed point,
the host-only part of the C ABI (defaults, validation, create without a
device), the graph compiler's parameter clamps, and how far a last-place
change of every sine moves the modulated flanger's output."""
import ctypes as C
import math

import numpy as np
import pytest

import delayfx_ref as R
from algodsp import _lib, effectchain as E, signals

NAN, INF = float("nan"), float("inf")


def noise(n, seed=0xDE1A):
    return signals.white_noise(n, seed)


def rel_rms(a, b):
    return float(np.sqrt(np.mean((a - b) ** 2)) / np.sqrt(np.mean(b ** 2)))


# ---- delay_test.go, on the restatement --------------------------------------
def test_delay_set_target_time_ramps_gradually():
    d = R.Delay(1000.0)
    d.SetTime(0.25)
    start = d.CurrentDelaySamples()
    d.SetTargetTime(0.01)
    d.process(np.zeros(10))
    assert 0.01 * 1000.0 < d.CurrentDelaySamples() < start


def test_delay_set_target_time_converges_to_target():
    d = R.Delay(1000.0)
    d.SetTime(0.25)
    d.SetTargetTime(0.01)
    d.process(np.zeros(500))
    assert abs(d.CurrentDelaySamples() - R.go_round(0.01 * 1000.0)) <= 0.5


def test_delay_set_time_snaps_immediately():
    d = R.Delay(1000.0)
    d.SetTime(0.25)
    d.SetTime(0.01)
    assert abs(d.CurrentDelaySamples() - R.go_round(0.01 * 1000.0)) <= 1e-9


def test_delay_process_in_place_matches_sample():
    x = np.sin(2 * math.pi * np.arange(128) / 29)
    d1, d2 = R.Delay(48000.0), R.Delay(48000.0)
    want = np.array([d1.ProcessSample(float(v)) for v in x])
    assert np.max(np.abs(d2.process(x) - want)) <= 1e-12


def test_delay_reset_restores_state():
    x = np.zeros(96)
    x[0] = 1
    d = R.Delay(48000.0)
    out1 = d.process(x)
    d.Reset()
    assert np.max(np.abs(d.process(x) - out1)) <= 1e-12


def test_delay_impulse_at_configured_time():
    d = R.Delay(1000.0)
    d.SetTime(0.01), d.SetMix(1), d.SetFeedback(0)
    x = np.zeros(20)
    x[0] = 1
    want = np.zeros(20)
    want[10] = 1
    assert np.max(np.abs(d.process(x) - want)) <= 1e-12


# ---- flanger_test.go, on the restatement ------------------------------------
def test_flanger_process_in_place_matches_process():
    x = np.sin(2 * math.pi * np.arange(128) / 29)
    f1, f2 = R.Flanger(48000.0), R.Flanger(48000.0)
    want = np.array([f1.Process(float(v)) for v in x])
    assert np.max(np.abs(f2.process(x) - want)) <= 1e-12


def test_flanger_reset_restores_state():
    x = np.zeros(96)
    x[0] = 1
    f = R.Flanger(48000.0)
    out1 = f.process(x)
    assert f.lfoPhase > 0
    f.Reset()
    assert f.lfoPhase == 0
    assert np.max(np.abs(f.process(x) - out1)) <= 1e-12


def test_flanger_impulse_at_configured_delay_when_depth_zero():
    f = R.Flanger(1000.0, base_delay_seconds=0.005, depth_seconds=0.0, mix=1.0, feedback=0.0)
    x = np.zeros(16)
    x[0] = 1
    want = np.zeros(16)
    want[5] = 1
    assert np.max(np.abs(f.process(x) - want)) <= 1e-12


def test_flanger_validation():
    with pytest.raises(ValueError):
        R.Flanger(0.0)
    with pytest.raises(ValueError):
        R.Flanger(48000.0, mix=2.0)
    with pytest.raises(ValueError):
        R.Flanger(48000.0, base_delay_seconds=0.009, depth_seconds=0.002)


def test_flanger_set_depth_rolls_back_on_invalid_combination():
    f = R.Flanger(48000.0, base_delay_seconds=0.0087, depth_seconds=0.0012)
    line = list(f.delayLine)
    with pytest.raises(ValueError):
        f.SetDepthSeconds(0.0014)
    assert (f.BaseDelaySeconds(), f.DepthSeconds()) == (0.0087, 0.0012) and f.delayLine == line
    f.SetDepthSeconds(0.0011)


def test_flanger_set_base_delay_rolls_back_on_invalid_combination():
    f = R.Flanger(48000.0, base_delay_seconds=0.004, depth_seconds=0.004)
    with pytest.raises(ValueError):
        f.SetBaseDelaySeconds(0.007)
    assert (f.BaseDelaySeconds(), f.DepthSeconds()) == (0.004, 0.004)
    f.SetBaseDelaySeconds(0.0055)


# ---- quirks -----------------------------------------------------------------
def test_delay_reset_keeps_current_samples_and_set_time_does_not_clamp():
    d = R.Delay(1000.0)
    d.SetTargetTime(0.01)
    d.process(noise(30))
    c = d.CurrentDelaySamples()
    assert 10 < c < 250
    d.Reset()
    assert d.CurrentDelaySamples() == c and d.write == 0 and not any(d.buffer)
    low = R.Delay(400.0)
    assert low.CurrentDelaySamples() == 100
    low.SetTime(0.001)  # round(0.4) = 0: SetTime does not clamp ...
    assert low.CurrentDelaySamples() == 0 and low.targetSamples == 0
    low.SetSampleRate(400.0)  # ... reconfigureBuffer does, also when the ring stays
    assert low.CurrentDelaySamples() == 1 and low.targetSamples == 1
    x = noise(50)
    low.SetTime(0.001)
    low.SetMix(1.0)
    y = low.process(x)  # delay 0 reads the slot about to be written: the sample of 801 samples ago
    assert not np.any(y)


def test_delay_resize_keeps_the_newest_history():
    d = R.Delay(8000.0)
    d.SetFeedback(0.0)
    x = noise(20000)
    d.process(x)
    assert len(d.buffer) == 16001 and d.write == 20000 - 16001
    d.SetSampleRate(11025.0)
    assert len(d.buffer) == 22051 and d.write == 0
    assert d.buffer[-16001:] == [float(v) for v in x[-16001:]] and not any(d.buffer[:-16001])
    assert d.currentSamples == d.targetSamples == R.go_round(0.25 * 11025.0)
    d.SetSampleRate(8000.0)
    assert d.buffer == [float(v) for v in x[-16001:]] and d.write == 0
    f = R.Flanger(48000.0, feedback=0.0, depth_seconds=0.0)
    f.process(x[:100])
    phase = f.lfoPhase
    assert len(f.delayLine) == 51
    f.SetBaseDelaySeconds(0.0005)
    assert len(f.delayLine) == 27 and f.delayLine == [float(v) for v in x[100 - 27:100]] and f.lfoPhase == phase
    f.SetDepthSeconds(0.0)  # the same length: nothing moves
    assert f.delayLine == [float(v) for v in x[100 - 27:100]] and f.write == 0


def test_simple_delay():
    x = noise(300)
    for ms, want in ((20.0, 160), (0.0, 0), (-5.0, 0), (900.0, 4000), (0.0625, 1)):
        s = R.SimpleDelay()
        s.Configure(8000.0, ms)
        assert s.delaySamples == want and len(s.buf) == want + 1
    s = R.SimpleDelay()
    s.Configure(8000.0, 12.5)
    y = np.concatenate([s.process(x[:7]), s.process(x[7:])])
    np.testing.assert_array_equal(y, np.concatenate([np.zeros(100), x[:200]]))
    s.Configure(8000.0, 12.5)  # the same size: state kept
    assert s.process(np.zeros(1))[0] == x[200]
    s.Configure(8000.0, 25.0)
    assert not any(s.buf) and s.write == 0


# ---- the dependency bounds --------------------------------------------------
def _delay_at(c, write=0, fs=48000.0, feedback=0.9):
    d = R.Delay(fs)
    d.SetFeedback(feedback)
    d.SetMix(0.5)
    d.currentSamples = d.targetSamples = c
    d.write = write
    return d


K = 48
DELAYS = [float(K), K + 0.5, K + 2.0 ** -40, K - 2.0 ** -40, 1.0, 2.0, 2.5, 0.0]


@pytest.mark.parametrize("write", [100, 70000, 95890])
@pytest.mark.parametrize("c", DELAYS)
def test_delay_block_form_equals_serial_up_to_the_bound(c, write):
    """Reading `raw` = max(1, floor(c) - 1) samples ahead of their writes
    changes no bit, nor does running `both` of them in the worst order.  For a
    c that is no integer and does not round to one, floor(c) + 1 samples do
    change bits (sample floor(c) of the block reads sample 0's write)."""
    x = noise(3 * K + 7)
    d = _delay_at(c, write)
    raw, both = d.block_bounds()
    assert raw == max(1, math.floor(c) - 1) and both == raw
    serial = d.process(x)
    np.testing.assert_array_equal(_delay_at(c, write).process(x, raw), serial)
    np.testing.assert_array_equal(_delay_at(c, write).process(x, both, reverse=True), serial)
    if c == K + 0.5:
        assert np.any(_delay_at(c, write).process(x, K + 1) != serial)


def test_delay_reference_fails_where_the_read_position_rounds_to_the_ring_length():
    """write - c just below 0 plus the ring length rounds to the ring length:
    the reference indexes one past its buffer there (Go panics).  The GPU
    kernel clamps r0 to len - 1, which makes frac 1 and the second tap slot 0,
    the value the unrounded position gives."""
    d = _delay_at(K + 2.0 ** -40, write=K)
    assert float(K) - d.currentSamples + 96001.0 == 96001.0
    with pytest.raises(IndexError):
        d.process(noise(1))


def test_delay_rounding_case_reads_one_slot_nearer():
    """float64(write) - c is rounded: for c just above an integer k and a write
    position of 2^14 or more it is write - k exactly, and the second tap is
    the write of only k - 1 samples ago, with weight 0.  A weight of 0 still
    makes NaN of a non-finite sample, so k - 1, not k, samples are free of
    each other: with an inf in the input a block of k samples changes bits."""
    c, write = K + 2.0 ** -40, 70000
    assert float(write) - c == float(write - K)
    x = noise(3 * K)
    x[K] = INF
    serial = _delay_at(c, write, feedback=0.0).process(x)
    assert math.isnan(serial[K + K - 1]) and not math.isnan(serial[K + K - 2])
    np.testing.assert_array_equal(_delay_at(c, write, feedback=0.0).process(x, K - 1), serial)
    ahead = _delay_at(c, write, feedback=0.0).process(x, K)
    assert not math.isnan(ahead[K + K - 1])
    # below 2^14 the difference is representable and the nearest tap is k samples back
    low = _delay_at(c, 5000, feedback=0.0)
    assert float(5000) - c != float(5000 - K)
    assert not math.isnan(low.process(x)[K + K - 1])


def test_delay_overwrite_bound_near_the_maximum_time():
    """At 2 s the read sits one slot ahead of the write: the sample read is
    overwritten by the very next one.  Read-ahead blocks stay exact (every
    read comes before every write); a launch without barriers may only take
    len - ceil(c) samples."""
    d = R.Delay(1000.0)
    d.SetTime(2.0)
    d.SetFeedback(0.9)
    assert d.block_bounds() == (1999, 1)
    x = noise(4500)

    def fresh():
        n = R.Delay(1000.0)
        n.SetTime(2.0), n.SetFeedback(0.9)
        return n

    serial = d.process(x)
    np.testing.assert_array_equal(fresh().process(x, 1999), serial)
    assert np.any(fresh().process(x, 2, reverse=True) != serial)
    d = R.Delay(1000.0)
    d.SetTime(1.9)
    assert d.block_bounds() == (1899, 101)
    serial = d.process(x)
    d = R.Delay(1000.0)
    d.SetTime(1.9)
    np.testing.assert_array_equal(d.process(x, 101, reverse=True), serial)
    d = R.Delay(1000.0)
    d.SetTime(1.9)
    assert np.any(d.process(x, 102, reverse=True) != serial)


@pytest.mark.parametrize("t0,t1", [(0.25, 0.01), (0.01, 0.25)])
def test_delay_bounds_hold_over_a_ramp(t0, t1):
    """The ramp is monotone and never leaves [min, max] of its start and its
    target, so the bounds taken at the call's start hold for the whole call."""
    x = noise(3000)

    def fresh():
        d = R.Delay(8000.0)
        d.SetTime(t0), d.SetTargetTime(t1), d.SetFeedback(0.9)
        return d

    d = fresh()
    raw, both = d.block_bounds()
    assert raw == 79 and both == 79
    lo, hi = sorted((d.currentSamples, d.targetSamples))
    prev = d.currentSamples
    for _ in range(3000):
        c = d.ramp_step()
        assert lo <= c <= hi and (c <= prev if t1 < t0 else c >= prev)
        prev = c
    serial = fresh().process(x)
    np.testing.assert_array_equal(fresh().process(x, raw), serial)
    np.testing.assert_array_equal(fresh().process(x, both, reverse=True), serial)


@pytest.mark.parametrize("base,fs,bound", [(0.0001, 48000.0, 3), (0.001, 48000.0, 47), (0.00101, 48000.0, 47),
                                           (0.0001, 8000.0, 1), (0.00025, 8000.0, 1), (0.008, 8000.0, 63)])
@pytest.mark.parametrize("depth", [0.0, 0.0015])
def test_flanger_block_form_equals_serial_up_to_the_bound(base, fs, bound, depth):
    """P = floor(max(1, base * fs)); max(1, P - 1) samples read none of each
    other's writes, whatever the modulation.  With depth 0 and a fractional
    base * fs one more sample changes bits (the tap at P - 1 has weight)."""
    x = noise(500)

    def run(block):
        f = R.Flanger(fs, base_delay_seconds=base, depth_seconds=depth, feedback=-0.9, rate_hz=5.0)
        assert f.block_bound() == bound
        return f.process(x, block)

    serial = run(1)
    np.testing.assert_array_equal(run(bound), serial)
    frac = base * fs - math.floor(base * fs)
    if depth == 0.0 and frac > 0 and base * fs > 2:
        assert np.any(run(bound + 1) != serial)


def test_flanger_modulation_stays_in_range():
    """mod = 0.5 (1 + s) is in [0, 1] for every s in [-1, 1], so the delay never drops below base * fs."""
    for s in (-1.0, math.nextafter(-1.0, 0.0), -0.0, 0.0, math.nextafter(1.0, 0.0), 1.0):
        mod = 0.5 * (1 + s)
        assert 0.0 <= mod <= 1.0
        for base in (0.0001, 0.001, 0.0087):
            assert (base + 0.0012 * mod) * 48000.0 >= base * 48000.0


# ---- the ramp's fixed point -------------------------------------------------
@pytest.mark.parametrize("fs", [8000.0, 48000.0, 192000.0])
def test_ramp_reaches_a_fixed_point(fs):
    """c += (target - c) k stops changing bitwise after finitely many steps and
    never moves again: the host computes the trajectory up to there and the
    kernel takes one scalar afterwards.  For the 0.25 s -> 2 s jump that takes
    2622, 14733 and 56273 steps at 8, 48 and 192 kHz with glibc's exp
    (about 30 time constants of fs / 100 samples); the host's trajectory of a
    call is never longer than that, whatever the call's length."""
    d = R.Delay(fs)
    d.SetTargetTime(2.0)
    steps, prev = 0, d.currentSamples
    while True:
        c = d.ramp_step()
        if c == prev:
            break
        assert c > prev
        prev, steps = c, steps + 1
    print(f"{fs} Hz: fixed point after {steps} steps, {d.targetSamples - c} short of the target")
    assert 25 * fs / 100 < steps < 45 * fs / 100
    for _ in range(1000):
        assert d.ramp_step() == c
    assert abs(d.targetSamples - c) * d.smoothCoeff <= math.ulp(c)  # it stalls where a step is under half an ulp


# ---- the host-only C ABI ----------------------------------------------------
BAD_DELAY_VALUES = [
    ("sample_rate", 0.0), ("sample_rate", -1.0), ("sample_rate", NAN), ("sample_rate", INF),
    ("time_seconds", 0.0009), ("time_seconds", 2.0001), ("time_seconds", NAN), ("time_seconds", INF),
    ("time_seconds", -1.0),
    ("feedback", -0.01), ("feedback", 0.991), ("feedback", NAN), ("feedback", INF),
    ("mix", -0.01), ("mix", 1.01), ("mix", NAN), ("mix", INF),
]
GOOD_DELAY_EDGES = [("sample_rate", 5e-324), ("time_seconds", 0.001), ("time_seconds", 2.0), ("feedback", 0.0),
                    ("feedback", 0.99), ("mix", 0.0), ("mix", 1.0)]
_DELAY_SETTER = {"sample_rate": "SetSampleRate", "time_seconds": "SetTime", "feedback": "SetFeedback", "mix": "SetMix"}

BAD_FLANGER_VALUES = [
    ("sample_rate", 0.0), ("sample_rate", -1.0), ("sample_rate", NAN), ("sample_rate", INF),
    ("rate_hz", 0.0), ("rate_hz", -1.0), ("rate_hz", NAN), ("rate_hz", INF),
    ("depth_seconds", -1e-9), ("depth_seconds", NAN), ("depth_seconds", INF), ("depth_seconds", 0.0091),
    ("base_delay_seconds", 0.00009), ("base_delay_seconds", 0.0101), ("base_delay_seconds", NAN),
    ("base_delay_seconds", INF), ("base_delay_seconds", 0.0086),
    ("feedback", -0.991), ("feedback", 0.991), ("feedback", NAN), ("feedback", INF),
    ("mix", -0.01), ("mix", 1.01), ("mix", NAN), ("mix", INF),
]
GOOD_FLANGER_EDGES = [("sample_rate", 5e-324), ("rate_hz", 5e-324), ("depth_seconds", 0.0), ("depth_seconds", 0.0089),
                      ("base_delay_seconds", 0.0001), ("base_delay_seconds", 0.0084), ("feedback", -0.99),
                      ("feedback", 0.99), ("mix", 0.0), ("mix", 1.0)]
_FLANGER_SETTER = {"sample_rate": "SetSampleRate", "rate_hz": "SetRateHz", "depth_seconds": "SetDepthSeconds",
                   "base_delay_seconds": "SetBaseDelaySeconds", "feedback": "SetFeedback", "mix": "SetMix"}


def _dcfg(fs=48000.0, **kv):
    cfg = _lib.DelayConfig()
    _lib.lib().ad_delay_default_config(C.byref(cfg), fs)
    for k, v in kv.items():
        setattr(cfg, k, v)
    return cfg


def _fcfg(fs=48000.0, **kv):
    cfg = _lib.FlangerConfig()
    _lib.lib().ad_flanger_default_config(C.byref(cfg), fs)
    for k, v in kv.items():
        setattr(cfg, k, v)
    return cfg


def _delay_state(d):
    return (d.sampleRate, d.delaySeconds, d.feedback, d.mix, d.targetSamples, d.currentSamples, d.smoothCoeff,
            list(d.buffer), d.write)


def _flanger_state(f):
    return (f.sampleRate, f.rateHz, f.depth, f.baseDelay, f.feedback, f.mix, f.lfoPhase, list(f.delayLine), f.write,
            f.maxDelay)


@pytest.mark.parametrize("field,value", BAD_DELAY_VALUES)
def test_delay_rejected_value_changes_nothing_and_fails_validation(field, value):
    d = R.Delay(1000.0)
    d.SetTargetTime(0.01)
    d.process(noise(40))
    before = _delay_state(d)
    with pytest.raises(ValueError):
        getattr(d, _DELAY_SETTER[field])(value)
    if field == "time_seconds":
        with pytest.raises(ValueError):
            d.SetTargetTime(value)
    assert _delay_state(d) == before
    assert _lib.lib().ad_delay_validate(C.byref(_dcfg(**{field: value}))) == _lib.AD_ERR_INVALID_ARGUMENT


@pytest.mark.parametrize("field,value", GOOD_DELAY_EDGES)
def test_delay_validation_accepts_range_edges(field, value):
    getattr(R.Delay(48000.0), _DELAY_SETTER[field])(value)
    assert _lib.lib().ad_delay_validate(C.byref(_dcfg(**{field: value}))) == _lib.AD_OK


@pytest.mark.parametrize("field,value", BAD_FLANGER_VALUES)
def test_flanger_rejected_value_changes_nothing_and_fails_validation(field, value):
    """0.0091 and 0.0086 are in their own ranges and fail base + depth > 0.01 (defaults 0.001 + 0.0015)."""
    f = R.Flanger(48000.0)
    f.process(noise(40))
    before = _flanger_state(f)
    with pytest.raises(ValueError):
        getattr(f, _FLANGER_SETTER[field])(value)
    assert _flanger_state(f) == before
    assert _lib.lib().ad_flanger_validate(C.byref(_fcfg(**{field: value}))) == _lib.AD_ERR_INVALID_ARGUMENT


@pytest.mark.parametrize("field,value", GOOD_FLANGER_EDGES)
def test_flanger_validation_accepts_range_edges(field, value):
    getattr(R.Flanger(48000.0), _FLANGER_SETTER[field])(value)
    assert _lib.lib().ad_flanger_validate(C.byref(_fcfg(**{field: value}))) == _lib.AD_OK


def test_validation_null_modes_and_oversized():
    L = _lib.lib()
    assert L.ad_delay_validate(None) == _lib.AD_ERR_INVALID_ARGUMENT
    assert L.ad_flanger_validate(None) == _lib.AD_ERR_INVALID_ARGUMENT
    assert L.ad_delay_validate(C.byref(_dcfg())) == _lib.AD_OK and L.ad_flanger_validate(C.byref(_fcfg())) == _lib.AD_OK
    assert L.ad_delay_validate(C.byref(_dcfg(smooth_coeff=0.25))) == _lib.AD_OK
    for k in (-0.1, 1.5, NAN):
        assert L.ad_delay_validate(C.byref(_dcfg(smooth_coeff=k))) == _lib.AD_ERR_INVALID_ARGUMENT
    assert L.ad_delay_validate(C.byref(_dcfg(mode=2))) == _lib.AD_ERR_INVALID_ARGUMENT
    # mode 1 looks at delay_samples only
    assert L.ad_delay_validate(C.byref(_dcfg(fs=0.0, mode=1, delay_samples=0))) == _lib.AD_OK
    assert L.ad_delay_validate(C.byref(_dcfg(mode=1, delay_samples=24000))) == _lib.AD_OK
    assert L.ad_delay_validate(C.byref(_dcfg(mode=1, delay_samples=-1))) == _lib.AD_ERR_INVALID_ARGUMENT
    assert L.ad_delay_validate(C.byref(_dcfg(mode=1, delay_samples=(1 << 27) + 1))) == _lib.AD_ERR_INVALID_ARGUMENT
    # rings the reference would allocate and this library refuses
    assert L.ad_delay_validate(C.byref(_dcfg(fs=1e8))) == _lib.AD_ERR_INVALID_ARGUMENT
    assert L.ad_flanger_validate(C.byref(_fcfg(fs=192000.0, base_delay_seconds=0.0001, depth_seconds=0.0098))) == _lib.AD_OK
    assert L.ad_flanger_validate(C.byref(_fcfg(fs=3e6))) == _lib.AD_ERR_INVALID_ARGUMENT


def test_default_configs_are_the_constructors():
    c = _dcfg(12345.0)
    assert [getattr(c, f) for f, _ in c._fields_] == [12345.0, 0.25, 0.35, 0.25, 0.0, 0, 0]
    d = R.Delay(12345.0)
    assert (d.sampleRate, d.delaySeconds, d.feedback, d.mix) == (12345.0, 0.25, 0.35, 0.25)
    assert d.currentSamples == d.targetSamples == 3086 and len(d.buffer) == 24691
    assert d.smoothCoeff == 1 - math.exp(-1 / (12345.0 * 0.010))
    c = _fcfg(12345.0)
    assert [getattr(c, f) for f, _ in c._fields_] == [12345.0, 0.25, 0.0015, 0.001, 0.25, 0.5]
    f = R.Flanger(12345.0)
    assert (f.sampleRate, f.rateHz, f.depth, f.baseDelay, f.feedback, f.mix) == (12345.0, 0.25, 0.0015, 0.001, 0.25, 0.5)
    assert len(f.delayLine) == 34 and f.maxDelay == 31


def test_create_validates_before_the_device():
    L = _lib.lib()
    h = C.c_void_p()
    for create, destroy, good, bad in (
            (L.ad_delay_create, L.ad_delay_destroy, _dcfg(), _dcfg(mix=1.5)),
            (L.ad_flanger_create, L.ad_flanger_destroy, _fcfg(), _fcfg(base_delay_seconds=0.009, depth_seconds=0.002))):
        assert create(C.byref(bad), 2, 0, C.byref(h)) == _lib.AD_ERR_INVALID_ARGUMENT and not h.value
        assert create(C.byref(good), 0, 0, C.byref(h)) == _lib.AD_ERR_INVALID_ARGUMENT
        assert create(None, 1, 0, C.byref(h)) == _lib.AD_ERR_INVALID_ARGUMENT
        rc = create(C.byref(good), 2, 0, C.byref(h))
        if _lib.device_count() == 0:
            assert rc == _lib.AD_ERR_NO_DEVICE and not h.value  # no CPU path
        else:
            assert rc == _lib.AD_OK
            destroy(h)
    assert L.ad_delay_set_param(None, 1, 0.5) == _lib.AD_ERR_INVALID_ARGUMENT
    assert L.ad_flanger_set_param(None, 1, 0.5) == _lib.AD_ERR_INVALID_ARGUMENT
    assert L.ad_delay_process_device(None, None, 0, 0, None) == _lib.AD_ERR_INVALID_ARGUMENT
    assert L.ad_flanger_process_device(None, None, 0, 0, None) == _lib.AD_ERR_INVALID_ARGUMENT


# ---- the graph compiler -----------------------------------------------------
def _fields(c):
    return [getattr(c, f) for f, _ in c._fields_]


def test_delay_params_defaults_and_clamps():
    assert _fields(E.delay_params(E.Params("d", "delay"), 48000.0)) == [48000.0, 0.25, 0.35, 0.25, 0.0, 0, 0]
    hi = E.delay_params(E.Params("d", "delay", num=dict(time=9, feedback=9, mix=9)), 44100.0)
    assert _fields(hi) == [44100.0, 2, 0.99, 1, 0.0, 0, 0]
    lo = E.delay_params(E.Params("d", "delay", num=dict(time=0, feedback=-1, mix=-1)), 44100.0)
    assert _fields(lo) == [44100.0, 0.001, 0, 0, 0.0, 0, 0]
    nan = E.delay_params(E.Params("d", "delay", num=dict(time=NAN, mix=INF)), 44100.0)
    assert (nan.time_seconds, nan.mix) == (0.25, 0.25)
    for c in (hi, lo):
        assert _lib.lib().ad_delay_validate(C.byref(c)) == _lib.AD_OK


def test_flanger_params_defaults_and_clamps():
    assert _fields(E.flanger_params(E.Params("f", "flanger"), 48000.0)) == [48000.0, 0.25, 0.0015, 0.001, 0.25, 0.5]
    hi = E.flanger_params(E.Params("f", "flanger", num=dict(rateHz=9, baseDelay=9, depth=9, feedback=9, mix=9)), 44100.0)
    assert _fields(hi) == [44100.0, 5, 0.0099, 0.01, 0.99, 1]
    # each value is inside its own clamp, the sum is not: configureFlanger fails there, and so does validation
    assert _lib.lib().ad_flanger_validate(C.byref(hi)) == _lib.AD_ERR_INVALID_ARGUMENT
    lo = E.flanger_params(E.Params("f", "flanger", num=dict(rateHz=0, baseDelay=0, depth=-1, feedback=-9, mix=-1)),
                          44100.0)
    assert _fields(lo) == [44100.0, 0.05, 0, 0.0001, -0.99, 0]
    assert _lib.lib().ad_flanger_validate(C.byref(lo)) == _lib.AD_OK


def test_simple_delay_samples_defaults_and_clamps():
    assert E.simple_delay_samples(E.Params("s", "delay-simple"), 48000.0) == 960
    for ms, fs, want in ((500, 48000.0, 24000), (900, 48000.0, 24000), (-3, 48000.0, 0), (0, 48000.0, 0),
                         (0.0625, 8000.0, 1), (0.06, 8000.0, 0), (NAN, 8000.0, 160)):
        assert E.simple_delay_samples(E.Params("s", "delay-simple", num=dict(delayMs=ms)), fs) == want
        s = R.SimpleDelay()
        s.Configure(fs, 20.0 if ms != ms else ms)
        assert s.delaySamples == want


def _graph(node):
    return E._graph_json([node], [(E.INPUT_NODE_ID, node["id"]), (node["id"], E.OUTPUT_NODE_ID)])


@pytest.mark.parametrize("node,kind", [({"id": "n", "type": "delay"}, "delay"),
                                       ({"id": "n", "type": "delay-simple"}, "delay"),
                                       ({"id": "n", "type": "flanger"}, "flanger")])
def test_graph_compiler_knows_the_delay_nodes(node, kind):
    """They compile; without a device they fail at the device, not as an unknown effect."""
    ch = E.Chain(48000.0, 2)
    if _lib.device_count() == 0:
        with pytest.raises(_lib.ADError) as e:
            ch.LoadGraph(_graph(node))
        assert e.value.code == _lib.AD_ERR_NO_DEVICE
    else:
        ch.LoadGraph(_graph(node))
        assert ch.spec[1]["type"] == kind


def test_fx_node_layout_keeps_the_old_fields_in_place():
    names = [f for f, _ in E._Node._fields_]
    assert names[-3:] == ["fdn", "delay", "flanger"] and names[0] == "type"
    assert E._Node.delay.offset == E._Node.fdn.offset + C.sizeof(C.c_void_p)
    assert (E.FXN_DELAY, E.FXN_FLANGER) == (9, 10)


@pytest.mark.parametrize("t", ["chorus", "dyn-lookahead", "filter-moog", "vocoder"])
def test_unknown_effect_still_raises(t):
    with pytest.raises(E.UnknownEffect):
        E.Chain(48000.0, 2).LoadGraph(_graph({"id": "n", "type": t}))


# ---- the sine spread --------------------------------------------------------
# (options, n): the modulated cases of tests/test_delayfx_gpu.py
MODULATED = [(dict(), 6000),
             (dict(rate_hz=5.0, base_delay_seconds=0.001, depth_seconds=0.0099 - 0.001, feedback=0.7), 6000)]


@pytest.mark.parametrize("options,n", MODULATED)
def test_flanger_sine_spread(options, n):
    """Every sine moved by a random -1 / 0 / +1 ulp moves the output by less
    than 2.5e-13 relative RMS and 2.5e-11 absolute, a quarter of the GPU
    tests' bars (1e-12, 1e-10)."""
    x = noise(n)
    plain, nudged = R.Flanger(48000.0, **options), R.Flanger(48000.0, sin=R.nudged_sin(0xF1A), **options)
    a, b = plain.process(x), nudged.process(x)
    spread, mx = rel_rms(b, a), float(np.max(np.abs(a - b)))
    print(f"{options}: sine spread rel rms {spread:.3g}, max abs {mx:.3g}")
    assert np.any(a != b)
    assert 4 * spread <= 1e-12 and 4 * mx <= 1e-10
