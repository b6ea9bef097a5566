"""The GPU lookahead limiter against the restatement in tests/lookahead_ref.py.

On float64 bits: the detector envelope of every sample, the delayed program
samples, and the output given the device's own gain row.  The gain goes through
the device math library's log and exp2, so the gain row and the output end to
end are held to the de-esser's bars, 1e-12 relative RMS and 1e-10 max abs.
Each of these is asserted on its own after every call.

Shapes: D = 0, 1 and 144 (3 ms at 48 kHz) in calls of [300, 1, 399] (a call of
one sample, calls shorter and longer than D, the walk's tile of 32 ending inside
a call) on 1, 3 and 65 channels; D = 9600 (200 ms) on 3 channels in calls
shorter than, equal to and longer than D.  Noise at amplitude 1 against a
threshold of -12 dB, so the limiter is at work most of the time.
"""
import math

import numpy as np
import pytest
import torch

import lookahead_ref as R
from algodsp import _lib, processors as P, signals

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
RMS_BAR, ABS_BAR = 1e-12, 1e-10  # the de-esser's bars
FS = 48000.0
CUTS = [300, 1, 399]
NAN, INF = float("nan"), float("inf")


def noise(n, channels, seed, amplitude=1.0):
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
    assert rms <= RMS_BAR, (what, "relative rms", rms)
    assert worst <= ABS_BAR, (what, "max abs", worst)


def apply(obj, setup):
    for name, v in setup:
        getattr(obj, name)(*([] if v is None else [v]))
    return obj


def gpu_call(h, prog, side=None, pad=5):
    """One device call on rows of stride n + pad; returns the rewritten program rows."""
    ch, n = prog.shape
    d = torch.full((ch, n + pad), -777.25, dtype=torch.float64, device=DEV)
    d[:, :n] = torch.from_numpy(np.array(prog)).to(DEV)
    ds = None if side is None else torch.from_numpy(np.array(side).reshape(ch, -1)).to(DEV)
    h.process(d[:, :n], ds)
    torch.cuda.synchronize()
    assert bool((d[:, n:] == -777.25).all()), "padding written"
    if ds is not None:
        same_bits(ds.cpu().numpy(), np.array(side).reshape(ch, -1), "the sidechain rows are read only")
    return d[:, :n].cpu().numpy()


def check_call(h, ref, prog, side, what):
    """One call on both; every item of the parity target on its own."""
    n = prog.shape[1]
    got = gpu_call(h, prog, side)
    want = ref.process_many(prog, side)
    env, gain, delayed = ref.trace
    same_bits(h.last_envelope(n), env, f"{what}: envelope")
    same_bits([h.get_state(c) for c in range(ref.channels)], ref.envelope, f"{what}: envelope state")
    dev_gain = h.gain(env)
    same_bits(got, delayed * dev_gain, f"{what}: output given the device's gain row")
    quiet = dev_gain == 1.0
    same_bits(got[quiet], delayed[quiet], f"{what}: the delayed program where the gain is 1")
    within_bars(dev_gain, gain, f"{what}: gain row")
    within_bars(got, want, f"{what}: output end to end")
    return got


def run_case(channels, setup, cuts, side_mode="none", seed=0x100A, what=""):
    n = sum(cuts)
    prog = noise(n, channels, seed)
    side = None if side_mode == "none" else noise(n, channels, seed + 0x777, 1.5)
    h = apply(P.LookaheadLimiter(FS, channels), setup)
    ref = apply(R.LookaheadLimiter(FS, channels), setup)
    assert h.DelaySamples() == ref.delaySamples
    pos = 0
    for k in cuts:
        s = None
        if side is not None:
            s = side[:, pos:pos + (k if side_mode == "full" else k // 3)]  # "short": a third of the call, then zeros
        check_call(h, ref, prog[:, pos:pos + k], s, f"{what} [{pos}:{pos + k}]")
        pos += k
    return h, ref


@pytest.mark.parametrize("channels", [1, 3, 65])
@pytest.mark.parametrize("ms,delay", [(0.0, 0), (1.0 / 48.0, 1), (3.0, 144)])
def test_delays(gpu, ms, delay, channels):
    h, _ = run_case(channels, [("SetThreshold", -12.0), ("SetLookahead", ms)], CUTS, what=f"D {delay}, {channels} ch")
    assert h.DelaySamples() == delay


@pytest.mark.parametrize("side_mode", ["full", "short"])
@pytest.mark.parametrize("delay_ms", [0.0, 3.0])
def test_sidechain(gpu, delay_ms, side_mode):
    run_case(3, [("SetThreshold", -12.0), ("SetLookahead", delay_ms)], CUTS, side_mode,
             what=f"{side_mode} sidechain, {delay_ms} ms")


def test_empty_sidechain_reads_as_zeros(gpu):
    """No detector samples at all: the gain is exactly 1 and the output is the delayed program."""
    prog = noise(400, 2, 0xE0)
    h, ref = P.LookaheadLimiter(FS, 2), R.LookaheadLimiter(FS, 2)
    got = gpu_call(h, prog, np.zeros((2, 0)))
    same_bits(got, ref.process_many(prog, np.zeros((2, 0))), "empty sidechain")
    same_bits(got[:, 144:], prog[:, :-144], "the program, 144 samples late")
    assert not got[:, :144].any()


def test_long_delay_calls_shorter_equal_and_longer(gpu):
    """D = 9600 (200 ms): the history carries a whole call, exactly one, and less than one."""
    h, _ = run_case(3, [("SetThreshold", -6.0), ("SetLookahead", 200.0), ("SetRelease", 20.0)],
                    [5000, 9600, 12001, 37], what="D 9600")
    assert h.DelaySamples() == 9600


@pytest.mark.parametrize("ms,fs,delay", [(0.5, 1000.0, 1), (2.5, 1000.0, 3), (10.0, 44050.0, 441), (0.03125, 48000.0, 2),
                                         (4.5, 1000.0, 5)])
def test_delay_rounds_halves_away_from_zero(gpu, ms, fs, delay):
    setup = [("SetSampleRate", fs), ("SetLookahead", ms), ("SetThreshold", -9.0)]
    h = apply(P.LookaheadLimiter(FS, 2), setup)
    ref = apply(R.LookaheadLimiter(FS, 2), setup)
    assert h.DelaySamples() == ref.delaySamples == delay
    check_call(h, ref, noise(2 * delay + 40, 2, 0x4A1F), None, f"{ms} ms at {fs} Hz")


def test_reset_and_setters_between_blocks(gpu):
    """Every setter and Reset between calls: SetLookahead and SetSampleRate rebuild the line zeroed, also with
    an unchanged value, and keep the envelope; Reset clears both."""
    ch, blk = 3, 260
    steps = [("SetThreshold", -20.0), ("SetRelease", 5.0), ("SetLookahead", 3.0), ("SetLookahead", 1.0),
             ("SetSampleRate", 48000.0), ("SetSampleRate", 44100.0), ("Reset", None), ("SetLookahead", 0.0),
             ("SetThreshold", 0.0)]
    prog = noise(blk * (len(steps) + 1), ch, 0x5E7)
    h, ref = P.LookaheadLimiter(FS, ch), R.LookaheadLimiter(FS, ch)
    for i in range(len(steps) + 1):
        check_call(h, ref, prog[:, i * blk:(i + 1) * blk], None, f"block {i}, after {steps[:i][-1:]}")
        if i < len(steps):
            apply(h, [steps[i]])
            apply(ref, [steps[i]])
            assert h.DelaySamples() == ref.delaySamples
            if steps[i][0] != "Reset":
                same_bits([h.get_state(c) for c in range(ch)], ref.envelope, "the envelope stays")


def test_nonfinite_samples(gpu):
    """inf, NaN, zeros and denormals in one channel's program and detector; the neighbours are untouched."""
    ch, n = 3, 400
    prog = noise(n, ch, 0xBAD)
    clean = prog.copy()
    prog[1, 50:58] = [INF, -INF, 0.0, -0.0, 5e-324, -5e-324, 1e-310, 1e308]
    prog[1, 300] = NAN
    setup = [("SetThreshold", -12.0), ("SetLookahead", 0.5)]
    h, ref = apply(P.LookaheadLimiter(FS, ch), setup), apply(R.LookaheadLimiter(FS, ch), setup)
    got = gpu_call(h, prog)
    want = ref.process_many(prog)
    env, gain, delayed = ref.trace
    same_bits(h.last_envelope(n), env, "envelope")
    same_bits(got, delayed * h.gain(env), "output given the device's gain row")
    other = apply(R.LookaheadLimiter(FS, ch), setup).process_many(clean)
    within_bars(got[[0, 2]], other[[0, 2]], "the neighbours")
    assert np.isnan(got[1, 324:]).all() and np.isnan(want[1, 324:]).all()


def test_host_rows_and_refused_values(gpu):
    prog, side = noise(500, 2, 0x40), noise(200, 2, 0x41, 2.0)
    h, ref = P.LookaheadLimiter(FS, 2, threshold_db=-12.0), apply(R.LookaheadLimiter(FS, 2), [("SetThreshold", -12.0)])
    a = prog[:, :250].copy()
    h.ProcessInPlace(a)
    within_bars(a, ref.process_many(prog[:, :250]), "ProcessInPlace")
    b = prog[:, 250:].copy()
    h.ProcessInPlaceSidechain(b, side)
    within_bars(b, ref.process_many(prog[:, 250:], side), "ProcessInPlaceSidechain, short row")
    before = tuple(getattr(h.config(), k) for k, _ in _lib.LookaheadConfig._fields_)
    for name, v in [("SetThreshold", -30.0), ("SetThreshold", 0.5), ("SetThreshold", NAN), ("SetRelease", 0.5),
                    ("SetRelease", 5001.0), ("SetLookahead", -1.0), ("SetLookahead", 200.5), ("SetLookahead", INF),
                    ("SetSampleRate", 0.0), ("SetSampleRate", NAN)]:
        with pytest.raises(_lib.ErrInvalidArgument):
            getattr(h, name)(v)
        assert tuple(getattr(h.config(), k) for k, _ in _lib.LookaheadConfig._fields_) == before
    assert (h.SampleRate(), h.Threshold(), h.Release(), h.Lookahead()) == (FS, -12.0, 100.0, 3.0)
    d = torch.zeros((2, 64), dtype=torch.float64, device=DEV)
    with pytest.raises(_lib.ErrInvalidArgument):
        h.process(d[:, :40], d[:, 20:60])
