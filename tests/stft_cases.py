"""The inputs, cases and bars the STFT tests share (test_stft_ref.py on the CPU,
test_stft_gpu.py on the device).

A case's bar comes from the restatement alone: its analysis spectra are
perturbed at PERTURB_UNITS of eps * sqrt(log2 N) * ||frame||_2 per bin (the
project's own transforms measure 5.6 units at worst, README), over SEEDS seeds,
and the bar is BAR_FACTOR times the largest deviation seen.  The factor covers
the inverse transform and the device's atan2, hypot and sincos, which the
perturbation does not model.  Deviations are taken on the overlap-add sums,
(a - b) * norm where norm > 1e-12, as relative RMS and max abs; after the time
stretch's resampling there is no norm left to multiply by and they are taken
on the output itself, for the bar and for the device alike.
"""
from __future__ import annotations

import functools
import math

import numpy as np

import stft_ref as R
from algodsp import signals

FS = 48000.0
AMPLITUDE = 0.5
SEED = 0x57F7
EPS = 2.0 ** -52
PERTURB_UNITS = 6.0
SEEDS = 5
BAR_FACTOR = 4.0
BAD_CASE_RMS = 2.5e-10  # a case whose perturbed deviation alone exceeds this is badly chosen
MARGIN_FLOOR = 1e-9
CUTS = (700, 1, 800)


def noise(n: int, channels: int, seed: int = SEED) -> np.ndarray:
    """Distinct noise per channel at amplitude 0.5."""
    return np.stack([signals.white_noise(n, seed + c) for c in range(channels)]) * AMPLITUDE


def lengths(frame: int, hop: int):
    return (1, frame - 1, 2 * frame + 37, 5 * hop + 3)


# (frame, hop, n, channels): every frame size with hops N/4, 3N/8 and N-1 at the four lengths, three channels;
# one and 65 channels at one shape each; hop 1 at N = 64
FREEZE_SHAPES = [(N, hop, n, 3) for N in (64, 256, 1024, 4096) for hop in (N // 4, 3 * N // 8, N - 1)
                 for n in lengths(N, hop)]
FREEZE_SHAPES += [(256, 64, 549, 1), (256, 96, 549, 65), (64, 1, 200, 3)]
FREEZE_SHAPES += [(128, 32, 293, 3), (512, 192, 1061, 3), (2048, 512, 4133, 3)]  # the frame sizes in between

# (ratio, frame, hop, n, channels); no length with (n - 1) % hop == 1 (a last frame of one windowed impulse: all ties)
PITCH_RATIOS_BINSHIFT = (0.9, 1.1, 1.15)
PITCH_RATIOS_STRETCH = (0.5, 1.5, 2.0 ** (5.0 / 12.0))
PITCH_CASES = [(r, 256, 64, 549, 3) for r in PITCH_RATIOS_BINSHIFT + PITCH_RATIOS_STRETCH]
PITCH_CASES += [(1.1, 1024, 256, 2085, 65), (1.5, 1024, 384, 2085, 65), (0.9, 64, 24, 165, 1), (0.5, 64, 63, 318, 1),
                (1.15, 4096, 1024, 8229, 1), (1.5, 4096, 1536, 8229, 1), (1.1, 64, 3, 200, 3),
                (1.2, 64, 2, 201, 3)]  # round(2 * 1.2) = 2: a time stretch whose synthesis hop equals the hop
# the frame sizes in between: the walk holds 1, 2, 3 or 5 bins per thread by the frame size
PITCH_CASES += [(1.1, 128, 32, 293, 3), (1.5, 512, 128, 1061, 3), (1.1, 2048, 512, 4133, 1), (1.5, 2048, 768, 4133, 1)]
# Hop 1 is a freeze shape only.  Under the pitch shifter its last frame is x[n-1] * w[0] = 0, silent, after a
# frame of one windowed impulse: delta = 0 - (pi - omega) - omega sits on the wrap boundary exactly, in a frame
# whose magnitudes are zero.  The margins below could not hold there, so the smallest pitch hops are 2 and 3.


def make_freeze(frame, hop, mix=1.0, mode=R.PHASE_ADVANCE, frozen=False):
    r = R.SpectralFreeze(FS)
    r.SetFrameSize(frame)
    r.SetHopSize(hop)
    r.SetMix(mix)
    r.SetPhaseMode(mode)
    r.SetFrozen(frozen)
    return r


def make_pitch(ratio, frame, hop):
    r = R.SpectralPitchShifter(FS)
    r.SetFrameSize(frame)
    r.SetAnalysisHop(hop)
    r.SetPitchRatio(ratio)
    return r


def perturb_hook(seed: int):
    rng = np.random.default_rng(seed)

    def hook(frame, X, frame_norm):
        n = len(X)
        sigma = PERTURB_UNITS * EPS * math.sqrt(math.log2(n)) * frame_norm
        return X + sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n)) / math.sqrt(2.0)

    return hook


def resampled(r) -> bool:
    return isinstance(r, R.SpectralPitchShifter) and not r.use_bin_shifting() and r.synthesisHop != r.analysisHop \
        and abs(r.pitchRatio - 1) > R.IDENTITY_EPS


def deviation(got, want, norm):
    """(relative RMS, max abs) of got - want on the overlap-add sums; norm None: on the output itself."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if norm is None:
        scale = np.ones(len(want))
    else:
        nn = np.zeros(len(want))
        m = min(len(want), len(norm))
        nn[:m] = norm[:m]
        scale = np.where(nn > R.NORM_FLOOR, nn, 1.0)
    d = (got - want) * scale
    w = want * scale
    rms = math.sqrt(float(np.mean(d * d))) / max(math.sqrt(float(np.mean(w * w))), 1e-300)
    return rms, float(np.max(np.abs(d)))


def run(make, x, cuts=None, hook=None):
    """One channel through a fresh restatement in calls of `cuts`: (outputs per call, norms per call, the instance)."""
    r = make()
    r.spectrum_hook = hook
    outs, norms = [], []
    pos = 0
    for m in cuts or (len(x),):
        outs.append(r.Process(x[pos:pos + m]))
        norms.append(None if resampled(r) or r.last_norm is None else r.last_norm)
        pos += m
    return outs, norms, r


class Bar:
    def __init__(self, rms, worst, clean, norms, margins, refs, held_abs):
        self.rms, self.abs = rms, worst
        self.refs = refs  # [channel] the clean instances after their last call
        self.held_abs = held_abs  # the freeze's heldMagnitude: max abs
        self.clean = clean  # [channel][call] unperturbed outputs
        self.norms = norms  # [channel][call]
        self.margins = margins
        self.perturbed_rms = rms / BAR_FACTOR

    def check(self, got, channel, call=0, what=""):
        rms, worst = deviation(got, self.clean[channel][call], self.norms[channel][call])
        print(f"{what} ch {channel} call {call}: relative rms {rms:.3e} (bar {self.rms:.3e}), "
              f"max abs {worst:.3e} (bar {self.abs:.3e})")
        assert rms <= self.rms and worst <= self.abs, (what, channel, call, rms, worst, self.rms, self.abs)
        return rms, worst


def bar_for(make, x, cuts=None, bar_channels=(0, 1, -1), on_output=False) -> Bar:
    """The clean outputs of every channel of x and the case's bar from the channels in bar_channels;
    on_output: deviations on the output itself (for outputs that are mixed further)."""
    x = np.atleast_2d(x)
    clean, norms, refs = [], [], []
    margins = R.Margins()
    for c in range(x.shape[0]):
        o, nm, r = run(make, x[c], cuts)
        if on_output:
            nm = [None] * len(nm)
        clean.append(o)
        norms.append(nm)
        refs.append(r)
        for f in ("peak_gap", "wrap_gap", "dc_re", "nyq_re"):
            setattr(margins, f, min(getattr(margins, f), getattr(r.margins, f)))
    rms = worst = held = 0.0
    for c in sorted({ch % x.shape[0] for ch in bar_channels}):
        for seed in range(SEEDS):
            o, _, r = run(make, x[c], cuts, perturb_hook(1000 * c + seed))
            if hasattr(r, "heldMagnitude"):
                held = max(held, float(np.max(np.abs(r.heldMagnitude - refs[c].heldMagnitude))))
            for k in range(len(o)):
                a, b = deviation(o[k], clean[c][k], norms[c][k])
                rms, worst = max(rms, a), max(worst, b)
    return Bar(BAR_FACTOR * rms, BAR_FACTOR * worst, clean, norms, margins, refs, BAR_FACTOR * held)


@functools.lru_cache(maxsize=None)
def freeze_bar(frame, hop, n, channels, mix=1.0, mode=R.PHASE_ADVANCE, frozen=False, cuts=None) -> Bar:
    return bar_for(lambda: make_freeze(frame, hop, mix, mode, frozen), noise(n, channels), cuts)


@functools.lru_cache(maxsize=None)
def pitch_bar(ratio, frame, hop, n, channels) -> Bar:
    return bar_for(lambda: make_pitch(ratio, frame, hop), noise(n, channels))
