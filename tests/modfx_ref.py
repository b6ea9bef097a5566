"""modulation.Phaser (dsp/effects/modulation/phaser.go), Tremolo (tremolo.go)
and RingModulator (ring_modulator.go) restated in plain Python: one instance,
a per-sample loop, IEEE doubles in the reference's operation order.  It is the
oracle of the phaser, tremolo and ring modulator tests.

Python floats do not fuse, and math.sin / math.tan / math.exp are the host C
library's.  What the GPU handle cannot share with Python bit for bit by
construction is an argument: `sin` and `tan` (math.sin and math.tan by
default), the tremolo's smoothing coefficient (assign `smoothingCoef`), and,
per call, `process(x, table)`: the per-sample values a GPU call took from the
phase (the phaser's allpass coefficient, the tremolo's gain currentMod, the
ring modulator's carrier), used instead of the instance's own.  The phase
always advances as the reference's does.
"""
from __future__ import annotations

import math

import numpy as np

# phaser.go:8-17
DEFAULT_PHASER = dict(rate_hz=0.4, min_freq_hz=300.0, max_freq_hz=1600.0, stages=6, feedback=0.2, mix=0.5)
MAX_PHASER_STAGES, PHASER_NYQUIST_SAFETY = 12, 0.49
# tremolo.go:8-13
DEFAULT_TREMOLO = dict(rate_hz=4.0, depth=0.6, smoothing_ms=5.0, mix=1.0)
# ring_modulator.go:8-11
DEFAULT_RINGMOD = dict(carrier_hz=440.0, mix=1.0)

TWO_PI = 2 * math.pi


def _bad(v):
    return math.isnan(v) or math.isinf(v)


def _pos(v, what):
    if v <= 0 or _bad(v):
        raise ValueError(f"{what} must be > 0 and finite")


def _unit(v, what):
    if v < 0 or v > 1 or _bad(v):
        raise ValueError(f"{what} must be in [0, 1]")


def phase_step(phase, inc):
    """phaser.go:279-282, tremolo.go:211-214, ring_modulator.go:147-150."""
    phase += inc
    if phase >= TWO_PI:
        phase -= TWO_PI
    return phase


def phases(phase, inc, n):
    """The phase each of the next n samples sees, and the one after them."""
    out = np.empty(n)
    for i in range(n):
        out[i] = phase
        phase = phase_step(phase, inc)
    return out, phase


def allpass_coefficient(freq_hz, sample_rate, tan=math.tan):
    """phaserAllpassCoefficient phaser.go:365-379."""
    max_freq = PHASER_NYQUIST_SAFETY * sample_rate
    if freq_hz < 1:
        freq_hz = 1.0
    elif freq_hz > max_freq:
        freq_hz = max_freq
    g = tan(math.pi * freq_hz / sample_rate)
    if _bad(g):
        return 0.0
    return (1 - g) / (1 + g)


class Phaser:
    """NewPhaser(sample_rate, options...) (:146-180); the options are keywords."""

    def __init__(self, sample_rate, sin=math.sin, tan=math.tan, **options):
        _pos(sample_rate, "phaser sample rate")
        cfg = dict(DEFAULT_PHASER)
        for k, v in options.items():  # the With* options (:43-110)
            if k not in cfg:
                raise TypeError(k)
            cfg[k] = v
        _pos(cfg["rate_hz"], "phaser rate")
        _pos(cfg["min_freq_hz"], "phaser min frequency")
        if cfg["max_freq_hz"] <= cfg["min_freq_hz"] or _bad(cfg["max_freq_hz"]):
            raise ValueError("phaser max frequency must be > min frequency and finite")
        self.sin, self.tan = sin, tan
        self.sampleRate = sample_rate
        self.rateHz, self.minFreqHz, self.maxFreqHz = cfg["rate_hz"], cfg["min_freq_hz"], cfg["max_freq_hz"]
        self.feedback, self.mix = cfg["feedback"], cfg["mix"]
        self.lfoPhase = self.feedbackSample = 0.0
        if cfg["stages"] < 1 or cfg["stages"] > MAX_PHASER_STAGES:
            raise ValueError("phaser stages must be in [1, 12]")
        self.stages = [[0.0, 0.0] for _ in range(cfg["stages"])]  # x1, y1
        self._validate()

    def _validate(self):  # validateParams :323-358
        _pos(self.sampleRate, "phaser sample rate")
        _pos(self.rateHz, "phaser rate")
        _pos(self.minFreqHz, "phaser min frequency")
        if self.maxFreqHz <= self.minFreqHz or _bad(self.maxFreqHz):
            raise ValueError("phaser max frequency must be > min frequency and finite")
        if self.maxFreqHz >= PHASER_NYQUIST_SAFETY * self.sampleRate:
            raise ValueError("phaser max frequency must be < 0.49 of the sample rate")
        if len(self.stages) < 1 or len(self.stages) > MAX_PHASER_STAGES:
            raise ValueError("phaser stages must be in [1, 12]")
        if self.feedback < -0.99 or self.feedback > 0.99 or _bad(self.feedback):
            raise ValueError("phaser feedback must be in [-0.99, 0.99]")
        _unit(self.mix, "phaser mix")

    def SetSampleRate(self, v):  # :183-191 (the value stays when validateParams then fails)
        _pos(v, "phaser sample rate")
        self.sampleRate = v
        self._validate()

    def SetRateHz(self, v):  # :194-202
        _pos(v, "phaser rate")
        self.rateHz = v

    def SetFrequencyRangeHz(self, lo, hi):  # :205-218 (the values stay when validateParams then fails)
        _pos(lo, "phaser min frequency")
        if hi <= lo or _bad(hi):
            raise ValueError("phaser max frequency must be > min frequency and finite")
        self.minFreqHz, self.maxFreqHz = lo, hi
        self._validate()

    def SetStages(self, k):  # :221-233
        if k < 1 or k > MAX_PHASER_STAGES:
            raise ValueError("phaser stages must be in [1, 12]")
        if k == len(self.stages):
            return
        self.stages = [[0.0, 0.0] for _ in range(k)]

    def SetFeedback(self, v):  # :236-244
        if v < -0.99 or v > 0.99 or _bad(v):
            raise ValueError("phaser feedback must be in [-0.99, 0.99]")
        self.feedback = v

    def SetMix(self, v):  # :247-255
        _unit(v, "phaser mix")
        self.mix = v

    def Reset(self):  # :258-265
        for s in self.stages:
            s[0] = s[1] = 0.0
        self.feedbackSample = 0.0
        self.lfoPhase = 0.0

    def inc(self):
        return TWO_PI * self.rateHz / self.sampleRate  # :279

    def coefficient(self):  # modulatedFrequency :360-363, then :365-379
        lfo = 0.5 * (1 + self.sin(self.lfoPhase))
        return allpass_coefficient(self.minFreqHz + (self.maxFreqHz - self.minFreqHz) * lfo, self.sampleRate, self.tan)

    def Process(self, sample, coef=None):  # :268-285
        x = sample + self.feedbackSample * self.feedback
        if coef is None:
            coef = self.coefficient()
        y = x
        for s in self.stages:  # phaserAllpassStage.process :122-128
            xin = y
            y = coef * xin + s[0] - coef * s[1]
            s[0], s[1] = xin, y
        self.feedbackSample = y
        self.lfoPhase = phase_step(self.lfoPhase, self.inc())
        return sample * (1 - self.mix) + y * self.mix

    def process(self, x, table=None) -> np.ndarray:
        x = np.asarray(x, dtype=np.float64)
        return np.array([self.Process(float(v), None if table is None else float(table[i])) for i, v in enumerate(x)],
                        dtype=np.float64)


def smoothing_coefficient(smoothing_ms, sample_rate):
    """updateSmoothingCoefficient tremolo.go:273-289."""
    if smoothing_ms <= 0:
        return 1.0
    tau = smoothing_ms / 1000
    den = tau * sample_rate
    k = 1 - math.exp(-1 / den) if den != 0 else 1.0  # Go: -1/0 is -Inf, and exp(-Inf) is 0
    return min(max(k, 0.0), 1.0)


class Tremolo:
    """NewTremolo(sample_rate, options...) (:100-135)."""

    def __init__(self, sample_rate, sin=math.sin, **options):
        _pos(sample_rate, "tremolo sample rate")
        cfg = dict(DEFAULT_TREMOLO)
        for k, v in options.items():
            if k not in cfg:
                raise TypeError(k)
            cfg[k] = v
        self.sin = sin
        self.sampleRate = sample_rate
        self.rateHz, self.depth, self.smoothing, self.mix = cfg["rate_hz"], cfg["depth"], cfg["smoothing_ms"], cfg["mix"]
        self.lfoPhase, self.currentMod = 0.0, 1.0
        _pos(self.rateHz, "tremolo rate")  # validateParams :249-271
        _unit(self.depth, "tremolo depth")
        if self.smoothing < 0 or _bad(self.smoothing):
            raise ValueError("tremolo smoothing must be >= 0 and finite")
        _unit(self.mix, "tremolo mix")
        self.smoothingCoef = smoothing_coefficient(self.smoothing, self.sampleRate)

    def SetSampleRate(self, v):  # :138-147
        _pos(v, "tremolo sample rate")
        self.sampleRate = v
        self.smoothingCoef = smoothing_coefficient(self.smoothing, self.sampleRate)

    def SetRateHz(self, v):  # :150-158
        _pos(v, "tremolo rate")
        self.rateHz = v

    def SetDepth(self, v):  # :161-169
        _unit(v, "tremolo depth")
        self.depth = v

    def SetSmoothingMs(self, v):  # :172-181
        if v < 0 or _bad(v):
            raise ValueError("tremolo smoothing must be >= 0 and finite")
        self.smoothing = v
        self.smoothingCoef = smoothing_coefficient(self.smoothing, self.sampleRate)

    def SetMix(self, v):  # :184-192
        _unit(v, "tremolo mix")
        self.mix = v

    def Reset(self):  # :195-198
        self.lfoPhase, self.currentMod = 0.0, 1.0

    def inc(self):
        return TWO_PI * self.rateHz / self.sampleRate  # :211

    def target(self):  # targetModulation :291-294
        lfo = 0.5 * (1 + self.sin(self.lfoPhase))
        return (1 - self.depth) + self.depth * lfo

    def Process(self, sample, gain=None):  # :201-217
        if gain is not None:
            self.currentMod = gain
        else:
            t = self.target()
            if self.smoothingCoef >= 1:
                self.currentMod = t
            else:
                self.currentMod += (t - self.currentMod) * self.smoothingCoef
        wet = sample * self.currentMod
        self.lfoPhase = phase_step(self.lfoPhase, self.inc())
        return sample * (1 - self.mix) + wet * self.mix

    def process(self, x, table=None) -> np.ndarray:
        x = np.asarray(x, dtype=np.float64)
        return np.array([self.Process(float(v), None if table is None else float(table[i])) for i, v in enumerate(x)],
                        dtype=np.float64)


class RingModulator:
    """NewRingModulator(sample_rate, options...) (:74-100)."""

    def __init__(self, sample_rate, sin=math.sin, **options):
        _pos(sample_rate, "ring modulator sample rate")
        cfg = dict(DEFAULT_RINGMOD)
        for k, v in options.items():
            if k not in cfg:
                raise TypeError(k)
            cfg[k] = v
        _pos(cfg["carrier_hz"], "ring modulator carrier frequency")  # :29-39
        _unit(cfg["mix"], "ring modulator mix")  # :42-52
        self.sin = sin
        self.sampleRate, self.carrierHz, self.mix = sample_rate, cfg["carrier_hz"], cfg["mix"]
        self.phase = 0.0
        self._update()

    def _update(self):  # updatePhaseIncrement :176-178
        self.phaseInc = TWO_PI * self.carrierHz / self.sampleRate

    def SetSampleRate(self, v):  # :103-112
        _pos(v, "ring modulator sample rate")
        self.sampleRate = v
        self._update()

    def SetCarrierHz(self, v):  # :115-124
        _pos(v, "ring modulator carrier frequency")
        self.carrierHz = v
        self._update()

    def SetMix(self, v):  # :127-135
        _unit(v, "ring modulator mix")
        self.mix = v

    def Reset(self):  # :138-140
        self.phase = 0.0

    def inc(self):
        return self.phaseInc

    def Process(self, sample, carrier=None):  # :143-153
        if carrier is None:
            carrier = self.sin(self.phase)
        wet = sample * carrier
        self.phase = phase_step(self.phase, self.phaseInc)
        return sample * (1 - self.mix) + wet * self.mix

    def process(self, x, table=None) -> np.ndarray:
        x = np.asarray(x, dtype=np.float64)
        return np.array([self.Process(float(v), None if table is None else float(table[i])) for i, v in enumerate(x)],
                        dtype=np.float64)


def process_many(ref, x, table=None) -> np.ndarray:
    """`ref` over x [channels][n], every channel an instance of its own in the
    same state: the per-sample loop with the channels as a numpy vector (the
    element-wise operations are the scalar ones, rounded one by one).  The
    phase, the sines and the tremolo's gain are one sequence for all of them."""
    x = np.asarray(x, dtype=np.float64)
    y = np.empty_like(x)
    with np.errstate(all="ignore"):
        for i in range(x.shape[1]):
            y[:, i] = ref.Process(x[:, i], None if table is None else float(table[i]))
    return y


def nudged(fn, seed: int, lo=-math.inf, hi=math.inf):
    """`fn` moved by a seeded random -1 / 0 / +1 ulp per call, kept in [lo, hi]."""
    rng = np.random.default_rng(seed)
    state = {"k": 0, "steps": rng.integers(-1, 2, size=1 << 16)}

    def f(v):
        k = state["k"]
        if k == state["steps"].size:
            state["steps"] = rng.integers(-1, 2, size=1 << 16)
            k = 0
        state["k"] = k + 1
        s = fn(v)
        step = state["steps"][k]
        if step == 0:
            return s
        return min(hi, max(lo, math.nextafter(s, math.inf if step > 0 else -math.inf)))

    return f


# (kind, sample rate, options, n): the modulated cases of the sine spread test
# (test_modfx_ref.py) and of the end-to-end GPU comparison (test_modfx_gpu.py).
# fs 8000 with rate 5 Hz wraps the phase every 1600 samples; 20 .. 3900 Hz at
# 8 kHz sweeps the coefficient up to the 0.49 fs clamp's neighbourhood, where
# g = tan(pi f / fs) is about 32.
_WORST_PHASER = dict(rate_hz=5.0, min_freq_hz=20.0, max_freq_hz=3900.0, stages=12, mix=1.0)
CASES = [
    ("phaser", 48000.0, dict(), 6000),
    ("phaser", 8000.0, dict(_WORST_PHASER, feedback=0.99), 6000),
    ("phaser", 8000.0, dict(_WORST_PHASER, feedback=-0.99), 6000),
    ("tremolo", 48000.0, dict(), 6000),
    ("tremolo", 8000.0, dict(rate_hz=20.0, depth=1.0, smoothing_ms=0.0), 6000),
    ("tremolo", 8000.0, dict(rate_hz=20.0, depth=1.0, smoothing_ms=200.0, mix=0.5), 6000),
    ("ringmod", 48000.0, dict(), 6000),
    ("ringmod", 8000.0, dict(carrier_hz=0.49 * 8000.0, mix=0.5), 6000),
]
KINDS = {"phaser": Phaser, "tremolo": Tremolo, "ringmod": RingModulator}
AMPLITUDE = 0.25


# (kind, field, value) every setter rejects: TestPhaserValidation (phaser_test.go:74-94),
# TestTremoloValidation (tremolo_test.go:93-108), TestRingModulatorValidation (:196-251) and
# TestRingModulatorSetterValidation (:253-288), then every setter's own range (phaser.go:183-255,
# tremolo.go:138-192).  "range" is SetFrequencyRangeHz(min, max).
REJECTED = [
    ("phaser", "sample_rate", 0.0), ("phaser", "stages", 0), ("phaser", "range", (1000.0, 800.0)),
    ("phaser", "range", (1000.0, 30000.0)),
    ("tremolo", "sample_rate", 0.0), ("tremolo", "depth", 1.2), ("tremolo", "smoothing_ms", -1.0),
    ("ringmod", "sample_rate", 0.0), ("ringmod", "sample_rate", -1.0), ("ringmod", "sample_rate", math.nan),
    ("ringmod", "sample_rate", math.inf), ("ringmod", "carrier_hz", 0.0), ("ringmod", "carrier_hz", -100.0),
    ("ringmod", "carrier_hz", math.nan), ("ringmod", "mix", -0.1), ("ringmod", "mix", 1.1), ("ringmod", "mix", math.nan),
    ("ringmod", "carrier_hz", -1.0),
    # the rest of the setters' ranges
    ("phaser", "sample_rate", math.nan), ("phaser", "sample_rate", math.inf), ("phaser", "sample_rate", 3000.0),
    ("phaser", "rate_hz", 0.0), ("phaser", "rate_hz", math.nan), ("phaser", "rate_hz", math.inf),
    ("phaser", "range", (0.0, 1600.0)), ("phaser", "range", (300.0, 300.0)), ("phaser", "range", (300.0, math.inf)),
    ("phaser", "range", (math.nan, 1600.0)), ("phaser", "range", (300.0, 0.49 * 48000.0)),
    ("phaser", "stages", 13), ("phaser", "stages", -1),
    ("phaser", "feedback", -0.991), ("phaser", "feedback", 0.991), ("phaser", "feedback", math.nan),
    ("phaser", "mix", -0.01), ("phaser", "mix", 1.01), ("phaser", "mix", math.nan),
    ("tremolo", "sample_rate", math.nan), ("tremolo", "rate_hz", 0.0), ("tremolo", "rate_hz", math.inf),
    ("tremolo", "depth", -0.1), ("tremolo", "depth", math.nan), ("tremolo", "smoothing_ms", math.nan),
    ("tremolo", "smoothing_ms", math.inf), ("tremolo", "mix", -0.1), ("tremolo", "mix", 1.1), ("tremolo", "mix", math.nan),
    ("ringmod", "carrier_hz", math.inf), ("ringmod", "mix", math.inf),
]
ACCEPTED = [
    ("phaser", "rate_hz", 5e-324), ("phaser", "range", (5e-324, 1.0)),
    ("phaser", "range", (300.0, math.nextafter(0.49 * 48000.0, 0.0))), ("phaser", "stages", 1), ("phaser", "stages", 12),
    ("phaser", "feedback", -0.99), ("phaser", "feedback", 0.99), ("phaser", "mix", 0.0), ("phaser", "mix", 1.0),
    ("tremolo", "sample_rate", 5e-324), ("tremolo", "depth", 0.0), ("tremolo", "depth", 1.0),
    ("tremolo", "smoothing_ms", 0.0), ("tremolo", "smoothing_ms", 1e300), ("tremolo", "mix", 0.0),
    ("ringmod", "sample_rate", 5e-324), ("ringmod", "carrier_hz", 5e-324), ("ringmod", "carrier_hz", 1e9),
    ("ringmod", "mix", 0.0), ("ringmod", "mix", 1.0),
]
SETTER = {"sample_rate": "SetSampleRate", "rate_hz": "SetRateHz", "range": "SetFrequencyRangeHz", "stages": "SetStages",
          "feedback": "SetFeedback", "mix": "SetMix", "depth": "SetDepth", "smoothing_ms": "SetSmoothingMs",
          "carrier_hz": "SetCarrierHz"}


def set_on(obj, field, value):
    getattr(obj, SETTER[field])(*(value if field == "range" else (value,)))
