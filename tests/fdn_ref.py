"""reverb.FDNReverb (dsp/effects/reverb/fdn_reverb.go, interp_helpers.go)
restated in plain Python: one instance, a per-sample loop, IEEE doubles in the
reference's operation order.  It is the oracle of the FDN tests.

Two things are arguments because the GPU handle cannot share them with
Python bit for bit by construction: the feedback gains (`gains`, or assign
`feedbackGain` after a setter; by default math.pow as updateFeedbackGains
computes them) and the sine (`sin`, math.sin by default).

`process(x, block=B)` is the block form the GPU kernel relies on: the reads of
B consecutive samples are all taken before any of their writes.  block=1 is
the reference's own loop.
"""
from __future__ import annotations

import math

import numpy as np

SIZE = 8
DELAY_SAMPLES = (1537.0, 1753.0, 1999.0, 2251.0, 2473.0, 2689.0, 2851.0, 3067.0)  # :24
REFERENCE_RATE = 44100.0
MIN_BUFFER = 4
HADAMARD = (
    (1, 1, 1, 1, 1, 1, 1, 1),
    (1, -1, 1, -1, 1, -1, 1, -1),
    (1, 1, -1, -1, 1, 1, -1, -1),
    (1, -1, -1, 1, 1, -1, -1, 1),
    (1, 1, 1, 1, -1, -1, -1, -1),
    (1, -1, 1, -1, -1, 1, -1, 1),
    (1, 1, -1, -1, -1, -1, 1, 1),
    (1, -1, -1, 1, -1, 1, 1, -1),
)
TWO_PI = 2 * math.pi


def _bad(v):
    return math.isnan(v) or math.isinf(v)


def hermite4(t, xm1, x0, x1, x2):  # interp_helpers.go:3-10
    c1 = 0.5 * (x1 - xm1)
    c2 = xm1 - 2.5 * x0 + 2 * x1 - 0.5 * x2
    c3 = 0.5 * (x2 - xm1) + 1.5 * (x0 - x1)
    return ((c3 * t + c2) * t + c1) * t + x0


class Line:  # fdnDelayLine :314-391
    __slots__ = ("buf", "pos", "max_delay")

    def __init__(self):
        self.buf, self.pos, self.max_delay = [], 0, 0

    def resize(self, n):
        n = max(n, MIN_BUFFER)
        if n == len(self.buf):
            return
        self.buf, self.pos, self.max_delay = [0.0] * n, 0, n - 3

    def reset(self):
        self.buf = [0.0] * len(self.buf)
        self.pos = 0

    def write(self, x):
        self.buf[self.pos] = x
        self.pos += 1
        if self.pos >= len(self.buf):
            self.pos = 0

    def read(self, delay, ahead=0):
        """sampleFractionalDelay as if `ahead` more samples had been written
        (their slots still hold what they held)."""
        buf = self.buf
        ln = len(buf)
        if delay < 0:
            delay = 0.0
        md = float(self.max_delay)
        if delay > md:
            delay = md
        p = int(math.floor(delay))
        t = delay - float(p)
        last = self.pos + ahead - 1

        def at(q):
            if q < 0 or q >= ln:
                return 0.0
            return buf[(last - q) % ln]

        return hermite4(t, at(max(0, p - 1)), at(p), at(p + 1), at(p + 2))


def lfo_step(phase, mod_rate, sample_rate):  # :215-218
    phase += TWO_PI * mod_rate / sample_rate
    if phase >= TWO_PI:
        phase -= TWO_PI
    return phase


class FDN:
    """NewFDNReverb(sample_rate) (:66-92)."""

    def __init__(self, sample_rate, gains=None, sin=math.sin):
        self.sampleRate, self.wet, self.dry, self.rt60Seconds = 44100.0, 0.2, 1.0, 1.8
        self.damp, self.preDelaySeconds, self.modDepthSeconds, self.modRateHz = 0.3, 0.01, 0.002, 0.1
        self.lfoPhase = 0.0
        self.baseDelaySamples = list(DELAY_SAMPLES)
        self.lineDelayScale = self.modDepthSamples = self.preDelaySamples = 0.0
        self.lines = [Line() for _ in range(SIZE)]
        self.filterState = [0.0] * SIZE
        self.feedbackGain = [0.0] * SIZE
        self.preDelayLine = Line()
        self.inputGain = self.outputGain = self.matrixScale = 1 / math.sqrt(float(SIZE))
        self.sin = sin
        self.SetSampleRate(sample_rate)
        if gains is not None:
            self.feedbackGain = [float(g) for g in gains]

    # ---- setters (:95-186)
    def SetSampleRate(self, v):
        if v <= 0 or _bad(v):
            raise ValueError("fdn reverb sample rate must be > 0")
        self.sampleRate = v
        self.lineDelayScale = v / REFERENCE_RATE
        self.modDepthSamples = self.modDepthSeconds * self.sampleRate
        self.preDelaySamples = self.preDelaySeconds * self.sampleRate
        self._reconfigure()

    def SetWet(self, v):
        if v < 0 or _bad(v):
            raise ValueError("fdn reverb wet must be >= 0")
        self.wet = v

    def SetDry(self, v):
        if v < 0 or _bad(v):
            raise ValueError("fdn reverb dry must be >= 0")
        self.dry = v

    def SetRT60(self, v):
        if v <= 0 or _bad(v):
            raise ValueError("fdn reverb RT60 must be > 0")
        self.rt60Seconds = v
        self._update_gains()

    def SetDamp(self, v):
        if v < 0 or v > 1 or _bad(v):
            raise ValueError("fdn reverb damp must be in [0,1]")
        self.damp = v

    def SetPreDelay(self, v):
        if v < 0 or _bad(v):
            raise ValueError("fdn reverb pre-delay must be >= 0")
        self.preDelaySeconds = v
        self.preDelaySamples = self.preDelaySeconds * self.sampleRate
        self._reconfigure()

    def SetModDepth(self, v):
        if v < 0 or _bad(v):
            raise ValueError("fdn reverb mod depth must be >= 0")
        self.modDepthSeconds = v
        self.modDepthSamples = self.modDepthSeconds * self.sampleRate
        self._reconfigure()

    def SetModRate(self, v):
        if v < 0 or _bad(v):
            raise ValueError("fdn reverb mod rate must be >= 0")
        self.modRateHz = v

    def Reset(self):  # :189-197
        for ln in self.lines:
            ln.reset()
        self.filterState = [0.0] * SIZE
        self.preDelayLine.reset()
        self.lfoPhase = 0.0

    def _reconfigure(self):  # reconfigureDelays :274-301
        for i in range(SIZE):
            n = max(int(math.ceil(self.baseDelaySamples[i] * self.lineDelayScale + self.modDepthSamples)) + 3,
                    MIN_BUFFER)
            self.lines[i].resize(n)
            self.filterState[i] = 0.0
        self.preDelayLine.resize(max(int(math.ceil(self.preDelaySamples)) + 3, MIN_BUFFER))
        self._update_gains()

    def _update_gains(self):  # updateFeedbackGains :303-312
        for i in range(SIZE):
            delay_seconds = (self.baseDelaySamples[i] * self.lineDelayScale) / self.sampleRate
            self.feedbackGain[i] = math.pow(10, -3 * delay_seconds / self.rt60Seconds)

    def block_bound(self) -> int:
        """max(1, P): this many consecutive samples read none of each other's writes."""
        return max(1, int(math.floor(self.baseDelaySamples[0] * self.lineDelayScale)))

    # ---- ProcessSample (:199-241) over a buffer
    def process(self, x, block: int = 1) -> np.ndarray:
        x = np.asarray(x, dtype=np.float64)
        y = np.empty_like(x)
        sin, lines, pre = self.sin, self.lines, self.preDelayLine
        rng8 = range(SIZE)
        offs = [(TWO_PI * float(i)) / float(SIZE) for i in rng8]
        for t0 in range(0, x.size, block):
            m = min(block, x.size - t0)
            ins, ds = [], []
            for s in range(m):
                inp = float(x[t0 + s])
                v = inp
                if self.preDelaySamples > 0:
                    pre.write(inp)
                    v = pre.read(self.preDelaySamples)
                ph = self.lfoPhase
                ds.append([lines[i].read(self.baseDelaySamples[i] * self.lineDelayScale
                                         + self.modDepthSamples * (0.5 * (1 + sin(ph + offs[i]))), s) for i in rng8])
                self.lfoPhase = lfo_step(ph, self.modRateHz, self.sampleRate)
                ins.append(v)
            for s in range(m):
                d = ds[s]
                for i in rng8:
                    fb = 0.0
                    for h, dj in zip(HADAMARD[i], d):
                        fb += h * dj
                    fb *= self.matrixScale
                    filtered = fb * (1 - self.damp) + self.filterState[i] * self.damp
                    self.filterState[i] = filtered
                    lines[i].write(ins[s] * self.inputGain + filtered * self.feedbackGain[i])
                out = 0.0
                for dj in d:
                    out += dj
                out *= self.outputGain
                y[t0 + s] = float(x[t0 + s]) * self.dry + out * self.wet
        return y


def nudged_sin(seed: int):
    """math.sin moved by a seeded random -1 / 0 / +1 ulp per call."""
    rng = np.random.default_rng(seed)
    state = {"k": 0, "steps": rng.integers(-1, 2, size=1 << 16)}

    def f(v):
        k = state["k"]
        if k == state["steps"].size:
            state["steps"] = rng.integers(-1, 2, size=1 << 16)
            k = 0
        state["k"] = k + 1
        s = math.sin(v)
        step = state["steps"][k]
        return s if step == 0 else math.nextafter(s, math.inf if step > 0 else -math.inf)

    return f
