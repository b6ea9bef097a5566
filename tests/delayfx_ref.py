"""effects.Delay (dsp/effects/delay.go), modulation.Flanger
(dsp/effects/modulation/flanger.go, with hermite4 of chorus.go:273-280) and the
graph's simpleDelayRuntime (dsp/effectchain/runtime_modulation.go:322-362)
restated in plain Python: one instance, a per-sample loop, IEEE doubles in the
reference's operation order.  It is the oracle of the delay and flanger tests.

Python floats do not fuse, and math.exp / math.sin are the host C library's.
Two things are arguments because the GPU handle cannot share them with Python
bit for bit by construction: the delay's smoothing coefficient (assign
`smoothCoeff`; by default 1 - math.exp(...) as computeSmoothCoeff computes it)
and the flanger's sine (`sin`, math.sin by default).

`process(x, block=B)` is the block form the GPU kernels rely on: the reads of B
consecutive samples are all taken before any of their writes.  block=1 is the
reference's own loop.  Delay.process(x, block=B, reverse=True) instead runs
each block's samples last to first, every sample reading and then writing at
once: a sample then sees the writes of all later samples of its block and of
no earlier one, the worst order a launch without barriers can take.
"""
from __future__ import annotations

import math

import numpy as np

# delay.go:8-20
DEFAULT_DELAY_TIME, DEFAULT_DELAY_FEEDBACK, DEFAULT_DELAY_MIX = 0.25, 0.35, 0.25
MAX_DELAY_TIME, MIN_DELAY_TIME, DELAY_SMOOTH_SECONDS = 2.0, 0.001, 0.010
# flanger.go:8-17
MIN_FLANGER_DELAY, MAX_FLANGER_DELAY = 0.0001, 0.0100


def _bad(v):
    return math.isnan(v) or math.isinf(v)


def go_round(v: float) -> float:
    """math.Round: to the nearest integer, halves away from zero."""
    a = abs(v)
    if a >= 2.0 ** 52 or _bad(v):
        return v
    f = math.floor(a)
    return math.copysign(f + 1 if a - f >= 0.5 else f, v)


def compute_smooth_coeff(sample_rate):  # :255-257
    tau = sample_rate * DELAY_SMOOTH_SECONDS
    return 1 - math.exp(-1 / tau) if tau != 0 else 1.0  # Go: -1/0 is -Inf, and exp(-Inf) is 0


def _resized(old, old_write, n):
    """The history-preserving copy of reconfigureBuffer (delay.go:220-242) and
    reconfigureDelayLine (flanger.go:365-387); the new write position is 0."""
    new = [0.0] * n
    if len(old) > 0:
        for i in range(min(len(old), n)):
            src = old_write - 1 - i
            if src < 0:
                src += len(old)
            dst = 0 - 1 - i
            if dst < 0:
                dst += n
            new[dst] = old[src]
    return new


class Delay:
    """NewDelay(sample_rate) (:40-60)."""

    def __init__(self, sample_rate):
        if sample_rate <= 0 or _bad(sample_rate):
            raise ValueError("delay sample rate must be > 0")
        self.sampleRate = sample_rate
        self.delaySeconds, self.feedback, self.mix = DEFAULT_DELAY_TIME, DEFAULT_DELAY_FEEDBACK, DEFAULT_DELAY_MIX
        self.targetSamples = self.currentSamples = 0.0
        self.smoothCoeff = compute_smooth_coeff(sample_rate)
        self.buffer, self.write = [], 0
        self._reconfigure()

    def SetSampleRate(self, v):  # :63-72
        if v <= 0 or _bad(v):
            raise ValueError("delay sample rate must be > 0")
        self.sampleRate = v
        self.smoothCoeff = compute_smooth_coeff(v)
        self._reconfigure()

    def SetTime(self, v):  # :77-89
        self._validate_time(v)
        self.delaySeconds = v
        self.targetSamples = self.currentSamples = go_round(v * self.sampleRate)  # no clamp to one sample

    def SetTargetTime(self, v):  # :95-106
        self._validate_time(v)
        self.delaySeconds = v
        self.targetSamples = go_round(v * self.sampleRate)

    def SetFeedback(self, v):  # :109-117
        if v < 0 or v > 0.99 or _bad(v):
            raise ValueError("delay feedback must be in [0, 0.99]")
        self.feedback = v

    def SetMix(self, v):  # :120-128
        if v < 0 or v > 1 or _bad(v):
            raise ValueError("delay mix must be in [0, 1]")
        self.mix = v

    def Reset(self):  # :131-137: currentSamples stays
        self.buffer = [0.0] * len(self.buffer)
        self.write = 0

    def SampleRate(self):
        return self.sampleRate

    def Time(self):
        return self.delaySeconds

    def Feedback(self):
        return self.feedback

    def Mix(self):
        return self.mix

    def CurrentDelaySamples(self):
        return self.currentSamples

    def _validate_time(self, v):  # :191-199
        if v < MIN_DELAY_TIME or v > MAX_DELAY_TIME or _bad(v):
            raise ValueError("delay time must be in [0.001, 2]")

    def _reconfigure(self):  # reconfigureBuffer :201-253
        max_samples = int(math.ceil(MAX_DELAY_TIME * self.sampleRate)) + 1
        if max_samples != len(self.buffer):
            self.buffer = _resized(self.buffer, self.write, max_samples)
            self.write = 0
        samples = go_round(self.delaySeconds * self.sampleRate)
        if samples < 1:
            samples = 1.0
        self.targetSamples = self.currentSamples = samples

    def ramp_step(self):  # :142
        self.currentSamples += (self.targetSamples - self.currentSamples) * self.smoothCoeff
        return self.currentSamples

    def _read(self, write, c):  # :145-156 for write position `write`
        buf = self.buffer
        read_exact = float(write) - c
        buf_len = float(len(buf))
        while read_exact < 0:
            read_exact += buf_len
        r0 = int(math.floor(read_exact))
        frac = read_exact - float(r0)
        r1 = (r0 + 1) % len(buf)
        return buf[r0] * (1 - frac) + buf[r1] * frac

    def ProcessSample(self, x):  # :140-166
        delayed = self._read(self.write, self.ramp_step())
        self.buffer[self.write] = x + delayed * self.feedback
        self.write += 1
        if self.write >= len(self.buffer):
            self.write = 0
        return x * (1 - self.mix) + delayed * self.mix

    def block_bounds(self):
        """(raw, both): `raw` consecutive samples read none of each other's
        writes while the delay moves between its current value and its target;
        `both` of them also overwrite nothing that another still has to read."""
        lo, hi = min(self.currentSamples, self.targetSamples), max(self.currentSamples, self.targetSamples)
        raw = max(1, int(math.floor(lo)) - 1)
        return raw, min(raw, max(1, len(self.buffer) - int(math.ceil(hi))))

    def process(self, x, block: int = 1, reverse: bool = False) -> np.ndarray:
        x = np.asarray(x, dtype=np.float64)
        y = np.empty_like(x)
        ln = len(self.buffer)
        for t0 in range(0, x.size, block):
            m = min(block, x.size - t0)
            cs = [self.ramp_step() for _ in range(m)]
            w0 = self.write
            if reverse:
                for s in range(m - 1, -1, -1):
                    inp = float(x[t0 + s])
                    delayed = self._read((w0 + s) % ln, cs[s])
                    self.buffer[(w0 + s) % ln] = inp + delayed * self.feedback
                    y[t0 + s] = inp * (1 - self.mix) + delayed * self.mix
            else:
                ds = [self._read((w0 + s) % ln, cs[s]) for s in range(m)]
                for s in range(m):
                    inp = float(x[t0 + s])
                    self.buffer[(w0 + s) % ln] = inp + ds[s] * self.feedback
                    y[t0 + s] = inp * (1 - self.mix) + ds[s] * self.mix
            self.write = (w0 + m) % ln
        return y


def hermite4(t, xm1, x0, x1, x2):  # chorus.go:273-280
    c0 = x0
    c1 = 0.5 * (x1 - xm1)
    c2 = xm1 - 2.5 * x0 + 2 * x1 - 0.5 * x2
    c3 = 0.5 * (x2 - xm1) + 1.5 * (x0 - x1)
    return ((c3 * t + c2) * t + c1) * t + c0


def lfo_step(phase, rate_hz, sample_rate):  # flanger.go:276-279
    phase += 2 * math.pi * rate_hz / sample_rate
    if phase >= 2 * math.pi:
        phase -= 2 * math.pi
    return phase


class Flanger:
    """NewFlanger(sample_rate, options...) (:124-162); the options are keywords."""

    def __init__(self, sample_rate, rate_hz=0.25, depth_seconds=0.0015, base_delay_seconds=0.001, feedback=0.25,
                 mix=0.5, sin=math.sin):
        if sample_rate <= 0 or _bad(sample_rate):
            raise ValueError("flanger sample rate must be > 0 and finite")
        self.sampleRate, self.rateHz, self.depth = sample_rate, rate_hz, depth_seconds
        self.baseDelay, self.feedback, self.mix = base_delay_seconds, feedback, mix
        self.lfoPhase = 0.0
        self.delayLine, self.write, self.maxDelay = [], 0, 0
        self.sin = sin
        self._reconfigure()

    def SetSampleRate(self, v):  # :165-173
        if v <= 0 or _bad(v):
            raise ValueError("flanger sample rate must be > 0 and finite")
        self.sampleRate = v
        self._reconfigure()

    def SetRateHz(self, v):  # :176-184
        if v <= 0 or _bad(v):
            raise ValueError("flanger rate must be > 0 and finite")
        self.rateHz = v

    def SetDepthSeconds(self, v):  # :187-203
        if v < 0 or _bad(v):
            raise ValueError("flanger depth must be >= 0 and finite")
        prev, self.depth = self.depth, v
        try:
            self._reconfigure()
        except ValueError:
            self.depth = prev
            raise

    def SetBaseDelaySeconds(self, v):  # :206-224
        if v < MIN_FLANGER_DELAY or v > MAX_FLANGER_DELAY or _bad(v):
            raise ValueError("flanger base delay must be in [0.0001, 0.01]")
        prev, self.baseDelay = self.baseDelay, v
        try:
            self._reconfigure()
        except ValueError:
            self.baseDelay = prev
            raise

    def SetFeedback(self, v):  # :227-235
        if v < -0.99 or v > 0.99 or _bad(v):
            raise ValueError("flanger feedback must be in [-0.99, 0.99]")
        self.feedback = v

    def SetMix(self, v):  # :238-246
        if v < 0 or v > 1 or _bad(v):
            raise ValueError("flanger mix must be in [0, 1]")
        self.mix = v

    def Reset(self):  # :249-256
        self.delayLine = [0.0] * len(self.delayLine)
        self.write = 0
        self.lfoPhase = 0.0

    def SampleRate(self):
        return self.sampleRate

    def RateHz(self):
        return self.rateHz

    def DepthSeconds(self):
        return self.depth

    def BaseDelaySeconds(self):
        return self.baseDelay

    def Feedback(self):
        return self.feedback

    def Mix(self):
        return self.mix

    def _validate(self):  # validateParams :317-350
        if self.sampleRate <= 0 or _bad(self.sampleRate):
            raise ValueError("flanger sample rate must be > 0 and finite")
        if self.rateHz <= 0 or _bad(self.rateHz):
            raise ValueError("flanger rate must be > 0 and finite")
        if self.depth < 0 or _bad(self.depth):
            raise ValueError("flanger depth must be >= 0 and finite")
        if self.baseDelay < MIN_FLANGER_DELAY or self.baseDelay > MAX_FLANGER_DELAY or _bad(self.baseDelay):
            raise ValueError("flanger base delay must be in [0.0001, 0.01]")
        if self.baseDelay + self.depth > MAX_FLANGER_DELAY:
            raise ValueError("flanger max delay exceeds 0.01 seconds")
        if self.feedback < -0.99 or self.feedback > 0.99 or _bad(self.feedback):
            raise ValueError("flanger feedback must be in [-0.99, 0.99]")
        if self.mix < 0 or self.mix > 1 or _bad(self.mix):
            raise ValueError("flanger mix must be in [0, 1]")

    def _reconfigure(self):  # reconfigureDelayLine :352-390
        self._validate()
        needed = max(int(math.ceil((self.baseDelay + self.depth) * self.sampleRate)) + 3, 4)
        if needed == len(self.delayLine):
            self.maxDelay = needed - 3
            return
        self.delayLine = _resized(self.delayLine, self.write, needed)
        self.write = 0
        self.maxDelay = needed - 3

    def _read(self, write, delay):  # sampleFractionalDelay :392-411, sampleDelayInt :413-424
        line = self.delayLine
        ln = len(line)
        if delay < 0:
            delay = 0.0
        md = float(self.maxDelay)
        if delay > md:
            delay = md
        p = int(math.floor(delay))
        t = delay - float(p)

        def at(q):
            if q < 0 or q >= ln:
                return 0.0
            idx = write - q
            if idx < 0:
                idx += ln
            return line[idx]

        return hermite4(t, at(max(0, p - 1)), at(p), at(p + 1), at(p + 2))

    def _delay_samples(self):  # :260-265
        mod = 0.5 * (1 + self.sin(self.lfoPhase))
        d = (self.baseDelay + self.depth * mod) * self.sampleRate
        return 1.0 if d < 1 else d

    def Process(self, x):  # :259-282
        delayed = self._read(self.write, self._delay_samples())
        self.delayLine[self.write] = x + delayed * self.feedback
        self.write += 1
        if self.write >= len(self.delayLine):
            self.write = 0
        self.lfoPhase = lfo_step(self.lfoPhase, self.rateHz, self.sampleRate)
        return x * (1 - self.mix) + delayed * self.mix

    def block_bound(self) -> int:
        """max(1, P - 1), P = floor(max(1, base * fs)): this many consecutive
        samples read none of each other's writes."""
        return max(1, int(math.floor(max(1.0, self.baseDelay * self.sampleRate))) - 1)

    def process(self, x, block: int = 1) -> np.ndarray:
        x = np.asarray(x, dtype=np.float64)
        y = np.empty_like(x)
        ln = len(self.delayLine)
        for t0 in range(0, x.size, block):
            m = min(block, x.size - t0)
            w0 = self.write
            ds = []
            for s in range(m):
                ds.append(self._read((w0 + s) % ln, self._delay_samples()))
                self.lfoPhase = lfo_step(self.lfoPhase, self.rateHz, self.sampleRate)
            for s in range(m):
                inp = float(x[t0 + s])
                self.delayLine[(w0 + s) % ln] = inp + ds[s] * self.feedback
                y[t0 + s] = inp * (1 - self.mix) + ds[s] * self.mix
            self.write = (w0 + m) % ln
        return y


class SimpleDelay:
    """simpleDelayRuntime (runtime_modulation.go:322-362)."""

    def __init__(self):
        self.sampleRate = self.delayMs = 0.0
        self.delaySamples, self.write, self.buf = 0, 0, []

    def Configure(self, sample_rate, delay_ms=20.0):  # :330-344
        self.sampleRate = sample_rate
        self.delayMs = min(max(delay_ms, 0.0), 500.0)
        self.delaySamples = max(int(go_round(self.delayMs * self.sampleRate / 1000.0)), 0)
        size = max(self.delaySamples + 1, 1)
        if len(self.buf) != size:
            self.buf = [0.0] * size
            self.write = 0

    def process(self, x) -> np.ndarray:  # :346-362
        y = np.array(x, dtype=np.float64)
        if len(self.buf) <= 1:
            return y
        for i in range(y.size):
            self.buf[self.write] = float(y[i])
            read_pos = self.write + 1
            if read_pos >= len(self.buf):
                read_pos = 0
            y[i] = self.buf[read_pos]
            self.write = read_pos
        return y


def nudged_sin(seed: int):
    """math.sin moved by a seeded random -1 / 0 / +1 ulp per call, kept in [-1, 1]."""
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
        if step == 0:
            return s
        return min(1.0, max(-1.0, math.nextafter(s, math.inf if step > 0 else -math.inf)))

    return f
