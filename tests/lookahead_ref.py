"""Line-by-line restatement of dynamics.LookaheadLimiter
(dsp/effects/dynamics/lookahead_limiter.go) over the feed-forward peak path of
the Compressor core it wraps (core.go:274-359, 486-487, 520-528): every product
and sum is one IEEE double operation, nothing is contracted.  The detector
coefficients come from Python's math (the C library), as the GPU runtime's host
side takes them from the C library; math.Log2 and math.Pow(2, x) are restated
as tests/dynfx_ref.py restates them for the de-esser.

One instance carries `channels` reference instances that share the
configuration.  ProcessSampleSidechain walks channel 0 in Python floats;
process_many walks every channel with numpy elementwise operations for the
envelope and the ring, and the scalar gain function per sample, so the bits
are the floats'.

A refused setter raises ValueError and changes nothing.
"""
from __future__ import annotations

import math

import numpy as np

from dynfx_ref import LOG2_OF_10_DIV_20, finite, go_log2

LN2 = 0.6931471805599453  # math.Ln2


def go_round(x: float) -> float:
    """math.Round: halves away from zero (Python's round goes to even)."""
    if x != x or math.isinf(x):
        return x
    t = float(math.trunc(x))
    if abs(x - t) >= 0.5:
        t += math.copysign(1.0, x)
    return t


class LookaheadLimiter:
    """lookahead_limiter.go:23-239 for `channels` instances.  `gain_fn(levels) -> gains` (arrays) replaces
    GainForLevel where a test substitutes the device's curve."""

    RATIO, ATTACK_MS, KNEE_DB = 100.0, 0.1, 0.0  # NewLookaheadLimiter :47-57

    def __init__(self, sampleRate, channels=1, gain_fn=None):  # :36-96
        if sampleRate <= 0 or not finite(sampleRate):
            raise ValueError("lookahead limiter sample rate must be positive and finite")
        self.channels = int(channels)
        self.sampleRate = float(sampleRate)
        self.gain_fn = gain_fn
        self.envelope = np.zeros(self.channels)  # core.Reset :572-573
        self.thresholdDB, self.releaseMs, self.lookaheadMs = -0.1, 100.0, 3.0  # :9-11
        self.SetThreshold(self.thresholdDB)
        self.SetRelease(self.releaseMs)
        self.SetLookahead(self.lookaheadMs)
        self.trace = None  # (envelope, gain, delayed) rows of the last process_many

    # ---- the core's cached values -------------------------------------------
    def _detector(self):  # recalculateDetectorCoefficients core.go:486-487
        self.attackCoeff = 1.0 - math.exp(-LN2 / (self.ATTACK_MS * 0.001 * self.sampleRate))
        self.releaseCoeff = math.exp(-LN2 / (self.releaseMs * 0.001 * self.sampleRate))

    def SetThreshold(self, dB):  # :99-113
        if dB < -24.0 or dB > 0.0 or not finite(dB):
            raise ValueError("lookahead limiter threshold")
        self.thresholdDB = float(dB)
        self.thresholdLog2 = self.thresholdDB * LOG2_OF_10_DIV_20  # core.go:521

    def SetRelease(self, ms):  # :116-130
        if ms < 1.0 or ms > 5000.0 or not finite(ms):
            raise ValueError("lookahead limiter release")
        self.releaseMs = float(ms)
        self._detector()

    def SetLookahead(self, ms):  # :133-143
        if ms < 0.0 or ms > 200.0 or not finite(ms):
            raise ValueError("lookahead limiter lookahead")
        self.lookaheadMs = float(ms)
        self.rebuildDelayBuffer()

    def SetSampleRate(self, sr):  # :146-161; the core's envelope stays (core.SetSampleRate recalculates only)
        if sr <= 0 or not finite(sr):
            raise ValueError("lookahead limiter sample rate")
        self.sampleRate = float(sr)
        self._detector()
        self.rebuildDelayBuffer()

    def Threshold(self):  # :164-173
        return self.thresholdDB

    def Release(self):
        return self.releaseMs

    def Lookahead(self):
        return self.lookaheadMs

    def SampleRate(self):
        return self.sampleRate

    def Reset(self):  # :176-183
        self.envelope[:] = 0
        self.writePos = 0
        self.delayBuf[:] = 0

    def rebuildDelayBuffer(self):  # :232-239
        self.delaySamples = max(int(go_round(self.lookaheadMs * self.sampleRate / 1000.0)), 0)
        size = max(self.delaySamples + 1, 1)
        self.delayBuf = np.zeros((self.channels, size))
        self.writePos = 0

    def GainForLevel(self, level: float) -> float:  # core.go:288-309, knee 0
        if level <= 0:
            return 1.0
        levelLog2 = go_log2(level)
        overshoot = levelLog2 - self.thresholdLog2
        compressionFactor = 1.0 - 1.0 / self.RATIO
        if overshoot <= 0:
            return 1.0
        gainLog2 = -overshoot * compressionFactor
        return math.pow(2.0, gainLog2)

    # ---- processing ---------------------------------------------------------
    def ProcessSampleSidechain(self, input: float, sidechain: float, ch: int = 0) -> float:  # :191-210
        source = abs(sidechain)  # detectorSource core.go:336, no prefilter
        env = float(self.envelope[ch])  # detectorLevel core.go:352-356
        if source > env:
            env += (source - env) * self.attackCoeff
        else:
            env = source + (env - source) * self.releaseCoeff
        self.envelope[ch] = env
        gain = self.GainForLevel(env)
        self.delayBuf[ch, self.writePos] = input
        readPos = self.writePos + 1
        if readPos >= self.delayBuf.shape[1]:
            readPos = 0
        delayed = float(self.delayBuf[ch, readPos])
        self.writePos = readPos
        return delayed * gain

    def ProcessSample(self, input: float) -> float:  # :186-188
        return self.ProcessSampleSidechain(input, input)

    def ProcessInPlaceSidechain(self, program, sidechain):  # :221-230, one channel
        for i in range(len(program)):
            det = float(sidechain[i]) if i < len(sidechain) else 0.0
            program[i] = self.ProcessSampleSidechain(float(program[i]), det)
        return program

    def ProcessInPlace(self, buf):  # :213-217
        for i in range(len(buf)):
            buf[i] = self.ProcessSample(float(buf[i]))
        return buf

    def process_many(self, program, sidechain=None) -> np.ndarray:
        """ProcessInPlace (sidechain None) or ProcessInPlaceSidechain on [channels][n] rows; a sidechain with
        fewer columns reads as 0 beyond them.  Leaves (envelope, gain, delayed) rows in self.trace."""
        x = np.asarray(program, dtype=np.float64).reshape(self.channels, -1)
        n = x.shape[1]
        det = np.zeros_like(x)
        if sidechain is None:
            det[:] = x
        else:
            s = np.asarray(sidechain, dtype=np.float64).reshape(self.channels, -1)
            k = min(n, s.shape[1])
            det[:, :k] = s[:, :k]
        env_rows, delayed = np.empty_like(x), np.empty_like(x)
        size = self.delayBuf.shape[1]
        with np.errstate(all="ignore"):
            for t in range(n):
                source = np.abs(det[:, t])
                env = self.envelope
                self.envelope = np.where(source > env, env + (source - env) * self.attackCoeff,
                                         source + (env - source) * self.releaseCoeff)
                env_rows[:, t] = self.envelope
                self.delayBuf[:, self.writePos] = x[:, t]
                readPos = self.writePos + 1
                if readPos >= size:
                    readPos = 0
                delayed[:, t] = self.delayBuf[:, readPos]
                self.writePos = readPos
            if self.gain_fn is not None:
                gain = np.asarray(self.gain_fn(env_rows), dtype=np.float64)
            else:
                gain = np.array([self.GainForLevel(float(v)) for v in env_rows.reshape(-1)]).reshape(x.shape)
            out = delayed * gain
        self.trace = (env_rows, gain, delayed)
        return out
