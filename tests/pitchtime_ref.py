"""Line-by-line restatement of pitch.PitchShifter
(dsp/effects/pitch/pitch_shifter.go) with interp.Hermite4
(dsp/interp/interp.go:51-58): every product and sum is one IEEE double
operation, nothing is contracted.

The processor is stateless and mono; Process takes one channel.  The search
(findBestOverlap :359-389) is vectorised over the candidates and loops over
the overlap's terms i = 0 ... overlapLen-1, so every candidate's dot and energy
are summed in the reference's term order (numpy's multiply and add are
separate operations).  The winner is the first candidate, ascending, whose
score is strictly greater than the best so far: numpy's argmax over the scores
with NaN replaced by -Inf returns the first maximum, and a maximum of -Inf
leaves `predicted`, as the scan does.

The fade-in table (rebuild :288-293) comes from Python's math (the C library);
the GPU processor's Python side computes the same table with the same function
and hands it to the library, so parity does not rest on two cosines.

A refused setter raises ValueError and changes nothing.
"""
from __future__ import annotations

import math

import numpy as np

MIN_RATIO, MAX_RATIO = 0.25, 4.0  # :19-20
MIN_SEQUENCE_MS, MAX_SEQUENCE_MS = 20.0, 120.0  # :22-27
MIN_OVERLAP_MS, MAX_OVERLAP_MS = 4.0, 60.0
MIN_SEARCH_MS, MAX_SEARCH_MS = 2.0, 40.0
IDENTITY_EPS = 1e-9  # :29
TINY = 1e-12  # :30


def go_round(x: float) -> float:
    """math.Round: halves away from zero (Python's round goes to even)."""
    if x != x or math.isinf(x):
        return x
    t = float(math.trunc(x))
    if abs(x - t) >= 0.5:
        t += math.copysign(1.0, x)
    return t


def finite_positive(v) -> bool:  # isFinitePositive :456-458
    return v > 0 and not math.isnan(v) and not math.isinf(v)


def fade_in_table(overlap_len: int) -> np.ndarray:  # rebuild :278-293
    if overlap_len == 1:
        return np.ones(1)
    out = np.empty(overlap_len)
    for i in range(overlap_len):
        t = float(i) / float(overlap_len - 1)
        out[i] = 0.5 - 0.5 * math.cos(math.pi * t)
    return out


def hermite4(t, xm1, x0, x1, x2):  # interp.go:51-58, on arrays or floats
    c0 = x0
    c1 = 0.5 * (x1 - xm1)
    c2 = ((xm1 - 2.5 * x0) + 2 * x1) - 0.5 * x2
    c3 = 0.5 * (x2 - xm1) + 1.5 * (x0 - x1)
    return ((c3 * t + c2) * t + c1) * t + c0


def sample_zero(x: np.ndarray, start: int, count: int) -> np.ndarray:
    """pitchSampleZero :432-438 for idx = start ... start + count - 1."""
    out = np.zeros(count)
    lo, hi = max(start, 0), min(start + count, len(x))
    if hi > lo:
        out[lo - start:hi - start] = x[lo:hi]
    return out


def resample_positions(in_len: int, out_len: int) -> np.ndarray:
    """pos of :410-416: accumulated, pos += step, not i * step."""
    step = float(in_len - 1) / float(out_len - 1)
    pos = np.empty(out_len)
    p = 0.0
    for i in range(out_len):
        pos[i] = p
        p += step
    return pos


def resample_hermite(inp: np.ndarray, out_len: int) -> np.ndarray:  # pitchResampleHermite :391-419
    if out_len <= 0 or len(inp) == 0:
        return np.zeros(0)
    if len(inp) == 1:
        return np.full(out_len, inp[0])
    if out_len == 1:
        return np.array([inp[0]])
    pos = resample_positions(len(inp), out_len)
    idx = np.floor(pos).astype(np.int64)  # pitchSampleHermite :421-430
    frac = pos - idx.astype(np.float64)
    last = len(inp) - 1
    at = lambda k: inp[np.clip(idx + k, 0, last)]  # pitchSampleClamp :440-454
    with np.errstate(all="ignore"):
        return hermite4(frac, at(-1), at(0), at(1), at(2))


class PitchShifter:
    """pitch_shifter.go:44-389."""

    def __init__(self, sampleRate):  # NewPitchShifter :62-81
        if not finite_positive(sampleRate):
            raise ValueError("pitch shifter sample rate must be positive and finite")
        self.sampleRate = float(sampleRate)
        self.pitchRatio = 1.0
        self.sequenceMs, self.overlapMs, self.searchMs = 82.0, 10.0, 28.0  # :15-17
        self.selections = []  # candStart of every frame of the last Process
        self._rebuild()

    def SampleRate(self):
        return self.sampleRate

    def PitchRatio(self):
        return self.pitchRatio

    def PitchSemitones(self):  # :90
        return 12.0 * math.log2(self.pitchRatio)

    def Sequence(self):
        return self.sequenceMs

    def Overlap(self):
        return self.overlapMs

    def Search(self):
        return self.searchMs

    def _set(self, field, value):  # the setters' rebuild-or-restore :107-119
        old = getattr(self, field)
        setattr(self, field, float(value))
        try:
            self._rebuild()
        except ValueError:
            setattr(self, field, old)
            self._rebuild()
            raise

    def SetSampleRate(self, sampleRate):  # :102-120
        if not finite_positive(sampleRate):
            raise ValueError("pitch shifter sample rate must be positive and finite")
        self._set("sampleRate", sampleRate)

    def SetPitchRatio(self, ratio):  # :123-132
        if not finite_positive(ratio) or ratio < MIN_RATIO or ratio > MAX_RATIO:
            raise ValueError("pitch shifter ratio must be in [0.25, 4]")
        self.pitchRatio = float(ratio)

    def SetPitchSemitones(self, semitones):  # :135-148
        if math.isnan(semitones) or math.isinf(semitones):
            raise ValueError("pitch shifter semitones must be finite")
        self.SetPitchRatio(math.pow(2, semitones / 12.0))

    def SetSequence(self, ms):  # :151-171
        if ms < MIN_SEQUENCE_MS or ms > MAX_SEQUENCE_MS or math.isnan(ms) or math.isinf(ms):
            raise ValueError("pitch shifter sequence must be in [20, 120] ms")
        self._set("sequenceMs", ms)

    def SetOverlap(self, ms):  # :174-194
        if ms < MIN_OVERLAP_MS or ms > MAX_OVERLAP_MS or math.isnan(ms) or math.isinf(ms):
            raise ValueError("pitch shifter overlap must be in [4, 60] ms")
        self._set("overlapMs", ms)

    def SetSearch(self, ms):  # :197-217
        if ms < MIN_SEARCH_MS or ms > MAX_SEARCH_MS or math.isnan(ms) or math.isinf(ms):
            raise ValueError("pitch shifter search must be in [2, 40] ms")
        self._set("searchMs", ms)

    def Reset(self):  # :222
        pass

    def _rebuild(self):  # :252-296
        if not finite_positive(self.sampleRate):
            raise ValueError("pitch shifter sample rate must be positive and finite")
        if self.overlapMs >= self.sequenceMs:
            raise ValueError("pitch shifter overlap must be smaller than sequence")
        sequenceLen = max(int(go_round(self.sequenceMs * 0.001 * self.sampleRate)), 32)
        overlapLen = max(int(go_round(self.overlapMs * 0.001 * self.sampleRate)), 8)
        if overlapLen >= sequenceLen:
            raise ValueError("pitch shifter overlap too large for sequence")
        stepOut = sequenceLen - overlapLen
        if stepOut < 4:
            raise ValueError("pitch shifter output hop too small")
        self.sequenceLen, self.overlapLen, self.stepOut = sequenceLen, overlapLen, stepOut
        self.searchLen = max(int(go_round(self.searchMs * 0.001 * self.sampleRate)), 1)
        self.fadeIn = fade_in_table(overlapLen)
        self.fadeOut = 1 - self.fadeIn

    def Process(self, inp) -> np.ndarray:  # :225-240
        inp = np.asarray(inp, dtype=np.float64)
        if len(inp) == 0:
            return np.zeros(0)
        if abs(self.pitchRatio - 1) <= IDENTITY_EPS:
            return inp.copy()
        return resample_hermite(self.timeStretch(inp), len(inp))

    def ProcessInPlace(self, buf):  # :243-250
        buf[:] = self.Process(buf)
        return buf

    def timeStretch(self, inp: np.ndarray) -> np.ndarray:  # :298-357
        n = len(inp)
        targetLen = max(int(go_round(float(n) * self.pitchRatio)), 1)
        nominalInStep = float(self.stepOut) / self.pitchRatio
        if nominalInStep < 1:
            nominalInStep = 1.0
        nFrames = targetLen // self.stepOut + 4
        out = np.zeros(nFrames * self.stepOut + self.sequenceLen + 1)
        out[:self.sequenceLen] = sample_zero(inp, 0, self.sequenceLen)
        outLen = self.sequenceLen
        prevStart = 0
        nextNominal = nominalInStep
        self.selections = []
        with np.errstate(all="ignore"):
            while outLen < targetLen + self.sequenceLen:
                ref = sample_zero(inp, prevStart + self.stepOut, self.overlapLen)
                predicted = int(go_round(nextNominal))
                candStart = self.findBestOverlap(ref, inp, predicted)
                self.selections.append(candStart)
                outStart = outLen - self.overlapLen
                new = sample_zero(inp, candStart, self.sequenceLen)
                ov = self.overlapLen
                out[outStart:outStart + ov] = out[outStart:outStart + ov] * self.fadeOut + new[:ov] * self.fadeIn
                out[outStart + ov:outStart + self.sequenceLen] = new[ov:]
                outLen = outStart + self.sequenceLen
                prevStart = candStart
                nextNominal += nominalInStep
                if prevStart > n + self.sequenceLen and outLen >= targetLen:
                    break
        return out[:targetLen]  # targetLen <= len(out) always: nFrames * stepOut > targetLen

    def findBestOverlap(self, ref: np.ndarray, inp: np.ndarray, predicted: int) -> int:  # :359-389
        searchStart = predicted - self.searchLen
        count = 2 * self.searchLen + 1
        refEnergy = TINY
        for v in ref:
            refEnergy += v * v
        window = sample_zero(inp, searchStart, count + self.overlapLen - 1)
        dot = np.zeros(count)
        candEnergy = np.full(count, TINY)
        for i in range(self.overlapLen):
            cv = window[i:i + count]
            dot = dot + ref[i] * cv
            candEnergy = candEnergy + cv * cv
        score = dot / np.sqrt(refEnergy * candEnergy)
        score = np.where(np.isnan(score), -np.inf, score)  # `score > bestScore` is false for NaN
        k = int(np.argmax(score))  # the first maximum
        if score[k] == -np.inf:  # nothing is greater than -Inf: best stays predicted
            return predicted
        return searchStart + k
