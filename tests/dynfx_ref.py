"""Line-by-line restatement of dynamics.TransientShaper
(dsp/effects/dynamics/transient_shaper.go) and dynamics.DeEsser (deesser.go)
for one channel, in Python floats: every product and sum is one IEEE double
operation, nothing is contracted.  Envelope coefficients and the section come
from Python's math (the C library) and algodsp.design, as the GPU runtime's
host side takes them from the C library.

A refused setter raises ValueError and changes nothing, as the reference's
setters return an error before they assign.
"""
from __future__ import annotations

import math

import numpy as np

from algodsp import design

LOG2_OF_10_DIV_20 = 0.166096404744  # compressor.go:27
INV_LN2 = 1.4426950408889634  # 1/Ln2, the constant of math.Log2


def finite(v) -> bool:
    return not (math.isnan(v) or math.isinf(v))


def fdiv(a: float, b: float) -> float:
    """a / b as IEEE division (Python raises where the hardware gives inf or NaN)."""
    try:
        return a / b
    except ZeroDivisionError:
        if a == 0 or a != a:
            return math.nan
        return math.copysign(math.inf, a) * math.copysign(1.0, b)


def time_ms_to_coeff(ms: float, fs: float) -> float:  # timeMsToCoeff transient_shaper.go:184-200
    seconds = ms / 1000.0
    if seconds <= 0:
        return 1.0
    coeff = 1.0 - math.exp(-1.0 / (seconds * fs))
    if coeff < 0:
        return 0.0
    if coeff > 1:
        return 1.0
    return coeff


class TransientShaper:
    """transient_shaper.go:25-182."""

    def __init__(self, fs: float):  # NewTransientShaper :38-54
        if fs <= 0 or not finite(fs):  # validateSampleRate core.go:588-594
            raise ValueError("transient shaper sample rate must be positive and finite")
        self.attackAmount, self.sustainAmount = 0.0, 0.0  # :9-12
        self.attackMs, self.releaseMs = 10.0, 120.0
        self.sampleRate = float(fs)
        self.envelope = 0.0
        self.updateCoefficients()

    def SetAttackAmount(self, v):  # :57-66
        if v < -1.0 or v > 1.0 or not finite(v):
            raise ValueError("attack amount")
        self.attackAmount = float(v)

    def SetSustainAmount(self, v):  # :69-78
        if v < -1.0 or v > 1.0 or not finite(v):
            raise ValueError("sustain amount")
        self.sustainAmount = float(v)

    def SetAttack(self, ms):  # :81-91
        if ms < 0.1 or ms > 200.0 or not finite(ms):
            raise ValueError("attack")
        self.attackMs = float(ms)
        self.updateCoefficients()

    def SetRelease(self, ms):  # :94-104
        if ms < 1.0 or ms > 2000.0 or not finite(ms):
            raise ValueError("release")
        self.releaseMs = float(ms)
        self.updateCoefficients()

    def SetSampleRate(self, fs):  # :107-117
        if fs <= 0 or not finite(fs):
            raise ValueError("sample rate")
        self.sampleRate = float(fs)
        self.updateCoefficients()

    def Reset(self):  # :135-137
        self.envelope = 0.0

    def updateCoefficients(self):  # :179-182
        self.attackCoeff = time_ms_to_coeff(self.attackMs, self.sampleRate)
        self.releaseCoeff = time_ms_to_coeff(self.releaseMs, self.sampleRate)

    def ProcessSample(self, x: float) -> float:  # :140-170
        prev = self.envelope
        a = abs(x)
        coeff = self.releaseCoeff
        if a > prev:
            coeff = self.attackCoeff
        self.envelope = prev + coeff * (a - prev)
        delta = self.envelope - prev
        norm = fdiv(abs(delta), prev + 1e-9)
        if norm > 1:
            norm = 1.0
        gain = 1.0
        if delta >= 0:
            gain += self.attackAmount * norm
        else:
            gain += self.sustainAmount * norm
        if gain < 0:
            gain = 0.0
        return x * gain

    def ProcessInPlace(self, buf):  # :173-177
        for i in range(len(buf)):
            buf[i] = self.ProcessSample(float(buf[i]))
        return buf


class Section:
    """biquad.Section (dsp/filter/biquad/section.go:47-53), direct form II transposed."""

    def __init__(self, coeffs):
        self.B0, self.B1, self.B2, self.A1, self.A2 = (float(c) for c in coeffs)
        self.d0 = self.d1 = 0.0

    def ProcessSample(self, x: float) -> float:
        y = self.B0 * x + self.d0
        self.d0 = self.B1 * x - self.A1 * y + self.d1
        self.d1 = self.B2 * x - self.A2 * y
        return y

    def Reset(self):
        self.d0 = self.d1 = 0.0


def go_log2(x: float) -> float:  # math.Log2: frexp, Log(frac) * (1/Ln2) + exp
    frac, e = math.frexp(x)
    if frac == 0.5:
        return float(e - 1)
    return math.log(frac) * INV_LN2 + float(e)


SPLIT_BAND, WIDEBAND = 0, 1  # DeEsserMode deesser.go:15-25
DETECT_BANDPASS, DETECT_HIGHPASS = 0, 1  # DeEsserDetector :30-39


class DeEsser:
    """deesser.go:100-622.  `gain_fn(env) -> gain` replaces calculateGain where a test substitutes the device's
    curve; `trace` collects the envelope calculateGain sees, sample by sample."""

    def __init__(self, fs: float, gain_fn=None):  # NewDeEsser :155-181
        if fs <= 0 or not finite(fs):
            raise ValueError("de-esser sample rate must be positive and finite")
        self.freqHz, self.q, self.thresholdDB, self.ratio, self.kneeDB = 6000.0, 1.5, -20.0, 4.0, 3.0  # :43-54
        self.attackMs, self.releaseMs, self.rangeDB = 0.5, 20.0, -24.0
        self.mode, self.detector, self.listen, self.filterOrder = SPLIT_BAND, DETECT_BANDPASS, False, 2
        self.sampleRate = float(fs)
        self.envLevel = 0.0
        self.metrics = [0.0, 1.0]  # DetectionLevel, GainReduction
        self.gain_fn = gain_fn
        self.trace = None
        self.clamped = [0, 0]  # samples that kept the split-band value, samples the clamp :467 replaced
        self.updateCoefficients()
        self.rebuildFilters()

    # --- setters :228-409
    def SetFrequency(self, hz):
        if hz < 1000.0 or hz > 20000.0 or not finite(hz):
            raise ValueError("frequency")
        if hz >= self.sampleRate / 2:
            raise ValueError("frequency must be < Nyquist")
        self.freqHz = float(hz)
        self.rebuildFilters()

    def SetQ(self, q):
        if q < 0.1 or q > 10.0 or not finite(q):
            raise ValueError("q")
        self.q = float(q)
        self.rebuildFilters()

    def SetThreshold(self, db):
        if not finite(db):
            raise ValueError("threshold")
        self.thresholdDB = float(db)
        self.updateCoefficients()

    def SetRatio(self, r):
        if r < 1.0 or r > 100.0 or not finite(r):
            raise ValueError("ratio")
        self.ratio = float(r)
        self.updateCoefficients()

    def SetKnee(self, db):
        if db < 0.0 or db > 12.0 or not finite(db):
            raise ValueError("knee")
        self.kneeDB = float(db)
        self.updateCoefficients()

    def SetAttack(self, ms):
        if ms < 0.01 or ms > 50.0 or not finite(ms):
            raise ValueError("attack")
        self.attackMs = float(ms)
        self.updateTimeConstants()

    def SetRelease(self, ms):
        if ms < 1.0 or ms > 500.0 or not finite(ms):
            raise ValueError("release")
        self.releaseMs = float(ms)
        self.updateTimeConstants()

    def SetRange(self, db):
        if db < -60.0 or db > 0.0 or not finite(db):
            raise ValueError("range")
        self.rangeDB = float(db)
        self.updateCoefficients()

    def SetMode(self, mode):
        if mode < SPLIT_BAND or mode > WIDEBAND:
            raise ValueError("mode")
        self.mode = int(mode)

    def SetDetector(self, det):
        if det < DETECT_BANDPASS or det > DETECT_HIGHPASS:
            raise ValueError("detector")
        self.detector = int(det)
        self.rebuildFilters()

    def SetListen(self, on):
        self.listen = bool(on)

    def SetFilterOrder(self, order):
        if order < 1 or order > 4:
            raise ValueError("filter order")
        self.filterOrder = int(order)
        self.rebuildFilters()

    def SetSampleRate(self, fs):
        if fs <= 0 or not finite(fs):
            raise ValueError("sample rate")
        if self.freqHz >= fs / 2:
            raise ValueError("frequency exceeds Nyquist for the sample rate")
        self.sampleRate = float(fs)
        self.updateCoefficients()
        self.rebuildFilters()

    # --- processing :414-475
    def ProcessSample(self, x: float) -> float:
        detected = x
        for f in self.detectFilters:
            detected = f.ProcessSample(detected)
        if self.listen:
            return detected
        level = abs(detected)
        if level > self.envLevel:
            self.envLevel += (level - self.envLevel) * self.attackCoeff
        else:
            self.envLevel = level + (self.envLevel - level) * self.releaseCoeff
        if self.trace is not None:
            self.trace.append(self.envLevel)
        gain = self.gain_fn(self.envLevel) if self.gain_fn else self.calculateGain(self.envLevel)
        if level > self.metrics[0]:
            self.metrics[0] = level
        if self.metrics[1] == 1.0 or gain < self.metrics[1]:
            self.metrics[1] = gain
        if self.mode == WIDEBAND:
            return x * gain
        band = x
        for f in self.bandFilters:
            band = f.ProcessSample(band)
        band *= self.bandNorm
        out = x + band * (gain - 1)
        wide = x * gain
        if abs(out) > abs(wide):
            self.clamped[1] += 1
            return wide
        self.clamped[0] += 1
        return out

    def ProcessInPlace(self, buf):  # :478-482
        for i in range(len(buf)):
            buf[i] = self.ProcessSample(float(buf[i]))
        return buf

    def Reset(self):  # :485-496
        self.envLevel = 0.0
        for f in self.detectFilters + self.bandFilters:
            f.Reset()
        self.metrics = [0.0, 1.0]

    def GetMetrics(self):  # :499-501
        return tuple(self.metrics)

    def ResetMetrics(self):  # :504-506
        self.metrics = [0.0, 1.0]

    # --- internal :513-622
    def calculateGain(self, env: float) -> float:
        if env <= 0:
            return 1.0
        overshoot = go_log2(env) - self.thresholdLog2
        if self.kneeDB <= 0:
            if overshoot <= 0:
                return 1.0
            gain = math.pow(2.0, -overshoot * (1.0 - 1.0 / self.ratio))
            return self.rangeLin if gain < self.rangeLin else gain
        half = self.kneeWidthLog2 * 0.5
        if overshoot < -half:
            return 1.0
        if overshoot > half:
            eff = overshoot
        else:
            scratch = overshoot + half
            eff = scratch * scratch * 0.5 * self.invKneeWidthLog2
        gain = math.pow(2.0, -eff * (1.0 - 1.0 / self.ratio))
        return self.rangeLin if gain < self.rangeLin else gain

    def updateCoefficients(self):  # :559-571
        self.thresholdLog2 = self.thresholdDB * LOG2_OF_10_DIV_20
        self.kneeWidthLog2 = self.kneeDB * LOG2_OF_10_DIV_20
        self.invKneeWidthLog2 = fdiv(1.0, self.kneeWidthLog2) if self.kneeDB > 0 else 0.0
        self.rangeLin = math.pow(10.0, self.rangeDB / 20.0)
        self.updateTimeConstants()

    def updateTimeConstants(self):  # :573-576
        ln2 = math.log(2.0)
        self.attackCoeff = 1.0 - math.exp(-ln2 / (self.attackMs * 0.001 * self.sampleRate))
        self.releaseCoeff = math.exp(-ln2 / (self.releaseMs * 0.001 * self.sampleRate))

    def section(self):
        fn = design.highpass if self.detector == DETECT_HIGHPASS else design.bandpass
        return fn(self.freqHz, self.q, self.sampleRate)

    def rebuildFilters(self):  # :578-622
        self.detectFilters = [Section(self.section()) for _ in range(self.filterOrder)]
        self.bandFilters = [Section(self.section()) for _ in range(self.filterOrder)]
        self.bandNorm = 1.0 / math.pow(self.q, float(self.filterOrder))

    def states(self):
        """(detect [4][2], band [4][2]): {d0, d1} of each section, zero past the order."""
        out = np.zeros((2, 4, 2))
        for k, casc in enumerate((self.detectFilters, self.bandFilters)):
            for i, f in enumerate(casc):
                out[k, i] = (f.d0, f.d1)
        return out[0], out[1]


def run_rows(make, x, cuts=None):
    """One instance per row of x [channels][n] from make(channel), processed in calls of `cuts` samples;
    returns (out, instances)."""
    x = np.asarray(x, dtype=np.float64)
    out = np.empty_like(x)
    inst = [make(c) for c in range(x.shape[0])]
    cuts = cuts or [x.shape[1]]
    for c, p in enumerate(inst):
        row, at = x[c].copy(), 0
        for m in cuts:
            row[at:at + m] = p.ProcessInPlace(row[at:at + m].copy())
            at += m
        out[c] = row
    return out, inst
