"""Line-by-line restatement of effects.Vocoder (dsp/effects/vocoder.go): every
product and sum is one IEEE double operation, nothing is contracted.  The band
tables, Q values, sections, downsample factors and groups and the envelope
coefficients come from Python's math (the C library) in the reference's
operation order, as the GPU runtime's host side takes them from the C library.

One instance carries `channels` reference instances that share the
configuration: the states are arrays [channels][...].  ProcessSample walks
channel 0 in Python floats, as the reference reads; process_many walks every
channel with numpy elementwise operations only, which round as the floats do.

A refused option or setter raises ValueError and changes nothing, as the
reference's return an error before they assign.
"""
from __future__ import annotations

import math

import numpy as np

THIRD_OCTAVE, BARK = 0, 1  # BandLayout :15-25

thirdOctaveFrequencies = [16, 20, 25, 31, 40, 50, 63, 80, 100, 125, 160, 200, 250, 315, 400, 500,
                          630, 800, 1000, 1250, 1600, 2000, 2500, 3150, 4000, 5000, 6300, 8000,
                          10000, 12500, 16000, 20000]  # :27-31
barkFrequencies = [100, 200, 300, 400, 510, 630, 770, 920, 1080, 1270, 1480, 1720, 2000,
                   2320, 2700, 3150, 3700, 4400, 5300, 6400, 7700, 9500, 12000, 15500]  # :33-36
thirdOctaveQ = 4.3184727050832485  # :39

LIMITS = {"attack": (0.01, 100.0), "release": (0.01, 1000.0), "level": (0.0, 10.0), "synthQ": (0.1, 20.0)}  # :49-56


def finite(v) -> bool:
    return not (math.isnan(v) or math.isinf(v))


def _check(kind, name, v):
    lo, hi = LIMITS[kind]
    if v < lo or v > hi or not finite(v):
        raise ValueError(f"vocoder: {name} must be in [{lo:g}, {hi:g}]: {v:g}")
    return float(v)


def cpgBandpass(freq, q, sampleRate):  # :527-547 -> (b0, b1, b2, a1, a2)
    w0 = 2 * math.pi * freq / sampleRate
    if w0 <= 0 or w0 >= math.pi:
        return (0.0, 0.0, 0.0, 0.0, 0.0)
    cw = math.cos(w0)
    sw = math.sin(w0)
    alpha = sw / (2 * q)
    a0 = 1 + alpha
    inv = 1.0 / a0
    return (alpha * inv, 0.0, -alpha * inv, -2 * cw * inv, (1 - alpha) * inv)


def antiAliasDecimatorLowpass(sampleRate, factor):  # :493-521
    if factor <= 1:
        return (1.0, 0.0, 0.0, 0.0, 0.0)
    cutoff = 0.35 * sampleRate / float(factor)
    if cutoff <= 0 or cutoff >= 0.5 * sampleRate:
        return (1.0, 0.0, 0.0, 0.0, 0.0)
    w0 = 2 * math.pi * cutoff / sampleRate
    cw = math.cos(w0)
    sw = math.sin(w0)
    q = 0.7071067811865476
    alpha = sw / (2 * q)
    a0 = 1 + alpha
    inv = 1.0 / a0
    return (((1 - cw) * 0.5) * inv, (1 - cw) * inv, ((1 - cw) * 0.5) * inv, (-2 * cw) * inv, (1 - alpha) * inv)


def barkBandQ(i):  # :550-572
    freqs = barkFrequencies
    lower = freqs[0] * 0.5 if i == 0 else (freqs[i - 1] + freqs[i]) / 2
    upper = freqs[i] * 1.25 if i >= len(freqs) - 1 else (freqs[i] + freqs[i + 1]) / 2
    bw = upper - lower
    if bw <= 0:
        return thirdOctaveQ
    return freqs[i] / bw


def _section_sample(c, s, ch, i, x):
    """biquad.Section.ProcessSample section.go:47-53 on states s[ch][i] in Python floats."""
    b0, b1, b2, a1, a2 = c
    s0, s1 = float(s[ch, i, 0]), float(s[ch, i, 1])
    y = b0 * x + s0
    s[ch, i, 0] = b1 * x - a1 * y + s1
    s[ch, i, 1] = b2 * x - a2 * y
    return y


def _section_many(c, s, i, x):
    """The same for every channel: x [channels], states s[:, i]."""
    b0, b1, b2, a1, a2 = c
    y = b0 * x + s[:, i, 0]
    s0 = b1 * x - a1 * y + s[:, i, 1]
    s1 = b2 * x - a2 * y
    return y, s0, s1


class Vocoder:
    """vocoder.go:199-833 for `channels` instances."""

    def __init__(self, sampleRate, channels=1, layout=THIRD_OCTAVE, synthQ=None, attackMs=0.5, releaseMs=2.0,
                 inputLevel=0.0, synthLevel=0.0, vocoderLevel=1.0, downsample=False):  # NewVocoder :241-280
        if sampleRate <= 0 or not finite(sampleRate):
            raise ValueError(f"vocoder: sample rate must be > 0: {sampleRate}")
        if layout not in (THIRD_OCTAVE, BARK):  # WithBandLayout :98-108
            raise ValueError(f"vocoder: invalid band layout: {layout}")
        self.channels = int(channels)
        self.sampleRate = float(sampleRate)
        self.layout = layout
        self.synthQ = thirdOctaveQ if synthQ is None else _check("synthQ", "synthesis Q", synthQ)  # :110-123
        self.synthQOverridden = synthQ is not None
        self.attackMs = _check("attack", "attack", attackMs)
        self.releaseMs = _check("release", "release", releaseMs)
        self.inputLevel = _check("level", "input level", inputLevel)
        self.synthLevel = _check("level", "synth level", synthLevel)
        self.vocoderLevel = _check("level", "vocoder level", vocoderLevel)
        self.downsample = bool(downsample)
        self.downsampleFactors = None
        self.downsampleCount = 0
        self.downsampleMax = 0
        self.downsampleAnalysisFilters = None
        self.downsampleGroupFactors = None
        self.computeEnvelopeCoeffs()
        self.buildFilterBanks()

    # ---- construction -------------------------------------------------------
    def computeEnvelopeCoeffs(self):  # :282-295
        sr = self.sampleRate
        self.attackCoeff = 1.0 - math.exp(-1.0 / (self.attackMs * 0.001 * sr)) if self.attackMs > 0 else 1.0
        self.releaseCoeff = math.exp(-1.0 / (self.releaseMs * 0.001 * sr)) if self.releaseMs > 0 else 0.0

    def _freqs(self):
        return thirdOctaveFrequencies if self.layout == THIRD_OCTAVE else barkFrequencies

    def _usable(self, sampleRate):
        nyquist = sampleRate / 2
        return sum(1 for f in self._freqs() if f < nyquist * 0.9)

    def buildFilterBanks(self):  # :297-395
        n = self._usable(self.sampleRate)
        if n == 0:
            kind = "bands" if self.layout == THIRD_OCTAVE else "Bark bands"
            raise ValueError(f"vocoder: no usable {kind} at sample rate {self.sampleRate:g} Hz")
        self.numBands = n
        freqs = self._freqs()
        self.analysisQ = [thirdOctaveQ if self.layout == THIRD_OCTAVE else barkBandQ(i) for i in range(n)]
        self.analysisCoeffs, self.synthesisCoeffs = [], []
        for i in range(n):
            q = self.analysisQ[i]
            synthQ = q if (self.layout == BARK and not self.synthQOverridden) else self.synthQ  # :339, :381-384
            self.analysisCoeffs.append(cpgBandpass(freqs[i], q, self.sampleRate))
            self.synthesisCoeffs.append(cpgBandpass(freqs[i], synthQ, self.sampleRate))
        self.analysisFilters = np.zeros((self.channels, n, 2))  # NewSection: zero states
        self.synthesisFilters = np.zeros((self.channels, n, 2))
        self.envelopes = np.zeros((self.channels, n))
        if self.downsample:
            self.computeDownsampleFactors()

    def computeDownsampleFactors(self):  # :401-438
        freqs = self._freqs()[:self.numBands]
        self.downsampleFactors = []
        maxFactor = 1
        threshold = 0.1 * self.sampleRate
        for i in range(self.numBands):
            factor = 1
            while float(2 * (factor << 1)) * freqs[i] < threshold:
                factor <<= 1
            self.downsampleFactors.append(factor)
            if factor > maxFactor:
                maxFactor = factor
        self.buildDownsampleGroups()
        self.downsampleAnalysisCoeffs = []
        for i in range(self.numBands):
            dsRate = self.sampleRate / float(self.downsampleFactors[i])
            ac = cpgBandpass(freqs[i], self.analysisQ[i], dsRate)
            if ac == (0.0, 0.0, 0.0, 0.0, 0.0):
                ac = cpgBandpass(freqs[i], self.analysisQ[i], self.sampleRate)
            self.downsampleAnalysisCoeffs.append(ac)
        self.downsampleAnalysisFilters = np.zeros((self.channels, self.numBands, 2))
        self.downsampleMax = maxFactor
        self.downsampleCount = 0
        self.computeDownsampleEnvelopeCoeffs()

    def buildDownsampleGroups(self):  # :440-468
        factors = sorted(set(self.downsampleFactors))
        self.downsampleGroupFactors = factors
        self.downsampleGroupMasks = [f - 1 for f in factors]
        self.downsampleGroupAACoeffs = [antiAliasDecimatorLowpass(self.sampleRate, f) for f in factors]
        self.downsampleGroupAAFilters = np.zeros((self.channels, len(factors), 2))
        self.downsampleGroupBands = [[b for b, f in enumerate(self.downsampleFactors) if f == g] for g in factors]

    def computeDownsampleEnvelopeCoeffs(self):  # :470-489
        if not self.downsampleFactors:
            return
        self.downsampleAttackCoeffs, self.downsampleReleaseCoeffs = [], []
        for factor in self.downsampleFactors:
            scale = float(factor)
            self.downsampleAttackCoeffs.append(
                1.0 - math.exp(-scale / (self.attackMs * 0.001 * self.sampleRate)) if self.attackMs > 0 else 1.0)
            self.downsampleReleaseCoeffs.append(
                math.exp(-scale / (self.releaseMs * 0.001 * self.sampleRate)) if self.releaseMs > 0 else 0.0)

    # ---- processing ---------------------------------------------------------
    def _multirate(self):
        return self.downsample and self.downsampleGroupFactors is not None and len(self.downsampleGroupFactors) > 0

    def ProcessSample(self, modulator: float, carrier: float, ch: int = 0) -> float:  # :578-630
        vocoded = 0.0
        if self._multirate():
            cnt = self.downsampleCount
            for g in range(len(self.downsampleGroupFactors)):
                decimated = _section_sample(self.downsampleGroupAACoeffs[g], self.downsampleGroupAAFilters, ch, g,
                                            modulator)
                if cnt & self.downsampleGroupMasks[g] != 0:
                    continue
                for i in self.downsampleGroupBands[g]:
                    bandSignal = _section_sample(self.downsampleAnalysisCoeffs[i], self.downsampleAnalysisFilters, ch,
                                                 i, decimated)
                    a = abs(bandSignal)
                    env = float(self.envelopes[ch, i])
                    if a > env:
                        env += (a - env) * self.downsampleAttackCoeffs[i]
                    else:
                        env = a + (env - a) * self.downsampleReleaseCoeffs[i]
                    self.envelopes[ch, i] = env
            for i in range(self.numBands):
                vocoded += float(self.envelopes[ch, i]) * _section_sample(self.synthesisCoeffs[i],
                                                                          self.synthesisFilters, ch, i, carrier)
            self.downsampleCount += 1
            if self.downsampleCount >= self.downsampleMax:
                self.downsampleCount = 0
        else:
            for i in range(self.numBands):
                bandSignal = _section_sample(self.analysisCoeffs[i], self.analysisFilters, ch, i, modulator)
                a = abs(bandSignal)
                env = float(self.envelopes[ch, i])
                if a > env:
                    env += (a - env) * self.attackCoeff
                else:
                    env = a + (env - a) * self.releaseCoeff
                self.envelopes[ch, i] = env
                vocoded += env * _section_sample(self.synthesisCoeffs[i], self.synthesisFilters, ch, i, carrier)
        return self.vocoderLevel * vocoded + self.synthLevel * carrier + self.inputLevel * modulator

    def ProcessBlock(self, modulator, carrier):  # :634-645, one channel
        if len(modulator) != len(carrier):
            raise ValueError("vocoder: buffer length mismatch")
        return np.array([self.ProcessSample(float(m), float(c)) for m, c in zip(modulator, carrier)], dtype=np.float64)

    def _many_sample(self, m, c):
        """ProcessSample for every channel: m, c [channels]."""
        vocoded = np.zeros(self.channels)
        if self._multirate():
            cnt = self.downsampleCount
            for g in range(len(self.downsampleGroupFactors)):
                aa = self.downsampleGroupAAFilters
                decimated, aa[:, g, 0], aa[:, g, 1] = _section_many(self.downsampleGroupAACoeffs[g], aa, g, m)
                if cnt & self.downsampleGroupMasks[g] != 0:
                    continue
                for i in self.downsampleGroupBands[g]:
                    d = self.downsampleAnalysisFilters
                    bandSignal, d[:, i, 0], d[:, i, 1] = _section_many(self.downsampleAnalysisCoeffs[i], d, i, decimated)
                    a = np.abs(bandSignal)
                    env = self.envelopes[:, i]
                    self.envelopes[:, i] = np.where(a > env, env + (a - env) * self.downsampleAttackCoeffs[i],
                                                    a + (env - a) * self.downsampleReleaseCoeffs[i])
            for i in range(self.numBands):
                s = self.synthesisFilters
                y, s[:, i, 0], s[:, i, 1] = _section_many(self.synthesisCoeffs[i], s, i, c)
                vocoded = vocoded + self.envelopes[:, i] * y
            self.downsampleCount += 1
            if self.downsampleCount >= self.downsampleMax:
                self.downsampleCount = 0
        else:
            for i in range(self.numBands):
                an, s = self.analysisFilters, self.synthesisFilters
                bandSignal, an[:, i, 0], an[:, i, 1] = _section_many(self.analysisCoeffs[i], an, i, m)
                a = np.abs(bandSignal)
                env = self.envelopes[:, i]
                env = np.where(a > env, env + (a - env) * self.attackCoeff, a + (env - a) * self.releaseCoeff)
                self.envelopes[:, i] = env
                y, s[:, i, 0], s[:, i, 1] = _section_many(self.synthesisCoeffs[i], s, i, c)
                vocoded = vocoded + env * y
        return self.vocoderLevel * vocoded + self.synthLevel * c + self.inputLevel * m

    def process_many(self, modulator, carrier) -> np.ndarray:
        """ProcessBlock on [channels][n] rows; the counter advances once per sample for all channels."""
        m = np.asarray(modulator, dtype=np.float64).reshape(self.channels, -1)
        c = np.asarray(carrier, dtype=np.float64).reshape(self.channels, -1)
        if m.shape != c.shape:
            raise ValueError("vocoder: buffer length mismatch")
        out = np.empty_like(m)
        with np.errstate(all="ignore"):
            for t in range(m.shape[1]):
                out[:, t] = self._many_sample(m[:, t], c[:, t])
        return out

    # ---- Reset, setters, getters --------------------------------------------
    def Reset(self):  # :648-670
        self.envelopes[:] = 0
        self.analysisFilters[:] = 0
        if self.downsampleAnalysisFilters is not None:
            self.downsampleAnalysisFilters[:] = 0
        if self.downsampleGroupFactors is not None:
            self.downsampleGroupAAFilters[:] = 0
        self.synthesisFilters[:] = 0
        self.downsampleCount = 0

    def SetSampleRate(self, sampleRate):  # :673-683
        if sampleRate <= 0 or not finite(sampleRate):
            raise ValueError(f"vocoder: sample rate must be > 0: {sampleRate}")
        if self._usable(float(sampleRate)) == 0:
            # the reference assigns before buildFilterBanks fails and leaves an instance that cannot process;
            # the GPU runtime refuses and changes nothing, and so does this restatement
            kind = "bands" if self.layout == THIRD_OCTAVE else "Bark bands"
            raise ValueError(f"vocoder: no usable {kind} at sample rate {sampleRate:g} Hz")
        self.sampleRate = float(sampleRate)
        self.computeEnvelopeCoeffs()
        self.envelopes = None
        self.buildFilterBanks()

    def SetDownsampling(self, enabled):  # :737-769
        self.downsample = bool(enabled)
        if enabled:
            self.computeDownsampleFactors()
        else:
            self.downsampleFactors = None
            self.downsampleAnalysisFilters = None
            self.downsampleGroupFactors = None
            self.downsampleGroupMasks = None
            self.downsampleGroupAAFilters = None
            self.downsampleGroupBands = None
            self.downsampleAttackCoeffs = None
            self.downsampleReleaseCoeffs = None
            self.downsampleCount = 0
            self.downsampleMax = 0

    def SetAttack(self, ms):  # :772-783
        self.attackMs = _check("attack", "attack", ms)
        self.computeEnvelopeCoeffs()
        self.computeDownsampleEnvelopeCoeffs()

    def SetRelease(self, ms):  # :786-797
        self.releaseMs = _check("release", "release", ms)
        self.computeEnvelopeCoeffs()
        self.computeDownsampleEnvelopeCoeffs()

    def SetInputLevel(self, level):  # :800-809
        self.inputLevel = _check("level", "input level", level)

    def SetSynthLevel(self, level):  # :812-821
        self.synthLevel = _check("level", "synth level", level)

    def SetVocoderLevel(self, level):  # :824-833
        self.vocoderLevel = _check("level", "vocoder level", level)

    def SampleRate(self):  # :688-717
        return self.sampleRate

    def Layout(self):
        return self.layout

    def NumBands(self):
        return self.numBands

    def SynthesisQ(self):
        return self.synthQ

    def Attack(self):
        return self.attackMs

    def Release(self):
        return self.releaseMs

    def InputLevel(self):
        return self.inputLevel

    def SynthLevel(self):
        return self.synthLevel

    def VocoderLevel(self):
        return self.vocoderLevel

    def Downsampling(self):
        return self.downsample

    def DownsampleFactors(self):  # :722-731
        if not self.downsample or self.downsampleFactors is None:
            return None
        return list(self.downsampleFactors)
