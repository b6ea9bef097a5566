"""Restatement of effects.SpectralFreeze (dsp/effects/spectral_freeze.go) and
pitch.SpectralPitchShifter (dsp/effects/pitch/pitch_shift_spectral.go) for one
channel in numpy float64: the bins of a frame are taken together, every
product and sum is one IEEE double operation per element, nothing is
contracted, and the frames run in the reference's order.

One stated deviation, shared with the device: the imaginary parts
of analysis bins 0 and N/2 are set to +0.0 before the polar conversion.  What
the reference's FFT library leaves there is an accident of that library, and the
bin-shift path is chaotic in its sign.

The transforms are numpy's (pocketfft); `spectrum_hook(frame, X)` may return a
perturbed analysis spectrum, which is how the tests derive their bars, and
`margins` collects how close the run came to each data-dependent decision.

A refused setter raises ValueError and changes nothing, as the reference's
setters return an error before they assign.
"""
from __future__ import annotations

import math

import numpy as np

import resample_ref
from algodsp import resample as rs

NORM_FLOOR = 1e-12  # spectral_freeze.go:17, pitch_shift_spectral.go:19
MIN_FRAME = 64  # :16, :18
BIN_SHIFT_THRESHOLD = 0.15  # pitch_shift_spectral.go:24
IDENTITY_EPS = 1e-9  # pitch_shifter.go:29
MIN_RATIO, MAX_RATIO = 0.25, 4.0  # pitch_shifter.go:19-20
PHASE_HOLD, PHASE_ADVANCE = 0, 1  # spectral_freeze.go:23-28
TYPE_RECTANGULAR, TYPE_HANN, TYPE_HAMMING, TYPE_BLACKMAN = range(4)  # window.go:12-16
_COSINE = {TYPE_HANN: (0.5, -0.5), TYPE_HAMMING: (0.54, -0.46), TYPE_BLACKMAN: (0.42, -0.5, 0.08)}  # tables.go:4-6


def finite_positive(v) -> bool:
    return v > 0 and not (math.isnan(v) or math.isinf(v))


def is_pow2(n: int) -> bool:
    return n > 0 and (n & (n - 1)) == 0


def window_periodic(t: int, n: int) -> np.ndarray:
    """window.Generate(t, n, WithPeriodic()) (window.go:140-162): samplePosition
    i / n (:404-415), evalWindow -> cosineFromCoeffs (:339-341, :393-402)."""
    if t == TYPE_RECTANGULAR:
        return np.ones(n)  # :344-345
    if t not in _COSINE:
        raise ValueError(f"window type {t} is not restated")
    x = np.arange(n, dtype=np.float64) / float(n) if n > 1 else np.zeros(n)
    phase = 2 * np.pi * x
    s = np.zeros(n)
    for k, c in enumerate(_COSINE[t]):
        s = s + c * np.cos(float(k) * phase)
    return s


def omega_table(n: int) -> np.ndarray:
    """omega[k] = 2 * math.Pi * float64(k) / float64(N) (spectral_freeze.go:397-400)."""
    return np.array([2 * math.pi * float(k) / float(n) for k in range(n // 2 + 1)])


def wrap_phase(x: np.ndarray) -> np.ndarray:  # wrapPhase pitch_shift_spectral.go:627-634
    x = np.fmod(x + math.pi, 2 * math.pi)
    x = np.where(x < 0, x + 2 * math.pi, x)
    return x - math.pi


def fit_length(a: np.ndarray, n: int) -> np.ndarray:  # fitLength :620-625
    out = np.zeros(n)
    m = min(n, len(a))
    out[:m] = a[:m]
    return out


class Margins:
    """How close a run came to a data-dependent decision (smaller is closer)."""

    def __init__(self):
        self.peak_gap = math.inf  # relative gap in a peak comparison
        self.wrap_gap = math.inf  # distance of an unwrapped delta from +-pi (mod 2 pi), bins 1 ... N/2-1
        self.dc_re = math.inf  # |Re X[0]| / ||frame||
        self.nyq_re = math.inf  # |Re X[N/2]| / ||frame||

    def real_bins(self, X, frame_norm):
        if frame_norm > 0:
            h = len(X) // 2
            self.dc_re = min(self.dc_re, abs(X[0].real) / frame_norm)
            self.nyq_re = min(self.nyq_re, abs(X[h].real) / frame_norm)

    def peaks(self, mag):
        a, b = mag[1:], mag[:-1]
        scale = np.maximum(np.maximum(np.abs(a), np.abs(b)), 1e-300)
        if len(a) and np.any(mag > 0):
            self.peak_gap = min(self.peak_gap, float(np.min(np.abs(a - b) / scale)))

    def wrap(self, raw_delta):
        inner = raw_delta[1:-1]
        if len(inner):
            d = np.abs(np.fmod(np.abs(inner), 2 * math.pi) - math.pi)
            self.wrap_gap = min(self.wrap_gap, float(np.min(d)))

    def least(self):
        return min(self.peak_gap, self.wrap_gap, self.dc_re, self.nyq_re)


class _Stft:
    """The framing both effects share: analysis of one frame and the overlap-add."""

    def __init__(self):
        self.spectrum_hook = None
        self.margins = Margins()
        self.last_norm = None  # norm of the last call's overlap-add, [outLen]
        self.last_sum = None  # the overlap-add sums before the division

    def _rebuild_tables(self):
        self.windowCoeffs = window_periodic(self.windowType, self.frameSize)  # :388
        self.omega = omega_table(self.frameSize)

    def _analysis(self, x, pos, frame):
        """The windowed zero-padded frame (:232-241) and its half spectrum with bins 0 and N/2 pinned."""
        n = self.frameSize
        seg = np.zeros(n)
        m = max(0, min(n, len(x) - pos))
        seg[:m] = x[pos:pos + m]
        seg = seg * self.windowCoeffs
        X = np.fft.fft(seg)
        if self.spectrum_hook is not None:
            X = self.spectrum_hook(frame, X, float(np.sqrt(np.sum(seg * seg))))
        half = n // 2
        self.margins.real_bins(X, float(np.sqrt(np.sum(seg * seg))))
        re = X.real[:half + 1].copy()
        im = X.imag[:half + 1].copy()
        im[0] = 0.0  # the stated deviation
        im[half] = 0.0
        return re, im

    def _synthesis(self, mag, phase):
        """mag cos, mag sin, the conjugate mirror, the inverse transform, the window (:268-306)."""
        n = self.frameSize
        half = n // 2
        S = np.zeros(n, dtype=np.complex128)
        S[:half + 1] = mag * np.cos(phase) + 1j * (mag * np.sin(phase))
        S[0] = complex(S[0].real, 0.0)
        S[half] = complex(S[half].real, 0.0)
        S[half + 1:] = np.conj(S[1:half][::-1])
        return np.fft.ifft(S).real * self.windowCoeffs

    def _overlap_add(self, frames, hop, out_len):
        """wet[idx] += frame[i]; norm[idx] += w*w, frame after frame (:301-306); the floor test (:312-314)."""
        n = self.frameSize
        wet = np.zeros(out_len)
        norm = np.zeros(out_len)
        w2 = self.windowCoeffs * self.windowCoeffs
        for j, fr in enumerate(frames):
            pos = j * hop
            wet[pos:pos + n] = wet[pos:pos + n] + fr
            norm[pos:pos + n] = norm[pos:pos + n] + w2
        self.last_norm, self.last_sum = norm.copy(), wet.copy()
        ok = norm > NORM_FLOOR
        wet[ok] = wet[ok] / norm[ok]
        return wet


class SpectralFreeze(_Stft):
    def __init__(self, sample_rate: float):  # NewSpectralFreeze :60-80
        super().__init__()
        if not finite_positive(sample_rate):
            raise ValueError("spectral freeze sample rate must be > 0")
        self.sampleRate = sample_rate
        self.frameSize, self.hopSize = 1024, 256
        self.mix = 1.0
        self.windowType = TYPE_HANN
        self.phaseMode = PHASE_ADVANCE
        self.frozen = False
        self._rebuild()

    def _rebuild(self):  # rebuildState :371-410
        if self.frameSize < MIN_FRAME or not is_pow2(self.frameSize):
            raise ValueError("spectral freeze frame size must be power-of-two and >= 64")
        if self.hopSize <= 0 or self.hopSize >= self.frameSize:
            raise ValueError("spectral freeze hop size out of range")
        self._rebuild_tables()
        bins = self.frameSize // 2 + 1
        self.heldMagnitude = np.zeros(bins)
        self.phaseAcc = np.zeros(bins)
        self.hasFrozenFrame = False

    def SetSampleRate(self, v):  # :104-112
        if not finite_positive(v):
            raise ValueError("spectral freeze sample rate must be > 0")
        self.sampleRate = v

    def SetFrameSize(self, size):  # :115-127
        if size < MIN_FRAME or not is_pow2(size):
            raise ValueError("spectral freeze frame size must be power-of-two and >= 64")
        self.frameSize = size
        if self.hopSize >= self.frameSize:
            self.hopSize = max(self.frameSize // 4, 1)
        self._rebuild()

    def SetHopSize(self, hop):  # :130-138
        if hop <= 0 or hop >= self.frameSize:
            raise ValueError("spectral freeze hop size out of range")
        self.hopSize = hop

    def SetMix(self, mix):  # :141-149
        if not (0 <= mix <= 1):
            raise ValueError("spectral freeze mix must be in [0, 1]")
        self.mix = mix

    def SetWindowType(self, t):  # :152-155
        window_periodic(t, 4)
        self.windowType = t
        self._rebuild()

    def SetPhaseMode(self, mode):  # :158-166
        if mode not in (PHASE_HOLD, PHASE_ADVANCE):
            raise ValueError("spectral freeze phase mode invalid")
        self.phaseMode = mode

    def SetFrozen(self, frozen):  # :169-175
        if bool(frozen) != self.frozen:
            self.hasFrozenFrame = False
        self.frozen = bool(frozen)

    def Freeze(self):
        self.SetFrozen(True)

    def Unfreeze(self):
        self.SetFrozen(False)

    def Reset(self):  # :184-189
        self.hasFrozenFrame = False
        self.phaseAcc[:] = 0.0

    def Process(self, x) -> np.ndarray:  # ProcessWithError :210-320
        x = np.asarray(x, dtype=np.float64)
        if len(x) == 0:
            return np.zeros(0)
        hop = self.hopSize
        frame_count = 1 + (len(x) - 1) // hop
        out_len = (frame_count - 1) * hop + self.frameSize
        hop_f = float(hop)
        frames = []
        for frame in range(frame_count):
            re, im = self._analysis(x, frame * hop, frame)
            just_captured = False
            if self.frozen and not self.hasFrozenFrame:  # :250-260
                self.heldMagnitude = np.hypot(re, im)
                self.phaseAcc = np.arctan2(im, re)
                self.hasFrozenFrame = True
                just_captured = True
            if self.frozen and self.hasFrozenFrame:  # :262-274
                if self.phaseMode == PHASE_ADVANCE and not just_captured:
                    self.phaseAcc = self.phaseAcc + self.omega * hop_f
                mag, phase = self.heldMagnitude, self.phaseAcc
            else:  # :275-286
                mag, phase = np.hypot(re, im), np.arctan2(im, re)
            frames.append(self._synthesis(mag, phase))
        wet = self._overlap_add(frames, hop, out_len)
        return x * (1 - self.mix) + wet[:len(x)] * self.mix  # :316


# ---- the graph runtimes (dsp/effectchain) ---------------------------------------
def go_round(v: float) -> float:
    """math.Round: half away from zero."""
    a = abs(v)
    f = math.floor(a)
    return math.copysign(f + 1 if a - f >= 0.5 else f, v)  # a - f is exact; a + 0.5 would round


def clamp(v, lo, hi):  # core.Clamp
    return lo if v < lo else (hi if v > hi else v)


def get_num(num: dict, key: str, default: float) -> float:  # Params.GetNum params.go:15-27
    v = num.get(key)
    if v is None or math.isnan(v) or math.isinf(v):
        return default
    return v


def sanitize_spectral_pitch_frame_size(n: int) -> int:  # configure.go:563-593
    if n < 256:
        return 256
    if n > 4096:
        return 4096
    if n > 0 and (n & (n - 1)) == 0:
        return n
    lower = 256
    while lower < n:
        lower <<= 1
    upper = lower
    lower >>= 1
    if lower < 256:
        lower = 256
    if n - lower <= upper - n:
        return lower
    return upper


def normalize_spectral_freeze_phase_mode(raw) -> int:  # normalize.go:174-183
    if raw == "hold":
        return PHASE_HOLD
    return PHASE_ADVANCE  # "advance" falls through to the default


def _runtime_frame_hop(num: dict):  # runtime_filter_pitch_reverb.go:253-259 and :279-285
    frame = sanitize_spectral_pitch_frame_size(int(go_round(get_num(num, "frameSize", 1024))))
    hop = max(int(go_round(float(frame) * clamp(get_num(num, "hopRatio", 0.25), 0.01, 0.99))), 1)
    if hop >= frame:
        hop = frame - 1
    return frame, hop


def spectral_freeze_runtime(sample_rate: float, num: dict, strs: dict) -> "SpectralFreeze":
    """spectralFreezeRuntime.Configure (runtime_filter_pitch_reverb.go:278-299) on the factory's
    NewSpectralFreeze(fs), through configureSpectralFreeze (configure.go:391-433) in its setter order."""
    frame, hop = _runtime_frame_hop(num)
    frozen = get_num(num, "frozen", 1) >= 0.5
    fx = SpectralFreeze(sample_rate)
    fx.SetSampleRate(sample_rate)
    fx.SetFrameSize(frame)
    fx.SetHopSize(hop)
    fx.SetWindowType(TYPE_HANN)
    fx.SetMix(clamp(get_num(num, "mix", 1), 0, 1))
    fx.SetPhaseMode(normalize_spectral_freeze_phase_mode(strs.get("phaseMode")))
    fx.SetFrozen(frozen)
    return fx


def spectral_pitch_runtime(sample_rate: float, num: dict) -> "SpectralPitchShifter":
    """spectralPitchRuntime.Configure (runtime_filter_pitch_reverb.go:252-268) on the factory's
    NewSpectralPitchShifter(fs), through configureSpectralPitch (configure.go:372-389) in its setter order."""
    frame, hop = _runtime_frame_hop(num)
    fx = SpectralPitchShifter(sample_rate)
    fx.SetSampleRate(sample_rate)
    fx.SetPitchSemitones(clamp(get_num(num, "semitones", 0), -24, 24))
    fx.SetFrameSize(frame)
    fx.SetAnalysisHop(hop)
    return fx


def nearest_peak_walk(peaks, half: int) -> np.ndarray:
    """The forward walk of :460-471: pk for every k in [0, half]."""
    out = np.zeros(half + 1, dtype=np.int64)
    idx = 0
    for k in range(half + 1):
        while idx + 1 < len(peaks):
            curr, nxt = peaks[idx], peaks[idx + 1]
            if abs(nxt - k) < abs(curr - k):
                idx += 1
            else:
                break
        out[k] = peaks[idx]
    return out


def nearest_peak_vec(peaks, half: int) -> np.ndarray:
    """Nearest peak of every k in [0, half], a tie to the lower: what the walk settles on."""
    p = np.asarray(peaks, dtype=np.int64)
    k = np.arange(half + 1, dtype=np.int64)
    hi = np.searchsorted(p, k, side="left")  # first peak >= k
    up = p[np.minimum(hi, len(p) - 1)]
    lo = p[np.maximum(hi - 1, 0)]
    use_up = (hi < len(p)) & ((hi == 0) | (np.abs(up - k) < np.abs(k - lo)))
    return np.where(use_up, up, lo)


class SpectralPitchShifter(_Stft):
    def __init__(self, sample_rate: float):  # NewSpectralPitchShifter :66-87
        super().__init__()
        if not finite_positive(sample_rate):
            raise ValueError("spectral pitch shifter sample rate must be positive and finite")
        self.sampleRate = sample_rate
        self.pitchRatio = 1.0
        self.frameSize, self.analysisHop = 1024, 256
        self.windowType = TYPE_HANN
        self.resampleQuality = rs.QualityBalanced
        self._update_synthesis_hop()
        self._rebuild_tables()

    def _update_synthesis_hop(self):  # :614-618 (math.Round: half away from zero)
        v = float(self.analysisHop) * self.pitchRatio
        self.synthesisHop = max(int(math.floor(v + 0.5)) if v >= 0 else int(math.ceil(v - 0.5)), 1)

    def use_bin_shifting(self) -> bool:  # :230-232
        return abs(self.pitchRatio - 1) <= BIN_SHIFT_THRESHOLD

    def EffectivePitchRatio(self) -> float:  # :108-114
        if self.use_bin_shifting():
            return self.pitchRatio
        return float(self.synthesisHop) / float(self.analysisHop)

    def SynthesisHop(self) -> int:  # :123-129
        return self.analysisHop if self.use_bin_shifting() else self.synthesisHop

    def SetSampleRate(self, v):  # :140-148
        if not finite_positive(v):
            raise ValueError("spectral pitch shifter sample rate must be positive and finite")
        self.sampleRate = v

    def SetPitchRatio(self, ratio):  # :151-161
        if not finite_positive(ratio) or ratio < MIN_RATIO or ratio > MAX_RATIO:
            raise ValueError("spectral pitch ratio must be in [0.25, 4]")
        self.pitchRatio = ratio
        self._update_synthesis_hop()

    def SetPitchSemitones(self, semitones):  # :164-177
        if math.isnan(semitones) or math.isinf(semitones):
            raise ValueError("spectral pitch shifter semitones must be finite")
        self.SetPitchRatio(2.0 ** (semitones / 12.0))

    def SetFrameSize(self, size):  # :180-196
        if size < MIN_FRAME or not is_pow2(size):
            raise ValueError("spectral frame size must be power-of-two and >= 64")
        self.frameSize = size
        if self.analysisHop >= self.frameSize:
            self.analysisHop = max(self.frameSize // 4, 1)
        self._update_synthesis_hop()
        self._rebuild_tables()

    def SetAnalysisHop(self, hop):  # :199-208
        if hop <= 0 or hop >= self.frameSize:
            raise ValueError("spectral analysis hop out of range")
        self.analysisHop = hop
        self._update_synthesis_hop()

    def SetWindowType(self, t):  # :211-214
        window_periodic(t, 4)
        self.windowType = t
        self._rebuild_tables()

    def SetResampleQuality(self, q):  # :217-219
        self.resampleQuality = q

    def Process(self, x) -> np.ndarray:  # :238-259
        x = np.asarray(x, dtype=np.float64)
        if len(x) == 0:
            return np.zeros(0)
        if abs(self.pitchRatio - 1) <= IDENTITY_EPS:
            return x.copy()
        if self.use_bin_shifting():
            return self._bin_shift(x)
        return self._time_stretch(x)

    def _inst_freqs(self, re, im, prev, hop_f):  # :320-331, :426-437
        mag = np.hypot(re, im)
        phase = np.arctan2(im, re)
        raw = phase - prev - self.omega * hop_f
        self.margins.wrap(raw)
        delta = wrap_phase(raw)
        return mag, phase, self.omega + delta / hop_f

    def _bin_shift(self, x):  # processBinShift :287-390
        hop = self.analysisHop
        frame_count = 1 + (len(x) - 1) // hop
        out_len = (frame_count - 1) * hop + self.frameSize
        half = self.frameSize // 2
        hop_f = float(hop)
        ratio = self.pitchRatio
        prev = np.zeros(half + 1)  # Reset :222-227
        total = np.zeros(half + 1)
        k = np.arange(half + 1)
        src = k.astype(np.float64) / ratio  # :335
        dead = src >= float(half)
        lo = np.where(dead, 0, src.astype(np.int64))
        frac = src - lo.astype(np.float64)
        hi = np.minimum(lo + 1, half)
        frames = []
        for frame in range(frame_count):
            re, im = self._analysis(x, frame * hop, frame)
            mag, phase, inst = self._inst_freqs(re, im, prev, hop_f)
            prev = phase
            smag = np.where(dead, 0.0, mag[lo] * (1 - frac) + mag[hi] * frac)  # :337-346
            sfreq = np.where(dead, self.omega, (inst[lo] * (1 - frac) + inst[hi] * frac) * ratio)
            total = total + sfreq * hop_f  # :354
            frames.append(self._synthesis(smag, total))
        return fit_length(self._overlap_add(frames, hop, out_len), len(x))

    def _time_stretch(self, x):  # processTimeStretch :393-527
        ha, hs = self.analysisHop, self.synthesisHop
        frame_count = 1 + (len(x) - 1) // ha
        stretched_len = (frame_count - 1) * hs + self.frameSize
        half = self.frameSize // 2
        ha_f, hs_f = float(ha), float(hs)
        prev = np.zeros(half + 1)
        total = np.zeros(half + 1)
        frames = []
        for frame in range(frame_count):
            re, im = self._analysis(x, frame * ha, frame)
            mag, phase, inst = self._inst_freqs(re, im, prev, ha_f)
            prev = phase
            self.margins.peaks(mag)
            is_peak = np.zeros(half + 1, dtype=bool)
            is_peak[1:half] = (mag[1:half] >= mag[0:half - 1]) & (mag[1:half] > mag[2:half + 1])  # :441-445
            peaks = np.flatnonzero(is_peak)
            if len(peaks) == 0:  # :447-454
                total = total + inst * hs_f
            else:
                total[peaks] = total[peaks] + inst[peaks] * hs_f  # :456-458
                pk = nearest_peak_vec(peaks, half)
                locked = total[pk] + (prev - prev[pk])  # :473-476 (prevPhase is this frame's phase by now)
                total = np.where(is_peak, total, locked)
            frames.append(self._synthesis(mag, total))
        stretched = self._overlap_add(frames, hs, stretched_len)
        if hs == ha:  # :512-514
            return fit_length(stretched, len(x))
        shifted = self.resample(stretched)
        return fit_length(shifted, len(x))

    def resample_taps(self):
        g = math.gcd(self.analysisHop, self.synthesisHop)
        p = rs.QualityProfile(self.resampleQuality)
        return rs.design_polyphase_fir(self.analysisHop // g, self.synthesisHop // g, p.TapsPerPhase, p.CutoffScale,
                                       p.KaiserBeta)

    def resample(self, stretched):  # resample.Resample(stretched, analysisHop, synthesisHop, quality) :516-521
        return resample_ref.Ref(self.analysisHop, self.synthesisHop, self.resample_taps()).process_vec(stretched)
