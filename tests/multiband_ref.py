"""Restatement of crossover.MultiBand (dsp/filter/crossover/crossover.go:113-222)
and dynamics.MultibandCompressor (dsp/effects/dynamics/multiband.go) for one
channel, on the oracle: every crossover cascade is or_biquad_chain_process_block
on design.crossover's sections, every band's compressor is the oracle's
(or_comp_*), and the bands are summed in band order.

The setters keep the reference's semantics: a value a Compressor setter rejects
(compressor.go:16-23, core.go:131-250, 542-564) raises ValueError and changes
nothing, SetBandMakeupGain turns auto makeup off, a bad band index raises,
SetAllBands* stops at the first band that rejects, SetBandConfig skips a field
that is None (or 0 for Ratio / AttackMs / ReleaseMs).
"""
from __future__ import annotations

import math

import numpy as np

import oracle_lib as O
from algodsp import design

MAX_ORDER, MIN_ORDER, MAX_BANDS, MIN_FREQ = 24, 2, 8, 20.0  # multiband.go:12-18


class MultiBand:
    """crossover.MultiBand: stage i's highpass output is stage i + 1's input."""

    def __init__(self, freqs, order, fs):
        freqs = [float(f) for f in freqs]
        if not freqs:  # :136-138
            raise ValueError("crossover: at least one frequency is required")
        for a, b in zip(freqs, freqs[1:]):  # :140-144
            if b <= a:
                raise ValueError("crossover: frequencies must be strictly ascending")
        self.stages = []
        for f in freqs:  # crossover.New :32-65
            secs = design.crossover(f, order, fs)
            if secs is None:
                raise ValueError(f"crossover: cannot design LR{order} at {f} Hz, fs {fs}")
            self.stages.append([np.array(side, dtype=np.float64) for side in secs])
        self.bands = len(freqs) + 1
        self.Reset()

    def NumBands(self):
        return self.bands

    def sections(self):
        """[stages][2 (LP, HP)][S][5]"""
        return np.array(self.stages)

    def Reset(self):  # :218-222
        self.state = [[np.zeros(2 * len(side)) for side in st] for st in self.stages]

    def get_state(self):
        """[stages][2][S][2] {s0, s1}"""
        return np.array([[s.reshape(-1, 2) for s in st] for st in self.state])

    def set_state(self, state):
        self.state = [[np.array(s, dtype=np.float64).reshape(-1).copy() for s in st] for st in state]

    def ProcessBlock(self, x):  # :194-215 -> [bands][n]
        rem = np.array(x, dtype=np.float64)
        out = []
        for i, (lp, hp) in enumerate(self.stages):
            lo, self.state[i][0] = O.biquad_chain_block(lp.reshape(-1), self.state[i][0], 1.0, rem)
            rem, self.state[i][1] = O.biquad_chain_block(hp.reshape(-1), self.state[i][1], 1.0, rem)
            out.append(lo)
        out.append(rem)
        return np.array(out).reshape(self.bands, -1)

    def ProcessSample(self, x):  # :176-189
        return self.ProcessBlock([x])[:, 0]


def _finite(v):
    return not (math.isnan(v) or math.isinf(v))


def validate_compressor(cfg: dict):
    """What the dynamics setters accept (compressor.go:16-23, core.go:10-12, 106-250, 542-564)."""
    fs = cfg["sample_rate"]
    ok = (_finite(cfg["threshold_db"]) and 1.0 <= cfg["ratio"] <= 100.0 and 0.0 <= cfg["knee_db"] <= 24.0
          and 0.1 <= cfg["attack_ms"] <= 1000.0 and 1.0 <= cfg["release_ms"] <= 5000.0
          and 1.0 <= cfg["rms_window_ms"] <= 1000.0 and _finite(cfg["makeup_db"])
          and cfg["topology"] in (0, 1) and cfg["detector_mode"] in (0, 1))
    lo, hi = cfg["sidechain_low_cut_hz"], cfg["sidechain_high_cut_hz"]
    ok = ok and _finite(lo) and _finite(hi) and lo >= 0 and hi >= 0
    ok = ok and (lo == 0 or 1.0 <= lo < fs / 2) and (hi == 0 or 1.0 <= hi < fs / 2)
    ok = ok and not (lo > 0 and hi > 0 and lo >= hi)
    if not ok:
        raise ValueError(f"dynamics: rejected config {cfg}")


def validate_multiband(freqs, order, fs):
    """validateMultibandParams multiband.go:661-709."""
    if not (fs > 0) or not _finite(fs):
        raise ValueError("multiband compressor: sample rate must be positive and finite")
    if len(freqs) < 1:
        raise ValueError("multiband compressor: at least one crossover frequency is required")
    if len(freqs) + 1 > MAX_BANDS:
        raise ValueError("multiband compressor: too many bands")
    if order < MIN_ORDER or order > MAX_ORDER or order % 2:
        raise ValueError("multiband compressor: order must be even and in [2, 24]")
    for i, f in enumerate(freqs):
        if not _finite(f) or f < MIN_FREQ or f >= fs / 2 or (i > 0 and f <= freqs[i - 1]):
            raise ValueError(f"multiband compressor: crossover frequency {i} rejected: {f}")


# BandConfig fields in applyBandConfig's order (:563-658) -> (setter, the "keep" value besides None)
BAND_CONFIG = (("ThresholdDB", "SetBandThreshold", None), ("Ratio", "SetBandRatio", 0), ("KneeDB", "SetBandKnee", None),
               ("AttackMs", "SetBandAttack", 0), ("ReleaseMs", "SetBandRelease", 0),
               ("MakeupGainDB", "SetBandMakeupGain", None), ("AutoMakeup", "SetBandAutoMakeup", None),
               ("Topology", "SetBandTopology", None), ("DetectorMode", "SetBandDetectorMode", None),
               ("FeedbackRatioScale", "SetBandFeedbackRatioScale", None), ("RMSWindowMs", "SetBandRMSWindow", None),
               ("SidechainLowCutHz", "SetBandSidechainLowCut", None),
               ("SidechainHighCutHz", "SetBandSidechainHighCut", None))


class MultibandCompressor:
    def __init__(self, freqs, order, fs, configs=None):
        freqs = [float(f) for f in freqs]
        if configs is not None and len(configs) != len(freqs) + 1:  # :131-135
            raise ValueError("multiband compressor: wrong number of band configs")
        validate_multiband(freqs, order, fs)
        self.xover = MultiBand(freqs, order, fs)
        self.compressors = [O.Compressor(fs) for _ in range(self.xover.bands)]
        self.freqs, self.order, self.fs = freqs, order, fs
        for i, cfg in enumerate(configs or ()):
            self.SetBandConfig(i, cfg)

    def NumBands(self):
        return len(self.compressors)

    def CrossoverFreqs(self):
        return list(self.freqs)

    def CrossoverOrder(self):
        return self.order

    def SampleRate(self):
        return self.fs

    def Band(self, i):
        """The band's config as the reference's getters report it."""
        return self.compressors[i].config()

    def _check(self, band):  # checkBand :555-561
        if band < 0 or band >= len(self.compressors):
            raise IndexError(f"multiband compressor: band index {band} out of range")

    def _set(self, band, **kv):
        self._check(band)
        cfg = self.compressors[band].config()
        cfg.update(kv)
        validate_compressor(cfg)  # rejected: nothing has changed
        self.compressors[band].reconfigure(**kv)

    def SetBandThreshold(self, band, db):
        self._set(band, threshold_db=float(db))

    def SetBandRatio(self, band, ratio):
        self._set(band, ratio=float(ratio))

    def SetBandKnee(self, band, db):
        self._set(band, knee_db=float(db))

    def SetBandAttack(self, band, ms):
        self._set(band, attack_ms=float(ms))

    def SetBandRelease(self, band, ms):
        self._set(band, release_ms=float(ms))

    def SetBandMakeupGain(self, band, db):  # :242-249
        self._set(band, makeup_db=float(db), auto_makeup=0)

    def SetBandAutoMakeup(self, band, on):
        self._set(band, auto_makeup=int(bool(on)))

    def SetBandTopology(self, band, topology):
        self._set(band, topology=int(topology))

    def SetBandDetectorMode(self, band, mode):
        self._set(band, detector_mode=int(mode))

    def SetBandFeedbackRatioScale(self, band, on):
        self._set(band, feedback_ratio_scale=int(bool(on)))

    def SetBandRMSWindow(self, band, ms):
        self._set(band, rms_window_ms=float(ms))

    def SetBandSidechainLowCut(self, band, hz):
        self._set(band, sidechain_low_cut_hz=float(hz))

    def SetBandSidechainHighCut(self, band, hz):
        self._set(band, sidechain_high_cut_hz=float(hz))

    def SetBandConfig(self, band, cfg):  # :322-329, :563-658
        self._check(band)
        for key, setter, keep in BAND_CONFIG:
            v = cfg.get(key)
            if v is None or (keep is not None and v == keep):
                continue
            getattr(self, setter)(band, v)

    def _all(self, setter, v):  # :331-437
        for b in range(self.NumBands()):
            getattr(self, setter)(b, v)

    def SetAllBandsThreshold(self, db):
        self._all("SetBandThreshold", db)

    def SetAllBandsRatio(self, ratio):
        self._all("SetBandRatio", ratio)

    def SetAllBandsKnee(self, db):
        self._all("SetBandKnee", db)

    def SetAllBandsAttack(self, ms):
        self._all("SetBandAttack", ms)

    def SetAllBandsRelease(self, ms):
        self._all("SetBandRelease", ms)

    def SetAllBandsTopology(self, topology):
        self._all("SetBandTopology", topology)

    def SetAllBandsDetectorMode(self, mode):
        self._all("SetBandDetectorMode", mode)

    def SetAllBandsFeedbackRatioScale(self, on):
        self._all("SetBandFeedbackRatioScale", on)

    def SetAllBandsRMSWindow(self, ms):
        self._all("SetBandRMSWindow", ms)

    def ProcessInPlaceMulti(self, x):  # :507-523 -> [bands][n]
        x = np.asarray(x, dtype=np.float64)
        if x.size == 0:
            return np.zeros((self.NumBands(), 0))
        bands = self.xover.ProcessBlock(x)
        return np.array([c.process_in_place(b) for c, b in zip(self.compressors, bands)])

    def ProcessInPlace(self, x):  # :468-489: copy band 0, add the others in order
        x = np.asarray(x, dtype=np.float64)
        if x.size == 0:
            return x.copy()
        bands = self.ProcessInPlaceMulti(x)
        out = bands[0].copy()
        for b in bands[1:]:
            out += b
        return out

    def ProcessSample(self, v):  # :443-452: sum := 0.0; sum += band
        bands = self.xover.ProcessSample(v)
        total = 0.0
        for c, b in zip(self.compressors, bands):
            total += c.process_sample(float(b))
        return total

    def ProcessSampleMulti(self, v):  # :457-464
        bands = self.xover.ProcessSample(v)
        return np.array([c.process_sample(float(b)) for c, b in zip(self.compressors, bands)])

    def Reset(self):  # :528-534
        self.xover.Reset()
        for c in self.compressors:
            c.reset()

    def GetMetrics(self):  # :537-544 -> per band (InputPeak, OutputPeak, GainReduction)
        return [c.metrics() for c in self.compressors]
