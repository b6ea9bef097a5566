"""effects.Distortion (dsp/effects/distortion.go) and effects.BitCrusher
(bit_crusher.go) restated for the tests, with the three node runtimes that
configure them (distortion, dist-cheb, bitcrusher; effectchain/
runtime_modulation.go:71-171, normalize.go:102-161, configure.go:94-215).

One instance is one channel of the reference.  The arithmetic is numpy
float64, one rounded operation per written operation and in the written order
(numpy fuses nothing), so an instance may also be handed a vector and then is
that many independent channels at once: `process_many` walks time and takes a
column [channels] per step.  Branches are np.where over both sides, so a NaN
takes the side the reference's comparison gives it (the false one).
"""
from __future__ import annotations

import math

import numpy as np

MODES = ("softclip", "hardclip", "tanh", "waveshaper1", "waveshaper2", "waveshaper3", "waveshaper4", "waveshaper5",
         "waveshaper6", "waveshaper7", "waveshaper8", "saturate", "saturate2", "softsat", "chebyshev")  # :36-52
EXACT, POLYNOMIAL = 0, 1            # :57-60
ALL, ODD, EVEN = 0, 1, 2            # :65-69
DC_BYPASS_POLE = 0.995              # :30
CHEBYSHEV = MODES.index("chebyshev")

# modes made of + - * / and comparisons only (bit-exact on any IEEE machine) ...
ALGEBRAIC = ("softclip", "hardclip", "waveshaper1", "waveshaper2", "waveshaper3", "waveshaper4", "waveshaper6",
             "saturate", "saturate2", "chebyshev")
# ... these too with the polynomial approximation; exact, they call tanh, atan or exp, as waveshaper5 and 8 do
POLY_ALGEBRAIC = ("tanh", "waveshaper7", "softsat")
TRANSCENDENTAL = ("tanh", "waveshaper5", "waveshaper7", "waveshaper8", "softsat")


class Invalid(ValueError):
    """A setter's or constructor's error."""


def _f(x):
    return np.asarray(x, dtype=np.float64)


def is_finite(x):  # :799-801
    return ~np.isnan(x) & ~np.isinf(x)


def clamp(x, lo, hi):  # :783-793: two comparisons, a NaN passes
    return np.where(x < lo, lo, np.where(x > hi, hi, x))


def clamp_unit(x):  # :795-797
    return clamp(x, -1.0, 1.0)


def fast_tanh(x):  # fastTanhApprox :769-781
    x2 = x * x
    return np.where(x > 3, 1.0, np.where(x < -3, -1.0, clamp_unit(x * (27 + x2) / (27 + 9 * x2))))


def _bad(v, lo, hi):
    return v < lo or v > hi or math.isnan(v) or math.isinf(v)


def validate_parity(order, harmonic):  # validateChebyshevParity :750-767
    if harmonic == ODD and order % 2 == 0:
        raise Invalid(f"chebyshev odd harmonic mode requires odd order: {order}")
    if harmonic == EVEN and order % 2 != 0:
        raise Invalid(f"chebyshev even harmonic mode requires even order: {order}")
    if harmonic not in (ALL, ODD, EVEN):
        raise Invalid(f"chebyshev harmonic mode is invalid: {harmonic}")


class Distortion:
    """NewDistortion(sampleRate, options...) :320-362 with the options as keywords."""

    def __init__(self, sample_rate=48000.0, mode=0, approx=EXACT, drive=1.0, mix=1.0, output_level=1.0, clip_level=1.0,
                 shape=0.5, bias=0.0, cheb_order=3, cheb_harmonic=ALL, cheb_invert=False, cheb_gain=1.0,
                 cheb_dc_bypass=False, cheb_weights=()):
        if sample_rate <= 0 or math.isnan(sample_rate) or math.isinf(sample_rate):
            raise Invalid("distortion sample rate must be > 0 and finite")
        self.sampleRate = float(sample_rate)
        self.mode, self.approxMode = 0, EXACT
        self.chebyshevOrder, self.chebyshevMode = 3, ALL
        self.chebyshevWeights = [0.0] * 16
        self.dcPrevIn = self.dcPrevOut = 0.0
        self.atanScale = None  # atan(1 + 4 shape) from elsewhere (the GPU host's C library); None: math.atan
        # the options check as the setters do; the parity rule is checked once at the end (:356)
        self.chebyshevOrder, self.chebyshevMode = int(cheb_order), int(cheb_harmonic)
        if not 1 <= self.chebyshevOrder <= 16:
            raise Invalid("chebyshev order must be in [1, 16]")
        validate_parity(self.chebyshevOrder, self.chebyshevMode)
        self.SetMode(mode), self.SetApproxMode(approx), self.SetDrive(drive), self.SetMix(mix)
        self.SetOutputLevel(output_level), self.SetClipLevel(clip_level), self.SetShape(shape), self.SetBias(bias)
        self.SetChebyshevInvert(cheb_invert), self.SetChebyshevGainLevel(cheb_gain)
        self.SetChebyshevDCBypass(cheb_dc_bypass), self.SetChebyshevWeights(cheb_weights)

    # ---- setters :364-529.  A rejected value changes nothing here (the reference's order and harmonic
    # setters keep it; the GPU handles do not, and neither does this restatement)
    def SetSampleRate(self, v):
        if v <= 0 or math.isnan(v) or math.isinf(v):
            raise Invalid("distortion sample rate must be > 0 and finite")
        self.sampleRate = float(v)

    def SetMode(self, v):
        if v != int(v) or not 0 <= v < len(MODES):
            raise Invalid(f"distortion mode is invalid: {v}")
        self.mode = int(v)

    def SetApproxMode(self, v):
        if v not in (EXACT, POLYNOMIAL):
            raise Invalid(f"distortion approximation mode is invalid: {v}")
        self.approxMode = int(v)

    def SetDrive(self, v):
        if _bad(v, 0.01, 20.0):
            raise Invalid("distortion drive must be in [0.01, 20]")
        self.drive = float(v)

    def SetMix(self, v):
        if _bad(v, 0.0, 1.0):
            raise Invalid("distortion mix must be in [0, 1]")
        self.mix = float(v)

    def SetOutputLevel(self, v):
        if _bad(v, 0.0, 4.0):
            raise Invalid("distortion output level must be in [0, 4]")
        self.outputLevel = float(v)

    def SetClipLevel(self, v):
        if _bad(v, 0.05, 1.0):
            raise Invalid("distortion clip level must be in [0.05, 1]")
        self.clipLevel = float(v)

    def SetShape(self, v):
        if _bad(v, 0.0, 1.0):
            raise Invalid("distortion shape must be in [0, 1]")
        self.shape = float(v)

    def SetBias(self, v):
        if _bad(v, -1.0, 1.0):
            raise Invalid("distortion bias must be in [-1, 1]")
        self.bias = float(v)

    def SetChebyshevOrder(self, v):
        if v != int(v) or not 1 <= v <= 16:
            raise Invalid("chebyshev order must be in [1, 16]")
        validate_parity(int(v), self.chebyshevMode)
        self.chebyshevOrder = int(v)

    def SetChebyshevHarmonicMode(self, v):
        if v not in (ALL, ODD, EVEN):
            raise Invalid(f"chebyshev harmonic mode is invalid: {v}")
        validate_parity(self.chebyshevOrder, int(v))
        self.chebyshevMode = int(v)

    def SetChebyshevInvert(self, on):
        self.chebyshevInvert = bool(on)

    def SetChebyshevGainLevel(self, v):
        if _bad(v, 0.0, 4.0):
            raise Invalid("chebyshev gain level must be in [0, 4]")
        self.chebyshevGain = float(v)

    def SetChebyshevDCBypass(self, on):
        self.chebyshevDCBypass = bool(on)

    def SetChebyshevWeights(self, weights):  # :514-529
        w = [float(x) for x in weights]
        if len(w) > 16:
            raise Invalid("chebyshev weights length must be <= 16")
        if any(math.isnan(x) or math.isinf(x) for x in w):
            raise Invalid("chebyshev weights must be finite")
        self.chebyshevWeights = w + [0.0] * (16 - len(w))

    def Reset(self):  # :532-535
        self.dcPrevIn = self.dcPrevOut = 0.0

    def has_weights(self):  # :688-695: the first `order` slots only
        return any(w != 0 for w in self.chebyshevWeights[:self.chebyshevOrder])

    # ---- shapeSample :608-645
    def softClip(self, x):  # :659-666
        ax = np.abs(x)
        return np.where(ax < 1, 1.5 * (x - (x * x * x) / 3), np.copysign(1.0, x))

    def hardClip(self, x):  # :647-657
        c = self.clipLevel
        x = np.where(x > c, c, x)
        x = np.where(x < -c, -c, x)
        return x / c

    def tanhShape(self, x):  # :668-674
        return fast_tanh(x) if self.approxMode == POLYNOMIAL else np.tanh(x)

    def softSat(self, x):  # :676-682
        if self.approxMode == POLYNOMIAL:
            return clamp_unit(x * (27 + x * x) / (27 + 9 * x * x))
        # (2 / math.Pi) and (math.Pi / 2) are exact constant expressions in Go, rounded once
        return clamp_unit(0.6366197723675814 * np.arctan(1.5707963267948966 * x))

    def chebyshevShape(self, x):  # :684-728
        x = clamp(x, -1.0, 1.0)
        w, has = self.chebyshevWeights, self.has_weights()
        t0, t1 = np.ones_like(x), x
        weighted = w[0] * t1 if has else np.zeros_like(x)
        tn = t1
        for n in range(2, self.chebyshevOrder + 1):
            tn = 2 * x * t1 - t0
            if has:
                weighted = weighted + w[n - 1] * tn
            t0, t1 = t1, tn
        out = (weighted if has else tn) * self.chebyshevGain
        if self.chebyshevInvert:
            out = -out
        return clamp_unit(out)

    def shapeSample(self, x):
        x = _f(x)
        s, m = self.shape, MODES[self.mode]
        with np.errstate(all="ignore"):
            if m == "softclip":
                return self.softClip(x)
            if m == "hardclip":
                return self.hardClip(x)
            if m == "tanh":
                return self.tanhShape(x)
            if m == "waveshaper1":
                return clamp_unit(x / (1 + s * np.abs(x)))
            if m == "waveshaper2":
                return clamp_unit(((1 + s) * x) / (1 + s * np.abs(x)))
            if m == "waveshaper3":
                return clamp_unit(x - s * x * x * x / 3)
            if m == "waveshaper4":
                return clamp_unit((3 * x) / (2 + np.abs(2 * x)))
            if m == "waveshaper5":
                scale = 1 + 4 * s
                return clamp_unit(np.arctan(x * scale) / (self.atanScale or math.atan(scale)))
            if m == "waveshaper6":
                return clamp_unit((1 + s) * x / (1 + s * x * x))
            if m == "waveshaper7":
                return self.tanhShape(x * (1 + 6 * s))
            if m == "waveshaper8":
                a = 1 + 6 * s
                return clamp_unit(np.copysign(1 - np.exp(-np.abs(x) * a), x))
            if m == "saturate":
                return clamp_unit(x / (1 + np.abs(x)))
            if m == "saturate2":
                return self.softClip(x * (1 + 2 * s))
            if m == "softsat":
                return self.softSat(x)
            return self.chebyshevShape(x)

    def curve(self, x):
        """shapeSample(x) * outputLevel with the finite check, without the DC bypass: what ad_distortion_curve plots."""
        with np.errstate(all="ignore"):
            wet = self.shapeSample(x) * self.outputLevel
            return np.where(is_finite(wet), wet, 0.0)

    def dc_active(self):
        return self.mode == CHEBYSHEV and self.chebyshevDCBypass

    def ProcessSample(self, inp, wet=None):  # :538-554; `wet`: shapeSample(x) * outputLevel from elsewhere (the device)
        inp = _f(inp)
        with np.errstate(all="ignore"):
            if wet is None:
                x = (inp + self.bias) * self.drive
                wet = self.shapeSample(x) * self.outputLevel
            if self.dc_active():  # dcBypass :730-736
                y = wet - self.dcPrevIn + DC_BYPASS_POLE * self.dcPrevOut
                self.dcPrevIn, self.dcPrevOut = wet, y
                wet = y
            wet = np.where(is_finite(wet), wet, 0.0)
            return inp * (1 - self.mix) + wet * self.mix

    def argument(self, inp):
        """x = (input + bias) * drive :540."""
        with np.errstate(all="ignore"):
            return (_f(inp) + self.bias) * self.drive

    def process_many(self, x, curve=None):
        """ProcessInPlace :557-561 of every row of x [channels][n], each its own
        instance (the DC states become vectors).  `curve` [channels][n]: the
        device's shapeSample(x) * outputLevel for these inputs."""
        x = _f(x)
        if not self.dc_active():
            return self.ProcessSample(x, curve)
        out = np.empty_like(x)
        self.dcPrevIn = np.broadcast_to(_f(self.dcPrevIn), x.shape[:1]).copy()
        self.dcPrevOut = np.broadcast_to(_f(self.dcPrevOut), x.shape[:1]).copy()
        for t in range(x.shape[1]):
            out[:, t] = self.ProcessSample(x[:, t], None if curve is None else curve[:, t])
        return out


def go_round(v):
    """math.Round: halves away from zero, the sign of zero kept (v - trunc(v) is exact)."""
    v = _f(v)
    with np.errstate(all="ignore"):
        t = np.trunc(v)
        return np.where(np.abs(v - t) >= 0.5, t + np.copysign(1.0, v), t)


class BitCrusher:
    """NewBitCrusher(sampleRate, options...) :108-135 with the options as keywords."""

    def __init__(self, sample_rate=48000.0, bit_depth=8.0, downsample=1, mix=1.0):
        self.SetSampleRate(sample_rate)
        self.SetBitDepth(bit_depth), self.SetDownsample(downsample), self.SetMix(mix)
        self.holdCounter, self.holdValue = 0, 0.0

    def SetSampleRate(self, v):  # :138-146
        if v <= 0 or math.isnan(v) or math.isinf(v):
            raise Invalid("bit crusher sample rate must be > 0 and finite")
        self.sampleRate = float(v)

    def SetBitDepth(self, v):  # :149-160
        if _bad(v, 1.0, 32.0):
            raise Invalid("bit crusher bit depth must be in [1, 32]")
        self.bitDepth = float(v)
        self.quantLevels = 2.0 ** (self.bitDepth - 1)  # updateQuantLevels :222-224

    def SetDownsample(self, v):  # :163-172
        if v != int(v) or not 1 <= v <= 256:
            raise Invalid("bit crusher downsample factor must be in [1, 256]")
        self.downsample = int(v)

    def SetMix(self, v):  # :175-183
        if _bad(v, 0.0, 1.0):
            raise Invalid("bit crusher mix must be in [0, 1]")
        self.mix = float(v)

    def Reset(self):  # :186-189
        self.holdCounter, self.holdValue = 0, 0.0

    def quantize(self, sample):  # :228-230
        with np.errstate(all="ignore"):
            return go_round(_f(sample) * self.quantLevels) / self.quantLevels

    def ProcessSample(self, inp):  # :192-201
        inp = _f(inp)
        self.holdCounter += 1
        if self.holdCounter >= self.downsample:
            self.holdCounter = 0
            self.holdValue = self.quantize(inp)
        with np.errstate(all="ignore"):
            return inp * (1 - self.mix) + self.holdValue * self.mix

    def process_many(self, x):
        """ProcessInPlace :204-208 of every row of x [channels][n]: one counter, a hold value per row."""
        x = _f(x)
        out = np.empty_like(x)
        self.holdValue = np.broadcast_to(_f(self.holdValue), x.shape[:1]).copy()
        for t in range(x.shape[1]):
            out[:, t] = self.ProcessSample(x[:, t])
        return out


# ---- what the GPU host computes instead of counting ------------------------
def first_update(downsample, c0):
    """The first sample of a call at which holdValue is updated, the counter being c0 before it."""
    return max(downsample - 1 - c0, 0)


def counter_after(downsample, c0, n):
    """holdCounter after a call of n samples."""
    t0 = first_update(downsample, c0)
    return (n - 1 - t0) % downsample if n > t0 else c0 + n


# ---- the node runtimes ------------------------------------------------------
def core_clamp(v, lo, hi):  # core.Clamp
    return lo if v < lo else (hi if v > hi else v)


def get_num(num, key, default):  # Params.GetNum params.go:15-27
    v = num.get(key)
    if v is None or math.isnan(v) or math.isinf(v):
        return default
    return v


def round_int(v):  # int(math.Round(v))
    return int(go_round(v))


def normalize_mode(raw):  # normalizeDistortionMode normalize.go:102-137
    return MODES.index(raw) if raw in MODES else 0


def normalize_approx(raw):  # normalize.go:139-148
    return POLYNOMIAL if raw == "polynomial" else EXACT


def normalize_harmonic(raw):  # normalize.go:150-161
    return {"odd": ODD, "even": EVEN}.get(raw, ALL)


def adjust_order(order, harmonic):  # configureDistortion configure.go:131-153
    if harmonic == ODD and order % 2 == 0:
        order += 1
    if harmonic == EVEN and order % 2 != 0:
        order += 1
    if order > 16:
        order = 16
    if harmonic == ODD and order % 2 == 0:
        order -= 1
    if harmonic == EVEN and order % 2 != 0:
        order -= 1
    if order < 1:
        order = 1
    return order


def distortion_node(num, strs, fs):
    """distortionRuntime.Configure runtime_modulation.go:95-116."""
    return Distortion(fs, mode=normalize_mode(strs.get("mode")), approx=normalize_approx(strs.get("approx")),
                      drive=core_clamp(get_num(num, "drive", 1.8), 0.01, 20), mix=core_clamp(get_num(num, "mix", 1.0), 0, 1),
                      output_level=core_clamp(get_num(num, "output", 1.0), 0, 4),
                      clip_level=core_clamp(get_num(num, "clip", 1.0), 0.05, 1),
                      shape=core_clamp(get_num(num, "shape", 0.5), 0, 1), bias=core_clamp(get_num(num, "bias", 0), -1, 1),
                      cheb_order=adjust_order(3, ALL), cheb_harmonic=ALL, cheb_invert=False, cheb_gain=1.0,
                      cheb_dc_bypass=False)


def dist_cheb_node(num, strs, fs):
    """distChebRuntime.Configure runtime_modulation.go:126-167."""
    harmonic = normalize_harmonic(strs.get("harmonic"))
    order = min(max(round_int(get_num(num, "order", 3)), 1), 16)
    return Distortion(fs, mode=CHEBYSHEV, approx=normalize_approx(strs.get("approx")),
                      drive=core_clamp(get_num(num, "drive", 1.0), 0.01, 20), mix=core_clamp(get_num(num, "mix", 1.0), 0, 1),
                      output_level=core_clamp(get_num(num, "output", 1.0), 0, 4), clip_level=1.0, shape=0.5, bias=0.0,
                      cheb_order=adjust_order(order, harmonic), cheb_harmonic=harmonic,
                      cheb_invert=get_num(num, "invert", 0) >= 0.5, cheb_gain=core_clamp(get_num(num, "gain", 1.0), 0, 4),
                      cheb_dc_bypass=get_num(num, "dcBypass", 0) >= 0.5,
                      cheb_weights=[get_num(num, f"w{k + 1}", 0) for k in range(16)])


def bitcrusher_node(num, strs, fs):
    """bitCrusherRuntime.Configure runtime_modulation.go:75-85."""
    return BitCrusher(fs, bit_depth=core_clamp(get_num(num, "bitDepth", 8), 1, 32),
                      downsample=min(max(round_int(get_num(num, "downsample", 4)), 1), 256),
                      mix=core_clamp(get_num(num, "mix", 1), 0, 1))


NODES = {"distortion": distortion_node, "dist-cheb": dist_cheb_node, "bitcrusher": bitcrusher_node}

# ---- config fields of the GPU structures, from an instance -------------------
DIST_FIELDS = {"sample_rate": "sampleRate", "drive": "drive", "mix": "mix", "output_level": "outputLevel",
               "clip_level": "clipLevel", "shape": "shape", "bias": "bias", "cheb_gain": "chebyshevGain",
               "mode": "mode", "approx": "approxMode", "cheb_order": "chebyshevOrder", "cheb_harmonic": "chebyshevMode",
               "cheb_invert": "chebyshevInvert", "cheb_dc_bypass": "chebyshevDCBypass"}
CRUSH_FIELDS = {"sample_rate": "sampleRate", "bit_depth": "bitDepth", "mix": "mix", "downsample": "downsample"}


def config_of(ref) -> dict:
    """The instance's configuration under the GPU structures' field names."""
    if isinstance(ref, Distortion):
        d = {k: getattr(ref, v) for k, v in DIST_FIELDS.items()}
        d["cheb_invert"], d["cheb_dc_bypass"] = int(d["cheb_invert"]), int(d["cheb_dc_bypass"])
        d["cheb_weights"] = list(ref.chebyshevWeights)
        return d
    return {k: getattr(ref, v) for k, v in CRUSH_FIELDS.items()}


# ---- validation tables: (field of the GPU config, value) ----------------------
# every range edge is accepted, the value just outside it and the non-finite ones are refused
DIST_EDGES = {"sample_rate": (5e-324, 1.7976931348623157e308), "drive": (0.01, 20.0), "mix": (0.0, 1.0),
              "output_level": (0.0, 4.0), "clip_level": (0.05, 1.0), "shape": (0.0, 1.0), "bias": (-1.0, 1.0),
              "cheb_gain": (0.0, 4.0)}
CRUSH_EDGES = {"sample_rate": (5e-324, 1.7976931348623157e308), "bit_depth": (1.0, 32.0), "mix": (0.0, 1.0)}
NONFINITE = (float("nan"), float("inf"), float("-inf"))


def _outside(lo, hi):
    out = [math.nextafter(lo, -math.inf)]
    if hi < 1.7e308:
        out.append(math.nextafter(hi, math.inf))
    return out


def accepted(kind):
    edges = DIST_EDGES if kind == "distortion" else CRUSH_EDGES
    out = [(f, v) for f, (lo, hi) in edges.items() for v in (lo, hi)]
    if kind == "distortion":
        out += [("mode", 0), ("mode", 14), ("approx", 0), ("approx", 1), ("cheb_order", 1), ("cheb_order", 16),
                ("cheb_harmonic", 0), ("cheb_harmonic", 1), ("cheb_invert", 1), ("cheb_dc_bypass", 1)]
    else:
        out += [("downsample", 1), ("downsample", 256)]
    return out


def rejected(kind):
    edges = DIST_EDGES if kind == "distortion" else CRUSH_EDGES
    out = [(f, v) for f, (lo, hi) in edges.items() for v in _outside(lo, hi) + list(NONFINITE)]
    out += [("sample_rate", 0.0), ("sample_rate", -1.0)]
    if kind == "distortion":  # TestDistortionValidation: drive 100, mode 999, even harmonic with the default order 3
        out += [("drive", 100.0), ("mode", 999), ("mode", -1), ("mode", 15), ("approx", 2), ("approx", -1), ("cheb_order", 0),
                ("cheb_order", 17), ("cheb_harmonic", 3), ("cheb_harmonic", -1), ("cheb_harmonic", EVEN)]
    else:  # TestBitCrusherValidation :222-289, TestBitCrusherSetterValidation :291-336
        out += [("bit_depth", 0.5), ("bit_depth", 33.0), ("downsample", 0), ("downsample", -1), ("downsample", 257),
                ("mix", -0.1), ("mix", 1.1)]
    return out


# ---- one setter by the GPU config's field name, on a GPU handle or on an instance here ----
PARAMS = {"distortion": ("sample_rate", "drive", "mix", "output_level", "clip_level", "shape", "bias", "cheb_gain", "mode",
                         "approx", "cheb_order", "cheb_harmonic", "cheb_invert", "cheb_dc_bypass"),  # AD_DISTORTION_*
          "bitcrusher": ("sample_rate", "bit_depth", "mix", "downsample")}                           # AD_BITCRUSHER_*
SETTERS = {"sample_rate": "SetSampleRate", "drive": "SetDrive", "mix": "SetMix", "output_level": "SetOutputLevel",
           "clip_level": "SetClipLevel", "shape": "SetShape", "bias": "SetBias", "cheb_gain": "SetChebyshevGainLevel",
           "mode": "SetMode", "approx": "SetApproxMode", "cheb_order": "SetChebyshevOrder",
           "cheb_harmonic": "SetChebyshevHarmonicMode", "cheb_invert": "SetChebyshevInvert",
           "cheb_dc_bypass": "SetChebyshevDCBypass", "bit_depth": "SetBitDepth", "downsample": "SetDownsample"}


def set_on(obj, field, value):
    """`field` set to `value` through the named setter; a GPU handle takes the raw parameter, so a value the
    Python wrapper would coerce still reaches the library's check."""
    if isinstance(obj, (Distortion, BitCrusher)):
        return getattr(obj, SETTERS[field])(value)
    return obj._set(PARAMS[obj._kind].index(field), value)
