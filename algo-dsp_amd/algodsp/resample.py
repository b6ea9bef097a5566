"""dsp/resample: rational polyphase FIR sample-rate conversion
(dsp/resample/resample.go, resample_design.go).

The designer, the ratio approximation and every validation run on the host and
need no device; Process runs the HIP kernel behind ad_resampler_* for
`channels` independent streams at once.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import math
from collections import namedtuple

import numpy as np

from ._lib import check, f64, lib, ptr

# Quality (resample.go:16-25)
QualityFast = 0
QualityBalanced = 1
QualityBest = 2

Profile = namedtuple("Profile", "TapsPerPhase CutoffScale KaiserBeta NominalStopbandDB")


class ErrInvalidRatio(ValueError):  # resample.go:10
    def __init__(self):
        super().__init__("resample: invalid ratio")


class ErrInvalidRate(ValueError):  # resample.go:12
    def __init__(self):
        super().__init__("resample: invalid sample rate")


def QualityProfile(q: int) -> Profile:
    """resample.go:36-45"""
    if q == QualityFast:
        return Profile(16, 0.88, 5.0, 55.0)
    if q == QualityBest:
        return Profile(64, 0.96, 9.0, 90.0)
    return Profile(32, 0.92, 7.5, 75.0)


def _gcd(a: int, b: int) -> int:  # resample_design.go:116-134
    return math.gcd(a, b) or 1


def _i0(x: np.ndarray) -> np.ndarray:
    """Power series of the modified Bessel function (resample_design.go:157-173),
    every element with its own stopping point."""
    x = np.asarray(x, dtype=np.float64)
    s = np.ones_like(x)
    term = np.ones_like(x)
    x2 = (x * x) / 4
    live = np.ones(x.shape, dtype=bool)
    for k in range(1, 64):
        term = np.where(live, term * (x2 / float(k * k)), term)
        s = np.where(live, s + term, s)
        live &= ~(term < 1e-16 * s)
        if not live.any():
            break
    return s


def _kaiser(i: np.ndarray, n: int, beta: float) -> np.ndarray:  # resample_design.go:146-155
    if n <= 1 or beta == 0:
        return np.ones(i.shape)
    t = 2 * i.astype(np.float64) / float(n - 1) - 1
    a = np.sqrt(np.maximum(0.0, 1 - t * t))
    return _i0(beta * a) / _i0(np.float64(beta))


def _sinc(x: np.ndarray) -> np.ndarray:  # resample_design.go:136-144
    small = np.abs(x) < 1e-12
    pix = math.pi * np.where(small, 1.0, x)
    return np.where(small, 1.0, np.sin(pix) / pix)


def design_polyphase_fir(up: int, down: int, taps_per_phase: int, cutoff_scale: float,
                         kaiser_beta: float) -> np.ndarray:
    """designPolyphaseFIR (resample_design.go:9-50): the windowed-sinc prototype
    of taps_per_phase * up taps, scaled to sum to `up`.  Phase p is
    taps[p::up].  Host only."""
    if up <= 0 or down <= 0:
        raise ErrInvalidRatio()
    if taps_per_phase <= 0:
        raise ValueError("resample: taps per phase must be > 0")
    if not (0 < cutoff_scale <= 1):
        raise ValueError("resample: cutoff scale must be in (0,1]")
    n_taps = taps_per_phase * up
    fc = (0.5 / float(max(up, down))) * cutoff_scale
    if fc <= 0 or fc >= 0.5:
        raise ValueError(f"resample: invalid cutoff {fc:.6f}")
    center = 0.5 * float(n_taps - 1)
    n = np.arange(n_taps)
    t = n.astype(np.float64) - center
    taps = 2 * fc * _sinc(2 * fc * t) * _kaiser(n, n_taps, float(kaiser_beta))
    total = 0.0
    for v in taps:  # the reference's running sum, in order
        total += float(v)
    if total == 0:
        raise ValueError("resample: designed zero-sum filter")
    taps *= float(up) / total
    return taps


def approximate_ratio(v: float, max_den: int = 4096):
    """approximateRatio (resample_design.go:71-114): continued fraction of v,
    stopped before the denominator passes max_den."""
    if max_den <= 0:
        max_den = 4096
    if not (v > 0) or math.isinf(v):
        return 1, 1
    a0 = math.floor(v)
    p0, q0 = 1.0, 0.0
    p1, q1 = float(a0), 1.0
    x = v
    while True:
        frac = x - math.floor(x)
        if frac == 0:
            break
        x = 1 / frac
        a = float(math.floor(x))
        p2 = a * p1 + p0
        q2 = a * q1 + q0
        if q2 > float(max_den):
            break
        p0, q0 = p1, q1
        p1, q1 = p2, q2
    num = int(round(p1))
    den = int(round(q1))
    if den <= 0:
        return 1, 1
    g = _gcd(num, den)
    return num // g, den // g


def _config(quality, taps_per_phase, cutoff_scale, kaiser_beta, max_denominator):
    """The options' acceptance rules and finalized() (resample.go:58-132): an
    option value outside its range is ignored, and what is still unset takes
    the quality profile's value."""
    q = QualityBalanced if quality is None else int(quality)
    p = QualityProfile(q)
    T = int(taps_per_phase) if taps_per_phase is not None and taps_per_phase > 0 else p.TapsPerPhase
    cs = float(cutoff_scale) if cutoff_scale is not None and 0 < cutoff_scale <= 1 else p.CutoffScale
    kb = float(kaiser_beta) if kaiser_beta is not None and kaiser_beta > 0 else p.KaiserBeta
    md = int(max_denominator) if max_denominator is not None and max_denominator > 0 else 4096
    return q, T, cs, kb, md


class Resampler:
    """resample.Resampler over `channels` streams that share the ratio, the
    prototype and the scalar state.  `taps` replaces the designed prototype
    (its length must be a multiple of the reduced up)."""

    def __init__(self, up: int, down: int, *, quality=None, taps_per_phase=None, cutoff_scale=None,
                 kaiser_beta=None, max_denominator=None, channels: int = 1, device: int = 0, taps=None):
        self._h = C.c_void_p()
        up, down = int(up), int(down)
        if up <= 0 or down <= 0:
            raise ErrInvalidRatio()
        g = _gcd(up, down)
        up //= g
        down //= g
        q, T, cs, kb, _ = _config(quality, taps_per_phase, cutoff_scale, kaiser_beta, max_denominator)
        self.quality = q
        self.channels = int(channels)
        self.device = int(device)
        self.taps = design_polyphase_fir(up, down, T, cs, kb) if taps is None else f64(taps).reshape(-1).copy()
        check(lib().ad_resampler_create(up, down, ptr(self.taps), self.taps.size, self.channels, self.device,
                                        C.byref(self._h)))

    # -- reference API ---------------------------------------------------
    def Process(self, x) -> np.ndarray:
        """Process (resample.go:249-292): x is 1-D for one channel (a 1-D
        result), else [channels][n] -> [channels][n_out]."""
        a = f64(x)
        one_d = a.ndim == 1
        if one_d:
            if self.channels != 1:
                raise ValueError("1-D input needs a one-channel resampler")
            a = a.reshape(1, -1)
        if a.ndim != 2 or a.shape[0] != self.channels:
            raise ValueError(f"input must be [{self.channels}][n]")
        n_in = a.shape[1]
        cap = self.PredictOutputLen(n_in)
        out = np.empty((self.channels, cap), dtype=np.float64)
        n_out = C.c_int64(0)
        check(lib().ad_resampler_process(self._h, ptr(a), n_in, ptr(out), cap, C.byref(n_out)))
        assert n_out.value == cap
        return out[0] if one_d else out

    def process_device(self, d_in: int, in_stride: int, n_in: int, d_out: int, out_stride: int, out_cap: int,
                       stream: int | None = None) -> int:
        """ad_resampler_process_device on device pointers; returns n_out."""
        n_out = C.c_int64(0)
        check(lib().ad_resampler_process_device(self._h, C.c_void_p(d_in), int(in_stride), int(n_in),
                                                C.c_void_p(d_out), int(out_stride), int(out_cap), C.byref(n_out),
                                                C.c_void_p(stream or 0)))
        return n_out.value

    def PredictOutputLen(self, n_in: int) -> int:  # :295-313
        n = C.c_int64(0)
        check(lib().ad_resampler_predict_output_len(self._h, int(n_in), C.byref(n)))
        return n.value

    def Reset(self):  # :241-246
        check(lib().ad_resampler_reset(self._h))

    def Ratio(self):  # :316-318
        u, d = C.c_int64(0), C.c_int64(0)
        check(lib().ad_resampler_ratio(self._h, C.byref(u), C.byref(d)))
        return u.value, d.value

    def Quality(self) -> int:  # :321-323
        return self.quality

    def TapsPerPhase(self) -> int:  # :326-332
        return lib().ad_resampler_taps_per_phase(self._h)

    def Prototype(self) -> np.ndarray:  # :335-340
        return self.taps.copy()

    def kernel_info(self) -> dict:
        """The launch layout (ad_resampler_kernel_info)."""
        tile, tpw, tl, wl, pf, nb = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0), C.c_int64(0)
        check(lib().ad_resampler_kernel_info(self._h, C.byref(tile), C.byref(tpw), C.byref(tl), C.byref(wl),
                                             C.byref(pf), C.byref(nb)))
        return {"tile": tile.value, "tiles_per_workgroup": tpw.value, "table_in_lds": bool(tl.value),
                "window_in_lds": bool(wl.value), "window_prefetch": bool(pf.value), "lds_bytes": nb.value}

    def close(self):
        if self._h:
            lib().ad_resampler_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def NewRational(up: int, down: int, **opts) -> Resampler:
    """NewRational (resample.go:153-187).  Options: quality, taps_per_phase,
    cutoff_scale, kaiser_beta, max_denominator, channels, device."""
    return Resampler(up, down, **opts)


def NewForRates(in_rate: float, out_rate: float, **opts) -> Resampler:
    """NewForRates (resample.go:190-208): out_rate / in_rate approximated by a
    ratio whose denominator stays within max_denominator."""
    if not (in_rate > 0) or not (out_rate > 0):  # also rejects NaN
        raise ErrInvalidRate()
    md = _config(None, None, None, None, opts.get("max_denominator"))[4]
    up, down = approximate_ratio(out_rate / in_rate, md)
    return Resampler(up, down, **opts)


def Resample(x, up: int, down: int, **opts) -> np.ndarray:
    """One-shot Resample (resample.go:231-238); x is 1-D or [channels][n]."""
    a = f64(x)
    r = NewRational(up, down, channels=1 if a.ndim == 1 else a.shape[0], **opts)
    try:
        if a.shape[-1] == 0:  # :250-252
            return a[..., :0].copy()
        return r.Process(a)
    finally:
        r.close()


def Upsample2x(x, **opts) -> np.ndarray:  # :211-218
    return Resample(x, 2, 1, **opts)


def Downsample2x(x, **opts) -> np.ndarray:  # :221-228
    return Resample(x, 1, 2, **opts)
