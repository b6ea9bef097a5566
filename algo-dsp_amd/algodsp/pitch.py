"""Time-domain pitch shifter (dsp/effects/pitch/pitch_shifter.go) for many channels.

    ps = PitchShifter(48000.0, channels=256, semitones=7)   # pitch.NewPitchShifter + SetPitchSemitones
    ps.ProcessInPlace(block)                                # [channels][n] float64, every channel its own Process
    ps.process_device(d_buf, stride, n, stream)             # the same on device rows

A WSOLA stretch and a 4-point Hermite resample, bit for bit the reference's:
the GPU sums every candidate of the cross-correlation search in the
reference's term order.  The processor keeps nothing between calls and a call
transforms its whole block, so the result depends on the length of the call,
as the reference's does on its block.

The library runs it as the node AD_FXN_PITCHTIME of an fx graph
(include/algodsp.h); this class builds the graph input -> pitch-time -> output
through ad_fx_graph_create_cfg and needs no entry point of its own.  A setter
validates with the reference's rule, leaves the object as it was on error, and
builds the graph anew (there is no state to lose).  The cross-fade table is
computed here (math.cos) and handed to the library.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from ._lib import AD_ERR_INVALID_ARGUMENT, ErrInvalidArgument, FxNodeCfg, check, lib, ptr

FXN_PITCHTIME = 25  # AD_FXN_PITCHTIME
DEFAULT_SEQUENCE_MS, DEFAULT_OVERLAP_MS, DEFAULT_SEARCH_MS = 82.0, 10.0, 28.0  # pitch_shifter.go:15-17
MAX_FRAME = 1 << 24  # the library's bound on sequenceLen and searchLen


class PitchTimeConfig(C.Structure):
    """ad_pitchtime_config (include/algodsp.h); fade_in points at the caller's table."""

    _fields_ = [("sample_rate", C.c_double), ("pitch_ratio", C.c_double), ("sequence_ms", C.c_double),
                ("overlap_ms", C.c_double), ("search_ms", C.c_double), ("fade_in", C.POINTER(C.c_double)),
                ("fade_len", C.c_int64)]


def go_round(v: float) -> float:  # math.Round: halves away from zero
    a = abs(v)
    if a >= 2.0 ** 52:
        return v
    f = math.floor(a)
    return math.copysign(f + 1 if a - f >= 0.5 else f, v)  # a - f is exact; a + 0.5 would round


def _bad(msg: str):
    return ErrInvalidArgument(AD_ERR_INVALID_ARGUMENT, msg)


def _finite_positive(v: float) -> bool:  # isFinitePositive :456-458
    return v > 0 and not math.isnan(v) and not math.isinf(v)


def _in(v: float, lo: float, hi: float) -> bool:  # the setters' range test: false for NaN
    return lo <= v <= hi


def frame_lengths(sample_rate: float, sequence_ms: float, overlap_ms: float, search_ms: float):
    """rebuild :252-276: (sequenceLen, overlapLen, searchLen, stepOut), or ErrInvalidArgument."""
    if not _finite_positive(sample_rate):
        raise _bad("pitch shifter sample rate must be positive and finite")
    if overlap_ms >= sequence_ms:
        raise _bad("pitch shifter overlap must be smaller than sequence")
    seq = go_round(sequence_ms * 0.001 * sample_rate)
    sea = go_round(search_ms * 0.001 * sample_rate)
    if seq > MAX_FRAME or sea > MAX_FRAME:
        raise _bad("pitch shifter: the sample rate makes a frame longer than the kernels index")
    sequence_len = max(int(seq), 32)
    overlap_len = max(int(go_round(overlap_ms * 0.001 * sample_rate)), 8)
    if overlap_len >= sequence_len:
        raise _bad("pitch shifter overlap too large for sequence")
    step_out = sequence_len - overlap_len
    if step_out < 4:
        raise _bad("pitch shifter output hop too small")
    return sequence_len, overlap_len, max(int(sea), 1), step_out


def fade_in_table(overlap_len: int) -> np.ndarray:
    """fadeIn of rebuild :278-293; fadeOut is 1 - fadeIn, which the kernel forms itself."""
    if overlap_len == 1:
        return np.ones(1)
    return np.array([0.5 - 0.5 * math.cos(math.pi * (float(i) / float(overlap_len - 1))) for i in range(overlap_len)])


def validate(sample_rate: float, pitch_ratio: float, sequence_ms: float, overlap_ms: float, search_ms: float):
    """The setters' ranges (:122-217) and rebuild's rules; returns frame_lengths."""
    if not _finite_positive(pitch_ratio) or not _in(pitch_ratio, 0.25, 4.0):
        raise _bad("pitch shifter ratio must be in [0.25, 4]")
    if not _in(sequence_ms, 20.0, 120.0):
        raise _bad("pitch shifter sequence must be in [20, 120] ms")
    if not _in(overlap_ms, 4.0, 60.0):
        raise _bad("pitch shifter overlap must be in [4, 60] ms")
    if not _in(search_ms, 2.0, 40.0):
        raise _bad("pitch shifter search must be in [2, 40] ms")
    return frame_lengths(sample_rate, sequence_ms, overlap_ms, search_ms)


def make_config(sample_rate: float, pitch_ratio: float, sequence_ms: float, overlap_ms: float, search_ms: float):
    """(ad_pitchtime_config, its fade-in table) of validated values; the table must outlive the create call."""
    _, overlap_len, _, _ = validate(sample_rate, pitch_ratio, sequence_ms, overlap_ms, search_ms)
    cfg = PitchTimeConfig(float(sample_rate), float(pitch_ratio), float(sequence_ms), float(overlap_ms),
                          float(search_ms))
    table = fade_in_table(overlap_len)
    cfg.fade_in, cfg.fade_len = ptr(table), table.size
    return cfg, table


def _graph(cfg: PitchTimeConfig, channels: int, device: int) -> C.c_void_p:
    """input -> AD_FXN_PITCHTIME -> output."""
    from .effectchain import FXN_INPUT, FXN_OUTPUT, _Node

    nodes = (_Node * 3)()
    cfgs = (FxNodeCfg * 3)()
    parents = [(C.c_int32 * 1)(0), (C.c_int32 * 1)(1)]
    nodes[0].type = FXN_INPUT
    nodes[1].type = FXN_PITCHTIME
    nodes[2].type = FXN_OUTPUT
    for k in (1, 2):
        nodes[k].n_parents = 1
        nodes[k].parents = C.cast(parents[k - 1], C.POINTER(C.c_int32))
    cfgs[1].config, cfgs[1].bytes = C.addressof(cfg), C.sizeof(cfg)
    h = C.c_void_p()
    check(lib().ad_fx_graph_create_cfg(C.cast(nodes, C.c_void_p), None, C.cast(cfgs, C.c_void_p), 3, int(channels),
                                       int(device), C.byref(h)))
    return h


class PitchShifter:
    """pitch.PitchShifter for `channels` independent channels.  Options: pitch_ratio or semitones,
    sequence_ms, overlap_ms, search_ms (the reference's defaults 82 / 10 / 28 ms)."""

    _options = ("pitch_ratio", "semitones", "sequence_ms", "overlap_ms", "search_ms")

    def __init__(self, sample_rate: float = 48000.0, channels: int = 1, device: int = 0, **options):
        unknown = set(options) - set(self._options)
        if unknown:
            raise TypeError(f"unknown pitch shifter option {min(unknown)!r}")
        if "pitch_ratio" in options and "semitones" in options:
            raise TypeError("pitch shifter: give pitch_ratio or semitones, not both")
        self._h = None
        self.channels = int(channels)
        self.device = int(device)
        ratio = float(options.get("pitch_ratio", 1.0))
        if "semitones" in options:
            ratio = self._semitone_ratio(options["semitones"])
        self._p = {"sample_rate": float(sample_rate), "pitch_ratio": ratio,
                   "sequence_ms": float(options.get("sequence_ms", DEFAULT_SEQUENCE_MS)),
                   "overlap_ms": float(options.get("overlap_ms", DEFAULT_OVERLAP_MS)),
                   "search_ms": float(options.get("search_ms", DEFAULT_SEARCH_MS))}
        self._h = self._build(self._p)

    @staticmethod
    def _semitone_ratio(semitones) -> float:  # SetPitchSemitones :135-148
        semitones = float(semitones)
        if math.isnan(semitones) or math.isinf(semitones):
            raise _bad("pitch shifter semitones must be finite")
        return math.pow(2, semitones / 12.0)

    def _build(self, p) -> C.c_void_p:
        if self.channels <= 0:
            raise _bad("channels must be positive")
        cfg, table = make_config(**p)  # ErrInvalidArgument before the device is touched
        h = _graph(cfg, self.channels, self.device)
        del table  # the library has copied it
        return h

    def _set(self, **changes):
        """One setter: the new values validated and a graph built from them, then the old graph freed.  On an
        error the object, its graph included, is as it was."""
        p = dict(self._p, **{k: float(v) for k, v in changes.items()})
        h = self._build(p)
        old, self._h, self._p = self._h, h, p
        lib().ad_fx_graph_destroy(old)

    def SampleRate(self) -> float:
        return self._p["sample_rate"]

    def PitchRatio(self) -> float:
        return self._p["pitch_ratio"]

    def PitchSemitones(self) -> float:  # :90
        return 12.0 * math.log2(self._p["pitch_ratio"])

    def Sequence(self) -> float:
        return self._p["sequence_ms"]

    def Overlap(self) -> float:
        return self._p["overlap_ms"]

    def Search(self) -> float:
        return self._p["search_ms"]

    def SetSampleRate(self, sample_rate):  # :102-120
        self._set(sample_rate=sample_rate)

    def SetPitchRatio(self, ratio):  # :123-132
        self._set(pitch_ratio=ratio)

    def SetPitchSemitones(self, semitones):  # :135-148
        self._set(pitch_ratio=self._semitone_ratio(semitones))

    def SetSequence(self, ms):  # :151-171
        self._set(sequence_ms=ms)

    def SetOverlap(self, ms):  # :174-194
        self._set(overlap_ms=ms)

    def SetSearch(self, ms):  # :197-217
        self._set(search_ms=ms)

    def frame_lengths(self):
        """(sequenceLen, overlapLen, searchLen, stepOut) of the current settings."""
        p = self._p
        return frame_lengths(p["sample_rate"], p["sequence_ms"], p["overlap_ms"], p["search_ms"])

    def Reset(self):  # :222: a no-op there; here every node's Reset, which is one
        check(lib().ad_fx_graph_reset(self._h))

    def ProcessInPlace(self, buf):  # :243-250 on host rows [channels][n] (or [n] for one channel)
        if not isinstance(buf, np.ndarray) or buf.dtype != np.float64 or not buf.flags.c_contiguous:
            raise TypeError("buffer must be a C-contiguous float64 numpy array")
        b = buf.reshape(1, -1) if buf.ndim == 1 else buf
        if b.shape[0] != self.channels:
            raise ValueError(f"buffer has {b.shape[0]} channels, processor has {self.channels}")
        if b.shape[1]:
            check(lib().ad_fx_graph_process(self._h, ptr(b), b.shape[1]))
        return buf

    def Process(self, x) -> np.ndarray:  # :225-240: a new block of equal length
        return self.ProcessInPlace(np.array(x, dtype=np.float64, order="C"))

    def process_device(self, d_buf: int, stride: int, n: int, stream: int | None = None):
        """Device rows [channels][stride], n samples each, in place on `stream`."""
        check(lib().ad_fx_graph_process_device(self._h, C.c_void_p(d_buf), int(stride), int(n), C.c_void_p(stream or 0)))

    def close(self):
        if self._h:
            lib().ad_fx_graph_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
