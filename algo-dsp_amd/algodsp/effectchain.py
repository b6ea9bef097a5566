"""Batched effectchain runtime: `channels` copies of one
dsp/effectchain graph processed together on the GPU.

Mirrors the reference's Chain API (dsp/effectchain/chain.go, chain_process.go):

    ch = Chain(48000.0, channels=256)            # effectchain.New(ctx, DefaultRegistry(...))
    ch.LoadGraph(json_graph)                      # chain.go LoadGraph: parse + Kahn order + Configure
    ch.Process(block)                             # chain_process.go:11-33, block [channels][n] in place

The host side here is the graph compiler: JSON parsing and the topological
order restate graph.go:57-165; each node's parameters are clamped exactly as
its runtime's Configure does (runtime_dynamics.go, runtime_filter_pitch_reverb.go,
chain_process.go:177-227 for split-freq).  The compiled node list goes to
ad_fx_graph_create (include/algodsp.h), which runs every node on the GPU;
there is no CPU path.  Node types outside {filter*, dyn-compressor,
dyn-limiter, dyn-gate, dyn-expander, dyn-deesser, dyn-transient,
reverb-freeverb, reverb-fdn, reverb, reverb-conv, delay, delay-simple, flanger,
phaser, tremolo, ringmod, distortion, dist-cheb, bitcrusher, spectral-freeze,
pitch-spectral, split-freq, split, sum, _input, _output} raise
UnknownEffect (the GPU runtime's ErrUnknownEffect).  The phaser, tremolo and
ringmod nodes carry their configuration in a parallel array (_NodeExt,
ad_fx_graph_create_ext); _Node keeps its layout.  The distortion, dist-cheb
and bitcrusher nodes carry theirs as (structure, size) in a second parallel
array (FxNodeCfg, ad_fx_graph_create_cfg), and so do dyn-deesser,
dyn-transient, spectral-freeze and pitch-spectral (whose structures point at the
Hann table and the resampling prototype computed here).  With
Chain(sidechain=True) the dyn-lookahead and vocoder nodes run as well: their
structures (ad_fx_lookahead_node, ad_fx_vocoder_node) carry the effect's config
and the side parents, the edges with toPortIndex 1.  With
Chain(pitch_time=True) the pitch-time node runs too (ad_pitchtime_config,
whose structure lives in algodsp.pitch).
"""
from __future__ import annotations

import ctypes as C
import json
import math

import numpy as np

from . import design
from ._lib import (BitCrusherConfig, CompressorConfig, DeEsserConfig, DelayConfig, DistortionConfig, FdnConfig,
                   FlangerConfig, FxNodeCfg, LookaheadConfig, PhaserConfig, PitchSpecConfig, RingModConfig,
                   SpecFreezeConfig, TransientConfig, TremoloConfig, VocoderConfig, check, lib, ptr)
from .processors import section_table

INPUT_NODE_ID = "_input"  # graph.go:10-13
OUTPUT_NODE_ID = "_output"
NODE_TYPE_SPLIT_FREQ = "split-freq"

FXN_INPUT, FXN_OUTPUT, FXN_PASS, FXN_SPLIT_FREQ, FXN_BIQUAD, FXN_COMPRESSOR, FXN_FREEVERB, FXN_CONV_REVERB = range(8)
FXN_FDN_REVERB = 8
FXN_DELAY, FXN_FLANGER = 9, 10
FXN_PHASER, FXN_TREMOLO, FXN_RINGMOD = 11, 12, 13
FXN_DISTORTION, FXN_BITCRUSHER = 15, 16  # 14 is not assigned
FXN_DEESSER, FXN_TRANSIENT = 18, 19  # 17 is not assigned
FXN_SPECFREEZE, FXN_PITCHSPEC = 20, 21
FXN_LOOKAHEAD, FXN_VOCODER = 23, 24  # 22 is not assigned
FXN_PITCHTIME = 25
SIDECHAIN_TYPES = ("dyn-lookahead", "vocoder")  # splitMainAndSideParents chain_process.go:128
MAX_PARENTS = 8

FILTER_TYPES = ("filter", "filter-lowpass", "filter-highpass", "filter-bandpass", "filter-notch",
                "filter-allpass", "filter-peak", "filter-lowshelf", "filter-highshelf")  # registry_defaults.go:141-151


class UnknownEffect(ValueError):
    """effectchain.ErrUnknownEffect (chain.go:11) for node types the GPU runtime lacks."""


class GraphError(ValueError):
    """parseGraph errors (graph.go:63-66, 157-159)."""


class _Node(C.Structure):
    _fields_ = [("type", C.c_int), ("bypassed", C.c_int), ("n_parents", C.c_int),
                ("parents", C.POINTER(C.c_int32)), ("parent_ports", C.POINTER(C.c_int32)),
                ("sections", C.POINTER(C.c_double)), ("nsec", C.c_int),
                ("sections2", C.POINTER(C.c_double)), ("nsec2", C.c_int),
                ("comp", C.POINTER(CompressorConfig)), ("verb", C.c_double * 5),
                ("dyn_mode", C.c_int), ("dyn_range_db", C.c_double), ("dyn_hold_ms", C.c_double),
                ("ir", C.POINTER(C.c_double)), ("ir_len", C.c_int64), ("conv_min_order", C.c_int),
                ("conv_wet", C.c_double), ("conv_dry", C.c_double), ("fdn", C.POINTER(FdnConfig)),
                ("delay", C.POINTER(DelayConfig)), ("flanger", C.POINTER(FlangerConfig))]


class _NodeExt(C.Structure):
    """ad_fx_node_ext: the configurations of the node types added after ad_fx_node was laid out."""

    _fields_ = [("phaser", C.POINTER(PhaserConfig)), ("tremolo", C.POINTER(TremoloConfig)),
                ("ringmod", C.POINTER(RingModConfig))]


def _side_node(config_type):
    """ad_fx_lookahead_node / ad_fx_vocoder_node: the effect's config, then the side parents."""

    class _SideNode(C.Structure):
        _fields_ = [("config", config_type), ("n_side", C.c_int), ("side_parents", C.c_int * MAX_PARENTS),
                    ("side_ports", C.c_int * MAX_PARENTS)]

    return _SideNode


def clamp(v, lo, hi):  # core.Clamp
    return lo if v < lo else (hi if v > hi else v)


class Params:
    """effectchain.Params (params.go): ID, Type, Bypassed, Num, Str."""

    def __init__(self, id_, type_, bypassed=False, num=None, str_=None):
        self.ID, self.Type, self.Bypassed = id_, type_, bool(bypassed)
        self.Num, self.Str = num or {}, str_ or {}

    def GetNum(self, key, default):  # params.go:15-27
        v = self.Num.get(key)
        if v is None or math.isnan(v) or math.isinf(v):
            return default
        return v


def _parse_params(raw):  # parseNodeParams graph.go:169-199
    num, st = {}, {}
    if isinstance(raw, dict):
        for k, v in raw.items():
            if isinstance(v, bool):
                num[k] = 1.0 if v else 0.0
            elif isinstance(v, (int, float)):
                num[k] = float(v)
            elif isinstance(v, str):
                st[k] = v
    return num, st


class CompiledGraph:
    def __init__(self, nodes, incoming, outgoing, order):
        self.Nodes, self.Incoming, self.Outgoing, self.Order = nodes, incoming, outgoing, order


def parse_graph(raw: str) -> CompiledGraph:
    """parseGraph (graph.go:57-165): nodes without id/type are dropped, a graph
    without _input/_output is empty, edges to unknown nodes and self-loops are
    dropped, Kahn's algorithm orders the nodes (any topological order gives
    the same result), a cycle is an error."""
    if raw == "":
        return CompiledGraph({}, {}, {}, [])
    try:
        state = json.loads(raw)
    except json.JSONDecodeError as e:
        raise GraphError(f"invalid chain graph json: {e}") from e
    nodes = {}
    for n in state.get("nodes") or []:
        if not n.get("id") or not n.get("type"):
            continue
        num, st = _parse_params(n.get("params"))
        nodes[n["id"]] = Params(n["id"], n["type"], n.get("bypassed", False), num, st)
    if INPUT_NODE_ID not in nodes or OUTPUT_NODE_ID not in nodes:
        return CompiledGraph({}, {}, {}, [])
    incoming = {k: [] for k in nodes}
    outgoing = {k: [] for k in nodes}
    indeg = {k: 0 for k in nodes}
    for c in state.get("connections") or []:
        f, t = c.get("from", ""), c.get("to", "")
        if not f or not t or f == t or f not in nodes or t not in nodes:
            continue
        e = (f, t, max(0, int(c.get("fromPortIndex", 0) or 0)), max(0, int(c.get("toPortIndex", 0) or 0)))
        outgoing[f].append(e)
        incoming[t].append(e)
        indeg[t] += 1
    queue = [k for k in nodes if indeg[k] == 0]
    order = []
    while queue:
        k = queue.pop(0)
        order.append(k)
        for e in outgoing[k]:
            indeg[e[1]] -= 1
            if indeg[e[1]] == 0:
                queue.append(e[1])
    if len(order) != len(nodes):
        raise GraphError("invalid chain graph: contains cycle")
    return CompiledGraph(nodes, incoming, outgoing, order)


# ---- node configuration (each runtime's Configure) -------------------------
def compressor_config(p: Params, fs: float) -> CompressorConfig:
    """compressorRuntime.Configure (runtime_dynamics.go:15-57) on NewCompressor defaults."""
    c = CompressorConfig()
    lib().ad_compressor_default_config(C.byref(c), float(fs))
    c.threshold_db = clamp(p.GetNum("thresholdDB", -20), -60, 0)
    c.ratio = clamp(p.GetNum("ratio", 4), 1, 100)
    c.knee_db = clamp(p.GetNum("kneeDB", 6), 0, 24)
    c.attack_ms = clamp(p.GetNum("attackMs", 10), 0.1, 1000)
    c.release_ms = clamp(p.GetNum("releaseMs", 100), 1, 5000)
    c.auto_makeup = 0
    c.makeup_db = clamp(p.GetNum("makeupGainDB", 0), 0, 24)
    return c


def limiter_config(p: Params, fs: float) -> CompressorConfig:
    """NewLimiter (dynamics/limiter.go:11-44: ratio 100, attack 0.1 ms, hard
    knee, no makeup) + limiterRuntime.Configure (runtime_dynamics.go:67-85)."""
    c = CompressorConfig()
    lib().ad_compressor_default_config(C.byref(c), float(fs))
    c.ratio, c.attack_ms, c.knee_db, c.auto_makeup, c.makeup_db = 100.0, 0.1, 0.0, 0, 0.0
    c.threshold_db = clamp(p.GetNum("thresholdDB", -0.1), -24, 0)
    c.release_ms = clamp(p.GetNum("releaseMs", 100), 1, 5000)
    return c


def gate_config(p: Params, fs: float):
    """gateRuntime.Configure (runtime_dynamics.go:130-170) on NewGate defaults:
    (config, range dB, hold ms).  Topology and detector stay NewGate's
    (feed-forward, peak)."""
    c = CompressorConfig()
    lib().ad_compressor_default_config(C.byref(c), float(fs))
    c.threshold_db = clamp(p.GetNum("thresholdDB", -40), -80, 0)
    c.ratio = clamp(p.GetNum("ratio", 10), 1, 100)
    c.knee_db = clamp(p.GetNum("kneeDB", 6), 0, 24)
    c.attack_ms = clamp(p.GetNum("attackMs", 0.1), 0.1, 1000)
    c.release_ms = clamp(p.GetNum("releaseMs", 100), 1, 5000)
    c.auto_makeup, c.makeup_db, c.feedback_ratio_scale = 0, 0.0, 0
    return c, clamp(p.GetNum("rangeDB", -80), -120, 0), clamp(p.GetNum("holdMs", 50), 0, 5000)


def expander_config(p: Params, fs: float):
    """expanderRuntime.Configure (runtime_dynamics.go:180-235) on NewExpander
    defaults: (config, range dB, hold ms = 0)."""
    c = CompressorConfig()
    lib().ad_compressor_default_config(C.byref(c), float(fs))
    c.threshold_db = clamp(p.GetNum("thresholdDB", -35), -80, 0)
    c.ratio = clamp(p.GetNum("ratio", 2), 1, 100)
    c.knee_db = clamp(p.GetNum("kneeDB", 6), 0, 24)
    c.attack_ms = clamp(p.GetNum("attackMs", 1), 0.1, 1000)
    c.release_ms = clamp(p.GetNum("releaseMs", 100), 1, 5000)
    c.topology = 1 if p.Str.get("topology", "") == "feedback" else 0  # normalize.go:185-194
    c.detector_mode = 1 if p.Str.get("detector", "") == "rms" else 0  # normalize.go:196-205
    c.rms_window_ms = clamp(p.GetNum("rmsWindowMs", 30), 1, 1000)
    c.auto_makeup, c.makeup_db, c.feedback_ratio_scale = 0, 0.0, 0
    return c, clamp(p.GetNum("rangeDB", -60), -120, 0), 0.0


def freeverb_params(p: Params):
    """freeverbRuntime.Configure (runtime_filter_pitch_reverb.go:330-341)."""
    return (clamp(p.GetNum("wet", 0.22), 0, 1.5), clamp(p.GetNum("dry", 1), 0, 1.5),
            clamp(p.GetNum("roomSize", 0.72), 0, 0.98), clamp(p.GetNum("damp", 0.45), 0, 0.99),
            clamp(p.GetNum("gain", 0.015), 0, 0.1))


def fdn_params(p: Params, fs: float) -> FdnConfig:
    """fdnReverbRuntime.Configure (runtime_filter_pitch_reverb.go:351-363): the
    clamped values configureFDNReverb hands to the setters of a
    NewFDNReverb(fs).  Its wet and damp defaults are not NewFDNReverb's."""
    c = FdnConfig()
    c.sample_rate = float(fs)
    c.wet = clamp(p.GetNum("wet", 0.22), 0, 1.5)
    c.dry = clamp(p.GetNum("dry", 1), 0, 1.5)
    c.rt60_seconds = clamp(p.GetNum("rt60", 1.8), 0.2, 8)
    c.pre_delay_seconds = clamp(p.GetNum("preDelay", 0.01), 0, 0.1)
    c.damp = clamp(p.GetNum("damp", 0.45), 0, 0.99)
    c.mod_depth_seconds = clamp(p.GetNum("modDepth", 0.002), 0, 0.01)
    c.mod_rate_hz = clamp(p.GetNum("modRate", 0.1), 0, 1)
    return c


def _go_round(v: float) -> float:  # math.Round: halves away from zero
    a = abs(v)
    if a >= 2.0 ** 52:
        return v
    f = math.floor(a)
    return math.copysign(f + 1 if a - f >= 0.5 else f, v)  # a - f is exact; a + 0.5 would round


def delay_params(p: Params, fs: float) -> DelayConfig:
    """delayRuntime.Configure (runtime_modulation.go:308-316): the clamped
    values configureDelay (configure.go:329-346) hands to SetSampleRate(fs),
    SetTargetTime, SetFeedback and SetMix of a NewDelay.  ad_delay_create
    applies a config that way: the delay starts at round(0.25 fs) samples and
    ramps to round(time * fs)."""
    c = DelayConfig()
    c.sample_rate = float(fs)
    c.time_seconds = clamp(p.GetNum("time", 0.25), 0.001, 2)
    c.feedback = clamp(p.GetNum("feedback", 0.35), 0, 0.99)
    c.mix = clamp(p.GetNum("mix", 0.25), 0, 1)
    return c


def simple_delay_samples(p: Params, fs: float) -> int:
    """simpleDelayRuntime.Configure (runtime_modulation.go:330-344): delaySamples."""
    delay_ms = clamp(p.GetNum("delayMs", 20), 0, 500)
    return max(int(_go_round(delay_ms * fs / 1000.0)), 0)


def flanger_params(p: Params, fs: float) -> FlangerConfig:
    """flangerRuntime.Configure (runtime_modulation.go:38-48)."""
    c = FlangerConfig()
    c.sample_rate = float(fs)
    c.rate_hz = clamp(p.GetNum("rateHz", 0.25), 0.05, 5)
    c.base_delay_seconds = clamp(p.GetNum("baseDelay", 0.001), 0.0001, 0.01)
    c.depth_seconds = clamp(p.GetNum("depth", 0.0015), 0, 0.0099)
    c.feedback = clamp(p.GetNum("feedback", 0.25), -0.99, 0.99)
    c.mix = clamp(p.GetNum("mix", 0.5), 0, 1)
    return c


def phaser_params(p: Params, fs: float) -> PhaserConfig:
    """phaserRuntime.Configure (runtime_modulation.go:263-279): the clamped
    values configurePhaser (configure.go:276-303) hands to the setters.  A
    maxFreqHz that clamps to 0.49 fs itself fails validateParams there, as it
    fails ad_phaser_validate here."""
    c = PhaserConfig()
    c.sample_rate = float(fs)
    c.min_freq_hz = clamp(p.GetNum("minFreqHz", 300), 20, fs * 0.45)
    c.max_freq_hz = clamp(p.GetNum("maxFreqHz", 1600), c.min_freq_hz + 1, fs * 0.49)
    c.stages = min(max(int(_go_round(p.GetNum("stages", 6))), 1), 12)
    c.rate_hz = clamp(p.GetNum("rateHz", 0.4), 0.05, 5)
    c.feedback = clamp(p.GetNum("feedback", 0.2), -0.99, 0.99)
    c.mix = clamp(p.GetNum("mix", 0.5), 0, 1)
    return c


def tremolo_params(p: Params, fs: float) -> TremoloConfig:
    """tremoloRuntime.Configure (runtime_modulation.go:289-298); smoothing_coeff 0: the library derives it."""
    c = TremoloConfig()
    c.sample_rate = float(fs)
    c.rate_hz = clamp(p.GetNum("rateHz", 4), 0.05, 20)
    c.depth = clamp(p.GetNum("depth", 0.6), 0, 1)
    c.smoothing_ms = clamp(p.GetNum("smoothingMs", 5), 0, 200)
    c.mix = clamp(p.GetNum("mix", 1), 0, 1)
    return c


def ringmod_params(p: Params, fs: float) -> RingModConfig:
    """ringModRuntime.Configure (runtime_modulation.go:58-65)."""
    c = RingModConfig()
    c.sample_rate = float(fs)
    c.carrier_hz = clamp(p.GetNum("carrierHz", 440), 1, fs * 0.49)
    c.mix = clamp(p.GetNum("mix", 1), 0, 1)
    return c


DISTORTION_MODES = ("softclip", "hardclip", "tanh", "waveshaper1", "waveshaper2", "waveshaper3", "waveshaper4",
                    "waveshaper5", "waveshaper6", "waveshaper7", "waveshaper8", "saturate", "saturate2", "softsat",
                    "chebyshev")  # DistortionMode distortion.go:36-52


def _distortion_mode(raw) -> int:  # normalizeDistortionMode normalize.go:102-137: anything else is softclip
    return DISTORTION_MODES.index(raw) if raw in DISTORTION_MODES else 0


def _distortion_approx(raw) -> int:  # normalizeDistortionApproxMode normalize.go:139-148
    return 1 if raw == "polynomial" else 0


def _chebyshev_harmonic(raw) -> int:  # normalizeChebyshevHarmonicMode normalize.go:150-161
    return {"odd": 1, "even": 2}.get(raw, 0)


def adjust_chebyshev_order(order: int, harmonic: int) -> int:
    """configureDistortion's order adjustment (configure.go:131-153): up to the
    harmonic mode's parity, capped at 16, down to the parity again, at least 1."""
    odd, even = harmonic == 1, harmonic == 2
    if (odd and order % 2 == 0) or (even and order % 2 != 0):
        order += 1
    order = min(order, 16)
    if (odd and order % 2 == 0) or (even and order % 2 != 0):
        order -= 1
    return max(order, 1)


def _distortion_config(fs, mode, approx, drive, mix, output, clip, shape, bias, order, harmonic, invert, gain,
                       dc_bypass) -> DistortionConfig:
    """configureDistortion (configure.go:114-215): the values its setters end with."""
    c = DistortionConfig()
    c.sample_rate = float(fs)
    c.mode, c.approx = mode, approx
    c.drive, c.mix, c.output_level, c.clip_level, c.shape, c.bias = drive, mix, output, clip, shape, bias
    c.cheb_order = adjust_chebyshev_order(order, harmonic)
    c.cheb_harmonic, c.cheb_invert, c.cheb_gain, c.cheb_dc_bypass = harmonic, int(invert), gain, int(dc_bypass)
    return c


def distortion_params(p: Params, fs: float) -> DistortionConfig:
    """distortionRuntime.Configure (runtime_modulation.go:95-116): order 3,
    every harmonic, no inversion, gain 1, no DC bypass, no weights."""
    return _distortion_config(fs, _distortion_mode(p.Str.get("mode")), _distortion_approx(p.Str.get("approx")),
                              clamp(p.GetNum("drive", 1.8), 0.01, 20), clamp(p.GetNum("mix", 1.0), 0, 1),
                              clamp(p.GetNum("output", 1.0), 0, 4), clamp(p.GetNum("clip", 1.0), 0.05, 1),
                              clamp(p.GetNum("shape", 0.5), 0, 1), clamp(p.GetNum("bias", 0), -1, 1),
                              3, 0, False, 1.0, False)


def dist_cheb_params(p: Params, fs: float) -> DistortionConfig:
    """distChebRuntime.Configure (runtime_modulation.go:126-167): Chebyshev
    mode at clip 1, shape 0.5, bias 0, and the weights w1..w16 (GetNum drops a
    non-finite one for 0, so SetChebyshevWeights cannot fail)."""
    harmonic = _chebyshev_harmonic(p.Str.get("harmonic"))
    order = min(max(int(_go_round(p.GetNum("order", 3))), 1), 16)
    c = _distortion_config(fs, DISTORTION_MODES.index("chebyshev"), _distortion_approx(p.Str.get("approx")),
                           clamp(p.GetNum("drive", 1.0), 0.01, 20), clamp(p.GetNum("mix", 1.0), 0, 1),
                           clamp(p.GetNum("output", 1.0), 0, 4), 1.0, 0.5, 0.0, order, harmonic,
                           p.GetNum("invert", 0) >= 0.5, clamp(p.GetNum("gain", 1.0), 0, 4),
                           p.GetNum("dcBypass", 0) >= 0.5)
    for k in range(16):
        c.cheb_weights[k] = p.GetNum(f"w{k + 1}", 0)
    return c


def bitcrusher_params(p: Params, fs: float) -> BitCrusherConfig:
    """bitCrusherRuntime.Configure (runtime_modulation.go:75-85)."""
    c = BitCrusherConfig()
    c.sample_rate = float(fs)
    c.bit_depth = clamp(p.GetNum("bitDepth", 8), 1, 32)
    c.downsample = min(max(int(_go_round(p.GetNum("downsample", 4))), 1), 256)
    c.mix = clamp(p.GetNum("mix", 1), 0, 1)
    return c


def deesser_params(p: Params, fs: float) -> DeEsserConfig:
    """deesserRuntime.Configure (runtime_dynamics.go:244-310): the clamped
    values it hands to the setters of a NewDeEsser(fs), in its order; the mode
    and detector strings as normalize.go:207-227 reads them (anything unknown
    is split band / bandpass).  Coefficients 0: the library derives them."""
    c = DeEsserConfig()
    c.sample_rate = float(fs)
    c.freq_hz = clamp(p.GetNum("freqHz", 6000), 1000, fs * 0.49)
    c.q = clamp(p.GetNum("q", 1.5), 0.1, 10)
    c.threshold_db = clamp(p.GetNum("thresholdDB", -20), -80, 0)
    c.ratio = clamp(p.GetNum("ratio", 4), 1, 100)
    c.knee_db = clamp(p.GetNum("kneeDB", 3), 0, 12)
    c.attack_ms = clamp(p.GetNum("attackMs", 0.5), 0.01, 50)
    c.release_ms = clamp(p.GetNum("releaseMs", 20), 1, 500)
    c.range_db = clamp(p.GetNum("rangeDB", -24), -60, 0)
    c.mode = 1 if p.Str.get("mode") == "wideband" else 0
    c.detector = 1 if p.Str.get("detector") == "highpass" else 0
    c.filter_order = min(max(int(_go_round(p.GetNum("filterOrder", 2))), 1), 4)
    c.listen = 1 if p.GetNum("listen", 0) >= 0.5 else 0
    return c


def transient_params(p: Params, fs: float) -> TransientConfig:
    """transientShaperRuntime.Configure (runtime_dynamics.go:320-347).  Coefficients 0: the library derives them."""
    c = TransientConfig()
    c.sample_rate = float(fs)
    c.attack_amount = clamp(p.GetNum("attack", 0), -1, 1)
    c.sustain_amount = clamp(p.GetNum("sustain", 0), -1, 1)
    c.attack_ms = clamp(p.GetNum("attackMs", 10), 0.1, 200)
    c.release_ms = clamp(p.GetNum("releaseMs", 120), 1, 2000)
    return c


def sanitize_spectral_frame_size(n: int) -> int:
    """sanitizeSpectralPitchFrameSize (configure.go:563-593): [256, 4096], the nearer power of two, a tie to the lower."""
    if n < 256:
        return 256
    if n > 4096:
        return 4096
    if n & (n - 1) == 0:
        return n
    lower = 256
    while lower < n:
        lower <<= 1
    upper = lower
    lower = max(lower >> 1, 256)
    return lower if n - lower <= upper - n else upper


def _spectral_frame_hop(p: Params):
    """The frame and hop both spectral runtimes derive (runtime_filter_pitch_reverb.go:253-259, 279-285)."""
    frame = sanitize_spectral_frame_size(int(_go_round(p.GetNum("frameSize", 1024))))
    hop = max(int(_go_round(float(frame) * clamp(p.GetNum("hopRatio", 0.25), 0.01, 0.99))), 1)
    if hop >= frame:
        hop = frame - 1
    return frame, hop


def spectral_freeze_params(p: Params, fs: float):
    """spectralFreezeRuntime.Configure (runtime_filter_pitch_reverb.go:278-299) and configureSpectralFreeze
    (configure.go:391-433) on a NewSpectralFreeze(fs): (config, its Hann table).  phaseMode as
    normalizeSpectralFreezePhaseMode reads it (normalize.go:174-183: anything but "hold" advances)."""
    from .processors import WindowHann, spectral_window

    c = SpecFreezeConfig()
    c.sample_rate = float(fs)
    c.frame_size, c.hop_size = _spectral_frame_hop(p)
    c.mix = clamp(p.GetNum("mix", 1), 0, 1)
    c.phase_mode = 0 if p.Str.get("phaseMode") == "hold" else 1
    c.frozen = 1 if p.GetNum("frozen", 1) >= 0.5 else 0
    c.window_type = WindowHann
    w = spectral_window(WindowHann, c.frame_size)
    c.window = ptr(w)
    return c, w


def spectral_pitch_params(p: Params, fs: float):
    """spectralPitchRuntime.Configure (runtime_filter_pitch_reverb.go:252-268) and configureSpectralPitch
    (configure.go:372-389) on a NewSpectralPitchShifter(fs): (config, its Hann table, the resampling
    prototype of the time stretch or None)."""
    from .processors import WindowHann, pitchspec_resample_taps, spectral_window

    c = PitchSpecConfig()
    c.sample_rate = float(fs)
    c.pitch_ratio = 2.0 ** (clamp(p.GetNum("semitones", 0), -24, 24) / 12.0)  # SetPitchSemitones
    c.frame_size, c.analysis_hop = _spectral_frame_hop(p)
    c.window_type = WindowHann
    c.resample_quality = 1  # resample.QualityBalanced, NewSpectralPitchShifter's
    w = spectral_window(WindowHann, c.frame_size)
    c.window = ptr(w)
    taps = None
    shop = max(int(_go_round(float(c.analysis_hop) * c.pitch_ratio)), 1)  # updateSynthesisHop
    if abs(c.pitch_ratio - 1) > 0.15 and shop != c.analysis_hop:
        taps = pitchspec_resample_taps(c.analysis_hop, shop, c.resample_quality)
        c.resample_taps, c.n_resample_taps = ptr(taps), taps.size
    return c, w, taps


def time_pitch_params(p: Params, fs: float):
    """timePitchRuntime.Configure (runtime_filter_pitch_reverb.go:226-242) and configureTimePitch
    (configure.go:348-370) on a NewPitchShifter(fs): (config, its fade-in table)."""
    from . import pitch

    seq = clamp(p.GetNum("sequence", 40), 20, 120)
    ov = clamp(p.GetNum("overlap", 10), 4, 60)
    if ov >= seq:
        ov = seq - 1
    ratio = math.pow(2, clamp(p.GetNum("semitones", 0), -24, 24) / 12.0)  # SetPitchSemitones
    # the factory builds NewPitchShifter(fs) with its defaults first, and the setters run in configureTimePitch's
    # order, each rebuilding with the values set so far: a sample rate one of those steps refuses fails there
    steps = [pitch.DEFAULT_SEQUENCE_MS, pitch.DEFAULT_OVERLAP_MS, pitch.DEFAULT_SEARCH_MS]
    pitch.frame_lengths(fs, *steps)
    for k, v in enumerate((seq, ov, clamp(p.GetNum("search", 15), 2, 40))):
        steps[k] = v
        pitch.frame_lengths(fs, *steps)
    return pitch.make_config(fs, ratio, *steps)


def lookahead_params(p: Params, fs: float) -> LookaheadConfig:
    """lookaheadLimiterRuntime.Configure (runtime_dynamics.go:94-116) on NewLookaheadLimiter(fs)."""
    cfg = LookaheadConfig()
    lib().ad_lookahead_default_config(C.byref(cfg), fs)
    cfg.threshold_db = clamp(p.GetNum("thresholdDB", -1), -24, 0)
    cfg.release_ms = clamp(p.GetNum("releaseMs", 100), 1, 5000)
    cfg.lookahead_ms = clamp(p.GetNum("lookaheadMs", 3), 0, 200)
    return cfg


def vocoder_params(p: Params, fs: float) -> VocoderConfig:
    """vocoderRuntime.Configure (runtime_misc.go:74-106) on NewVocoder(fs): the node has no layout, band-count
    or downsampling parameter."""
    cfg = VocoderConfig()
    lib().ad_vocoder_default_config(C.byref(cfg), fs)
    cfg.attack_ms = clamp(p.GetNum("attackMs", 0.5), 0.01, 100)
    cfg.release_ms = clamp(p.GetNum("releaseMs", 2.0), 0.01, 1000)
    cfg.input_level = clamp(p.GetNum("inputLevel", 0), 0, 10)
    cfg.synth_level = clamp(p.GetNum("synthLevel", 0), 0, 10)
    cfg.vocoder_level = clamp(p.GetNum("vocoderLevel", 1), 0, 10)
    return cfg


def _config_dict(cfg) -> dict:
    """A config structure's fields as plain data (arrays as lists)."""
    return {f: (list(getattr(cfg, f)) if isinstance(getattr(cfg, f), C.Array) else getattr(cfg, f))
            for f, _ in cfg._fields_}


def _filter_kind(node_type, raw):  # normalizeFilterKind normalize.go:42-86
    k = raw.strip().lower()
    if k in ("bandeq", "band-eq", "bandeqpeak", "bell", "bandbell"):
        k = "peak"
    if raw.strip():
        return k if k in ("highpass", "lowpass", "bandpass", "notch", "allpass", "peak", "highshelf",
                          "lowshelf") else "peak"
    return {"filter-highpass": "highpass", "filter-bandpass": "bandpass", "filter-notch": "notch",
            "filter-allpass": "allpass", "filter-peak": "peak", "filter-lowshelf": "lowshelf",
            "filter-highshelf": "highshelf"}.get(node_type, "lowpass")


def filter_chain(p: Params, fs: float, designer):
    """filterRuntime.Configure (runtime_filter_pitch_reverb.go:40-176) -> (sections, gain).
    Without a designer the runtime keeps its passthrough chain {B0: 1}."""
    fam = (p.Str.get("family", "") or "").strip().lower() or "rbj"
    if p.Type == "filter-moog" or fam == "moog":  # normalizeFilterFamily: the moog ladder, designer or not
        raise UnknownEffect("filter-moog is not run by the GPU graph runtime")
    if designer is None:
        return [(1.0, 0.0, 0.0, 0.0, 0.0)], 1.0
    kind = _filter_kind(p.Type, p.Str.get("kind", ""))
    freq = clamp(p.GetNum("freq", 1200), 20, fs * 0.49)
    gain_db = clamp(p.GetNum("gain", 0), -24, 24)
    shape = clamp(p.GetNum("q", 0.707), 0.2, 8)
    fam = designer.NormalizeFamilyForType(kind, designer.NormalizeFamily(fam))
    order = designer.NormalizeOrder(kind, fam, int(round(p.GetNum("order", 2))))
    shape = designer.ClampShape(kind, fam, freq, fs, shape)
    try:
        return designer.BuildChain(fam, kind, order, freq, gain_db, shape, fs)
    except NotImplementedError as e:
        raise UnknownEffect(str(e)) from e


def split_freq_sections(p: Params, fs: float):
    """processSplitFreqNode (chain_process.go:177-227): LR4 at clamp(freqHz).
    crossover.New failing leaves both bands a copy (identity sections)."""
    freq = p.GetNum("freqHz", 1200)
    freq = max(freq, 20.0)
    max_freq = max(20.0, fs * 0.5 * 0.95)
    freq = min(freq, max_freq)
    xo = design.crossover(freq, 4, fs)
    if xo is None:
        ident = [(1.0, 0.0, 0.0, 0.0, 0.0)]
        return ident, ident
    return xo


def conv_reverb_kernel(p: Params, provider):
    """convReverbRuntime.Configure (runtime_misc.go:18-58): the IR at irIndex
    (default 0), stereo averaged to mono ((ch0 + ch1) * 0.5 over the shorter
    length, ch0's tail kept), and the wet level (default 0.35; dry 1.0).
    None when there is no provider or no such IR: the runtime then has no
    engine and Process leaves the block untouched (a pass-through node)."""
    ir_index = int(p.GetNum("irIndex", 0))
    wet = p.GetNum("wet", 0.35)
    if provider is None:
        return None
    samples, _fs, ok = provider.GetIR(ir_index)
    if not ok or samples is None or len(samples) == 0:
        return None
    ch0 = np.asarray(samples[0], dtype=np.float64)
    kernel = ch0.copy()
    if len(samples) > 1:
        ch1 = np.asarray(samples[1], dtype=np.float64)
        n = min(ch0.size, ch1.size)
        kernel[:n] = (ch0[:n] + ch1[:n]) * 0.5
    if kernel.size == 0:  # NewConvolutionReverb: "reverb: empty impulse response kernel"
        raise ValueError("effectchain: create convolution reverb: reverb: empty impulse response kernel")
    return kernel, wet


class Chain:
    """effectchain.Chain for `channels` independent channels of one graph.
    `ir_provider` is effectchain.WithIRProvider's IRProvider (GetIR(index) ->
    (samples [ch][n], sample_rate, ok)) for reverb-conv nodes.  `sidechain=True`
    admits the dyn-lookahead and vocoder nodes and routes their toPortIndex 1
    edges to the side input; the default keeps both types UnknownEffect.
    `pitch_time=True` admits the pitch-time node (algodsp.pitch, the WSOLA pitch
    shifter); the default keeps it UnknownEffect.  That node transforms each
    call's whole block, so its result depends on the length of the call, as the
    reference's does on its block."""

    def __init__(self, sample_rate: float = 48000.0, channels: int = 1, designer=None, device: int = 0,
                 ir_provider=None, sidechain: bool = False, pitch_time: bool = False):
        self.sample_rate = float(sample_rate)
        self.pitch_time = bool(pitch_time)  # opt-in, as sidechain is, for the same reason
        # the dyn-lookahead and vocoder nodes, with their side inputs, run on the GPU only where the caller asks:
        # a caller that takes UnknownEffect as "run this graph on the reference" keeps getting it for them
        self.sidechain = bool(sidechain)
        self.channels = int(channels)
        self.designer = designer
        self.ir_provider = ir_provider
        self.device = int(device)
        self.graph = CompiledGraph({}, {}, {}, [])
        self._h = None
        self._keep = []
        # the compiled nodes in execution order, as plain data (node id, kind,
        # bypassed, parents [(index, port)] and the designed parameters):
        # what the GPU runs, and what the parity tests hand to the oracle
        self.spec = []

    def HasGraph(self) -> bool:
        return bool(self.graph.Order)

    def _free(self):
        if self._h:
            lib().ad_fx_graph_destroy(self._h)
            self._h = None

    def LoadGraph(self, json_graph: str) -> None:
        g = parse_graph(json_graph)
        self._free()
        self.graph = g
        if not g.Order:
            return
        order = [INPUT_NODE_ID] + [k for k in g.Order if k != INPUT_NODE_ID]
        idx = {k: i for i, k in enumerate(order)}
        fs = self.sample_rate
        nodes = (_Node * len(order))()
        ext = (_NodeExt * len(order))()
        cfgs = (FxNodeCfg * len(order))()
        keep = []
        spec = []
        for i, k in enumerate(order):
            p = g.Nodes[k]
            d = nodes[i]
            # splitMainAndSideParents (chain_process.go:124-144): on a dyn-lookahead or vocoder node the edges
            # with toPortIndex 1 are side parents (Chain(sidechain=True); without it the two types stay
            # UnknownEffect); on every other node toPortIndex is ignored.  The rule is
            # applied afresh to the parsed edge list, where the reference filters g.Incoming[id] in place and
            # loses a side edge listed before a main edge from the second block on.
            sidechain = self.sidechain and p.Type in SIDECHAIN_TYPES
            par = [(idx[e[0]], e[2]) for e in g.Incoming[k] if not (sidechain and e[3] == 1)]
            side = [(idx[e[0]], 1 if g.Nodes[e[0]].Type == NODE_TYPE_SPLIT_FREQ and e[2] == 1 else 0)
                    for e in g.Incoming[k] if sidechain and e[3] == 1]
            if len(par) > MAX_PARENTS or len(side) > MAX_PARENTS:
                raise UnknownEffect(f"node {k}: more than {MAX_PARENTS} parents")
            if par:
                pa = (C.c_int32 * len(par))(*[q[0] for q in par])
                po = (C.c_int32 * len(par))(*[q[1] if g.Nodes[order[q[0]]].Type == NODE_TYPE_SPLIT_FREQ and q[1] == 1
                                              else 0 for q in par])
                keep += [pa, po]
                d.parents, d.parent_ports = C.cast(pa, C.POINTER(C.c_int32)), C.cast(po, C.POINTER(C.c_int32))
            d.n_parents = len(par)
            d.bypassed = 1 if p.Bypassed else 0
            t = p.Type
            sd = {"id": k, "bypassed": bool(p.Bypassed),
                  "parents": [(q[0], 1 if g.Nodes[order[q[0]]].Type == NODE_TYPE_SPLIT_FREQ and q[1] == 1 else 0)
                              for q in par]}
            if k == INPUT_NODE_ID:
                d.type = FXN_INPUT
                sd["type"] = "input"
            elif k == OUTPUT_NODE_ID:
                d.type = FXN_OUTPUT
                sd["type"] = "output"
            elif t == NODE_TYPE_SPLIT_FREQ:
                d.type = FXN_SPLIT_FREQ
                lp, hp = split_freq_sections(p, fs)
                sd.update(type="split", sections=lp, sections2=hp)
                a, b = section_table(np.asarray(lp)), section_table(np.asarray(hp))
                keep += [a, b]
                d.sections, d.nsec = ptr(a), a.shape[0]
                d.sections2, d.nsec2 = ptr(b), b.shape[0]
            elif t in ("split", "sum", INPUT_NODE_ID, OUTPUT_NODE_ID):
                d.type = FXN_PASS
                sd["type"] = "pass"
            elif t in FILTER_TYPES or t == "filter-moog":
                d.type = FXN_BIQUAD
                sd.update(type="biquad", sections=([], 1.0))
                if not p.Bypassed:
                    secs, gain = filter_chain(p, fs, self.designer)
                    sd["sections"] = (list(secs), gain)
                    a = section_table(np.asarray(secs, dtype=np.float64), gain)
                    keep.append(a)
                    d.sections, d.nsec = ptr(a), a.shape[0]
            elif t in ("dyn-compressor", "dyn-limiter"):
                d.type = FXN_COMPRESSOR
                cfg = compressor_config(p, fs) if t == "dyn-compressor" else limiter_config(p, fs)
                keep.append(cfg)
                d.comp = C.pointer(cfg)
                sd.update(type="comp", comp={f: getattr(cfg, f) for f, _ in cfg._fields_})
            elif t in ("dyn-gate", "dyn-expander"):
                d.type = FXN_COMPRESSOR
                gate = t == "dyn-gate"
                cfg, rng, hold = gate_config(p, fs) if gate else expander_config(p, fs)
                keep.append(cfg)
                d.comp = C.pointer(cfg)
                d.dyn_mode, d.dyn_range_db, d.dyn_hold_ms = (2 if gate else 1), rng, hold
                sd.update(type="comp", comp={f: getattr(cfg, f) for f, _ in cfg._fields_},
                          expander=dict(gate=gate, range_db=rng, hold_ms=hold))
            elif t == "reverb-fdn" or (t == "reverb" and p.Str.get("model") == "fdn"):
                d.type = FXN_FDN_REVERB
                cfg = fdn_params(p, fs)
                keep.append(cfg)
                d.fdn = C.pointer(cfg)
                sd.update(type="fdn", fdn={f: getattr(cfg, f) for f, _ in cfg._fields_})
            elif t == "delay":
                d.type = FXN_DELAY
                cfg = delay_params(p, fs)
                keep.append(cfg)
                d.delay = C.pointer(cfg)
                sd.update(type="delay", delay={f: getattr(cfg, f) for f, _ in cfg._fields_})
            elif t == "delay-simple":
                samples = simple_delay_samples(p, fs)
                if samples == 0:
                    d.type = FXN_PASS  # a one-slot buffer: Process returns at once (runtime_modulation.go:347-349)
                    sd["type"] = "pass"
                else:
                    d.type = FXN_DELAY
                    cfg = DelayConfig(sample_rate=fs, mode=1, delay_samples=samples)
                    keep.append(cfg)
                    d.delay = C.pointer(cfg)
                    sd.update(type="delay", delay={f: getattr(cfg, f) for f, _ in cfg._fields_})
            elif t == "flanger":
                d.type = FXN_FLANGER
                cfg = flanger_params(p, fs)
                keep.append(cfg)
                d.flanger = C.pointer(cfg)
                sd.update(type="flanger", flanger={f: getattr(cfg, f) for f, _ in cfg._fields_})
            elif t == "phaser":
                d.type = FXN_PHASER
                # the factory builds NewPhaser(fs) with its defaults first (registry_defaults.go:112-119): a
                # sample rate with 1600 >= 0.49 fs fails there, before the node's own range is read
                base = PhaserConfig()
                lib().ad_phaser_default_config(C.byref(base), fs)
                check(lib().ad_phaser_validate(C.byref(base)))
                cfg = phaser_params(p, fs)
                check(lib().ad_phaser_validate(C.byref(cfg)))
                keep.append(cfg)
                ext[i].phaser = C.pointer(cfg)
                sd.update(type="phaser", phaser={f: getattr(cfg, f) for f, _ in cfg._fields_})
            elif t == "tremolo":
                d.type = FXN_TREMOLO
                cfg = tremolo_params(p, fs)
                keep.append(cfg)
                ext[i].tremolo = C.pointer(cfg)
                sd.update(type="tremolo", tremolo={f: getattr(cfg, f) for f, _ in cfg._fields_})
            elif t == "ringmod":
                d.type = FXN_RINGMOD
                cfg = ringmod_params(p, fs)
                keep.append(cfg)
                ext[i].ringmod = C.pointer(cfg)
                sd.update(type="ringmod", ringmod={f: getattr(cfg, f) for f, _ in cfg._fields_})
            elif t in ("distortion", "dist-cheb"):
                d.type = FXN_DISTORTION
                cfg = distortion_params(p, fs) if t == "distortion" else dist_cheb_params(p, fs)
                check(lib().ad_distortion_validate(C.byref(cfg)))
                keep.append(cfg)
                cfgs[i].config, cfgs[i].bytes = C.addressof(cfg), C.sizeof(cfg)
                sd.update(type="distortion", distortion=_config_dict(cfg))
            elif t == "bitcrusher":
                d.type = FXN_BITCRUSHER
                cfg = bitcrusher_params(p, fs)
                check(lib().ad_bitcrusher_validate(C.byref(cfg)))
                keep.append(cfg)
                cfgs[i].config, cfgs[i].bytes = C.addressof(cfg), C.sizeof(cfg)
                sd.update(type="bitcrusher", bitcrusher=_config_dict(cfg))
            elif t == "dyn-deesser":
                d.type = FXN_DEESSER
                # the factory builds NewDeEsser(fs) first and Configure's SetSampleRate runs with the default
                # 6000 Hz in place (deesser.go:399): a sample rate <= 12 kHz fails before freqHz is read
                base = DeEsserConfig()
                lib().ad_deesser_default_config(C.byref(base), fs)
                check(lib().ad_deesser_validate(C.byref(base)))
                cfg = deesser_params(p, fs)
                check(lib().ad_deesser_validate(C.byref(cfg)))
                keep.append(cfg)
                cfgs[i].config, cfgs[i].bytes = C.addressof(cfg), C.sizeof(cfg)
                sd.update(type="deesser", deesser=_config_dict(cfg))
            elif t == "dyn-transient":
                d.type = FXN_TRANSIENT
                cfg = transient_params(p, fs)
                check(lib().ad_transient_validate(C.byref(cfg)))
                keep.append(cfg)
                cfgs[i].config, cfgs[i].bytes = C.addressof(cfg), C.sizeof(cfg)
                sd.update(type="transient", transient=_config_dict(cfg))
            elif t == "spectral-freeze":
                d.type = FXN_SPECFREEZE
                cfg, win = spectral_freeze_params(p, fs)
                check(lib().ad_specfreeze_validate(C.byref(cfg)))
                keep += [cfg, win]
                cfgs[i].config, cfgs[i].bytes = C.addressof(cfg), C.sizeof(cfg)
                sd.update(type="specfreeze", specfreeze={f: getattr(cfg, f) for f, _ in cfg._fields_ if f != "window"})
            elif t == "pitch-spectral":
                d.type = FXN_PITCHSPEC
                cfg, win, taps = spectral_pitch_params(p, fs)
                check(lib().ad_pitchspec_validate(C.byref(cfg)))
                keep += [cfg, win, taps]
                cfgs[i].config, cfgs[i].bytes = C.addressof(cfg), C.sizeof(cfg)
                sd.update(type="pitchspec", pitchspec={f: getattr(cfg, f) for f, _ in cfg._fields_
                                                       if f not in ("window", "resample_taps")})
            elif t == "pitch-time" and self.pitch_time:
                d.type = FXN_PITCHTIME
                cfg, fade = time_pitch_params(p, fs)
                keep += [cfg, fade]
                cfgs[i].config, cfgs[i].bytes = C.addressof(cfg), C.sizeof(cfg)
                sd.update(type="pitchtime", pitchtime={f: getattr(cfg, f) for f, _ in cfg._fields_
                                                       if f not in ("fade_in", "fade_len")})
            elif sidechain:
                lookahead = t == "dyn-lookahead"
                d.type = FXN_LOOKAHEAD if lookahead else FXN_VOCODER
                cfg = lookahead_params(p, fs) if lookahead else vocoder_params(p, fs)
                check((lib().ad_lookahead_validate if lookahead else lib().ad_vocoder_validate)(C.byref(cfg)))
                node = _side_node(type(cfg))()
                node.config = cfg
                node.n_side = len(side)
                for j, (sp, sport) in enumerate(side):
                    node.side_parents[j], node.side_ports[j] = sp, sport
                keep.append(node)
                cfgs[i].config, cfgs[i].bytes = C.addressof(node), C.sizeof(node)
                name = "lookahead" if lookahead else "vocoder"
                sd.update(type=name, side_parents=list(side))
                sd[name] = _config_dict(cfg)
            elif t in ("reverb-freeverb", "reverb"):  # reverbRuntime without model "fdn" is Freeverb
                d.type = FXN_FREEVERB
                for j, v in enumerate(freeverb_params(p)):
                    d.verb[j] = v
                sd.update(type="verb", verb=freeverb_params(p))
            elif t == "reverb-conv":
                kw = None if p.Bypassed else conv_reverb_kernel(p, self.ir_provider)
                if kw is None:
                    d.type = FXN_PASS  # no engine: Process is a no-op (runtime_misc.go:61-64)
                    sd["type"] = "pass"
                else:
                    kern, wet = kw
                    kern = np.ascontiguousarray(kern)
                    keep.append(kern)
                    d.type = FXN_CONV_REVERB
                    d.ir, d.ir_len = ptr(kern), kern.size
                    d.conv_min_order, d.conv_wet, d.conv_dry = 7, wet, 1.0  # NewConvolutionReverb(kernel, 7)
                    sd.update(type="conv", kernel=kern, min_order=7, wet=wet, dry=1.0)
            else:
                raise UnknownEffect(f"effect type {t!r} is not run by the GPU graph runtime")
            spec.append(sd)
        h = C.c_void_p()
        check(lib().ad_fx_graph_create_cfg(C.cast(nodes, C.c_void_p), C.cast(ext, C.c_void_p), C.cast(cfgs, C.c_void_p),
                                           len(order), self.channels, self.device, C.byref(h)))
        self._h = h
        self._keep = keep
        self.spec = spec

    def op_count(self):
        """(device ops per call, buffers, streams) of the compiled graph."""
        a, b, c = C.c_int(), C.c_int(), C.c_int()
        check(lib().ad_fx_graph_op_count(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def Process(self, block) -> bool:
        """chain_process.go:11-33; block [channels][n] float64, in place.
        False (block untouched) without a valid graph."""
        if not isinstance(block, np.ndarray) or block.dtype != np.float64 or not block.flags.c_contiguous:
            raise TypeError("block must be a C-contiguous float64 numpy array")
        b = block.reshape(1, -1) if block.ndim == 1 else block
        if b.shape[0] != self.channels:
            raise ValueError(f"block has {b.shape[0]} channels, chain has {self.channels}")
        if b.shape[1] == 0:
            return True
        if not self._h:
            return False
        check(lib().ad_fx_graph_process(self._h, ptr(b), b.shape[1]))
        return True

    def process_device(self, d_buf: int, stride: int, n: int, stream: int = 0) -> bool:
        if not self._h:
            return False
        check(lib().ad_fx_graph_process_device(self._h, C.c_void_p(d_buf), int(stride), int(n),
                                               C.c_void_p(stream)))
        return True

    def Reset(self) -> None:
        if self._h:
            check(lib().ad_fx_graph_reset(self._h))

    def close(self):
        self._free()

    def __del__(self):
        try:
            self._free()
        except Exception:
            pass


def _graph_json(nodes, edges):
    return json.dumps({
        "nodes": [{"id": INPUT_NODE_ID, "type": INPUT_NODE_ID}, {"id": OUTPUT_NODE_ID, "type": OUTPUT_NODE_ID}] + nodes,
        "connections": [dict(zip(("from", "to", "fromPortIndex"), e)) for e in edges],
    })


# Example graphs (bench.py --workload fx --graph ...).  config5: BASELINE
# config 5 as an effectchain graph (fuses into one launch); branched: an LR4
# split-freq crossover, a limiter -> compressor low band, an EQ -> Freeverb
# high band and a dry path, averaged at the output.
EXAMPLE_GRAPHS = {
    "config5": _graph_json(
        [{"id": "hp", "type": "filter-highpass", "params": {"freq": 40, "q": 0.707}},
         {"id": "ls", "type": "filter-lowshelf", "params": {"freq": 100, "gain": 3, "q": 0.707}},
         {"id": "pk", "type": "filter-peak", "params": {"freq": 1000, "gain": -2, "q": 1}},
         {"id": "hs", "type": "filter-highshelf", "params": {"freq": 8000, "gain": 2, "q": 0.707}},
         {"id": "lp", "type": "filter-lowpass", "params": {"freq": 18000, "q": 0.707}},
         {"id": "comp", "type": "dyn-compressor", "params": {"thresholdDB": -20, "ratio": 4}},
         {"id": "verb", "type": "reverb-freeverb", "params": {}}],
        [(INPUT_NODE_ID, "hp"), ("hp", "ls"), ("ls", "pk"), ("pk", "hs"), ("hs", "lp"), ("lp", "comp"),
         ("comp", "verb"), ("verb", OUTPUT_NODE_ID)]),
    "branched": _graph_json(
        [{"id": "xo", "type": "split-freq", "params": {"freqHz": 800}},
         {"id": "lim", "type": "dyn-limiter", "params": {"thresholdDB": -6, "releaseMs": 50}},
         {"id": "eq", "type": "filter-peak", "params": {"freq": 3000, "gain": 4, "q": 2}},
         {"id": "verb", "type": "reverb-freeverb", "params": {"wet": 0.5, "roomSize": 0.9}},
         {"id": "comp", "type": "dyn-compressor", "params": {"thresholdDB": -30, "ratio": 3, "kneeDB": 0}}],
        [(INPUT_NODE_ID, "xo"), ("xo", "lim", 0), ("xo", "eq", 1), ("eq", "verb"), (INPUT_NODE_ID, OUTPUT_NODE_ID),
         ("lim", "comp"), ("comp", OUTPUT_NODE_ID), ("verb", OUTPUT_NODE_ID)]),
}
