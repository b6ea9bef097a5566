"""The effect-graph topologies of the topology suite (a test helper): a named
set, each graph aimed at one rule of the graph compiler or scheduler
(csrc/capi_fxgraph.cpp), and a seeded family of generated DAGs.  Everything
here is host-side data: JSON graphs for effectchain.Chain.LoadGraph.

Two generated families.  The first (TYPES, SEEDS, generate(seed)) was drawn
before the distortion, dist-cheb, bitcrusher, dyn-deesser and dyn-transient
nodes existed; appending to TYPES would re-draw every one of its graphs, so it
stays as it is (tests/test_fxgraph_ref.py pins a digest of each graph).  The
second (TYPES2, SEEDS2, generate(seed, family=2)) draws from the old types and
the five newer ones with a random stream of its own.  It runs at 48 kHz, as
every graph with a de-esser does: NewDeEsser(fs) carries 6 kHz, which has to
be under Nyquist, so such a node cannot be built at the suite's 8 kHz.

The quantiser rule.  The bit crusher's quantiser round(x q) / q is a jump: a
last-place difference in its input can move a sample by a whole step 1 / q,
which is a correct result and far outside the suite's 1e-10 bar.  So in the
named and the generated graphs every node upstream of a bitcrusher is of a kind
the GPU reproduces on the bits (exact_node), and the generator re-draws the
type otherwise.  The distortion modes were read for the same reason
(tests/shaper_ref.py shapeSample): every one of the fifteen transfers is
continuous (the branches of softclip, hardclip, the tanh polynomial and the
clamps meet at their boundaries, waveshaper8's copysign meets at 0), so none of
them needs the rule.  Where a graph is compared on the bits the bit depth is a
whole number, for which quantLevels = 2^(depth - 1) is exact; a fractional
depth (exp2 of a C library) appears only in fanin_newer, a tolerance graph,
and there the GPU suite first compares the device's quantLevels with the
restatement's and hands the device's over if they differ.
"""
import json

import numpy as np

import shaper_ref

FS = 8000.0
FS2 = 48000.0  # the rate of every graph with a de-esser, and of the second family
IN, OUT = "_input", "_output"


def graph(nodes, edges):
    return json.dumps({
        "nodes": [{"id": IN, "type": IN}, {"id": OUT, "type": OUT}] + nodes,
        "connections": [dict(zip(("from", "to", "fromPortIndex"), e)) for e in edges],
    })


def node(id_, type_, bypassed=False, **params):
    d = {"id": id_, "type": type_, "params": params}
    if bypassed:
        d["bypassed"] = True
    return d


def line(nodes, extra=()):
    ids = [IN] + [n["id"] for n in nodes] + [OUT]
    return graph(nodes, list(zip(ids[:-1], ids[1:])) + list(extra))


PHASER12 = dict(stages=12, rateHz=3.0, minFreqHz=100, maxFreqHz=3000, feedback=0.6, mix=0.8)
FDN = dict(wet=0.4, rt60=0.9, preDelay=0.004, damp=0.6, modDepth=0.002, modRate=0.8)
COMP = dict(thresholdDB=-24, ratio=4, attackMs=2, releaseMs=40)
VERB = dict(wet=0.4, roomSize=0.8)

# one node per branch, all of different types (fanin8; lanes12 adds four)
BRANCHES = [
    node("b0", "filter-peak", freq=900, gain=6, q=2),
    node("b1", "dyn-compressor", **COMP),
    node("b2", "reverb-freeverb", **VERB),
    node("b3", "reverb-fdn", **FDN),
    node("b4", "delay", time=0.01, feedback=0.5, mix=0.5),
    node("b5", "flanger", rateHz=2.0, depth=0.002, feedback=-0.5),
    node("b6", "phaser", stages=4, rateHz=2.0),
    node("b7", "ringmod", carrierHz=700, mix=0.7),
    node("b8", "tremolo", rateHz=9, depth=0.8),
    node("b9", "delay-simple", delayMs=3.5),
    node("b10", "dyn-limiter", thresholdDB=-9, releaseMs=30),
    node("b11", "filter-highpass", freq=400, q=0.9),
]


def _fusion_in_order():
    kinds = ["filter-peak", "filter-lowshelf", "filter-highpass", "dyn-compressor", "reverb-freeverb", "filter-peak",
             "dyn-compressor", "dyn-compressor", "reverb-freeverb", "reverb-freeverb"]
    params = [dict(freq=900, gain=5, q=2), dict(freq=200, gain=3), dict(freq=80), COMP, VERB, dict(freq=2000, gain=-4),
              dict(thresholdDB=-30, ratio=2), dict(thresholdDB=-12, ratio=8, releaseMs=20), dict(wet=0.3, roomSize=0.5),
              dict(wet=0.6, damp=0.2)]
    return line([node(f"n{i}", k, **p) for i, (k, p) in enumerate(zip(kinds, params))])


# name -> (json graph, sample rate); NAMED_OPS: name -> expected Chain.op_count()
NAMED = {
    # A's buffer feeds B (in place) and the output's mix: B must work on a copy
    "diamond": (graph([node("A", "phaser", stages=4, rateHz=2.0), node("B", "delay", time=0.01, feedback=0.5, mix=1.0)],
                      [(IN, "A"), ("A", "B"), ("A", OUT), ("B", OUT)]), FS),
    "fanin8": (graph(BRANCHES[:8] + [node("s", "sum")],
                     [(IN, f"b{i}") for i in range(8)] + [(f"b{i}", "s") for i in range(8)] + [("s", OUT)]), FS),
    # 12 concurrent branches on 8 streams: the scheduler's i % kLanes fallback
    "lanes12": (graph(BRANCHES + [node("s8", "sum"), node("s4", "sum")],
                      [(IN, f"b{i}") for i in range(12)] + [(f"b{i}", "s8") for i in range(8)]
                      + [(f"b{i}", "s4") for i in range(8, 12)] + [("s8", OUT), ("s4", OUT)]), FS),
    # three bands, three node types; the upper band has two consumers
    "nested_split": (graph([node("xo1", "split-freq", freqHz=1200), node("xo2", "split-freq", freqHz=300),
                            node("lo", "flanger", rateHz=2.0, depth=0.002), node("mid", "reverb-freeverb", **VERB),
                            node("hi", "delay", time=0.005, feedback=0.3, mix=0.5),
                            node("hi2", "tremolo", rateHz=9, depth=0.8), node("s", "sum")],
                           [(IN, "xo1"), ("xo1", "xo2", 0), ("xo2", "lo", 0), ("xo2", "mid", 1), ("xo1", "hi", 1),
                            ("xo1", "hi2", 1), ("lo", "s"), ("mid", "s"), ("hi", "s"), ("hi2", "s"), ("s", OUT)]), FS),
    "same_port_twice": (graph([node("xo", "split-freq", freqHz=700)],
                              [(IN, "xo"), ("xo", OUT, 0), ("xo", OUT, 0), ("xo", OUT, 1)]), FS),
    # fusion boundaries of the chain kernel's stage order (sections, one dynamics stage, one Freeverb)
    "fusion_in_order": (_fusion_in_order(), FS),
    "fusion_verb_filter": (line([node("v", "reverb-freeverb", **VERB), node("f", "filter-peak", freq=900, gain=5)]), FS),
    "fusion_12_filters": (line([node(f"f{i}", "filter-peak", freq=150.0 * (i + 1), gain=(-1) ** i * 3.0, q=1.5)
                                for i in range(12)]), FS),
    "fusion_bypassed_comp": (line([node("f0", "filter-peak", freq=900, gain=5),
                                   node("c", "dyn-compressor", bypassed=True, ratio=10),
                                   node("f1", "filter-lowshelf", freq=200, gain=3)]), FS),
    "every_node_line": (line([
        node("f", "filter-peak", freq=900, gain=4, q=2), node("c", "dyn-compressor", **COMP),
        node("l", "dyn-limiter", thresholdDB=-9, releaseMs=30),
        node("e", "dyn-expander", thresholdDB=-30, ratio=3, rangeDB=-30, detector="rms"),
        node("g", "dyn-gate", thresholdDB=-34, holdMs=5, releaseMs=20), node("v", "reverb-freeverb", **VERB),
        node("r", "reverb-fdn", **FDN), node("cv", "reverb-conv", irIndex=1, wet=0.4),
        node("d", "delay", time=0.01, feedback=0.5, mix=0.5), node("ds", "delay-simple", delayMs=3.5),
        node("fl", "flanger", rateHz=2.0, depth=0.002, feedback=-0.5), node("p", "phaser", stages=4, rateHz=2.0),
        node("t", "tremolo", rateHz=9, depth=0.8), node("rm", "ringmod", carrierHz=700, mix=0.7),
        node("sp", "split"), node("xo", "split-freq", freqHz=900), node("sm", "sum")], [(IN, OUT)]), FS),
    # nodes without parents process zeros, keep state, and join the signal path's mix
    "orphans": (graph([node("v", "reverb-freeverb", **VERB), node("rm", "ringmod", carrierHz=700),
                       node("t", "tremolo", rateHz=9), node("f", "filter-peak", freq=900, gain=4), node("s", "sum")],
                      [(IN, "f"), ("v", "s"), ("f", "s"), ("rm", "s"), ("t", "s"), ("s", OUT)]), FS),
    # a 10 Hz highpass at 192 kHz: the chain's noise guard refuses the time-parallel engine, and the
    # staged engine is off in a graph with two streams
    "guarded_branch": (graph([node("hp", "filter-highpass", freq=10, q=0.707), node("c", "dyn-compressor", **COMP),
                              node("d", "delay-simple", delayMs=1.0)],
                             [(IN, "hp"), ("hp", "c"), (IN, "d"), ("c", OUT), ("d", OUT)]), 192000.0),
    # a long branch and a bare copy meet in a mix that is then overwritten in place
    "heavy_vs_light": (graph([node("p", "phaser", **PHASER12), node("r", "reverb-fdn", **FDN), node("cp", "split"),
                              node("m", "sum"), node("t", "tremolo", rateHz=9, depth=0.8)],
                             [(IN, "p"), ("p", "r"), (IN, "cp"), ("r", "m"), ("cp", "m"), ("m", "t"), ("t", OUT)]), FS),
}

# ---- the distortion, dist-cheb, bitcrusher, dyn-deesser and dyn-transient nodes ----
W16 = dict(zip((f"w{k + 1}" for k in range(16)),
               [0.5, -0.25, 0.125, 0.3, -0.2, 0.1, 0.05, -0.05, 0.02, 0.01, -0.01, 0.03, 0.002, -0.004, 0.001, 0.0005]))
HARDCLIP = dict(mode="hardclip", drive=2.0, clip=0.3)
TANH = dict(mode="tanh", drive=2.0, mix=0.8)
CHEB_DC = dict(order=4, w1=0.5, w2=-0.3, w3=0.2, w4=0.4, dcBypass=1, drive=2.2)
DEESS_SPLIT = dict(freqHz=6000, q=1.5, thresholdDB=-18, ratio=6, releaseMs=1.5, mode="splitband", detector="bandpass")
DEESS_WIDE = dict(freqHz=7000, thresholdDB=-22, ratio=4, releaseMs=2.0, mode="wideband", detector="highpass",
                  filterOrder=3)
TRANSIENT = dict(attack=0.6, sustain=-0.4, attackMs=1.0, releaseMs=20.0)

NEWER_BRANCHES = [
    node("b0", "distortion", **HARDCLIP),
    node("b1", "distortion", **TANH),
    node("b2", "dist-cheb", order=16, gain=1.5, drive=2.2, **W16),
    node("b3", "dist-cheb", order=3, dcBypass=1, drive=2.2),
    node("b4", "bitcrusher", bitDepth=4, downsample=1),
    node("b5", "bitcrusher", bitDepth=5.5, downsample=5, mix=0.75),  # the one fractional depth: a tolerance graph
    node("b6", "dyn-deesser", **DEESS_SPLIT),
    node("b7", "dyn-deesser", listen=1, **DEESS_WIDE),
    node("b8", "dyn-transient", **TRANSIENT),
    node("b9", "dyn-compressor", **COMP),
    node("b10", "phaser", stages=4, rateHz=2.0),
]

NAMED.update({
    # all five newer node types on one line: state across the calls (counter and hold value, DC states, envelopes)
    "newer_nodes_line": (line([
        node("bc", "bitcrusher", bitDepth=6, downsample=3), node("tr", "dyn-transient", **TRANSIENT),
        node("ws", "distortion", mode="waveshaper2", drive=2.5, shape=0.7, bias=0.05, mix=0.9),
        node("ch", "dist-cheb", **CHEB_DC), node("de", "dyn-deesser", **dict(DEESS_SPLIT, thresholdDB=-12)),
        node("dw", "dyn-deesser", **dict(DEESS_WIDE, thresholdDB=-10)), node("th", "distortion", **TANH)]), FS2),
    # 11 concurrent branches of the newer handles on 8 streams: the i % kLanes fallback, scratch that grows on a lane
    "fanin_newer": (graph(NEWER_BRANCHES + [node("s8", "sum"), node("s3", "sum")],
                          [(IN, f"b{i}") for i in range(11)] + [(f"b{i}", "s8") for i in range(8)]
                          + [(f"b{i}", "s3") for i in range(8, 11)] + [("s8", OUT), ("s3", OUT)]), FS2),
    # two diamonds: A and A' feed B and B' (in place) and the output's mix, so B and B' must work on copies
    "diamond_newer": (graph([node("A", "bitcrusher", bitDepth=5, downsample=4), node("B", "dist-cheb", **CHEB_DC),
                             node("A2", "dyn-transient", **TRANSIENT), node("B2", "dyn-deesser", **DEESS_SPLIT)],
                            [(IN, "A"), ("A", "B"), ("A", OUT), ("B", OUT), (IN, "A2"), ("A2", "B2"), ("A2", OUT),
                             ("B2", OUT)]), FS2),
    # a crossover (exact) whose high band has two consumers, a de-esser and a bit crusher; the low band's is in place
    "bands_newer": (graph([node("xo", "split-freq", freqHz=2500), node("lo", "dyn-transient", **TRANSIENT),
                           node("hi", "dyn-deesser", **dict(DEESS_SPLIT, q=3.0)),
                           node("hi2", "bitcrusher", bitDepth=7, downsample=2), node("s", "sum")],
                          [(IN, "xo"), ("xo", "lo", 0), ("xo", "hi", 1), ("xo", "hi2", 1), ("lo", "s"), ("hi", "s"),
                           ("hi2", "s"), ("s", OUT)]), FS2),
    # parentless newer nodes process zeros: a bias gives a constant, T4(0) = 1 decays through the DC bypass, the
    # de-esser takes the gain of a zero level
    "orphans_newer": (graph([node("d", "distortion", mode="hardclip", drive=2.0, clip=0.8, bias=0.25),
                             node("c", "dist-cheb", order=4, dcBypass=1), node("b", "bitcrusher", bitDepth=3, downsample=2),
                             node("de", "dyn-deesser", **DEESS_SPLIT), node("t", "dyn-transient", **TRANSIENT),
                             node("f", "filter-peak", freq=900, gain=4), node("s", "sum")],
                            [(IN, "f"), ("d", "s"), ("f", "s"), ("c", "s"), ("b", "s"), ("de", "s"), ("t", "s"),
                             ("s", OUT)]), FS2),
    # a distortion is no chain stage: the open group is flushed before it, and a new one opens after it
    "fusion_newer": (line([node("f0", "filter-peak", freq=900, gain=5), node("d", "distortion", **HARDCLIP),
                           node("f1", "filter-lowshelf", freq=200, gain=3)]), FS),
    # bypassed newer nodes only mix: the two filters around them still fuse
    "fusion_bypassed_newer": (line([node("f0", "filter-peak", freq=900, gain=5),
                                    node("de", "dyn-deesser", bypassed=True, **DEESS_SPLIT),
                                    node("bc", "bitcrusher", bypassed=True, bitDepth=4, downsample=3),
                                    node("f1", "filter-lowshelf", freq=200, gain=3)]), FS2),
})
NEWER = [k for k in NAMED if k.endswith("_newer") or k == "newer_nodes_line"]

# (launches, buffers, streams) where the compiler's decisions are part of the case
NAMED_OPS = {
    "fusion_in_order": (4, 1, 1),     # [f f f comp verb] [f comp] [comp verb] [verb], all on the caller's block
    "fusion_verb_filter": (2, 1, 1),  # a filter after Freeverb is out of stage order
    "fusion_12_filters": (1, 1, 1),   # 12 sections in one op (the chain runs them in passes of 8)
    "fusion_bypassed_comp": (1, 1, 1),
    "fusion_newer": (3, 1, 1),           # [f] [distortion] [f]: compile() flushes the open group before the op
    "fusion_bypassed_newer": (1, 1, 1),  # a bypassed node takes its parent's buffer over and adds no op
}
# diamond_newer's (launches, buffers): the input has two consumers, so A works on a copy of it (buffer 1), and A's
# buffer has two, so B works on a copy of that (buffer 2): copy, A, copy, B; the same four ops on buffers 3 and 4 for
# A' and B'; the output's mix of the four into buffer 5 and its copy into the caller's block (buffer 0).  B in A's
# buffer would be 8 launches and 4 buffers.
DIAMOND_NEWER_OPS = (10, 6)

# ---- the generated family ----------------------------------------------------
# JSON node types and their weights (reverb-conv costs an FFT tolerance, so it is drawn less often)
TYPES = ["filter-peak", "filter-lowpass", "filter-highshelf", "dyn-compressor", "dyn-limiter", "dyn-gate",
         "dyn-expander", "reverb-freeverb", "reverb-fdn", "reverb-conv", "delay", "delay-simple", "flanger", "phaser",
         "tremolo", "ringmod", "split-freq", "split", "sum"]
WEIGHTS = np.array([1.0 if t != "reverb-conv" else 0.35 for t in TYPES])
FANIN = ([0, 1, 2, 3, 5, 6, 8], [0.06, 0.52, 0.2, 0.1, 0.05, 0.04, 0.03])
SEEDS = list(range(1, 25))


def _params(t, rng):
    u = rng.uniform
    if t.startswith("filter"):
        return dict(freq=float(u(100, 3000)), gain=float(u(-9, 9)), q=float(u(0.5, 3)))
    if t == "dyn-compressor":
        return dict(thresholdDB=float(u(-36, -12)), ratio=float(u(2, 8)), attackMs=float(u(0.5, 10)),
                    releaseMs=float(u(10, 100)))
    if t == "dyn-limiter":
        return dict(thresholdDB=float(u(-18, -3)), releaseMs=float(u(10, 100)))
    if t == "dyn-gate":
        return dict(thresholdDB=float(u(-40, -25)), holdMs=float(u(0, 10)), releaseMs=float(u(10, 50)))
    if t == "dyn-expander":
        return dict(thresholdDB=float(u(-36, -24)), ratio=float(u(2, 5)), rangeDB=float(u(-50, -20)),
                    detector=str(rng.choice(["peak", "rms"])), topology=str(rng.choice(["feedforward", "feedback"])))
    if t == "reverb-freeverb":
        return dict(wet=float(u(0.2, 0.8)), roomSize=float(u(0.3, 0.95)), damp=float(u(0.1, 0.9)))
    if t == "reverb-fdn":
        return dict(wet=float(u(0.2, 0.8)), rt60=float(u(0.3, 1.5)), preDelay=float(u(0, 0.01)), damp=float(u(0, 0.9)),
                    modDepth=float(u(0, 0.003)), modRate=float(u(0.1, 1)))
    if t == "reverb-conv":
        return dict(irIndex=1, wet=float(u(0.2, 0.6)))
    if t == "delay":
        return dict(time=float(u(0.002, 0.1)), feedback=float(u(0, 0.8)), mix=float(u(0.2, 1)))
    if t == "delay-simple":
        return dict(delayMs=float(u(0.2, 40)))
    if t == "flanger":
        return dict(rateHz=float(u(0.2, 5)), baseDelay=float(u(0.0005, 0.004)), depth=float(u(0, 0.003)),
                    feedback=float(u(-0.8, 0.8)), mix=float(u(0.2, 1)))
    if t == "phaser":
        return dict(stages=int(rng.integers(1, 13)), rateHz=float(u(0.2, 5)), minFreqHz=float(u(50, 500)),
                    maxFreqHz=float(u(800, 3500)), feedback=float(u(-0.8, 0.8)), mix=float(u(0.2, 1)))
    if t == "tremolo":
        return dict(rateHz=float(u(1, 15)), depth=float(u(0.2, 1)), smoothingMs=float(u(0, 20)))
    if t == "ringmod":
        return dict(carrierHz=float(u(50, 2000)), mix=float(u(0.2, 1)))
    if t == "split-freq":
        return dict(freqHz=float(u(300, 2500)))
    # the second family's types; a de-esser's release is short against the bursts of the suite's input (the
    # reference's releaseMs is a half-life), and a bit depth is a whole number: the graph may be compared on the bits
    if t == "distortion":
        # drive / clip, the steepest slope of a transfer, stays at 10: a last-place difference of a device-library
        # function upstream is multiplied by it, and three distortions in a row must leave room under 1e-12
        return dict(mode=str(rng.choice(shaper_ref.MODES[:-1])), approx=str(rng.choice(["exact", "polynomial"])),
                    drive=float(u(0.5, 3)), mix=float(u(0.3, 1)), output=float(u(0.5, 1.5)), clip=float(u(0.3, 0.8)),
                    shape=float(u(0, 1)), bias=float(rng.choice([0.0, u(-0.3, 0.3)])))
    if t == "dist-cheb":
        order = int(rng.integers(1, 17))
        d = dict(order=order, harmonic=str(rng.choice(["all", "odd", "even"])), gain=float(u(0.3, 1.5)),
                 invert=int(rng.integers(0, 2)), dcBypass=int(rng.integers(0, 2)), drive=float(u(0.5, 2)),
                 mix=float(u(0.3, 1)))
        if rng.integers(0, 2):
            d.update({f"w{k + 1}": float(u(-0.5, 0.5)) for k in range(order)})
        return d
    if t == "bitcrusher":
        return dict(bitDepth=int(rng.integers(2, 13)), downsample=int(rng.integers(1, 10)), mix=float(u(0.3, 1)))
    if t == "dyn-deesser":
        return dict(freqHz=float(u(3000, 9000)), q=float(u(0.5, 4)), thresholdDB=float(u(-45, -25)), ratio=float(u(2, 10)),
                    kneeDB=float(rng.choice([0.0, u(0, 12)])), attackMs=float(u(0.05, 2)), releaseMs=float(u(1, 6)),
                    rangeDB=float(u(-40, -6)), mode=str(rng.choice(["splitband", "wideband"])),
                    detector=str(rng.choice(["bandpass", "highpass"])), filterOrder=int(rng.integers(1, 5)),
                    listen=int(rng.integers(0, 4) == 0))
    if t == "dyn-transient":
        return dict(attack=float(u(-1, 1)), sustain=float(u(-1, 1)), attackMs=float(u(0.1, 20)), releaseMs=float(u(1, 200)))
    return {}


# the JSON types whose GPU node is the reference's on the bits whatever its parameters
EXACT_TYPES = {"split-freq", "split", "sum", "reverb-freeverb", "delay", "delay-simple", "dist-cheb", "dyn-transient"}


def exact_node(n):
    """Whether the GPU reproduces this node of graph() on the bits: by type, and by configuration for the newer
    ones (tests/test_shaper_gpu.py and test_dynfx_gpu.py: which comparisons there are on the bits against the pure
    restatement).  A bypassed node only mixes."""
    t, p = n["type"], n.get("params", {})
    if n.get("bypassed") or t.startswith("filter") or t in EXACT_TYPES:
        return True
    if t == "distortion":
        mode = p.get("mode", "softclip") if p.get("mode", "softclip") in shaper_ref.MODES else "softclip"
        return mode in shaper_ref.ALGEBRAIC or (mode in shaper_ref.POLY_ALGEBRAIC and p.get("approx") == "polynomial")
    if t == "bitcrusher":
        return float(p.get("bitDepth", 8)) == int(p.get("bitDepth", 8))
    if t == "dyn-deesser":
        return p.get("listen", 0) >= 0.5
    return False


def upstream(id_, edges):
    """The ids of every node from which id_ can be reached."""
    seen, todo = set(), [id_]
    while todo:
        at = todo.pop()
        for f, t, _ in edges:
            if t == at and f not in seen:
                seen.add(f)
                todo.append(f)
    return seen


TYPES2 = TYPES + ["distortion", "dist-cheb", "bitcrusher", "dyn-deesser", "dyn-transient"]
# the newer types are what the second family is for; the older ones are company
WEIGHTS2 = np.array([0.35 if t == "reverb-conv" else (2.5 if t in TYPES2[len(TYPES):] else 1.0) for t in TYPES2])
# chosen so that tests/test_fxgraph_ref.py's coverage of the second family holds
SEEDS2 = list(range(1, 15)) + [17, 44, 52, 89, 90, 105, 146, 172, 201, 206]


def _generate2(seed):
    """generate() for the second family: TYPES2 with a stream of its own.  The parents are drawn before the type,
    so that a bitcrusher is re-drawn until everything upstream of the node is exact (the quantiser rule)."""
    rng = np.random.default_rng([seed, 0x2F])
    n = int(rng.integers(4, 13))
    ids, types, nodes, edges = [IN], [IN], [], []
    for i in range(n):
        k = min(int(rng.choice(FANIN[0], p=FANIN[1])), 8)
        if i == 0:
            k = max(k, 1)
        w = np.arange(1, len(ids) + 1, dtype=float) ** 2
        mine = [(ids[p], f"n{i}", int(rng.integers(0, 2)) if types[p] == "split-freq" else 0)
                for p in rng.choice(len(ids), size=k, p=w / w.sum())]
        edges += mine
        by_id = {m["id"]: m for m in nodes}
        clean = all(exact_node(by_id[a]) for a in upstream(f"n{i}", edges) if a != IN)
        t = "bitcrusher"
        while t == "bitcrusher":
            t = str(rng.choice(TYPES2, p=WEIGHTS2 / WEIGHTS2.sum()))
            if clean:
                break
        nodes.append(node(f"n{i}", t, bypassed=bool(rng.integers(0, 8) == 0), **_params(t, rng)))
        ids.append(f"n{i}")
        types.append(t)
    read = {e[0] for e in edges}
    sinks = [i for i in ids[1:] if i not in read][:8]
    for s in sinks:
        edges.append((s, OUT, int(rng.integers(0, 2)) if types[ids.index(s)] == "split-freq" else 0))
    return nodes, edges


def generate(seed, family=1):
    """A DAG of 4-12 nodes behind _input: types from TYPES (one in eight
    bypassed), 0-8 parents drawn from the earlier nodes (a parent may repeat:
    two edges), a port drawn for a split-freq parent; _output mixes the nodes
    nobody reads (the first 8).  Returns (nodes, edges) for graph().  Family 2
    draws from TYPES2 (_generate2); its graphs run at FS2."""
    if family == 2:
        return _generate2(seed)
    rng = np.random.default_rng(seed)
    n = int(rng.integers(4, 13))
    ids, types, nodes, edges = [IN], [IN], [], []
    for i in range(n):
        t = str(rng.choice(TYPES, p=WEIGHTS / WEIGHTS.sum()))
        k = min(int(rng.choice(FANIN[0], p=FANIN[1])), 8)
        if i == 0:
            k = max(k, 1)
        # mostly recent nodes, so that paths get long
        w = np.arange(1, len(ids) + 1, dtype=float) ** 2
        for p in rng.choice(len(ids), size=k, p=w / w.sum()):
            edges.append((ids[p], f"n{i}", int(rng.integers(0, 2)) if types[p] == "split-freq" else 0))
        nodes.append(node(f"n{i}", t, bypassed=bool(rng.integers(0, 8) == 0), **_params(t, rng)))
        ids.append(f"n{i}")
        types.append(t)
    read = {e[0] for e in edges}
    sinks = [i for i in ids[1:] if i not in read][:8]
    for s in sinks:
        edges.append((s, OUT, int(rng.integers(0, 2)) if types[ids.index(s)] == "split-freq" else 0))
    return nodes, edges


def coverage(nodes, edges):
    """What a graph of generate() exercises: (type counts, bypassed count, the
    fan-ins, has a split band with two or more consumers, has a diamond).  A
    diamond: a node or band whose consumers include a node that processes in
    place and another node downstream of that one."""
    types = {n["id"]: n["type"] for n in nodes}
    byp = {n["id"] for n in nodes if n.get("bypassed")}
    counts = {}
    for n in nodes:
        counts[n["type"]] = counts.get(n["type"], 0) + 1
    fanin, cons, out = {}, {}, {}
    for f, t, port in edges:
        fanin[t] = fanin.get(t, 0) + 1
        cons.setdefault((f, port), []).append(t)
        out.setdefault(f, set()).add(t)
    band = any(types.get(f) == "split-freq" and len(c) >= 2 for (f, _), c in cons.items())

    def reach(a):
        seen, todo = set(), [a]
        while todo:
            for c in out.get(todo.pop(), ()):
                if c not in seen:
                    seen.add(c)
                    todo.append(c)
        return seen

    in_place = lambda b: b in types and b not in byp and types[b] not in ("split", "sum", "split-freq")
    diamond = any(in_place(b) and fanin[b] == 1 and any(m != b and m in reach(b) for m in c)
                  for c in cons.values() for b in c)
    return counts, len(byp), sorted(set(fanin.values())), band, diamond


def coverage_by_type(nodes, edges):
    """Of a graph of generate(): (the types of the running nodes with two or more parents, the types of the
    in-place consumers in its diamonds (coverage's definition), the types of the bypassed nodes)."""
    types = {n["id"]: n["type"] for n in nodes}
    byp = {n["id"] for n in nodes if n.get("bypassed")}
    fanin, cons, out = {}, {}, {}
    for f, t, port in edges:
        fanin[t] = fanin.get(t, 0) + 1
        cons.setdefault((f, port), []).append(t)
        out.setdefault(f, set()).add(t)

    def reach(a):
        seen, todo = set(), [a]
        while todo:
            for c in out.get(todo.pop(), ()):
                if c not in seen:
                    seen.add(c)
                    todo.append(c)
        return seen

    in_place = lambda b: b in types and b not in byp and types[b] not in ("split", "sum", "split-freq")
    many = {types[b] for b, k in fanin.items() if b in types and b not in byp and k >= 2}
    diamond = {types[b] for c in cons.values() for b in c
               if in_place(b) and fanin[b] == 1 and any(m != b and m in reach(b) for m in c)}
    return many, diamond, {types[b] for b in byp}


def has_type(json_graph, *kinds):
    return any(n["type"] in kinds for n in json.loads(json_graph)["nodes"])
