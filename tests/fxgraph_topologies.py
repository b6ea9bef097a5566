"""The effect-graph topologies of the topology suite (a test helper): a named
set, each graph aimed at one rule of the graph compiler or scheduler
(csrc/capi_fxgraph.cpp), and a seeded family of generated DAGs.  Everything
here is host-side data: JSON graphs for effectchain.Chain.LoadGraph.
"""
import json

import numpy as np

FS = 8000.0
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

# (launches, buffers, streams) where the compiler's decisions are part of the case
NAMED_OPS = {
    "fusion_in_order": (4, 1, 1),     # [f f f comp verb] [f comp] [comp verb] [verb], all on the caller's block
    "fusion_verb_filter": (2, 1, 1),  # a filter after Freeverb is out of stage order
    "fusion_12_filters": (1, 1, 1),   # 12 sections in one op (the chain runs them in passes of 8)
    "fusion_bypassed_comp": (1, 1, 1),
}

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
    return {}


def generate(seed):
    """A DAG of 4-12 nodes behind _input: types from TYPES (one in eight
    bypassed), 0-8 parents drawn from the earlier nodes (a parent may repeat:
    two edges), a port drawn for a split-freq parent; _output mixes the nodes
    nobody reads (the first 8).  Returns (nodes, edges) for graph()."""
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


def has_type(json_graph, *kinds):
    return any(n["type"] in kinds for n in json.loads(json_graph)["nodes"])
