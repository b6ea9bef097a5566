"""Sidechain inputs in the GPU graph runtime: the dyn-lookahead and vocoder
nodes, against the one-channel interpreter of tests/sidechain_ref.py.

Every graph is a JSON graph through effectchain.Chain(sidechain=True).LoadGraph at 48 kHz and
takes three calls of 150, 1 and 97 samples with fresh noise per call and
channel, on 3 and on 65 channels; the interpreter checks channels 0, 1 and the
last.  Graphs whose nodes are all exact (filters, crossovers, mixes, the
vocoder) are compared on the bits; graphs with a limiter or a phaser (log,
exp2, tan of the device library) are held to the limiter's bars, 1e-12 relative
RMS and 1e-10 max abs.
"""
import functools
import json
import math

import numpy as np
import pytest

import fxgraph_topologies as T
import sidechain_ref
from algodsp import design, effectchain as E, signals

pytestmark = pytest.mark.gpu

FS = 48000.0
CALLS = [150, 1, 97]
RMS_BAR, ABS_BAR = 1e-12, 1e-10
IN, OUT = "_input", "_output"
VOC = dict(attackMs=0.3, releaseMs=5.0, inputLevel=0.25, synthLevel=0.5, vocoderLevel=2.0)
LIM = dict(thresholdDB=-14, releaseMs=20, lookaheadMs=0.5)
LOW = dict(freq=700, q=0.8)
HIGH = dict(freq=2500, q=0.7)
node = T.node


def graph(nodes, edges):
    """edges: (from, to), (from, to, fromPortIndex) or (from, to, fromPortIndex, toPortIndex)."""
    return json.dumps({
        "nodes": [{"id": IN, "type": IN}, {"id": OUT, "type": OUT}] + nodes,
        "connections": [dict(zip(("from", "to", "fromPortIndex", "toPortIndex"), e)) for e in edges],
    })


GRAPHS = {
    # no side edge: the side input is the node's own input
    "vocoder_alone": graph([node("v", "vocoder", **VOC)], [(IN, "v"), ("v", OUT)]),
    "limiter_alone": graph([node("l", "dyn-lookahead", **LIM)], [(IN, "l"), ("l", OUT)]),
    # the reference's own case (chain_test.go:570-588): a processed main path, the sidechain on port 1
    "limiter_input_side": graph([node("g", "filter-peak", freq=900, gain=6, q=2), node("l", "dyn-lookahead", **LIM)],
                                [(IN, "g"), ("g", "l"), (IN, "l", 0, 1), ("l", OUT)]),
    # modulator and carrier from two differently filtered branches
    "vocoder_two_branches": graph([node("m", "filter-lowpass", **LOW), node("c", "filter-highpass", **HIGH),
                                   node("v", "vocoder", **VOC)],
                                  [(IN, "m"), (IN, "c"), ("m", "v"), ("c", "v", 0, 1), ("v", OUT)]),
    # two side parents: the edge-order sum times 1/2
    "vocoder_two_sides": graph([node("a", "filter-lowpass", **LOW), node("b", "filter-highpass", **HIGH),
                                node("v", "vocoder", **VOC)],
                               [(IN, "a"), (IN, "b"), (IN, "v"), ("a", "v", 0, 1), ("b", "v", 0, 1), ("v", OUT)]),
    "limiter_two_sides": graph([node("a", "filter-lowpass", **LOW), node("b", "filter-highpass", **HIGH),
                                node("l", "dyn-lookahead", **LIM)],
                               [(IN, "a"), (IN, "b"), (IN, "l"), ("a", "l", 0, 1), ("b", "l", 0, 1), ("l", OUT)]),
    # a side parent that is a split-freq node's high band; the low band is the modulator
    "vocoder_split_high_side": graph([node("x", "split-freq", freqHz=1200), node("v", "vocoder", **VOC)],
                                     [(IN, "x"), ("x", "v", 0, 0), ("x", "v", 1, 1), ("v", OUT)]),
    # bypassed: the main parents' mix alone
    "vocoder_bypassed": graph([node("c", "filter-highpass", **HIGH), node("v", "vocoder", bypassed=True, **VOC)],
                              [(IN, "c"), (IN, "v"), ("c", "v", 0, 1), ("v", OUT)]),
    # the side edge listed before the main edge: the reference loses it from the second block on
    "vocoder_side_edge_first": graph([node("m", "filter-lowpass", **LOW), node("c", "filter-highpass", **HIGH),
                                      node("v", "vocoder", **VOC)],
                                     [(IN, "m"), (IN, "c"), ("c", "v", 0, 1), ("m", "v"), ("v", OUT)]),
    "limiter_side_edge_first": graph([node("g", "filter-peak", freq=900, gain=6, q=2), node("l", "dyn-lookahead", **LIM)],
                                     [(IN, "g"), (IN, "l", 0, 1), ("g", "l"), ("l", OUT)]),
    # P feeds A's main input and B's side input; A is in place and P's only main consumer, so without the side
    # consumer in the count A would take P's buffer over and B would read A's output
    "takeover_vocoder": graph([node("p", "filter-lowpass", **LOW), node("a", "delay-simple", delayMs=1.5),
                               node("b", "vocoder", **VOC)],
                              [(IN, "p"), ("p", "a"), (IN, "b"), ("p", "b", 0, 1), ("a", OUT), ("b", OUT)]),
    "takeover_limiter": graph([node("p", "filter-lowpass", **LOW), node("a", "delay-simple", delayMs=1.5),
                               node("b", "dyn-lookahead", **LIM)],
                              [(IN, "p"), ("p", "a"), (IN, "b"), ("p", "b", 0, 1), ("a", OUT), ("b", OUT)]),
    # toPortIndex 1 on another node type is still a main edge
    "phaser_port_1_is_main": graph([node("c", "filter-highpass", **HIGH), node("ph", "phaser", stages=4, rateHz=2.0)],
                                   [(IN, "c"), (IN, "ph"), ("c", "ph", 0, 1), ("ph", OUT)]),
}
TOLERANCE = {"limiter", "phaser"}  # a graph naming one of these is held to the bars, every other to the bits


def inputs(channels):
    return [np.stack([0.9 * signals.white_noise(n, 0x51DE + 1000 * k + c) for c in channels])
            for k, n in enumerate(CALLS)]


def chain(json_graph, C):
    ch = E.Chain(FS, C, designer=design.RBJDesigner(), sidechain=True)
    ch.LoadGraph(json_graph)
    return ch


@functools.lru_cache(maxsize=None)
def reference(name, c):
    """The interpreter's outputs of the calls for channel c, from Chain.spec of a one-channel chain."""
    ref = sidechain_ref.FxGraph(chain(GRAPHS[name], 1).spec, FS)
    return [ref.process(x[0]) for x in inputs([c])]


def same_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape, what
    bad = np.flatnonzero(got.view(np.int64) != want.view(np.int64))
    assert not bad.size, f"{what}: {bad.size} of {got.size} differ, first at {int(bad[0])}: {got[bad[0]]!r}, {want[bad[0]]!r}"


def within_bars(got, want, what):
    err = got - want
    rms = math.sqrt(float(np.mean(err ** 2))) / max(math.sqrt(float(np.mean(want ** 2))), 1e-300)
    worst = float(np.max(np.abs(err)))
    print(f"{what}: relative rms {rms:.3e}, max abs {worst:.3e}")
    assert rms <= RMS_BAR and worst <= ABS_BAR, (what, rms, worst)


@pytest.mark.parametrize("C", [3, 65])
@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_graph(gpu, name, C):
    ch = chain(GRAPHS[name], C)
    exact = not any(k in name for k in TOLERANCE)
    outs = []
    for x in inputs(range(C)):
        y = x.copy()
        assert ch.Process(y)
        outs.append(y)
    for c in sorted({0, 1, C - 1}):
        for k, want in enumerate(reference(name, c)):
            (same_bits if exact else within_bars)(outs[k][c], want, f"{name}, {C} ch, channel {c}, call {k}")
            assert np.abs(want).max() > 1e-3 or CALLS[k] == 1


def test_specs(gpu):
    """side_parents appears on the two node kinds only, in edge order, with the split's high band as port 1."""
    assert (E.FXN_LOOKAHEAD, E.FXN_VOCODER) == (23, 24)  # AD_FXN_*; 22 stays unassigned
    spec = {d["id"]: d for d in chain(GRAPHS["vocoder_two_sides"], 1).spec}
    ids = [d["id"] for d in chain(GRAPHS["vocoder_two_sides"], 1).spec]
    assert spec["v"]["type"] == "vocoder" and spec["v"]["parents"] == [(0, 0)]
    assert spec["v"]["side_parents"] == [(ids.index("a"), 0), (ids.index("b"), 0)]
    assert all("side_parents" not in d for k, d in spec.items() if k != "v")
    spec = {d["id"]: d for d in chain(GRAPHS["vocoder_split_high_side"], 1).spec}
    assert spec["v"]["parents"] == [(1, 0)] and spec["v"]["side_parents"] == [(1, 1)]
    spec = {d["id"]: d for d in chain(GRAPHS["phaser_port_1_is_main"], 1).spec}
    assert len(spec["ph"]["parents"]) == 2 and "side_parents" not in spec["ph"]
    lim = {d["id"]: d for d in chain(GRAPHS["limiter_input_side"], 1).spec}["l"]
    assert lim["type"] == "lookahead" and lim["side_parents"] == [(0, 0)]
    assert (lim["lookahead"]["threshold_db"], lim["lookahead"]["release_ms"], lim["lookahead"]["lookahead_ms"]) \
        == (-14.0, 20.0, 0.5)
    # the node's clamps (runtime_dynamics.go:100-110, runtime_misc.go:80-100) and defaults
    g = graph([node("l", "dyn-lookahead", thresholdDB=-40, releaseMs=0.1, lookaheadMs=500),
               node("v", "vocoder", attackMs=0.001, releaseMs=5000, inputLevel=-1, synthLevel=20)],
              [(IN, "l"), ("l", "v"), ("v", OUT)])
    spec = {d["id"]: d for d in chain(g, 1).spec}
    assert [spec["l"]["lookahead"][k] for k in ("threshold_db", "release_ms", "lookahead_ms")] == [-24.0, 1.0, 200.0]
    assert [spec["v"]["vocoder"][k] for k in ("attack_ms", "release_ms", "input_level", "synth_level", "vocoder_level")] \
        == [0.01, 1000.0, 0.0, 10.0, 1.0]
    d = {x["id"]: x for x in chain(graph([node("l", "dyn-lookahead")], [(IN, "l"), ("l", OUT)]), 1).spec}["l"]
    assert [d["lookahead"][k] for k in ("threshold_db", "release_ms", "lookahead_ms")] == [-1.0, 100.0, 3.0]


def test_existing_spec_is_unchanged(gpu):
    """A named topology from before: no side_parents key anywhere, the spec the host restatement gives."""
    import fxgraph_ref

    g, fs = T.NAMED["diamond_newer"]
    ch = E.Chain(fs, 1, designer=design.RBJDesigner())
    ch.LoadGraph(g)
    want = fxgraph_ref.host_spec(g, fs, design.RBJDesigner())
    assert len(ch.spec) == len(want)
    for a, b in zip(ch.spec, want):
        assert set(a) == set(b) and "side_parents" not in a
        assert a["id"] == b["id"] and a["type"] == b["type"] and a["parents"] == b["parents"]


def test_takeover_counts_the_side_consumer(gpu):
    """P's buffer has a main and a side consumer: the main one (in place) works on a copy.  Five buffers: the
    caller's block, copies of it for P and for B (the input has two main consumers), a copy of P's for A, and
    the output's mix.  A in P's buffer would be one buffer fewer, and B would read A's output."""
    ops, buffers, _ = chain(GRAPHS["takeover_vocoder"], 3).op_count()
    assert buffers == 5, (ops, buffers)


def test_reset(gpu):
    ch = chain(GRAPHS["limiter_input_side"], 3)
    x = inputs(range(3))[0]
    a, b = x.copy(), x.copy()
    ch.Process(a)
    ch.Reset()
    ch.Process(b)
    same_bits(a, b, "call 1 again after Reset")


def test_off_by_default(gpu):
    """Without sidechain=True both node types are UnknownEffect, as before."""
    for name in ("vocoder_alone", "limiter_input_side"):
        with pytest.raises(E.UnknownEffect):
            E.Chain(FS, 2, designer=design.RBJDesigner()).LoadGraph(GRAPHS[name])


def test_bad_side_lists_are_refused(gpu):
    nine = [node(f"s{i}", "filter-lowpass", freq=300 + 100 * i) for i in range(9)]
    g = graph(nine + [node("v", "vocoder")],
              [(IN, f"s{i}") for i in range(9)] + [(IN, "v")] + [(f"s{i}", "v", 0, 1) for i in range(9)] + [("v", OUT)])
    with pytest.raises(E.UnknownEffect):
        chain(g, 1)
