"""The pitch-time node in effect graphs: Chain(pitch_time=True) compiles it to
AD_FXN_PITCHTIME, and the graph's output equals, on bits, the reference
interpreter of tests/fxgraph_ref.py with tests/pitchtime_ref.py as the node's
runtime.  Without the keyword the node stays UnknownEffect, and a raw node of
the type with a missing, mis-sized or refused config is AD_ERR_INVALID_ARGUMENT.
"""
import ctypes as C

import numpy as np
import pytest

import fxgraph_ref
import pitchtime_ref as R
from algodsp import _lib, design, effectchain as E, pitch

pytestmark = pytest.mark.gpu

FS = 8000.0
NODE = {"id": "p", "type": "pitch-time", "params": {"semitones": 7, "sequence": 20, "overlap": 4, "search": 2}}


class Graph(fxgraph_ref.FxGraph):
    def node_runtime(self, d):
        if d["type"] != "pitchtime":
            return super().node_runtime(d)
        c = d["pitchtime"]
        r = R.PitchShifter(c["sample_rate"])
        r.SetSequence(c["sequence_ms"]), r.SetOverlap(c["overlap_ms"]), r.SetSearch(c["search_ms"])
        r.SetPitchRatio(c["pitch_ratio"])
        return ["pitchtime", lambda block: r.Process(np.asarray(block, dtype=np.float64)), r.Reset]


def noise(channels, n, seed):
    return 0.5 * np.random.default_rng(seed).standard_normal((channels, n))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def run_both(graph, x):
    ch = E.Chain(FS, x.shape[0], designer=design.RBJDesigner(), pitch_time=True)
    ch.LoadGraph(graph)
    got = x.copy()
    assert ch.Process(got)
    want = np.stack([Graph(ch.spec, FS).process(row) for row in x])
    return ch, got, want


def test_linear_graph(gpu):
    graph = E._graph_json([NODE], [(E.INPUT_NODE_ID, "p"), ("p", E.OUTPUT_NODE_ID)])
    x = noise(3, 2000, 1)
    ch, got, want = run_both(graph, x)
    assert [d["type"] for d in ch.spec] == ["input", "pitchtime", "output"]
    assert ch.spec[1]["pitchtime"]["pitch_ratio"] == 2.0 ** (7 / 12.0) == pitch.PitchShifter._semitone_ratio(7)
    assert np.array_equal(bits(got), bits(want))
    direct = pitch.PitchShifter(FS, 3, semitones=7, sequence_ms=20, overlap_ms=4, search_ms=2).Process(x)
    assert np.array_equal(bits(got), bits(direct))


def test_diamond_with_a_lowpass_branch(gpu):
    graph = E._graph_json(
        [NODE, {"id": "lp", "type": "filter-lowpass", "params": {"freq": 900, "q": 0.707}}],
        [(E.INPUT_NODE_ID, "p"), (E.INPUT_NODE_ID, "lp"), ("p", E.OUTPUT_NODE_ID), ("lp", E.OUTPUT_NODE_ID)])
    x = noise(2, 1800, 2)
    ch, got, want = run_both(graph, x)
    assert np.array_equal(bits(got), bits(want))
    # by hand: the output is (pitch + lowpass) * 0.5 in edge order
    r = R.PitchShifter(FS)
    r.SetSequence(20), r.SetOverlap(4), r.SetSearch(2), r.SetPitchSemitones(7)
    lp_only = E.Chain(FS, 2, designer=ch.designer)
    lp_only.LoadGraph(E._graph_json([{"id": "lp", "type": "filter-lowpass", "params": {"freq": 900, "q": 0.707}}],
                                    [(E.INPUT_NODE_ID, "lp"), ("lp", E.OUTPUT_NODE_ID)]))
    low = x.copy()
    lp_only.Process(low)
    hand = np.stack([((np.zeros(1800) + r.Process(x[c])) + low[c]) * 0.5 for c in range(2)])
    assert np.array_equal(bits(got), bits(hand))


def test_bypassed_node_is_a_pass_through(gpu):
    node = dict(NODE, bypassed=True)
    graph = E._graph_json([node], [(E.INPUT_NODE_ID, "p"), ("p", E.OUTPUT_NODE_ID)])
    x = noise(2, 700, 3)
    _, got, _ = run_both(graph, x)
    assert np.array_equal(bits(got), bits(x))


def test_chain_without_the_keyword_refuses(gpu):
    graph = E._graph_json([NODE], [(E.INPUT_NODE_ID, "p"), ("p", E.OUTPUT_NODE_ID)])
    for kw in ({}, {"sidechain": True}):
        with pytest.raises(E.UnknownEffect):
            E.Chain(FS, 2, **kw).LoadGraph(graph)


def raw_create(config, size):
    nodes = (E._Node * 3)()
    cfgs = (_lib.FxNodeCfg * 3)()
    parents = [(C.c_int32 * 1)(0), (C.c_int32 * 1)(1)]
    nodes[0].type, nodes[1].type, nodes[2].type = E.FXN_INPUT, E.FXN_PITCHTIME, E.FXN_OUTPUT
    for k in (1, 2):
        nodes[k].n_parents = 1
        nodes[k].parents = C.cast(parents[k - 1], C.POINTER(C.c_int32))
    if config is not None:
        cfgs[1].config, cfgs[1].bytes = C.addressof(config), size
    h = C.c_void_p()
    rc = _lib.lib().ad_fx_graph_create_cfg(C.cast(nodes, C.c_void_p), None, C.cast(cfgs, C.c_void_p), 3, 2, 0,
                                           C.byref(h))
    if h:
        _lib.lib().ad_fx_graph_destroy(h)
    return rc


def test_raw_node_config_errors(gpu):
    good, table = pitch.make_config(FS, 1.5, 20.0, 4.0, 2.0)
    size = C.sizeof(good)
    assert raw_create(good, size) == _lib.AD_OK
    assert raw_create(None, 0) == _lib.AD_ERR_INVALID_ARGUMENT
    assert raw_create(good, size - 8) == _lib.AD_ERR_INVALID_ARGUMENT
    assert raw_create(good, size + 8) == _lib.AD_ERR_INVALID_ARGUMENT
    for field, value in (("pitch_ratio", 5.0), ("sequence_ms", 10.0), ("overlap_ms", 20.0), ("search_ms", 41.0),
                         ("sample_rate", float("nan")), ("fade_len", 31)):
        bad = pitch.PitchTimeConfig()
        C.memmove(C.byref(bad), C.byref(good), size)
        setattr(bad, field, value)
        assert raw_create(bad, size) == _lib.AD_ERR_INVALID_ARGUMENT, field
    # a NULL table has the library compute the fade itself; the call runs
    own = pitch.PitchTimeConfig(FS, 1.5, 20.0, 4.0, 2.0)
    assert raw_create(own, size) == _lib.AD_OK
    del table
