"""The effect graph's reference interpreter (tests/fxgraph_ref.py) on graphs
small enough to work out by hand, and the coverage of the generated family of
the topology suite (tests/fxgraph_topologies.py).  No GPU."""
import json

import numpy as np

import fxgraph_ref
import fxgraph_topologies as T
from algodsp import effectchain as E

X = np.array([1.0, 2.0, -4.0, 0.5])
GAIN2 = ([(2.0, 0.0, 0.0, 0.0, 0.0)], 1.0)   # y[n] = 2 x[n]
DELAY1 = ([(0.0, 1.0, 0.0, 0.0, 0.0)], 1.0)  # y[n] = x[n-1]


def n(type_, parents, bypassed=False, **kw):
    return dict(type=type_, bypassed=bypassed, parents=parents, **kw)


def run(nodes, x=X):
    return fxgraph_ref.FxGraph(nodes, 8000.0).process(x)


def test_two_parent_mix_edge_order_and_scale():
    nodes = [n("input", []), n("biquad", [(0, 0)], sections=GAIN2), n("biquad", [(0, 0)], sections=DELAY1),
             n("output", [(2, 0), (1, 0)])]
    np.testing.assert_array_equal(run(nodes), [1.0, 2.5, -3.0, -1.5])  # ([0 1 2 -4] + [2 4 -8 1]) / 2
    # edge order: (1e16 + 1) - 1e16 is 0 and (1e16 - 1e16) + 1 is 1; one multiply by 1/3, not a division by 3
    big, neg = ([(1e16, 0.0, 0.0, 0.0, 0.0)], 1.0), ([(-1e16, 0.0, 0.0, 0.0, 0.0)], 1.0)
    nodes = [n("input", []), n("biquad", [(0, 0)], sections=big), n("biquad", [(0, 0)], sections=neg), None]
    one = np.array([1.0, 5.0])  # at 5e16 doubles are 8 apart
    nodes[3] = n("output", [(1, 0), (0, 0), (2, 0)])
    np.testing.assert_array_equal(run(nodes, one), [0.0, 8.0 * (1.0 / 3.0)])  # 5e16 + 5 rounds to 5e16 + 8
    nodes[3] = n("output", [(1, 0), (2, 0), (0, 0)])
    np.testing.assert_array_equal(run(nodes, one), [1.0 * (1.0 / 3.0), 5.0 * (1.0 / 3.0)])
    assert 5.0 * (1.0 / 3.0) != 5.0 / 3.0  # so the line above tells the two scalings apart


def test_split_read_by_port_also_when_bypassed():
    half = [(0.5, 0.0, 0.0, 0.0, 0.0)]
    for byp in (False, True):
        nodes = [n("input", []), n("split", [(0, 0)], byp, sections=half, sections2=DELAY1[0]),
                 n("pass", [(1, 1)]), n("output", [(2, 0), (1, 0)])]
        # high = x[n-1] = [0 1 2 -4] through the pass node, low = x / 2 = [0.5 1 -2 0.25]
        np.testing.assert_array_equal(run(nodes), [0.25, 1.0, 0.0, -1.875])
    nodes[3] = n("output", [(1, 0), (1, 0), (1, 1)])  # the low band twice
    np.testing.assert_array_equal(run(nodes), (np.array([1.0, 2.0, -4.0, 0.5]) + [0.0, 1.0, 2.0, -4.0]) * (1.0 / 3.0))


def test_bypassed_node_only_mixes():
    nodes = [n("input", []), n("biquad", [(0, 0)], True, sections=GAIN2), n("output", [(1, 0)])]
    np.testing.assert_array_equal(run(nodes), X)
    nodes = [n("input", []), n("biquad", [(0, 0)], sections=GAIN2),
             n("tremolo", [(0, 0), (1, 0)], True, tremolo=dict(sample_rate=8000.0, rate_hz=4.0, depth=1.0,
                                                               smoothing_ms=0.0, mix=1.0, smoothing_coeff=0.0)),
             n("biquad", [], sections=GAIN2), n("output", [(2, 0), (3, 0)])]
    np.testing.assert_array_equal(run(nodes), [0.75, 1.5, -3.0, 0.375])  # ((x + 2x) / 2 + 0) / 2


def test_python_runtimes_run_from_their_config_dicts():
    """Every node type of the Python references, from the dict Chain.spec carries: a ring modulator at a
    quarter of the rate multiplies by sin(k pi / 2) = 0 1 0 -1; a simple delay of two samples."""
    nodes = [n("input", []), n("ringmod", [(0, 0)], ringmod=dict(sample_rate=8000.0, carrier_hz=2000.0, mix=1.0)),
             n("output", [(1, 0)])]
    np.testing.assert_allclose(run(nodes), [0.0, 2.0, 0.0, -0.5], atol=1e-15)
    nodes[1] = n("delay", [(0, 0)], delay=dict(sample_rate=8000.0, mode=1, delay_samples=2))
    np.testing.assert_array_equal(run(nodes), [0.0, 0.0, 1.0, 2.0])
    plain = fxgraph_ref.FxGraph(nodes, 8000.0)
    np.testing.assert_array_equal(plain.process(X[:2]), [0.0, 0.0])
    np.testing.assert_array_equal(plain.process(X[2:]), [1.0, 2.0])  # state carries over calls


def test_generated_family_coverage():
    """What the seed list has to exercise, whatever the GPU then makes of it."""
    assert len(T.SEEDS) == len(set(T.SEEDS)) >= 24
    counts, bypassed, fanins, bands, diamonds = {}, 0, set(), 0, 0
    for seed in T.SEEDS:
        nodes, edges = T.generate(seed)
        assert (nodes, edges) == T.generate(seed)  # deterministic
        assert 4 <= len(nodes) <= 12
        g = E.parse_graph(T.graph(nodes, edges))
        assert len(g.Order) == len(nodes) + 2 and all(len(v) <= E.MAX_PARENTS for v in g.Incoming.values())
        assert g.Incoming[T.OUT]
        c, b, f, band, diamond = T.coverage(nodes, edges)
        for t, k in c.items():
            counts[t] = counts.get(t, 0) + k
        bypassed += b
        fanins |= set(f)
        bands += band
        diamonds += diamond
    print(json.dumps(counts), bypassed, sorted(fanins), bands, diamonds)
    assert all(counts.get(t, 0) >= 3 for t in T.TYPES), counts
    assert bypassed >= 3
    assert {2, 3} <= fanins and max(fanins) >= 5
    assert bands >= 3 and diamonds >= 3


def test_named_graphs_parse():
    for name, (g, fs) in T.NAMED.items():
        assert E.parse_graph(g).Order, name
    assert len(E.parse_graph(T.NAMED["lanes12"][0]).Incoming["s8"]) == 8
    assert [e[2] for e in E.parse_graph(T.NAMED["same_port_twice"][0]).Incoming[T.OUT]] == [0, 0, 1]
