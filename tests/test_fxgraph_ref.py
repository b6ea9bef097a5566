"""The effect graph's reference interpreter (tests/fxgraph_ref.py) on graphs
small enough to work out by hand, the coverage of the two generated families
of the topology suite (tests/fxgraph_topologies.py) with a digest of every
graph of the first, and the conditions under which the suite's inputs make the
distortion, bitcrusher, de-esser and transient shaper nodes of its named
graphs work.  No GPU."""
import hashlib
import json

import numpy as np
import pytest

import dynfx_ref
import fxgraph_ref
import fxgraph_topologies as T
import shaper_ref
import test_fxgraph_topologies_gpu as G  # its inputs and call lengths; nothing there touches a device on import
from algodsp import design, effectchain as E

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


# ---- the distortion, bitcrusher, deesser and transient runtimes -------------------------------------------------
M = {name: i for i, name in enumerate(shaper_ref.MODES)}


def dist(fs=8000.0, **options):
    return shaper_ref.config_of(shaper_ref.Distortion(fs, **options))


def crush(fs=8000.0, **options):
    return shaper_ref.config_of(shaper_ref.BitCrusher(fs, **options))


def one(type_, cfg, fs=8000.0, parents=((0, 0),)):
    return fxgraph_ref.FxGraph([n("input", []), n(type_, list(parents), **{type_: cfg}), n("output", [(1, 0)])], fs)


def test_distortion_runtime_hard_clip_and_bias():
    g = one("distortion", dist(mode=M["hardclip"], clip_level=0.5))
    # clip at 0.5, then / 0.5: values either side of the level, and on it
    np.testing.assert_array_equal(g.process(np.array([0.25, 0.5, 0.75, -2.0, -0.375])), [0.5, 1.0, 1.0, -1.0, -0.75])
    # without parents the node processes zeros: (0 + 0.125) * 2 = 0.25, / 0.5, * 0.75
    g = one("distortion", dist(mode=M["hardclip"], clip_level=0.5, drive=2.0, bias=0.125, output_level=0.75), parents=())
    np.testing.assert_array_equal(g.process(X), [0.375] * 4)
    # the same node behind the input at mix 0.5.  x = 1: (1 + 0.125) * 2 = 2.25 clips to 0.5, / 0.5, * 0.75 is
    # 0.75, and 1 * 0.5 + 0.75 * 0.5; x = 0: the constant above, 0.375 * 0.5
    g = one("distortion", dist(mode=M["hardclip"], clip_level=0.5, drive=2.0, bias=0.125, output_level=0.75, mix=0.5))
    np.testing.assert_array_equal(g.process(np.array([1.0, 0.0])), [0.875, 0.1875])


def test_bitcrusher_runtime_counter_and_hold_value_carry_over_calls():
    """Bit depth 2: quantLevels 2, steps of 0.5.  Downsample 2: the counter reaches 2 at every second sample, which
    is quantised and held; before the first update the hold value is 0.  math.Round: -0.5 goes to -1."""
    x = np.array([0.9, 0.3, -0.6, 1.3, 0.76, -0.25, 0.1])
    want = [0.0, 0.5, 0.5, 1.5, 1.5, -0.5, -0.5]  # round(0.6) / 2, round(2.6) / 2, round(-0.5) / 2
    cfg = crush(bit_depth=2.0, downsample=2)
    np.testing.assert_array_equal(one("bitcrusher", cfg).process(x), want)
    g = one("bitcrusher", cfg)
    np.testing.assert_array_equal(g.process(x[:3]), want[:3])  # the counter is 1 and the hold value 0.5 ...
    np.testing.assert_array_equal(g.process(x[3:]), want[3:])  # ... so 1.3 is an update and 0.76 is not
    g.reset()
    np.testing.assert_array_equal(g.process(x), want)
    np.testing.assert_array_equal(one("bitcrusher", crush(bit_depth=2.0, downsample=2, mix=0.5)).process(x[:2]),
                                  [0.45, 0.4])


DEESS = dict(sample_rate=48000.0, freq_hz=6000.0, q=1.5, threshold_db=-30.0, ratio=6.0, knee_db=3.0, attack_ms=0.5,
             release_ms=1.5, range_db=-24.0, attack_coeff=0.0, release_coeff=0.0, mode=0, detector=0, listen=0,
             filter_order=2)
TRANS = dict(sample_rate=48000.0, attack_amount=0.6, sustain_amount=-0.4, attack_ms=1.0, release_ms=20.0,
             attack_coeff=0.0, release_coeff=0.0)


def _bursts():
    return G._inputs(T.NAMED["newer_nodes_line"][0], [0])


def _deesser(c):
    r = dynfx_ref.DeEsser(c["sample_rate"])
    for name, f in (("SetFrequency", "freq_hz"), ("SetQ", "q"), ("SetThreshold", "threshold_db"), ("SetRatio", "ratio"),
                    ("SetKnee", "knee_db"), ("SetAttack", "attack_ms"), ("SetRelease", "release_ms"),
                    ("SetRange", "range_db"), ("SetMode", "mode"), ("SetDetector", "detector"),
                    ("SetFilterOrder", "filter_order"), ("SetListen", "listen")):
        getattr(r, name)(c[f])
    return r


def _transient(c):
    r = dynfx_ref.TransientShaper(c["sample_rate"])
    r.SetAttackAmount(c["attack_amount"]), r.SetSustainAmount(c["sustain_amount"])
    r.SetAttack(c["attack_ms"]), r.SetRelease(c["release_ms"])
    return r


@pytest.mark.parametrize("kind,cfg", [("deesser", DEESS), ("deesser", dict(DEESS, mode=1, detector=1, filter_order=3)),
                                      ("deesser", dict(DEESS, listen=1)), ("transient", TRANS)],
                         ids=["deesser", "deesser wideband", "deesser listen", "transient"])
def test_dynamics_runtimes_are_the_restatements_over_the_suites_calls(kind, cfg):
    """A one-node graph against the stand-alone restatement with the same setters, the input split 700 / 1 / 1500 /
    64, on the bits; reset() and the first call again."""
    g = one(kind, cfg, fs=48000.0)
    alone = (_deesser if kind == "deesser" else _transient)(cfg)
    xs = _bursts()
    assert [x.shape[1] for x in xs] == [700, 1, 1500, 64]
    first = None
    for x in xs:
        got, want = g.process(x[0]), alone.ProcessInPlace(x[0].copy())
        np.testing.assert_array_equal(got.view(np.int64), want.view(np.int64))
        assert np.any(got != x[0])
        first = got if first is None else first
    assert np.any(g.process(xs[0][0]) != first)  # the envelope and the cascades carried over
    g.reset()
    np.testing.assert_array_equal(g.process(xs[0][0]), first)


def test_dynamics_runtimes_take_a_coefficient_that_is_not_zero():
    """attack_coeff / release_coeff 0 is `derive`; anything else is the coefficient itself (capi_dynfx.cpp)."""
    x = _bursts()[0][0]
    for kind, cfg, make in (("deesser", DEESS, _deesser), ("transient", TRANS, _transient)):
        alone = make(cfg)
        g = one(kind, dict(cfg, attack_coeff=alone.attackCoeff, release_coeff=alone.releaseCoeff), fs=48000.0)
        np.testing.assert_array_equal(g.process(x), make(cfg).ProcessInPlace(x.copy()))
        alone.attackCoeff, alone.releaseCoeff = 0.25, 0.5
        g = one(kind, dict(cfg, attack_coeff=0.25, release_coeff=0.5), fs=48000.0)
        np.testing.assert_array_equal(g.process(x), alone.ProcessInPlace(x.copy()))


def test_shaper_runtimes_reset_and_dc_state():
    """Chebyshev with the DC bypass: T2(x) = 2 x^2 - 1 of zeros is -1, through y = w - w' + 0.995 y'."""
    g = one("distortion", dist(mode=M["chebyshev"], cheb_order=2, cheb_dc_bypass=True), parents=())
    np.testing.assert_array_equal(g.process(np.zeros(3)), [-1.0, -0.995, 0.995 * -0.995])
    np.testing.assert_array_equal(g.process(np.zeros(1)), [0.995 * (0.995 * -0.995)])  # the state carried over
    g.reset()
    np.testing.assert_array_equal(g.process(np.zeros(1)), [-1.0])


# ---- the two generated families ---------------------------------------------------------------------------------
FAMILY1_SHA256 = (  # sha256 of T.graph(*T.generate(seed)) for seed 1..24, from before TYPES2 existed
    "bbbecfd48112e3e7d46e851b94da36cf3fdf69e0245d08b4e756d5bfaab18edd",
    "0f49a7e2873a1213ee2c874b8596a57ca43a3b135927f6893ab725247556cd6d",
    "0335bfa82c6f2f48b86850c6be5557987a3279e3258f72ed0226ca50ec58f362",
    "7b7ff51efdeecb50ef1f3e541f6ff69f8cecaef4196a3378375e3a0398dd5f47",
    "74f6441900bcd43c9680630d667e3e291e1cdcf4987b6b33ba320fe8a675e688",
    "11b097711d6aa81a1a8960eb9380fba1e267e8cc26d8b5a068f1ad3fa7346c27",
    "ae0d34f3617386b535edef5b731e9ffb9f66b851ca9d3ec057a3357558d841e1",
    "bc095974c98b4a45d773d8aec401a2818f894648bbdeaabf742bed45637f7860",
    "25df7b684e6486c85c6709c841a1863ff529a4dbfd53652b3dc68d0ae58ca460",
    "f1d7aa8046ac5fabdb1276ec6a00ffeb3820ccfcbb72b41f7331e0a0a632bb39",
    "e74ab26dc50d9ec305e2270fcf9ade5548fb21f3745d4aa6ad3b04b900c9d829",
    "15f8d9da7fda9ff505d169e21ef0de3ca70295b39a730409ca8fdf44c9fe2e64",
    "b06e2f5cc5d17e915bf8d7f27b1f60fc3bf8b99788c926de8c8135672d3346f1",
    "57fb39f6ebc152f6db90e02059a0156278f02f1fc1e6be51579c535850395197",
    "72df73401e7262d438c29e953b2ac0de57c32ff3c7c37849b4390ae2870a9292",
    "65880ca4ddd75b84dcb78dc24519ba145cbec73d853836d1f620992bd279dc63",
    "0170bd4b7b4c026a01c4d444412f40bc14a8bca28d268560a88539036f795e1a",
    "df5b91bc2aa0233156d0dc1eca11ddb1683e78073e2a68866dffbf864c3ca2de",
    "62265a839114b76c56b4aa89686e3ee6ad5704bced208ae79db39d6dab7814ae",
    "62006deb188fc8e1f925bf32b26b308ca91b17c1a48e3ea5de8d9b26bb68e0fb",
    "75f75108381744fb609e87b769ce9f534661cf4f52cd865ae603dd2346d7d1d8",
    "0badc65667795497f59c3796c288243f5d486000336b93ff10e454467b1b592c",
    "9f6c0b79c0f0444492b02a5c3e219a20628ee431d84cd444eb75cb7ef52fd59a",
    "dd224b082f817d98ae7543ec6f37fbc96cfcb4b436b4bb4a622a635bcfdcc979",
)


def test_first_family_is_unchanged():
    assert T.SEEDS == list(range(1, 25)) and T.TYPES[-1] == "sum" and len(T.TYPES) == 19
    for seed, want in zip(T.SEEDS, FAMILY1_SHA256):
        assert hashlib.sha256(T.graph(*T.generate(seed)).encode()).hexdigest() == want, seed
        assert T.generate(seed) == T.generate(seed, family=1)


NEWER_TYPES = ["distortion", "dist-cheb", "bitcrusher", "dyn-deesser", "dyn-transient"]


def test_second_family_coverage():
    """The first family's thresholds over TYPES2, and each of the five newer types with two or more parents, as the
    in-place consumer in a diamond, and bypassed; the quantiser rule; the rate's de-esser is buildable."""
    assert T.TYPES2 == T.TYPES + NEWER_TYPES and len(T.SEEDS2) == len(set(T.SEEDS2)) >= 24
    counts, bypassed, fanins, bands, diamonds = {}, 0, set(), 0, 0
    many, in_diamond, byp_types = set(), set(), set()
    for seed in T.SEEDS2:
        nodes, edges = T.generate(seed, family=2)
        assert (nodes, edges) == T.generate(seed, family=2)
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
        m, d, bt = T.coverage_by_type(nodes, edges)
        many, in_diamond, byp_types = many | m, in_diamond | d, byp_types | bt
        by_id = {nd["id"]: nd for nd in nodes}
        for nd in nodes:
            if nd["type"] == "bitcrusher":
                assert nd["params"]["bitDepth"] == int(nd["params"]["bitDepth"])
                assert all(T.exact_node(by_id[a]) for a in T.upstream(nd["id"], edges) if a != T.IN), (seed, nd["id"])
            if nd["type"] == "dyn-deesser":
                assert 1000 <= nd["params"]["freqHz"] < 0.49 * T.FS2
    print(json.dumps(counts), bypassed, sorted(fanins), bands, diamonds, sorted(many), sorted(in_diamond), sorted(byp_types))
    assert all(counts.get(t, 0) >= 3 for t in T.TYPES2), counts
    assert bypassed >= 3
    assert {2, 3} <= fanins and max(fanins) >= 5
    assert bands >= 3 and diamonds >= 3
    assert set(NEWER_TYPES) <= many and set(NEWER_TYPES) <= in_diamond and set(NEWER_TYPES) <= byp_types


def test_exact_node_reads_the_configuration():
    assert T.exact_node(T.node("a", "distortion", mode="hardclip")) and T.exact_node(T.node("a", "distortion"))
    assert not T.exact_node(T.node("a", "distortion", mode="tanh"))
    assert T.exact_node(T.node("a", "distortion", mode="tanh", approx="polynomial"))
    assert not T.exact_node(T.node("a", "distortion", mode="waveshaper5", approx="polynomial"))
    assert T.exact_node(T.node("a", "bitcrusher", bitDepth=4)) and not T.exact_node(T.node("a", "bitcrusher", bitDepth=4.5))
    assert T.exact_node(T.node("a", "dyn-deesser", listen=1)) and not T.exact_node(T.node("a", "dyn-deesser"))
    assert T.exact_node(T.node("a", "dyn-compressor", bypassed=True)) and not T.exact_node(T.node("a", "phaser"))
    # the named graphs keep the quantiser rule too
    for name, (g, fs) in T.NAMED.items():
        d = json.loads(g)
        by_id = {nd["id"]: nd for nd in d["nodes"]}
        edges = [(e["from"], e["to"], e.get("fromPortIndex", 0)) for e in d["connections"]]
        for nd in d["nodes"]:
            if nd["type"] == "bitcrusher":
                assert all(T.exact_node(by_id[a]) for a in T.upstream(nd["id"], edges) if a != T.IN), (name, nd["id"])
            if nd["type"] == "dyn-deesser":
                assert fs == T.FS2, name


# ---- the newer named graphs' inputs make their nodes work -----------------------------------------------------
@pytest.mark.parametrize("name", T.NEWER)
def test_newer_named_graphs_inputs_make_the_nodes_work(name):
    """The interpreter alone over the suite's four calls of channel 0, with taps on the node inputs.  Of the
    running nodes that have a parent (a node without one processes zeros): every working de-esser reduces the gain
    on a tenth of the samples at least and leaves it at 1 on a tenth at least; every transient shaper's envelope
    rises on a tenth and falls on a tenth; every distortion with a clip (hardclip's level, Chebyshev's clamp of its
    argument to [-1, 1]) clips on some samples and not on others.  Every running bit crusher with a downsample
    factor above 1 ends a call with the counter off 0: the value it holds crosses into the next call."""
    g, fs = T.NAMED[name]
    spec = fxgraph_ref.host_spec(g, fs, design.RBJDesigner())
    ref = fxgraph_ref.FxGraph(spec, fs)
    taps, held = {}, {}
    for i, (d, r) in enumerate(zip(spec, ref.rt)):
        if d["type"] not in ("distortion", "bitcrusher", "deesser", "transient") or d["bypassed"]:
            continue

        def tapped(block, i=i, inner=r[1]):
            taps.setdefault(i, []).append(np.array(block))
            return inner(block)

        tapped.ref = r[1].ref
        r[1] = tapped
        if d["type"] == "deesser":
            tapped.ref.trace = []
        if d["type"] == "transient":
            tapped.ref.log = []

            def sample(x, p=tapped.ref, inner=tapped.ref.ProcessSample):
                y = inner(x)
                p.log.append(p.envelope)
                return y

            tapped.ref.ProcessSample = sample
    for x in G._inputs(g, [0]):
        assert np.all(np.isfinite(ref.process(x[0])))
        for i, r in enumerate(ref.rt):
            if spec[i]["type"] == "bitcrusher" and i in taps:
                held.setdefault(i, []).append(r[1].ref.holdCounter)
    seen = set()
    for i, blocks in taps.items():
        d, p = spec[i], ref.rt[i][1].ref
        x = np.concatenate(blocks)
        assert x.size == sum(G.CALLS)
        seen.add(d["type"])
        if d["type"] == "bitcrusher" and p.downsample > 1:
            assert any(c != 0 for c in held[i][:-1]), (d["id"], held[i])
        if not d["parents"]:
            assert not np.any(x)
            continue
        if d["type"] == "deesser" and not p.listen:
            gain = np.array([p.calculateGain(e) for e in p.trace])
            print(f"{name} {d['id']}: gain < 1 on {np.mean(gain < 1):.2f}, 1 on {np.mean(gain == 1):.2f}, least {gain.min():.3f}")
            assert gain.size == x.size and np.mean(gain < 1) >= 0.1 and np.mean(gain == 1) >= 0.1, d["id"]
        if d["type"] == "transient":
            step = np.diff(np.array([0.0] + p.log))
            print(f"{name} {d['id']}: envelope rises on {np.mean(step > 0):.2f}, falls on {np.mean(step < 0):.2f}")
            assert np.mean(step > 0) >= 0.1 and np.mean(step < 0) >= 0.1, d["id"]
        if d["type"] == "distortion" and p.mode in (M["hardclip"], M["chebyshev"]):
            level = p.clipLevel if p.mode == M["hardclip"] else 1.0
            clipped = np.abs(p.argument(x)) > level
            print(f"{name} {d['id']}: clips on {np.mean(clipped):.2f}")
            assert 0 < np.mean(clipped) < 1, d["id"]
    assert seen or name == "fusion_bypassed_newer"  # which bypasses its newer nodes: nothing to make work
