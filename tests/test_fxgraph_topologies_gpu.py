"""The effect-graph compiler and scheduler (csrc/capi_fxgraph.cpp) on a family
of topologies, against the one-channel reference interpreter
(tests/fxgraph_ref.py) of Chain.Process.

Every graph is a JSON graph through effectchain.Chain.LoadGraph, at 8 kHz
unless it names a rate (48 kHz wherever there is a de-esser, which cannot be
built at 8 kHz).  One handle takes four calls of 700, 1, 1500 and 64
samples with fresh noise per call and channel (the pool grows, is reallocated,
and is then longer than the call), is Reset, and takes call 1 again: the
interpreter's output after its own Reset, and call 1's output on the bits.  (A
graph with a feedback delay node cannot repeat call 1: the reference's
Delay.Reset clears the ring and keeps the delay-time ramp where it is, as
test_delayfx_gpu.py pins for the graph's reset, and the node starts at 0.25 s
ramping to its time.  For those graphs only the interpreter is the yardstick.)
The named graphs (tests/fxgraph_topologies.py: what each one aims at) run at 3
and at 65 channels, and again through process_device on a side stream with a
row stride of 2048 and no host synchronisation between the producer of the
input, the graph and the consumer of the output: the same bits as the host
path, and nothing written past the call's length.  The generated families run
at 3 channels: the first one's types end at ringmod; the second one adds the
distortion, dist-cheb, bitcrusher, dyn-deesser and dyn-transient nodes, which
the named graphs ending in _newer and newer_nodes_line aim at as well, at
48 kHz.  Their input is bursts wherever a de-esser or a transient shaper has
to work and to rest (tests/test_fxgraph_ref.py checks on the CPU that they
do).

Bars (the project's, test_fxgraph.py): relative RMS <= 1e-12 and max abs <
1e-10 per checked channel; with a reverb-conv node (Large Church, latency 128)
1e-7 and 1e-9; graphs whose nodes are all bit-exact against their references
(filters, crossovers, Freeverb, delays, mixes: no dynamics, no modulated node,
no convolution) are compared on the bits.  The newer nodes are exact or not by
their configuration (_exact): the transient shaper, the bit crusher at a whole
bit depth, the distortion's algebraic modes, polynomial approximations and
Chebyshev mode, and the de-esser with listen on are; the distortion's tanh,
atan and exp modes and the working de-esser (log and exp2 of the device
library) are not.  A bit crusher has only exact nodes upstream
(fxgraph_topologies.py: the quantiser rule); at a fractional bit depth the
device's quantLevels is compared with the restatement's first and handed over
if it differs, as test_shaper_gpu.py's sync_q does.
"""
import functools
import json

import numpy as np
import pytest

import fxgraph_ref
import fxgraph_topologies as T
import shaper_ref
from algodsp import _lib, design, effectchain as E, irlib, processors as P, signals

pytestmark = pytest.mark.gpu

CALLS = [700, 1, 1500, 64]
STRIDE = 2048
EXACT_KINDS = {"input", "output", "pass", "biquad", "split", "verb", "delay"}
EXACT_MODES = {shaper_ref.MODES.index(m) for m in shaper_ref.ALGEBRAIC}
POLY_MODES = {shaper_ref.MODES.index(m) for m in shaper_ref.POLY_ALGEBRAIC}


def _exact(d):
    """Whether spec node d is compared on the bits: by type, the newer nodes by configuration."""
    t = d["type"]
    if t == "transient":
        return True
    if t == "bitcrusher":
        return d[t]["bit_depth"] == int(d[t]["bit_depth"])
    if t == "distortion":
        return d[t]["mode"] in EXACT_MODES or (d[t]["mode"] in POLY_MODES and d[t]["approx"] == shaper_ref.POLYNOMIAL)
    if t == "deesser":
        return d[t]["listen"] != 0
    return t in EXACT_KINDS


def _input(json_graph, k, c, n, pos):
    """Call k's block of channel c: noise of its own seed, scaled 0.5; bursts
    where a gate or an expander has to open and close, a de-esser to reduce and
    to recover, a transient shaper's envelope to rise and to fall."""
    x = signals.white_noise(n, 0x70B0 + 1000 * k + c)
    if T.has_type(json_graph, "dyn-gate", "dyn-expander", "dyn-deesser", "dyn-transient"):
        return np.where(((pos + np.arange(n)) // 300) % 2 == 0, 0.6, 0.004) * x
    return 0.5 * x


def _inputs(json_graph, channels):
    pos = np.cumsum([0] + CALLS)
    return [np.stack([_input(json_graph, k, c, n, pos[k]) for c in channels]) for k, n in enumerate(CALLS)]


def _chain(json_graph, fs, C):
    prov = irlib.LibraryProvider()
    assert prov.IRNames()[1] == "Large Church"  # the graphs' irIndex
    ch = E.Chain(fs, C, designer=design.RBJDesigner(), ir_provider=prov)
    ch.LoadGraph(json_graph)
    return ch


@functools.lru_cache(maxsize=None)
def _graph_of(name):
    if name in T.NAMED:
        return T.NAMED[name]
    if name.startswith("2:"):  # the second family
        return T.graph(*T.generate(int(name[2:]), family=2)), T.FS2
    return T.graph(*T.generate(int(name))), T.FS


@functools.lru_cache(maxsize=None)
def _host_run(name, C):
    """The host path: (outputs of the four calls, call 1 again after Reset, op_count, spec)."""
    g, fs = _graph_of(name)
    ch = _chain(g, fs, C)
    outs = []
    for x in _inputs(g, range(C)):
        y = x.copy()
        assert ch.Process(y)
        outs.append(y)
    ch.Reset()
    again = _inputs(g, range(C))[0].copy()
    assert ch.Process(again)
    ops, spec = ch.op_count(), ch.spec
    ch.close()
    return outs, again, ops, spec


@functools.lru_cache(maxsize=None)
def _expected(name, c):
    """The interpreter's four outputs for channel c, and call 1 again after its
    reset (channel c's input does not depend on the channel count)."""
    g, fs = _graph_of(name)
    spec = _host_run(name, 3)[3]
    ref = fxgraph_ref.FxGraph(spec, fs)
    for d, r in zip(spec, ref.rt):
        if d["type"] == "bitcrusher" and not _exact(d):  # exp2 of a fractional depth: the device's, if it differs
            h = P.BitCrusher(channels=1, config=_lib.BitCrusherConfig(**d["bitcrusher"]))
            q, crusher = h.derived()["quant_levels"], r[1].ref
            h.close()
            print(f"{name}: bit depth {crusher.bitDepth}: quantLevels {crusher.quantLevels!r}, the device's {q!r}")
            assert np.nextafter(crusher.quantLevels, 0.0) <= q <= np.nextafter(crusher.quantLevels, np.inf)
            crusher.quantLevels = q
    xs = _inputs(g, [c])
    outs = [ref.process(x[0]) for x in xs]
    ref.reset()
    return outs + [ref.process(xs[0][0])]


def _check(name, C, channels):
    outs, again, ops, spec = _host_run(name, C)
    kinds = {d["type"] for d in spec if d["type"] == "split" or not d["bypassed"]}  # what runs: a bypassed split does
    exact = all(_exact(d) for d in spec if d["type"] == "split" or not d["bypassed"])
    rms_bar, abs_bar = (1e-7, 1e-9) if "conv" in kinds else (1e-12, 1e-10)
    for c in channels:
        for k, want in enumerate(_expected(name, c)):
            got = (outs + [again])[k][c]
            err = float(np.sqrt(np.mean((got - want) ** 2)) / max(np.sqrt(np.mean(want ** 2)), 1e-300))
            mx = float(np.max(np.abs(got - want)))
            print(f"{name} C={C} channel {c} call {k} (n={len(want)}): rel rms {err:.3g}, max abs {mx:.3g}, "
                  f"differing {int(np.sum(got != want))}, exact={exact}")
            assert np.all(np.isfinite(got))
            if exact:
                np.testing.assert_array_equal(got, want, err_msg=f"{name} channel {c} call {k}")
            else:
                assert err <= rms_bar and mx < abs_bar, f"{name} channel {c} call {k}: {err} {mx}"
    if not any(d["type"] == "delay" and d["delay"]["mode"] == 0 and not d["bypassed"] for d in spec):
        np.testing.assert_array_equal(again, outs[0], err_msg=f"{name}: call 1 after Reset")
    return ops, spec


@pytest.mark.parametrize("C", [3, 65])
@pytest.mark.parametrize("name", list(T.NAMED))
def test_named_graph(gpu, name, C):
    ops, spec = _check(name, C, range(3) if C == 3 else [0, 63, 64])
    if name in T.NAMED_OPS:
        assert ops == T.NAMED_OPS[name]
    if name == "lanes12":
        assert ops[2] == 8  # 12 concurrent branches: four of them on the fallback lane i % 8
    if name == "guarded_branch":
        assert ops[2] == 2
    if name == "every_node_line":
        assert {d["type"] for d in spec} == {"input", "output", "pass", "biquad", "comp", "verb", "fdn", "conv", "delay",
                                             "flanger", "phaser", "tremolo", "ringmod", "split"}
    if name == "diamond":
        assert ops[1] == 3  # B's copy of A's buffer, and the output's mix
    if name == "newer_nodes_line":
        assert {d["type"] for d in spec} == {"input", "output", "bitcrusher", "transient", "distortion", "deesser"}
    if name == "fanin_newer":
        assert ops[2] == 8  # 11 concurrent branches: three of them on the fallback lane i % 8
    if name == "diamond_newer":
        assert ops[:2] == T.DIAMOND_NEWER_OPS
    if name in T.NEWER and C == 3:  # the spec the CPU tests of these graphs' inputs work from is the chain's
        as_data = lambda sp: json.loads(json.dumps(sp))
        assert as_data(fxgraph_ref.host_spec(*T.NAMED[name], design.RBJDesigner())) == as_data(spec)


@pytest.mark.parametrize("seed", [str(s) for s in T.SEEDS] + [f"2:{s}" for s in T.SEEDS2])
def test_generated_graph(gpu, seed):
    _check(seed, 3, range(3))


@pytest.mark.parametrize("name", list(T.NAMED))
def test_named_graph_device_path_on_a_side_stream(gpu, name):
    """process_device on a non-default stream: the input is written by a torch
    op on that stream right before the call and the output copied out by one
    right after it, with no synchronisation until all four calls are queued."""
    import torch

    C = 65
    g, fs = _graph_of(name)
    outs, again, _, _ = _host_run(name, C)
    ch = _chain(g, fs, C)
    xs = [torch.from_numpy(x).cuda() for x in _inputs(g, range(C))]
    d = torch.empty((C, STRIDE), dtype=torch.float64, device="cuda")
    got = [torch.empty_like(d) for _ in range(len(CALLS) + 1)]
    torch.cuda.synchronize()
    s = torch.cuda.Stream()

    def call(k, into):
        n = CALLS[k]
        with torch.cuda.stream(s):
            d.fill_(float("nan"))
            d[:, :n] = xs[k]
            assert ch.process_device(d.data_ptr(), STRIDE, n, s.cuda_stream)
            into.copy_(d)

    for k in range(len(CALLS)):
        call(k, got[k])
    torch.cuda.synchronize()
    ch.Reset()
    call(0, got[-1])
    torch.cuda.synchronize()
    for k, want in enumerate(outs + [again]):
        y = got[k].cpu().numpy()
        n = want.shape[1]
        np.testing.assert_array_equal(y[:, :n], want, err_msg=f"{name}: device call {k} against the host path")
        assert np.all(np.isnan(y[:, n:])), f"{name}: call {k} wrote past its {n} samples"
    ch.close()
