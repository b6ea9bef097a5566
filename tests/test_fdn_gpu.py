"""reverb.FDNReverb on the GPU (processors.FDNReverb, the effect graph's
reverb-fdn node) against the restated reference (tests/fdn_ref.py), which is
fed the handle's own feedback gains.

Bars.  Where no sine is involved (mod depth 0: the modulation term is exactly
0) the outputs are bit-identical.  Everywhere else the GPU differs from the
oracle by the device math library's sine only: relative RMS <= 1e-12 and
max abs <= 1e-10, the project's bars for such a path; test_fdn_ref.py shows
that a last-place change of every sine stays under a tenth of that."""
import math

import numpy as np
import pytest
import torch

import fdn_ref as R
import layout_lib as LL
from algodsp import _lib, effectchain as E, processors as P, signals

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
RMS_BAR, ABS_BAR = 1e-12, 1e-10


def noise(n, channels=3, seed=0xFD00):
    return np.stack([signals.white_noise(n, seed + c) for c in range(channels)])


def sync_gains(h, refs):
    """The handle's gains are within 1 ulp of math.pow's; the oracle then runs on the handle's."""
    g, lens, pre_len, _ = h.derived()
    for r in refs:
        for i in range(8):
            w = r.feedbackGain[i]
            assert math.nextafter(w, -math.inf) <= g[i] <= math.nextafter(w, math.inf), (i, g[i], w)
        assert [len(ln.buf) for ln in r.lines] == list(lens) and len(r.preDelayLine.buf) == pre_len
        r.feedbackGain = [float(v) for v in g]


def apply(h, refs, name, value=None):
    for o in [h] + list(refs):
        getattr(o, name)(*(() if value is None else (value,)))
    sync_gains(h, refs)


def pair(fs, channels=3, sets=()):
    h = P.FDNReverb(fs, channels)
    refs = [R.FDN(fs) for _ in range(channels)]
    sync_gains(h, refs)
    for name, v in sets:
        apply(h, refs, name, v)
    return h, refs


def gpu_run(h, x, cuts=None):
    y = x.copy()
    if cuts is None:
        h.ProcessInPlace(y)
        return y
    pos = 0
    for m in cuts:
        blk = np.ascontiguousarray(y[:, pos:pos + m])
        h.ProcessInPlace(blk)
        y[:, pos:pos + m] = blk
        pos += m
    assert pos == x.shape[1]
    return y


def compare(got, want, exact, what=""):
    err = float(np.sqrt(np.mean((got - want) ** 2)) / max(np.sqrt(np.mean(want ** 2)), 1e-300))
    mx = float(np.max(np.abs(got - want)))
    print(f"{what}: rel rms {err:.3g}, max abs {mx:.3g}, differing samples {int(np.sum(got != want))}")
    if exact:
        np.testing.assert_array_equal(got, want)
    else:
        assert err <= RMS_BAR and mx <= ABS_BAR


def against_ref(h, refs, x, exact, what="", cuts=None):
    y = gpu_run(h, x, cuts)
    for c, r in enumerate(refs):
        compare(y[c], r.process(x[c]), exact, f"{what} channel {c}")
    return y


# ---- 1. no sine: bit-exact --------------------------------------------------
RATES = [(8000.0, 4096), (48000.0, 12000), (300.0, 256), (20.0, 64)]
VARIANTS = {
    "pre-delay default": lambda fs: [],
    "pre-delay 0": lambda fs: [("SetPreDelay", 0.0)],
    "pre-delay 0.3 samples": lambda fs: [("SetPreDelay", 0.3 / fs)],
    "damp 0": lambda fs: [("SetDamp", 0.0)],
    "damp 1": lambda fs: [("SetDamp", 1.0)],
    "wet 0": lambda fs: [("SetWet", 0.0)],
}


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("fs,n", RATES)
def test_mod_depth_zero_is_bit_exact(gpu, fs, n, variant):
    h, refs = pair(fs, 3, [("SetModDepth", 0.0)] + VARIANTS[variant](fs))
    block, sub, _ = h.kernel_info()
    assert block == refs[0].block_bound() and 1 <= sub <= block
    y = against_ref(h, refs, noise(n), True, f"{fs} Hz, {variant}")
    assert np.all(np.isfinite(y))


# ---- 2. defaults with modulation --------------------------------------------
@pytest.mark.parametrize("fs,rate,n", [(8000.0, 0.1, 4096), (8000.0, 1.0, 4096), (48000.0, 0.1, 12000)])
def test_modulated_defaults(gpu, fs, rate, n):
    h, refs = pair(fs, 3, [("SetModRate", rate)])
    against_ref(h, refs, noise(n), False, f"{fs} Hz, mod rate {rate}")


# ---- 3. the LFO phase -------------------------------------------------------
def test_lfo_phase_is_the_reference_sequence(gpu):
    n = 100003
    want, wraps = 0.0, 0
    for _ in range(n):
        nxt = R.lfo_step(want, 1.0, 8000.0)
        wraps += nxt < want
        want = nxt
    assert wraps == 12
    x = np.zeros((1, n))
    h, _ = pair(8000.0, 1, [("SetModRate", 1.0)])
    h.ProcessInPlace(x.copy())
    assert h.derived()[3] == want
    h2, _ = pair(8000.0, 1, [("SetModRate", 1.0)])
    gpu_run(h2, x, [1, 7, 277, 278, 279, 50000, n - 50842])
    assert h2.derived()[3] == want
    h2.Reset()
    assert h2.derived()[3] == 0.0


# ---- 4. call cutting --------------------------------------------------------
def test_results_do_not_depend_on_call_boundaries(gpu):
    sets = [("SetModRate", 1.0)]
    h, _ = pair(8000.0, 3, sets)
    block = h.kernel_info()[0]
    n = 3 * block + 5
    x = noise(n)
    whole = gpu_run(h, x)
    cuts = [1, 7, block - 1, block, block + 1]
    cuts.append(n - sum(cuts))
    h2, _ = pair(8000.0, 3, sets)
    np.testing.assert_array_equal(gpu_run(h2, x, cuts), whole)
    h3, _ = pair(8000.0, 3, sets)
    with_empty = [v for m in cuts for v in (0, m)] + [0]
    np.testing.assert_array_equal(gpu_run(h3, x, with_empty), whole)
    assert h3.derived()[3] == h.derived()[3]


def test_mixed_streams(gpu):
    """Calls on the NULL stream, a side stream and the host-buffer path, then
    Reset while a side-stream call is the last one enqueued, then the same
    again: the lines are shared by every stream, each call waits for the
    previous call's last operation, so the result is one sequential reverb's.
    44.1 kHz: the longest line (3067) is longer than every call, so the
    feedback crosses each call boundary.  Mod depth 0: bit-exact."""
    C, n = 3, 4000
    h, refs = pair(44100.0, C, [("SetModDepth", 0.0)])
    x = noise(n, C)
    want = [r.process(x[c]) for c, r in enumerate(refs)]
    d = torch.empty((C, n), dtype=torch.float64, device=DEV)
    side = torch.cuda.Stream()
    for rep in range(2):
        d.copy_(torch.from_numpy(x))
        h.process_device(d.data_ptr(), n, 1000, 0)
        h.process_device(d.data_ptr() + 8 * 1000, n, 1000, side.cuda_stream)
        blk = x[:, 2000:2500].copy()
        h.ProcessInPlace(blk)
        h.process_device(d.data_ptr() + 8 * 2500, n, 1500, 0)
        torch.cuda.synchronize()
        got = d.cpu().numpy()
        got[:, 2000:2500] = blk
        for c in range(C):
            compare(got[c], want[c], True, f"round {rep} channel {c}")
        h.process_device(d.data_ptr(), n, 700, side.cuda_stream)
        h.Reset()


# ---- 5. many channels -------------------------------------------------------
def test_seventy_channels(gpu):
    C, n, silent = 70, 1024, 33
    x = noise(n, C)
    x[silent] = 0.0
    h, _ = pair(8000.0, C, [("SetModRate", 1.0)])
    y = gpu_run(h, x)
    assert not np.any(y[silent])  # exact zeros: channels never mix
    for c in (0, 7, 8, 63, 64, 69):
        _, (r,) = pair(8000.0, 1, [("SetModRate", 1.0)])
        compare(y[c], r.process(x[c]), False, f"channel {c} of 70")


# ---- 6. setters mid-stream --------------------------------------------------
MIDSTREAM = [("SetModDepth", 0.004),         # every line longer: replaced by zeroed ones
             ("SetModDepth", 0.002 - 1e-9),  # the same lengths: contents kept, damping states zeroed
             ("SetPreDelay", 0.02), ("SetRT60", 0.9), ("SetDamp", 0.8), ("SetSampleRate", 11025.0),
             ("SetWet", 0.7), ("SetDry", 0.1), ("SetModRate", 0.5), ("Reset", None)]


@pytest.mark.parametrize("name,value", MIDSTREAM)
def test_setter_mid_stream(gpu, name, value):
    h, refs = pair(8000.0, 3, [("SetModRate", 1.0)])
    x = noise(2048)
    against_ref(h, refs, x[:, :1024].copy(), False, "before")
    apply(h, refs, name, value)
    against_ref(h, refs, x[:, 1024:].copy(), False, f"after {name}({value})")
    assert h.derived()[3] == refs[0].lfoPhase


@pytest.mark.parametrize("name,value", [("SetDamp", 1.5), ("SetSampleRate", 0.0), ("SetPreDelay", -1.0),
                                        ("SetModDepth", float("nan")), ("SetRT60", 0.0)])
def test_rejected_setter_changes_nothing(gpu, name, value):
    h, _ = pair(8000.0, 3, [("SetModRate", 1.0)])
    twin, _ = pair(8000.0, 3, [("SetModRate", 1.0)])
    x = noise(2048)
    np.testing.assert_array_equal(gpu_run(h, x[:, :1024].copy()), gpu_run(twin, x[:, :1024].copy()))
    before = [getattr(h.config(), f) for f, _ in _lib.FdnConfig._fields_]
    with pytest.raises(_lib.ErrInvalidArgument):
        getattr(h, name)(value)
    assert [getattr(h.config(), f) for f, _ in _lib.FdnConfig._fields_] == before
    np.testing.assert_array_equal(gpu_run(h, x[:, 1024:].copy()), gpu_run(twin, x[:, 1024:].copy()))


def test_getters(gpu):
    h = P.FDNReverb(48000.0, 2)
    assert (h.SampleRate(), h.Wet(), h.Dry(), h.RT60(), h.Damp(), h.PreDelay(), h.ModDepth(), h.ModRate()) == \
        (48000.0, 0.2, 1.0, 1.8, 0.3, 0.01, 0.002, 0.1)
    h.SetWet(0.4), h.SetModRate(0.7)
    assert (h.Wet(), h.ModRate()) == (0.4, 0.7)
    block, sub, lds = h.kernel_info()
    assert block == 1672 and sub <= block and 0 < lds <= 65536
    h.close()


# ---- 7. the device-buffer layout contract -----------------------------------
def test_process_device_layouts(gpu):
    n = 1500
    x = noise(n)

    def run(layout):
        h = P.FDNReverb(8000.0, 3)
        h.SetModRate(1.0)
        b = LL.place(x, layout, DEV)
        torch.cuda.synchronize()
        h.process_device(b.ptr, b.stride, 1000)         # a first call that leaves the last 500 columns alone
        h.process_device(b.ptr + 8 * 1000, b.stride, 500)
        torch.cuda.synchronize()
        LL.check_guards(b)
        return LL.payload(b)

    want = run(LL.LA(n))
    for layout in LL.variants(n):
        np.testing.assert_array_equal(run(layout), want)
    h = P.FDNReverb(8000.0, 3)
    h.SetModRate(1.0)
    np.testing.assert_array_equal(gpu_run(h, x, [1000, 500]), want)
    # a call that fails its checks touches nothing
    b = LL.place(x, LL.L1, DEV)
    torch.cuda.synchronize()
    with pytest.raises(_lib.ErrInvalidArgument):
        h.process_device(b.ptr, n - 1, n)
    with pytest.raises(_lib.ErrInvalidArgument):
        h.process_device(0, b.stride, n)
    with pytest.raises(_lib.ErrInvalidArgument):
        h.process_device(b.ptr, b.stride, -1)
    h.process_device(b.ptr, b.stride, 0)
    torch.cuda.synchronize()
    LL.check_unchanged(b, x)


# ---- 8. the effect graph ----------------------------------------------------
def _graph(node, dry_edge=False):
    edges = [(E.INPUT_NODE_ID, node["id"]), (node["id"], E.OUTPUT_NODE_ID)]
    if dry_edge:
        edges.append((E.INPUT_NODE_ID, E.OUTPUT_NODE_ID))
    return E._graph_json([node], edges)


FS = 8000.0
PARAMS = {"wet": 0.4, "rt60": 1.1, "preDelay": 0.004, "damp": 0.6, "modDepth": 0.003, "modRate": 0.8}


def _direct(x, params):
    cfg = E.fdn_params(E.Params("r", "reverb-fdn", num=params), FS)
    h = P.FDNReverb(channels=x.shape[0], config=cfg)
    return gpu_run(h, x)


@pytest.mark.parametrize("node", [{"id": "r", "type": "reverb-fdn", "params": PARAMS},
                                  {"id": "r", "type": "reverb", "params": dict(PARAMS, model="fdn")},
                                  {"id": "r", "type": "reverb-fdn"}])
def test_graph_fdn_node_is_the_processor(gpu, node):
    x = noise(1500)
    ch = E.Chain(FS, 3)
    ch.LoadGraph(_graph(node))
    assert ch.spec[1]["type"] == "fdn"
    num = {k: v for k, v in node.get("params", {}).items() if k != "model"}
    assert ch.spec[1]["fdn"] == {f: getattr(E.fdn_params(E.Params("r", "reverb-fdn", num=num), FS), f)
                                 for f, _ in _lib.FdnConfig._fields_}
    want = _direct(x, num)
    y = x.copy()
    assert ch.Process(y)
    np.testing.assert_array_equal(y, want)
    # state carries over calls; Reset restores the first run's output
    y2 = x.copy()
    assert ch.Process(y2)
    assert np.any(y2 != y)
    ch.Reset()
    y3 = x.copy()
    assert ch.Process(y3)
    np.testing.assert_array_equal(y3, y)


def test_graph_reverb_without_model_is_freeverb(gpu):
    x = 0.5 * noise(1500)
    params = {"wet": 0.3, "roomSize": 0.8}
    outs = []
    for t in ("reverb", "reverb-freeverb"):
        ch = E.Chain(FS, 3)
        ch.LoadGraph(_graph({"id": "r", "type": t, "params": params}))
        assert ch.spec[1]["type"] == "verb"
        y = x.copy()
        assert ch.Process(y)
        outs.append(y)
    np.testing.assert_array_equal(outs[0], outs[1])
    assert np.any(outs[0] != x)


def test_graph_fdn_with_dry_edge_and_bypass(gpu):
    x = noise(1500)
    node = {"id": "r", "type": "reverb-fdn", "params": PARAMS}
    ch = E.Chain(FS, 3)
    ch.LoadGraph(_graph(node, dry_edge=True))
    y = x.copy()
    assert ch.Process(y)
    np.testing.assert_array_equal(y, (_direct(x, PARAMS) + x) * 0.5)  # edge order: the node, then _input
    ch = E.Chain(FS, 3)
    ch.LoadGraph(_graph(dict(node, bypassed=True)))
    y = x.copy()
    assert ch.Process(y)
    np.testing.assert_array_equal(y, x)


# ---- 9. fdn_reverb_test.go on the GPU ---------------------------------------
def test_go_process_in_place_matches_sample(gpu):
    x = np.sin(2 * math.pi * np.arange(128) / 31).reshape(1, -1)
    h1, h2 = P.FDNReverb(44100.0), P.FDNReverb(44100.0)
    want = gpu_run(h1, x, [1] * 128)
    got = gpu_run(h2, x)
    assert np.max(np.abs(got - want)) <= 1e-12
    np.testing.assert_array_equal(got, want)


def test_go_reset_restores_state(gpu):
    x = np.zeros((1, 128))
    x[0, 0] = 1
    h = P.FDNReverb(44100.0)
    out1 = gpu_run(h, x)
    h.Reset()
    out2 = gpu_run(h, x)
    assert np.max(np.abs(out2 - out1)) <= 1e-12


def test_go_impulse_tail_exists(gpu):
    h = P.FDNReverb(44100.0)
    h.SetDry(0)
    x = np.zeros((1, 4096))
    x[0, 0] = 1
    y = gpu_run(h, x)
    assert np.any(np.abs(y[0, 1:]) > 1e-10)
    _, (r,) = pair(44100.0, 1, [("SetDry", 0)])
    compare(y[0], r.process(x[0]), False, "impulse response")
