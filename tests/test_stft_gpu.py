"""The GPU spectral freeze and spectral pitch shifter against the restatement
in tests/stft_ref.py, at the cases and within the bars of tests/stft_cases.py
(derived there from the restatement alone; tests/test_stft_ref.py asserts that
no bar exceeds 1e-9 and that every data-dependent decision has room).

Errors are taken on the overlap-add sums, (got - want) * norm where
norm > 1e-12, as relative RMS and max abs; after the time stretch's resampling
on the output itself.  norm, the freeze's phaseAcc given the captured phases,
mix 0, the identity shortcut, repeated calls and the host and device entry
points are compared on float64 bits.

Measured on one MI355X against the bars, relative RMS at worst:
unfrozen freeze 8.4e-16 (bars 2e-15 ... 1.4e-14), frozen 2.3e-14 (8.3e-14), bin
shift 4.3e-14 (bar 4.2e-13 there), time stretch 2.7e-13 (bar 6.6e-13 there).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import stft_cases as K
import stft_ref as R
from algodsp import _lib, effectchain as E, processors as P

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FS = K.FS


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def same_bits(got, want, what=""):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, what
    bad = np.flatnonzero(bits(got).reshape(-1) != bits(want).reshape(-1))
    if bad.size:
        i = int(bad[0])
        raise AssertionError(f"{what}: {bad.size} of {got.size} differ, first at flat index {i}: "
                             f"got {got.reshape(-1)[i]!r}, want {want.reshape(-1)[i]!r}")


def gpu_freeze(frame, hop, channels, mix=1.0, mode=R.PHASE_ADVANCE, frozen=False):
    return P.SpectralFreeze(FS, channels, frame_size=frame, hop_size=hop, mix=mix, phase_mode=mode, frozen=int(frozen))


def gpu_pitch(ratio, frame, hop, channels):
    h = P.SpectralPitchShifter(FS, channels, frame_size=frame, analysis_hop=hop)
    h.SetPitchRatio(ratio)
    return h


def run(h, x):
    y = x.copy()
    h.ProcessInPlace(y)
    return y


# ---- norm ---------------------------------------------------------------------
@pytest.mark.parametrize("frame,hop,n", [(64, 16, 165), (256, 96, 549), (1024, 1023, 2085), (4096, 1024, 5123),
                                          (64, 1, 200), (256, 64, 1)])
def test_norm_is_bit_exact(gpu, frame, hop, n):
    r = K.make_freeze(frame, hop)
    r.Process(np.ones(n))
    same_bits(gpu_freeze(frame, hop, 1).norm(n), r.last_norm[:n], "norm")


# ---- freeze, unfrozen -----------------------------------------------------------
@pytest.mark.parametrize("frame,hop,n,channels", K.FREEZE_SHAPES)
def test_unfrozen_freeze_reconstructs(gpu, frame, hop, n, channels):
    x = K.noise(n, channels)
    bar = K.freeze_bar(frame, hop, n, channels)
    y = run(gpu_freeze(frame, hop, channels), x)
    for c in range(channels):
        bar.check(y[c], c, what=f"unfrozen {frame}/{hop} n {n}")
        # and so the input itself on the sums: the restatement's own 1e-13 (test_stft_ref.py) plus the bar
        ok = bar.norms[c][0][:n] > R.NORM_FLOOR
        assert float(np.max(np.abs((y[c] - x[c])[ok] * bar.norms[c][0][:n][ok]), initial=0.0)) <= bar.abs + 1e-13


# ---- freeze, frozen ---------------------------------------------------------------
@pytest.mark.parametrize("mode", [R.PHASE_HOLD, R.PHASE_ADVANCE], ids=["hold", "advance"])
@pytest.mark.parametrize("mix", [1.0, 0.3])
def test_frozen_over_calls(gpu, mode, mix):
    n, channels, frame, hop = sum(K.CUTS), 65, 256, 64
    x = K.noise(n, channels)
    bar = K.freeze_bar(frame, hop, n, channels, mix, mode, True, K.CUTS)
    h = gpu_freeze(frame, hop, channels, mix, mode, True)
    pos, steps = 0, -1  # the captured frame is played back un-advanced
    for call, m in enumerate(K.CUTS):
        blk = x[:, pos:pos + m].copy()
        h.ProcessInPlace(blk)
        assert h.state()[2]
        steps += 1 + (m - 1) // hop
        for c in range(channels):
            bar.check(blk[c], c, call, what=f"frozen mode {mode} mix {mix}")
        pos += m
    held = h.state()[0]
    worst = float(np.max(np.abs(held - np.stack([r.heldMagnitude for r in bar.refs]))))
    print(f"held magnitude: max abs {worst:.3e} (bar {bar.held_abs:.3e})")
    assert worst <= bar.held_abs
    # phaseAcc on bits, given the captured phases the device holds: a Hold twin reads them back untouched
    twin = gpu_freeze(frame, hop, channels, mix, R.PHASE_HOLD, True)
    twin.ProcessInPlace(x[:, :K.CUTS[0]].copy())
    captured = twin.state()[1]
    want = captured.copy()
    if mode == R.PHASE_ADVANCE:
        om = R.omega_table(frame)
        for _ in range(steps):
            want = want + om * float(hop)
    same_bits(h.state()[1], want, "phaseAcc by repeated addition")


def test_frozen_mix_zero_returns_the_inputs_bits(gpu):
    x = K.noise(700, 3)
    for frozen in (False, True):
        same_bits(run(gpu_freeze(256, 64, 3, mix=0.0, frozen=frozen), x), x, "mix 0")


def test_freeze_state_recaptures(gpu):
    """Reset, a freeze -> unfreeze -> freeze toggle and SetFrameSize each capture again."""
    x = K.noise(1200, 3)
    h = gpu_freeze(256, 64, 3, frozen=True)
    a = run(h, x[:, :400])
    held_a = h.state()[0]
    run(h, x[:, 400:800])
    same_bits(h.state()[0], held_a, "later calls keep the capture")
    h.SetFrozen(True)  # no change
    assert h.state()[2]
    h.Reset()
    assert not h.state()[2] and np.all(h.state()[1] == 0)
    same_bits(run(h, x[:, :400]), a, "after Reset the first call repeats")
    h.Unfreeze()
    assert not h.state()[2]
    h.Freeze()
    run(h, x[:, 800:])
    assert h.state()[2] and not np.array_equal(h.state()[0], held_a)
    h.SetHopSize(200)
    h.SetFrameSize(128)
    assert (h.FrameSize(), h.HopSize()) == (128, 32) and not h.state()[2] and h.state()[0].shape == (3, 65)
    y = run(h, x[:, :400])
    bar = K.bar_for(lambda: K.make_freeze(128, 32, frozen=True), x[:, :400])
    for c in range(3):
        bar.check(y[c], c, what="after SetFrameSize")


# ---- pitch ---------------------------------------------------------------------------
@pytest.mark.parametrize("ratio,frame,hop,n,channels", K.PITCH_CASES)
def test_pitch_within_the_bar(gpu, ratio, frame, hop, n, channels):
    x = K.noise(n, channels)
    bar = K.pitch_bar(ratio, frame, hop, n, channels)
    h = gpu_pitch(ratio, frame, hop, channels)
    ref = bar.refs[0]
    assert h.path() == (1 if ref.use_bin_shifting() else 2)
    assert h.SynthesisHop() == ref.SynthesisHop() and h.EffectivePitchRatio() == ref.EffectivePitchRatio()
    y = run(h, x)
    for c in range(channels):
        bar.check(y[c], c, what=f"pitch {ratio:.4f} {frame}/{hop}")
    same_bits(run(h, x), y, "a second call: stateless, no atomics")


def test_pitch_paths_at_the_threshold(gpu):
    h = gpu_pitch(1.15, 1024, 256, 1)
    assert h.path() == 1 and h.SynthesisHop() == 256 and h.EffectivePitchRatio() == 1.15
    h.SetPitchRatio(1.1500001)
    assert h.path() == 2 and h.SynthesisHop() == 294 and h.EffectivePitchRatio() == 294 / 256
    h.SetPitchRatio(0.85)  # 0.85 - 1 = -0.15000000000000002
    assert h.path() == 2 and h.SynthesisHop() == 218
    h = gpu_pitch(1.2, 64, 2, 1)
    assert h.path() == 2 and h.SynthesisHop() == 2  # a time stretch without resampling
    h.SetPitchSemitones(7)
    assert h.PitchRatio() == 2.0 ** (7 / 12.0) and abs(h.PitchSemitones() - 7) < 1e-12


def test_pitch_identity_returns_the_inputs_bits(gpu):
    x = K.noise(549, 3)
    for ratio in (1.0, 1 + 5e-10):
        same_bits(run(gpu_pitch(ratio, 256, 64, 3), x), x, f"ratio {ratio!r}")


# ---- silence ---------------------------------------------------------------------------
def test_silence_gives_exact_zeros(gpu):
    z = np.zeros((2, 700))
    for frozen in (False, True):
        for mode in (0, 1):
            assert np.all(run(gpu_freeze(256, 64, 2, mode=mode, frozen=frozen), z) == 0.0)
    for ratio, hop in ((1.1, 64), (1.5, 64), (0.5, 64), (1.2, 2)):
        assert np.all(run(gpu_pitch(ratio, 256, hop, 2), z) == 0.0), ratio


# ---- bad arguments -----------------------------------------------------------------------
def fields(cfg):
    return {f: getattr(cfg, f) for f, _ in cfg._fields_ if f not in ("window", "resample_taps")}


def test_rejected_setters_change_nothing(gpu):
    bad = _lib.ErrInvalidArgument
    h = gpu_freeze(256, 64, 2, mix=0.7)
    before = fields(h.config())
    for call in (lambda: h.SetSampleRate(0), lambda: h.SetSampleRate(float("nan")), lambda: h.SetFrameSize(100),
                 lambda: h.SetFrameSize(32), lambda: h.SetFrameSize(8192), lambda: h.SetHopSize(0),
                 lambda: h.SetHopSize(256), lambda: h.SetHopSize(12.5), lambda: h.SetMix(-0.1), lambda: h.SetMix(1.5),
                 lambda: h.SetMix(float("nan")), lambda: h.SetPhaseMode(2)):
        with pytest.raises(bad):
            call()
    with pytest.raises(ValueError):
        h.SetWindowType(6)  # window.TypeKaiser: no table for it
    assert fields(h.config()) == before
    for t in (P.WindowRectangular, P.WindowHamming, P.WindowBlackman, P.WindowHann):
        h.SetWindowType(t)
        assert h.WindowType() == t
    p = gpu_pitch(1.5, 256, 64, 2)
    before = fields(p.config())
    for call in (lambda: p.SetPitchRatio(0), lambda: p.SetPitchRatio(0.1), lambda: p.SetPitchRatio(6),
                 lambda: p.SetPitchRatio(float("nan")), lambda: p.SetPitchRatio(float("inf")),
                 lambda: p.SetPitchSemitones(float("nan")), lambda: p.SetSampleRate(0), lambda: p.SetFrameSize(1000),
                 lambda: p.SetFrameSize(32), lambda: p.SetFrameSize(8192), lambda: p.SetAnalysisHop(0),
                 lambda: p.SetAnalysisHop(256)):
        with pytest.raises(bad):
            call()
    assert fields(p.config()) == before
    for rate in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(bad):
            P.SpectralFreeze(rate)
        with pytest.raises(bad):
            P.SpectralPitchShifter(rate)
    with pytest.raises(bad):
        P.SpectralFreeze(FS, 1, frame_size=8192, hop_size=2048)
    d = P.SpectralPitchShifter(FS)
    assert (d.PitchRatio(), d.FrameSize(), d.AnalysisHop(), d.SynthesisHop(), d.EffectivePitchRatio()) == \
        (1.0, 1024, 256, 256, 1.0)


# ---- buffers -------------------------------------------------------------------------------
@pytest.mark.parametrize("make", [lambda c: gpu_freeze(256, 64, c), lambda c: gpu_freeze(256, 64, c, frozen=True),
                                  lambda c: gpu_pitch(1.1, 256, 64, c), lambda c: gpu_pitch(1.5, 256, 64, c)],
                         ids=["unfrozen", "frozen", "binshift", "stretch"])
def test_device_entry_point_and_stride(gpu, make):
    channels, n, stride = 3, 549, 549 + 11
    x = K.noise(n, channels)
    want = run(make(channels), x)
    pad = np.full((channels, stride), 7.25)
    pad[:, :n] = x
    d = torch.from_numpy(pad).to(DEV)
    torch.cuda.synchronize()
    make(channels).process_device(d.data_ptr(), stride, n, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = d.cpu().numpy()
    same_bits(got[:, :n], want, "host and device entry points")
    assert np.all(got[:, n:] == 7.25), "the padding is untouched"


# ---- graph -----------------------------------------------------------------------------------
FREEZE_NODE = {"id": "fz", "type": "spectral-freeze", "params": {"frameSize": 300, "hopRatio": 0.25, "mix": 0.8,
                                                                  "phaseMode": "hold"}}
PITCH_NODE = {"id": "ps", "type": "pitch-spectral", "params": {"semitones": 5, "frameSize": 300, "hopRatio": 0.25}}


def _graph(nodes):
    ids = [E.INPUT_NODE_ID] + [n["id"] for n in nodes] + [E.OUTPUT_NODE_ID]
    return E._graph_json(nodes, list(zip(ids[:-1], ids[1:])))


def _chain_run(graph, x):
    ch = E.Chain(FS, x.shape[0])
    ch.LoadGraph(graph)
    y = x.copy()
    assert ch.Process(y)
    return ch, y


def test_graph_nodes_are_the_processors(gpu):
    x = K.noise(549, 3)
    ch, y = _chain_run(_graph([FREEZE_NODE]), x)
    spec = ch.spec[1]["specfreeze"]
    assert ch.spec[1]["type"] == "specfreeze" and ch.op_count()[0] == 1
    assert (spec["frame_size"], spec["hop_size"], spec["mix"], spec["phase_mode"], spec["frozen"]) == (256, 64, 0.8, 0, 1)
    same_bits(y, run(gpu_freeze(256, 64, 3, 0.8, R.PHASE_HOLD, True), x), "spectral-freeze")
    y2 = x.copy()
    assert ch.Process(y2)  # the capture carries over; Reset clears it
    ch.Reset()
    y3 = x.copy()
    assert ch.Process(y3)
    same_bits(y3, y, "spectral-freeze after Chain.Reset")
    ch, y = _chain_run(_graph([PITCH_NODE]), x)
    spec = ch.spec[1]["pitchspec"]
    assert (spec["frame_size"], spec["analysis_hop"], spec["pitch_ratio"]) == (256, 64, 2.0 ** (5 / 12.0))
    same_bits(y, run(gpu_pitch(2.0 ** (5 / 12.0), 256, 64, 3), x), "pitch-spectral")
    # the runtime's clamps
    for params, frame, hop in (({"frameSize": 5000, "hopRatio": 0.995}, 4096, 4055), ({"frameSize": 300, "hopRatio": 0.995}, 256, 253),
                               ({"frameSize": 100, "hopRatio": 0.001}, 256, 3), ({"frameSize": 384}, 256, 64),
                               ({"frameSize": 385}, 512, 128)):
        c = E.spectral_freeze_params(E.Params("n", "spectral-freeze", num={k: float(v) for k, v in params.items()}), FS)[0]
        assert (c.frame_size, c.hop_size, c.frozen, c.phase_mode, c.mix) == (frame, hop, 1, 1, 1.0), params
    ch, y = _chain_run(_graph([dict(FREEZE_NODE, params={"frameSize": 300, "hopRatio": 0.9999, "frozen": 0.4})]), x)
    assert ch.spec[1]["specfreeze"]["hop_size"] == 253 and ch.spec[1]["specfreeze"]["frozen"] == 0
    same_bits(y, run(gpu_freeze(256, 253, 3), x), "hopRatio clamped to 0.99, unfrozen")
    ch, y = _chain_run(_graph([dict(PITCH_NODE, params={"semitones": 0})]), x)
    same_bits(y, x, "pitch-spectral at 0 semitones: the identity shortcut")


def test_graph_behind_split_freq_and_through_sum(gpu):
    """split-freq -> {low: spectral-freeze, high: pitch-spectral} -> sum: the one-channel composition of the
    restatement on the bands the GPU's own crossover delivers."""
    x = K.noise(549, 3)
    xo = {"id": "xo", "type": "split-freq", "params": {"freqHz": 800}}
    fz = dict(FREEZE_NODE, params={"frameSize": 256, "hopRatio": 0.25, "frozen": 0})
    sm = {"id": "sm", "type": "sum"}
    bands = []
    for port in (0, 1):
        g = E._graph_json([xo], [(E.INPUT_NODE_ID, "xo"), ("xo", E.OUTPUT_NODE_ID, port)])
        bands.append(_chain_run(g, x)[1])
    ratio = 2.0 ** (5 / 12.0)
    bar_lo = K.bar_for(lambda: K.make_freeze(256, 64), bands[0], on_output=True)
    bar_hi = K.bar_for(lambda: K.make_pitch(ratio, 256, 64), bands[1], on_output=True)
    g = E._graph_json([xo, fz], [(E.INPUT_NODE_ID, "xo"), ("xo", "fz", 0), ("fz", E.OUTPUT_NODE_ID)])
    y = _chain_run(g, x)[1]
    for c in range(3):
        bar_lo.check(y[c], c, what="spectral-freeze behind the low band")
    g = E._graph_json([xo, fz, PITCH_NODE, sm], [(E.INPUT_NODE_ID, "xo"), ("xo", "fz", 0), ("xo", "ps", 1), ("fz", "sm"),
                                                 ("ps", "sm"), ("sm", E.OUTPUT_NODE_ID)])
    ch, y = _chain_run(g, x)
    for c in range(3):
        lo, hi = bar_lo.clean[c][0], bar_hi.clean[c][0]
        want = (lo + hi) * 0.5
        d = y[c] - want
        rms_bar = 0.5 * (bar_lo.rms * np.sqrt(np.mean(lo * lo)) + bar_hi.rms * np.sqrt(np.mean(hi * hi)))
        abs_bar = 0.5 * (bar_lo.abs + bar_hi.abs)
        rms, worst = float(np.sqrt(np.mean(d * d))), float(np.max(np.abs(d)))
        print(f"sum ch {c}: rms {rms:.3e} (bar {rms_bar:.3e}), max abs {worst:.3e} (bar {abs_bar:.3e})")
        assert rms <= rms_bar and worst <= abs_bar


def test_graph_refusals(gpu):
    for t in ("granular", "pitch-time", "vocoder", "dyn-multiband"):
        with pytest.raises(E.UnknownEffect):
            E.Chain(FS, 2).LoadGraph(_graph([{"id": "n", "type": t}]))
    L = _lib.lib()
    for t, make in ((E.FXN_SPECFREEZE, _lib.SpecFreezeConfig), (E.FXN_PITCHSPEC, _lib.PitchSpecConfig)):
        par, par2 = (C.c_int32 * 1)(0), (C.c_int32 * 1)(1)
        nodes = (E._Node * 3)()
        nodes[0].type = E.FXN_INPUT
        nodes[1].type, nodes[1].n_parents, nodes[1].parents = t, 1, C.cast(par, C.POINTER(C.c_int32))
        nodes[2].type, nodes[2].n_parents, nodes[2].parents = E.FXN_OUTPUT, 1, C.cast(par2, C.POINTER(C.c_int32))
        np_ = C.cast(nodes, C.c_void_p)
        cfgs = (_lib.FxNodeCfg * 3)()
        cp = C.cast(cfgs, C.c_void_p)
        h = C.c_void_p()
        bad = _lib.AD_ERR_INVALID_ARGUMENT
        assert L.ad_fx_graph_create(np_, 3, 2, 0, C.byref(h)) == bad and not h.value
        assert L.ad_fx_graph_create_cfg(np_, None, cp, 3, 2, 0, C.byref(h)) == bad and not h.value
        cfg = make()
        getattr(L, "ad_specfreeze_default_config" if t == E.FXN_SPECFREEZE else "ad_pitchspec_default_config")(C.byref(cfg), FS)
        cfgs[1].config, cfgs[1].bytes = C.addressof(cfg), C.sizeof(cfg)
        assert L.ad_fx_graph_create_cfg(np_, None, cp, 3, 2, 0, C.byref(h)) == bad and not h.value  # no window table
        w = P.spectral_window(P.WindowHann, 1024)
        cfg.window = _lib.ptr(w)
        cfgs[1].bytes = C.sizeof(cfg) - 4
        assert L.ad_fx_graph_create_cfg(np_, None, cp, 3, 2, 0, C.byref(h)) == bad and not h.value
        cfgs[1].bytes = C.sizeof(cfg)
        assert L.ad_fx_graph_create_cfg(np_, None, cp, 3, 2, 0, C.byref(h)) == _lib.AD_OK and h.value
        L.ad_fx_graph_destroy(h)
    for t in (14, 17, 22):
        nodes[1].type = t
        assert L.ad_fx_graph_create_cfg(np_, None, cp, 3, 2, 0, C.byref(h)) == 10  # AD_ERR_UNKNOWN_EFFECT
