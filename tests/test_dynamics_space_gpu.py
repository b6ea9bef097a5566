"""The dynamics processors (Compressor, Expander, Gate) and Freeverb against
the CPU oracle over the parts of their input space the other GPU tests leave
out: setters between calls, the limits of every parameter range, Freeverb's
comb flush, and edge input values (zeros, subnormals, overflow, Inf, NaN).

Every case runs in two or three calls (state crosses a call boundary), on 70
channels (two workgroups, the second ragged; channels 0, 33 and 69 checked, the
edge-value block has 8), on the fused, the staged, the default and, where the
chain admits it, the time-parallel engine; ad_fx_chain_last_engine says which
ran.  Each checked channel is compared with the oracle, never one engine with
another.

Tolerances.  Freeverb and EQ-only chains: bit-exact.  Dynamics: the project's
bar, rms <= 1e-12 s and max|d| <= 1e-12 s with s = max(1, rms(want)) (auto
makeup at -90 dB gives outputs of rms ~ 45 once the envelope has settled),
times max(1, A / 100), where
A = max|oracle(x) - oracle(x (1 + 2^-40))| / (s 2^-40) is the reference's own
sensitivity to a relative input perturbation, computed per case and channel
from the oracle alone.  A is below 15 for every case but one, so the bar is
the plain 1e-12 s nearly everywhere; it widens only where the reference itself
amplifies rounding by more than 100.  A gate or expander whose oracle output
jumps under the perturbation (a hold flip, A >> 1000) would be a knife-edge
case and gets another seed instead of a wider bar (no seed below needed
that; _sensitivity asserts A < 1000).  The edge-value block uses the plain bar.

Measured A (and s where it is not 1), the largest of the three checked
channels, CPU oracle:

  case                                         8000 Hz     44100 Hz     192000 Hz
  compressor ratio 1                           0.90        0.90         0.90
  ratio 100                                    8.8         6.4 (1.4)    3.6 (2.5)
  knee 0 / knee 24                             5.0 / 4.9   5.1 / 5.0    3.3 / 3.6 (1.5)
  attack 0.1 ms                                0.62        2.3          4.9
  attack 1000 ms                               2.3 (2.2)   2.3 (2.2)    2.3 (2.2)
  release 1 ms                                 3.9 (1.3)   3.2 (1.6)    2.4 (2.1)
  release 5000 ms                              5.0         5.1          3.4 (1.5)
  RMS window 1 ms                              5.0         5.1          3.5 (1.5)
  RMS window 1000 ms                           3.6 (1.4)   2.5 (2.1)    2.3 (2.2)
  attack 200 ms > release 5 ms                 2.4 (2.1)   2.3 (2.2)    2.3 (2.2)
  ratio 100, feedback, ratio-scaled, knee 0    437 (1.1)   295 (2.5)    2.3 (3.8)
  attack 1000 ms, release 1 ms                 2.3 (2.2)   2.3 (2.2)    2.3 (2.2)
  threshold -90 dB, auto makeup                8.6         12.8 (2.4)   13.3 (7.1)
  gate corners (range, hold, ratio)            0.90        0.90 .. 5.9  0.90 .. 6.4
  expander corners (range, ratio)              0.90 .. 6.2 0.90 .. 7.0  0.90 .. 6.8
  setter schedules (48000 Hz)                  0.50 .. 3.1

(s stays below 8 here because the 0.9 / 0.02 burst signal is 6000 samples long
and the -90 dB threshold's 89 dB of makeup meets an envelope that is still
attacking; the scaling by s is what keeps that case on the project's bar.)
"""
import functools
import json
import pathlib

import numpy as np
import pytest

import oracle_lib as O
from algodsp import _lib, design, processors as P, signals

pytestmark = pytest.mark.gpu

KATS = json.loads((pathlib.Path(__file__).parent / "golden" / "reference_kats.json").read_text())
FX = P.EffectChain
C_ALL, CHECK = 70, (0, 33, 69)
TOL = 1e-12
EPS40 = 2.0 ** -40
ENGINES = {"fused": FX.ENGINE_FUSED, "staged": FX.ENGINE_STAGED, "auto": FX.ENGINE_AUTO,
           "tp": FX.ENGINE_TIME_PARALLEL}


def _rms(a):
    return float(np.sqrt(np.mean(np.square(a)))) if len(a) else 0.0


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _dyn_engine(engine, serial):
    """capi_dsp.cpp fx_run for a dynamics-only chain: the gate (its hold counter)
    and the feedback topology are serial in the gain and run fused on every
    engine; otherwise the default is the time-parallel engine and the staged
    engine has no EQ stage to split."""
    if engine == FX.ENGINE_FUSED or serial:
        return FX.ENGINE_FUSED
    if engine in (FX.ENGINE_AUTO, FX.ENGINE_TIME_PARALLEL):
        return FX.ENGINE_TIME_PARALLEL
    return FX.ENGINE_STAGED_NOSPLIT


def _verb_engine(engine):
    if engine == FX.ENGINE_FUSED:
        return FX.ENGINE_FUSED
    return FX.ENGINE_TIME_PARALLEL if engine == FX.ENGINE_TIME_PARALLEL else FX.ENGINE_STAGED_NOSPLIT


def _chain_engine(engine):  # EQ (5 sections) + compressor + Freeverb
    if engine == FX.ENGINE_FUSED:
        return FX.ENGINE_FUSED
    return FX.ENGINE_STAGED if engine == FX.ENGINE_STAGED else FX.ENGINE_TIME_PARALLEL


# --------------------------------------------------------------------------- dynamics plumbing
GPU_KIND = {"compressor": P.Compressor, "expander": P.Expander, "gate": P.Gate}
SETTERS = {
    "threshold_db": "SetThreshold", "ratio": "SetRatio", "knee_db": "SetKnee", "attack_ms": "SetAttack",
    "release_ms": "SetRelease", "rms_window_ms": "SetRMSWindow", "sidechain_low_cut_hz": "SetSidechainLowCut",
    "sidechain_high_cut_hz": "SetSidechainHighCut", "auto_makeup": "SetAutoMakeup", "makeup_gain": "SetMakeupGain",
    "topology": "SetTopology", "detector_mode": "SetDetectorMode", "range_db": "SetRange", "hold_ms": "SetHold",
}


def _gpu_dyn(kind, fs, cfg, channels):
    return GPU_KIND[kind](fs, channels=channels, **cfg)


def _oracle_dyn(kind, fs, cfg):
    return O.Compressor(fs, **cfg) if kind == "compressor" else O.Expander(fs, gate=kind == "gate", **cfg)


def _gpu_change(obj, change):
    for k, v in change.items():
        getattr(obj, SETTERS[k])(v)


def _oracle_change(o, change):
    for k, v in change.items():
        if k == "makeup_gain":
            o.set_makeup_gain(v)
        else:
            o.reconfigure(**{k: v})


def _serial(kind, cfg):
    return kind == "gate" or cfg.get("topology", 0) == 1


def _oracle_run(kind, fs, cfg, x, cuts, changes):
    """One channel through the oracle with the schedule: ([block outputs], [metrics after each block])."""
    o = _oracle_dyn(kind, fs, cfg)
    outs, mets = [], []
    edges = [0, *cuts, len(x)]
    for i in range(len(edges) - 1):
        if i:
            _oracle_change(o, changes[i - 1])
        outs.append(o.process_in_place(x[edges[i]:edges[i + 1]]))
        mets.append(o.metrics())
    return outs, mets


def _sensitivity(kind, fs, cfg, x, cuts, changes, want):
    """(s, A) of the module docstring for one channel, from the oracle alone."""
    pert, _ = _oracle_run(kind, fs, cfg, x * (1.0 + EPS40), cuts, changes)
    s = max(1.0, _rms(want))
    A = float(np.max(np.abs(np.concatenate(pert) - want))) / (s * EPS40)
    assert A < 1000.0, ("knife-edge case: choose another seed", kind, cfg, A)
    return s, A


@functools.lru_cache(maxsize=None)
def _burst(n, hi, lo, seed0):
    env = np.where((np.arange(n) // 900) % 2 == 0, hi, lo)
    x = np.stack([env * signals.white_noise(n, seed0 + c) for c in range(C_ALL)])
    x.setflags(write=False)
    return x


def _run_dyn_case(kind, fs, cfg, x, cuts, changes, engines=ENGINES, report=None):
    """The schedule on every engine against the oracle: outputs and Metrics()
    after every call, for the channels in CHECK."""
    edges = [0, *cuts, x.shape[1]]
    ref = {}
    for c in CHECK:
        outs, mets = _oracle_run(kind, fs, cfg, x[c], cuts, changes)
        s, A = _sensitivity(kind, fs, cfg, x[c], cuts, changes, np.concatenate(outs))
        ref[c] = (outs, mets, s, max(1.0, A / 100.0))
        if report is not None:
            report.append(A)
    for name, engine in engines.items():
        g = _gpu_dyn(kind, fs, cfg, x.shape[0])
        g.SetEngine(engine)
        now = dict(cfg)
        for i in range(len(edges) - 1):
            if i:
                _gpu_change(g, changes[i - 1])
                now.update(changes[i - 1])
            blk = x[:, edges[i]:edges[i + 1]].copy()
            g.ProcessInPlace(blk)
            ran = g.LastEngine()[0]
            assert ran == _dyn_engine(engine, _serial(kind, now)), (name, i, ran)
            # metrics: the processors' 1e-12 relative bar, 1e-11 on the time-parallel
            # engine (test_staged_engine_matches_fused), scaled like the outputs'
            mtol = 1e-11 if ran == FX.ENGINE_TIME_PARALLEL else 1e-12
            for c in CHECK:
                outs, mets, s, k = ref[c]
                d = blk[c] - outs[i]
                print(f"{kind} {name} call {i} ch {c}: rms {_rms(d):.3e} max {np.max(np.abs(d)):.3e} bar {TOL * s * k:.3e}")
                assert _rms(d) <= TOL * s * k, (name, i, c, _rms(d), s, k)
                assert float(np.max(np.abs(d))) <= TOL * s * k, (name, i, c, float(np.max(np.abs(d))), s, k)
                np.testing.assert_allclose(np.array(g.Metrics(c)), np.array(mets[i]), rtol=mtol * k, atol=0,
                                           err_msg=f"{name} call {i} ch {c}")
        g.close()


# --------------------------------------------------------------------------- B1: setter schedules
GATE_FAST = {"threshold_db": -20.0, "attack_ms": 0.1, "release_ms": 1.0, "hold_ms": 10.0, "knee_db": 0.0}
# the burst signal is loud on [0, 900), [1800, 2700), [3600, 4500), [5400, 6000) and quiet between
SCHEDULES = {
    "threshold": ("compressor", {}, [{"threshold_db": -35.0}, {"threshold_db": -10.0}], (2100, 4100)),
    "ratio-feedback-scaled": ("compressor", {"topology": 1, "feedback_ratio_scale": 1},
                              [{"ratio": 12.0}, {"ratio": 1.5}], (2100, 4100)),
    "knee-6-0-12": ("compressor", {"knee_db": 6.0}, [{"knee_db": 0.0}, {"knee_db": 12.0}], (2100, 4100)),
    "attack-release": ("compressor", {}, [{"attack_ms": 0.5, "release_ms": 400.0},
                                          {"attack_ms": 50.0, "release_ms": 5.0}], (2100, 4100)),
    # a default-constructed compressor has auto makeup on: SetMakeupGain must turn it off (core.go:201-210)
    "makeup-gain-then-auto": ("compressor", {}, [{"makeup_gain": 6.0}, {"auto_makeup": True}], (2100, 4100)),
    "rms-window-30-5-30-rms": ("compressor", {"detector_mode": 1, "rms_window_ms": 30.0},
                               [{"rms_window_ms": 5.0}, {"rms_window_ms": 30.0}], (1300, 4100)),
    # peak mode: the window only sizes an unused ring; the envelope and the metrics carry on
    "rms-window-peak": ("compressor", {}, [{"rms_window_ms": 5.0}, {"rms_window_ms": 30.0}], (1300, 4100)),
    "detector-peak-rms-peak": ("compressor", {"rms_window_ms": 10.0}, [{"detector_mode": 1}, {"detector_mode": 0}],
                               (2100, 4100)),
    # a cut set to 0 zeroes that one-pole (core.go:606-650): turned on again it starts from zero
    "sidechain-on-off-on": ("compressor", {"sidechain_low_cut_hz": 80.0, "sidechain_high_cut_hz": 6000.0},
                            [{"sidechain_low_cut_hz": 0.0, "sidechain_high_cut_hz": 0.0},
                             {"sidechain_high_cut_hz": 6000.0, "sidechain_low_cut_hz": 80.0}], (2100, 4100)),
    "sidechain-moved": ("compressor", {"sidechain_low_cut_hz": 80.0, "sidechain_high_cut_hz": 6000.0},
                        [{"sidechain_low_cut_hz": 200.0}, {"sidechain_high_cut_hz": 3000.0}], (2100, 4100)),
    "topology-ff-fb-ff": ("compressor", {}, [{"topology": 1}, {"topology": 0}], (2100, 4100)),
    # both changes land while the hold counts down (quiet stretches): it must keep counting
    "gate-hold-range-in-countdown": ("gate", GATE_FAST, [{"hold_ms": 50.0, "range_db": -30.0},
                                                         {"hold_ms": 5.0, "range_db": -80.0}], (1300, 3000)),
    "gate-threshold-ratio-knee": ("gate", {}, [{"threshold_db": -30.0, "ratio": 4.0},
                                               {"knee_db": 0.0, "attack_ms": 1.0, "release_ms": 20.0}], (2100, 4100)),
    "gate-rms-window-topology": ("gate", {"detector_mode": 1, "rms_window_ms": 20.0, "threshold_db": -25.0},
                                 [{"rms_window_ms": 3.0}, {"topology": 1}], (1300, 4100)),
    "expander-threshold-ratio-range": ("expander", {}, [{"threshold_db": -25.0, "ratio": 4.0, "range_db": -30.0},
                                                        {"knee_db": 0.0, "detector_mode": 1}], (2100, 4100)),
    "expander-feedback-rms-window": ("expander", {"topology": 1, "detector_mode": 1, "rms_window_ms": 20.0,
                                                  "threshold_db": -25.0},
                                     [{"rms_window_ms": 3.0}, {"topology": 0, "sidechain_high_cut_hz": 5000.0}],
                                     (1300, 4100)),
}


@pytest.mark.parametrize("case", list(SCHEDULES), ids=list(SCHEDULES))
def test_setter_schedule_vs_oracle(gpu, case):
    """A | change | B | change | C: the reference's setters between calls
    (core.go:101-250, gate.go:196-234) re-derive parameters and keep the
    envelope, the feedback memory, the metrics and the hold counter; only a
    changed RMS window length restarts the ring, only a cut set to 0 clears
    its filter.  The oracle gets the same changes through reconfigure()."""
    kind, cfg, changes, cuts = SCHEDULES[case]
    _run_dyn_case(kind, 48000.0, cfg, _burst(6000, 0.5, 0.003, 60), cuts, changes)


def test_gate_hold_counts_on_through_setters(gpu):
    """The gate-hold schedule's premise, from the oracle: at both change points
    the hold counter is strictly between 0 and its full value."""
    kind, cfg, changes, cuts = SCHEDULES["gate-hold-range-in-countdown"]
    x = _burst(6000, 0.5, 0.003, 60)
    for c in CHECK:
        o = _oracle_dyn(kind, 48000.0, cfg)
        o.process_in_place(x[c][:cuts[0]])
        assert 0 < o.hold_counter() < 480
        _oracle_change(o, changes[0])
        o.process_in_place(x[c][cuts[0]:cuts[1]])
        assert 0 < o.hold_counter() < 2400


def test_gate_setter_limits(gpu):
    """gate_test.go:199-291: the values SetHold / SetRelease / SetRange accept
    and reject; a rejected value leaves the gate as it was."""
    k = KATS["dynamics_setters"]["gate"]
    nonfinite = {"nan": float("nan"), "inf": float("inf"), "-inf": float("-inf")}
    g = P.Gate(float(KATS["dynamics_setters"]["sample_rate"]), channels=2)
    for field, vals in k.items():
        for v in vals["valid"]:
            getattr(g, SETTERS[field])(float(v))
        for v in vals["invalid"]:
            with pytest.raises(_lib.ADError) as e:
                getattr(g, SETTERS[field])(nonfinite.get(v, v))
            assert e.value.code == _lib.AD_ERR_INVALID_ARGUMENT, (field, v)
    # the last accepted value of each is what the gate holds
    assert (g.hold_ms, g.range_db, g.cfg.release_ms) == (5000.0, -120.0, 5000.0)
    g.close()


# --------------------------------------------------------------------------- B2: range corners
RATES = (8000.0, 44100.0, 192000.0)
COMP_CORNERS = {
    "ratio-1": {"ratio": 1.0},
    "ratio-100": {"ratio": 100.0},
    "knee-0": {"knee_db": 0.0},
    "knee-24": {"knee_db": 24.0},
    "attack-0.1": {"attack_ms": 0.1},
    "attack-1000": {"attack_ms": 1000.0},
    "release-1": {"release_ms": 1.0},
    "release-5000": {"release_ms": 5000.0},
    # 192 kHz: a 192000-slot ring per channel that never fills; 8 kHz: 8 slots that wrap constantly
    "rms-window-1": {"detector_mode": 1, "rms_window_ms": 1.0},
    "rms-window-1000": {"detector_mode": 1, "rms_window_ms": 1000.0},
    "attack-slower-than-release": {"attack_ms": 200.0, "release_ms": 5.0},  # env_c2 < 0 (dsp_device.hpp env_step)
    "ratio-100-feedback-scaled-knee-0": {"ratio": 100.0, "topology": 1, "feedback_ratio_scale": 1, "knee_db": 0.0},
    "attack-1000-release-1": {"attack_ms": 1000.0, "release_ms": 1.0},
    "threshold--90-auto-makeup": {"threshold_db": -90.0, "auto_makeup": 1},
}
# threshold -20 dB, a 1 ms release (and hold): the 0.02 stretches close the gate / expander at every rate
# (with the constructors' -40 / -35 dB and 100 ms they would stay open throughout)
GATE_BASE = {"threshold_db": -20.0, "release_ms": 1.0}
GATE_HOLD = {"hold_ms": 1.0}  # the gate's 50 ms would outlast the 900-sample quiet stretches above 18 kHz
GATE_CORNERS = {
    "gate-range--120": ("gate", {"range_db": -120.0}),
    "gate-range-0": ("gate", {"range_db": 0.0}),
    "gate-hold-0": ("gate", {"hold_ms": 0.0}),
    "gate-hold-5000": ("gate", {"hold_ms": 5000.0}),
    "gate-ratio-1": ("gate", {"ratio": 1.0}),
    "gate-ratio-100": ("gate", {"ratio": 100.0}),
    "expander-range--120": ("expander", {"range_db": -120.0}),
    "expander-range-0": ("expander", {"range_db": 0.0}),
    "expander-ratio-1": ("expander", {"ratio": 1.0}),
    "expander-ratio-100": ("expander", {"ratio": 100.0}),
}


@pytest.mark.parametrize("fs", RATES, ids=lambda f: f"{int(f)}Hz")
@pytest.mark.parametrize("corner", list(COMP_CORNERS), ids=list(COMP_CORNERS))
def test_compressor_range_corners(gpu, corner, fs):
    """Every limit check_comp_config admits, and three combinations, at 8, 44.1
    and 192 kHz, on the 0.9 / 0.02 burst signal, two calls."""
    _run_dyn_case("compressor", fs, COMP_CORNERS[corner], _burst(6000, 0.9, 0.02, 60), (2500,), [{}])


@pytest.mark.parametrize("fs", RATES, ids=lambda f: f"{int(f)}Hz")
@pytest.mark.parametrize("corner", list(GATE_CORNERS), ids=list(GATE_CORNERS))
def test_gate_expander_range_corners(gpu, corner, fs):
    """The gate's and the expander's own limits: range -120 and 0 dB, hold 0 and
    5000 ms, ratio 1 and 100."""
    kind, cfg = GATE_CORNERS[corner]
    _run_dyn_case(kind, fs, {**GATE_BASE, **(GATE_HOLD if kind == "gate" else {}), **cfg}, _burst(6000, 0.9, 0.02, 60), (2500,), [{}])


# --------------------------------------------------------------------------- B3: Freeverb
COMB_LEN = (1116, 1188, 1277, 1356, 1422, 1491, 1557, 1617)  # reverb.go:12-19
AP_LEN = (556, 441, 341, 225)                                  # reverb.go:21-24


def _freeverb_restated(x, wet, dry, room, damp, gain, flush):
    """reverb.go:57-68, 101-117, 169-182 in a few lines: eight parallel damped
    combs summed in order, four allpasses in series, wet / dry mix; `flush`
    switches the comb's `if |filterStore| < 1e-23 { filterStore = 0 }`."""
    n = len(x)
    xg = (gain * np.asarray(x)).tolist()
    d1, d2 = damp, 1 - damp
    acc = np.zeros(n)
    for L in COMB_LEN:
        buf, idx, fs, out = [0.0] * L, 0, 0.0, [0.0] * n
        for t in range(n):
            o = buf[idx]
            fs = o * d2 + fs * d1
            if flush and abs(fs) < 1e-23:
                fs = 0.0
            buf[idx] = xg[t] + fs * room
            idx = idx + 1 if idx + 1 < L else 0
            out[t] = o
        acc = acc + np.array(out)
    for L in AP_LEN:  # a block of L samples reads the line before it writes it
        buf, out = np.zeros(L), np.empty(n)
        for t0 in range(0, n, L):
            m = min(L, n - t0)
            bo, inp = buf[:m].copy(), acc[t0:t0 + m]
            out[t0:t0 + m] = bo - inp
            buf[:m] = inp + bo * 0.5
        acc = out
    return acc * wet + np.asarray(x) * dry


VERB_FLUSH = {
    # 500 samples of noise at 0.5, then silence: the tail decays through 1e-23 inside the test
    "burst-silence": dict(params=(0.22, 1.0, 0.3, 0.45, 0.015), n=30000, scale=0.5, burst=500),
    # noise at 1e-21: the comb stores hover around the flush threshold from the start
    "noise-1e-21": dict(params=(0.22, 1.0, 0.72, 0.45, 0.015), n=8000, scale=1e-21, burst=None),
}


@functools.lru_cache(maxsize=None)
def _verb_flush_input(case):
    v = VERB_FLUSH[case]
    x = np.stack([v["scale"] * signals.white_noise(v["n"], 700 + c) for c in range(C_ALL)])
    if v["burst"]:
        x[:, v["burst"]:] = 0.0
    x.setflags(write=False)
    return x


def _verb_oracle(params, x, cuts=()):
    o = O.Freeverb()
    o.set(*params)
    return o.process_in_place(x)


def _flush_premise(case, x, params, want):
    """From the oracle side alone: without the flush the output differs from
    the oracle's inside the test length (so the kernels' flush is exercised),
    and the restatement with the flush is the oracle bit for bit."""
    first = {}
    for c in CHECK:
        off = _freeverb_restated(x[c], *params, flush=False)
        diff = np.flatnonzero(_bits(off) != _bits(want[c]))
        assert diff.size, (case, c, "the flush never acts")
        first[c] = (int(diff[0]), int(diff.size))
    assert np.array_equal(_bits(_freeverb_restated(x[0], *params, flush=True)), _bits(want[0]))
    return first


@pytest.mark.parametrize("case", list(VERB_FLUSH), ids=list(VERB_FLUSH))
def test_freeverb_comb_flush_bit_exact(gpu, case):
    """The comb's flush-to-zero (reverb.go:108-110) in every kernel that has it:
    k_chain (fused), k_fx_comb (staged; also the default for a Freeverb-only
    chain) and k_fxtp_verb (time-parallel), bit-exact against the oracle on
    inputs where the flush changes the output.  Measured first differing
    sample / differing samples without the flush, channels 0, 33, 69:
    burst-silence 13923 / 8860, 16397 / 8798, 14405 / 9516 of 30000;
    noise-1e-21 2232 / 5768 of 8000 on each.

    The time-parallel kernel runs a comb piece as lane segments whose damping
    filter warms up from zero; where the flush acts on the serial run and not
    on the warm-up a segment starts off the serial value (before
    comb_piece_settle in fx_tp.hip, channel 33 of burst-silence differed at
    sample 21413 on that engine)."""
    v = VERB_FLUSH[case]
    x, params, n = _verb_flush_input(case), v["params"], v["n"]
    want = {c: _verb_oracle(params, x[c]) for c in CHECK}
    first = _flush_premise(case, x, params, want)
    print(case, "first difference / count without the flush:", first)
    assert all(f < n for f, _ in first.values())
    for name, engine in ENGINES.items():
        rv = P.Reverb(channels=C_ALL)
        rv.SetWet(params[0]), rv.SetDry(params[1]), rv.SetRoomSize(params[2]), rv.SetDamp(params[3])
        rv.SetGain(params[4])
        rv.SetEngine(engine)
        a, b = x[:, :n // 3 + 1].copy(), x[:, n // 3 + 1:].copy()
        rv.ProcessInPlace(a)
        assert rv.LastEngine()[0] == _verb_engine(engine), name
        rv.ProcessInPlace(b)
        got = np.concatenate([a, b], axis=1)
        for c in CHECK:
            bad = np.flatnonzero(_bits(got[c]) != _bits(want[c]))
            assert bad.size == 0, (name, c, int(bad[0]), bad.size)
        rv.close()


def test_freeverb_comb_flush_in_chain_bit_exact(gpu):
    """The flush in the full chain's kernels (k_chain_pipe on the fused engine,
    the staged pipeline's comb stage behind the EQ and gain stages): EQ ->
    compressor -> Freeverb with the compressor at ratio 1, manual makeup 0 dB,
    which multiplies by exactly 1.0 on both sides, so the chain is bit-exact
    (the time-parallel engine's EQ is a tolerance and is left to the
    Freeverb-only test).  The 1e-21 noise: behind the EQ's slow low-frequency
    sections a burst's tail would not reach the threshold inside the test."""
    fs = 48000.0
    v = VERB_FLUSH["noise-1e-21"]
    params, n = v["params"], v["n"]
    x = _verb_flush_input("noise-1e-21")
    eq = design.config5_eq(fs)
    comp = {"ratio": 1.0, "auto_makeup": 0, "makeup_db": 0.0}
    mid, want = {}, {}
    for c in CHECK:
        u = x[c].copy()
        for co, g in eq:
            u, _ = O.biquad_chain_block(np.ravel(co), np.zeros(2 * len(co)), g, u)
        mid[c] = O.Compressor(fs, **comp).process_in_place(u)
        assert np.array_equal(_bits(mid[c]), _bits(u))  # the ratio-1 compressor is the identity
        want[c] = _verb_oracle(params, mid[c])
    print("chain: first difference / count without the flush:", _flush_premise("chain", mid, params, want))
    for name in ("fused", "staged"):
        fx = P.EffectChain(C_ALL, eq, comp, params, fs)
        fx.SetEngine(ENGINES[name])
        a, b = x[:, :n // 3 + 1].copy(), x[:, n // 3 + 1:].copy()
        fx.Process(a)
        assert fx.LastEngine()[0] == _chain_engine(ENGINES[name]), name
        fx.Process(b)
        got = np.concatenate([a, b], axis=1)
        for c in CHECK:
            bad = np.flatnonzero(_bits(got[c]) != _bits(want[c]))
            assert bad.size == 0, (name, c, int(bad[0]), bad.size)
        fx.close()


def test_freeverb_schedule_bit_exact(gpu):
    """SetRoomSize / SetDamp / SetWet / SetGain between calls keep the delay
    lines and filter stores (reverb.go:192-220); Reset() between calls clears
    them (reverb.go:158-166).  Five calls, bit-exact against the oracle driven
    the same way, on every engine."""
    n = 7000
    x = np.stack([0.5 * signals.white_noise(n, 800 + c) for c in range(C_ALL)])
    edges = [0, 1500, 3000, 4200, 5600, n]
    steps = [None, ("SetRoomSize", 0.9), ("SetDamp", 0.1), "reset", ("SetWet", 0.6)]
    want = {}
    for c in CHECK:
        o, p, outs = O.Freeverb(), dict(wet=0.22, dry=1.0, room=0.72, damp=0.45, gain=0.015), []
        for i, st in enumerate(steps):
            if st == "reset":
                o.reset()
            elif st:
                p[{"SetRoomSize": "room", "SetDamp": "damp", "SetWet": "wet", "SetGain": "gain"}[st[0]]] = st[1]
                if st[0] == "SetWet":
                    p["gain"] = 0.03  # SetGain rides along with the last change
                o.set(p["wet"], p["dry"], p["room"], p["damp"], p["gain"])
            outs.append(o.process_in_place(x[c][edges[i]:edges[i + 1]]))
        want[c] = np.concatenate(outs)
    for name, engine in ENGINES.items():
        rv = P.Reverb(channels=C_ALL)
        rv.SetEngine(engine)
        parts = []
        for i, st in enumerate(steps):
            if st == "reset":
                rv.Reset()
            elif st:
                getattr(rv, st[0])(st[1])
                if st[0] == "SetWet":
                    rv.SetGain(0.03)
            blk = x[:, edges[i]:edges[i + 1]].copy()
            rv.ProcessInPlace(blk)
            assert rv.LastEngine()[0] == _verb_engine(engine), name
            parts.append(blk)
        got = np.concatenate(parts, axis=1)
        for c in CHECK:
            bad = np.flatnonzero(_bits(got[c]) != _bits(want[c]))
            assert bad.size == 0, (name, c, int(bad[0]), bad.size)
        rv.close()


# --------------------------------------------------------------------------- B4: edge values
EDGE_N, EDGE_CUT, EDGE_BAD = 6000, 2500, 1700  # the bad sample is in the first call: its state crosses the boundary
# channel roles of the edge block
E_PZERO, E_NZERO, E_SILENCE, E_SUBNORMAL, E_HUGE, E_INF, E_CLEAN, E_NAN = range(8)
E_POISON = (E_HUGE, E_INF, E_NAN)


@functools.lru_cache(maxsize=None)
def _edge_block(poisoned=True):
    x = np.stack([0.5 * signals.white_noise(EDGE_N, 900 + c) for c in range(8)])
    x[E_PZERO, :] = 0.0
    x[E_NZERO, :] = -0.0
    x[E_SILENCE, 1000:1800] = 0.0          # a silence run inside noise ...
    x[E_SILENCE, 5000:] = 5e-324           # ... and a tail of the smallest subnormal
    x[E_SUBNORMAL, :] = signals.white_noise(EDGE_N, 903) * 1e-310
    if poisoned:
        x[E_HUGE, EDGE_BAD] = 1e200        # finite in the peak detector; its square overflows in the RMS detector
        x[E_INF, EDGE_BAD] = np.inf
        x[E_NAN, EDGE_BAD] = np.nan
    x.setflags(write=False)
    return x


def _edge_run(make, engine, x, expected):
    h = make()
    h.SetEngine(engine)
    a, b = x[:, :EDGE_CUT].copy(), x[:, EDGE_CUT:].copy()
    h._process(a)
    assert h.LastEngine()[0] == expected, (engine, h.LastEngine()[0])
    h._process(b)
    return h, np.concatenate([a, b], axis=1)


def _edge_check(label, make, oracle, expected_engine, exact, engines=ENGINES, nan_forever=()):
    """The edge block through `make()` on each engine against `oracle(x_c)`.

    * the channels without a poisoned sample equal, bit for bit, a run in which
      the poisoned channels hold clean noise (no leak across a wave's lanes);
    * every channel equals the oracle up to the sample before the bad one, and
      the finite channels over the whole stream (bit-exact, or the dynamics bar);
    * from the bad sample on, the NaN mask and the exact zeros equal the
      oracle's, and the remaining samples meet the bar; for the channels in
      `nan_forever` the documented deviation holds instead (include/algodsp.h:
      NaN from the bad sample to the end of the stream);
    * after Reset() the next block equals a fresh handle's bits."""
    x, clean = _edge_block(True), _edge_block(False)
    with np.errstate(all="ignore"):
        want = [oracle(x[c]) for c in range(8)]
        # finite edge inputs meet the plain bar (no sensitivity scaling here)
        bars = [0.0 if exact else TOL * max(1.0, _rms(want[c][:EDGE_BAD] if c in E_POISON else want[c]))
                for c in range(8)]
    for name, engine in engines.items():
        exp = expected_engine(engine)
        h, got = _edge_run(make, engine, x, exp)
        h2, got_clean = _edge_run(make, engine, clean, exp)
        h2.close()
        for c in range(8):
            w, g = want[c], got[c]
            if c not in E_POISON:
                assert np.array_equal(_bits(g), _bits(got_clean[c])), (label, name, c, "a poisoned neighbour leaked")
            end = EDGE_BAD if c in E_POISON else EDGE_N
            d = np.abs(g[:end] - w[:end])
            print(f"{label} {name} ch {c}: max {float(np.max(d)):.3e} bar {bars[c]:.3e}")
            assert np.all(np.isfinite(g[:end])) and float(np.max(d)) <= bars[c], (label, name, c, float(np.max(d)))
            if c in (E_PZERO, E_NZERO) or exact:
                # signed zeros keep their sign; bit-exact chains keep every bit
                assert np.array_equal(_bits(g[:end]), _bits(w[:end])), (label, name, c)
            if c not in E_POISON:
                continue
            gt, wt = g[EDGE_BAD:], w[EDGE_BAD:]
            if c in nan_forever:
                assert np.all(np.isnan(gt)), (label, name, c, "documented: NaN until Reset")
                continue
            assert np.array_equal(np.isnan(gt), np.isnan(wt)), \
                (label, name, c, "NaN mask", int(np.isnan(gt).sum()), int(np.isnan(wt).sum()))
            assert np.array_equal(gt == 0.0, wt == 0.0), (label, name, c, "exact zeros")
            assert np.array_equal(np.isinf(gt), np.isinf(wt)), (label, name, c, "infinities")
            fin = np.isfinite(wt)
            if exact:
                assert np.array_equal(_bits(gt[fin]), _bits(wt[fin])), (label, name, c)
            else:
                if fin[0]:  # the bad sample's own output (the 1e200 one: ~1e200 times the gain), relative
                    assert abs(gt[0] - wt[0]) <= TOL * max(1.0, abs(wt[0])), (label, name, c, gt[0], wt[0])
                fin[0] = False
                if fin.any():
                    assert float(np.max(np.abs(gt[fin] - wt[fin]))) <= TOL * max(1.0, _rms(wt[fin])), (label, name, c)
        # Reset() clears whatever the bad samples left in the state
        h.Reset()
        fresh = make()
        fresh.SetEngine(engine)
        a, b = clean[:, :EDGE_CUT].copy(), clean[:, :EDGE_CUT].copy()
        h._process(a)
        fresh._process(b)
        assert np.array_equal(_bits(a), _bits(b)), (label, name, "Reset() left state behind")
        h.close()
        fresh.close()


EDGE_DYN = {
    "compressor-peak": ("compressor", {}),
    "compressor-rms": ("compressor", {"detector_mode": 1, "rms_window_ms": 5.0}),
    "compressor-feedback": ("compressor", {"topology": 1}),
    "gate": ("gate", {"threshold_db": -20.0}),
    "expander-rms": ("expander", {"detector_mode": 1, "rms_window_ms": 5.0}),
}


@pytest.mark.parametrize("case", list(EDGE_DYN), ids=list(EDGE_DYN))
def test_dynamics_edge_values(gpu, case):
    """Zeros of both signs (the `level <= 0` branches), a silence run, subnormal
    noise, a 5e-324 tail, a 1e200 sample (finite in the peak detector, an
    overflow in the RMS detector's square), an Inf and a NaN sample, with a
    clean channel between the poisoned ones.  With the attack faster than the
    release (env_c2 > 0) the device's envelope step agrees with the
    reference's on a non-finite level: same NaN mask, same exact zeros."""
    kind, cfg = EDGE_DYN[case]
    fs = 48000.0
    _edge_check(case, lambda: _gpu_dyn(kind, fs, cfg, 8), lambda v: _oracle_dyn(kind, fs, cfg).process_in_place(v),
                lambda e: _dyn_engine(e, _serial(kind, cfg)), exact=False)


def test_compressor_slow_attack_non_finite_documented(gpu):
    """The documented deviation (include/algodsp.h, ad_compressor_config): with
    an attack coefficient not above 1 - release coefficient (an attack slower
    than the release: env_c2 <= 0 in env_step's two-FMA form) an infinite
    detector level makes the envelope inf - inf = NaN, and the output stays
    NaN until Reset(), where the reference's envelope stays +Inf and its
    output is exact zeros.  The oracle shows the reference's side (zeros after
    the Inf sample), the device the documented one; everything before the bad
    sample, the finite channels, the NaN channel, lane isolation and Reset()
    hold as in test_dynamics_edge_values."""
    fs, cfg = 48000.0, {"attack_ms": 200.0, "release_ms": 5.0}
    with np.errstate(all="ignore"):
        w = O.Compressor(fs, **cfg).process_in_place(_edge_block(True)[E_INF])
    assert np.isnan(w[EDGE_BAD]) and np.all(w[EDGE_BAD + 1:] == 0.0)  # the reference: silence
    _edge_check("compressor-slow-attack", lambda: _gpu_dyn("compressor", fs, cfg, 8),
                lambda v: O.Compressor(fs, **cfg).process_in_place(v), lambda e: _dyn_engine(e, False), exact=False,
                nan_forever=(E_INF,))


def test_freeverb_edge_values_bit_exact(gpu):
    """The edge block through Freeverb: every finite output bit equals the
    oracle's (signed zeros, subnormals and the flush on the 5e-324 tail
    included), a 1e200 sample stays finite, and an Inf or NaN sample poisons
    the same samples as in the oracle.

    The 1e200 channel is what the time-parallel kernel's warm-started comb
    segments could not do before comb_piece_settle (fx_tp.hip): a warm-up
    forgets its start only relative to that start's size, and behind a 1e200
    sample the serial filter value stays far above 2^-60 of the following
    samples for ~630 samples."""
    params = (0.3, 0.8, 0.8, 0.3, 0.02)

    def make():
        rv = P.Reverb(channels=8)
        rv.SetWet(params[0]), rv.SetDry(params[1]), rv.SetRoomSize(params[2]), rv.SetDamp(params[3])
        rv.SetGain(params[4])
        return rv

    _edge_check("freeverb", make, lambda v: _verb_oracle(params, v), _verb_engine, exact=True)


def test_config5_chain_edge_values(gpu):
    """The edge block through EQ -> compressor -> Freeverb (config 5's chain):
    the dynamics bar on the finite samples, the oracle's NaN mask after a bad
    sample (the EQ's state turns NaN at once on both sides), lane isolation,
    Reset()."""
    fs = 48000.0
    eq = design.config5_eq(fs)
    comp = {"auto_makeup": 0, "makeup_db": 0.0}
    verb = (0.22, 1.0, 0.72, 0.45, 0.015)

    def oracle(v):
        u = v.copy()
        for co, g in eq:
            u, _ = O.biquad_chain_block(np.ravel(co), np.zeros(2 * len(co)), g, u)
        return _verb_oracle(verb, O.Compressor(fs, **comp).process_in_place(u))

    _edge_check("config5", lambda: P.EffectChain(8, eq, comp, verb, fs), oracle, _chain_engine, exact=False)
