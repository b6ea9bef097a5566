"""FDN reverb checks that need no GPU: the reference restatement
(tests/fdn_ref.py) against fdn_reverb_test.go and the reference's setter side
effects, the dependency bound the GPU kernel's blocks rest on, the host-only
part of the C ABI (defaults, validation, create without a device), the graph
compiler's fdn_params, and how far a last-place change of every sine moves the
output (the GPU path differs from the oracle by its math library's sine only)."""
import ctypes as C
import math

import numpy as np
import pytest

import fdn_ref as R
from algodsp import _lib, effectchain as E, signals


def rel_rms(a, b):
    return float(np.sqrt(np.mean((a - b) ** 2)) / np.sqrt(np.mean(b ** 2)))


def noise(n, channels=3, seed=0xFD00):
    """The FDN tests' input: `channels` rows of seeded white noise."""
    return np.stack([signals.white_noise(n, seed + c) for c in range(channels)])


# ---- fdn_reverb_test.go, on the restatement ---------------------------------
def test_process_in_place_matches_sample():
    x = np.sin(2 * math.pi * np.arange(128) / 31)
    r1, r2 = R.FDN(44100.0), R.FDN(44100.0)
    want = np.array([r1.process(x[i:i + 1])[0] for i in range(x.size)])
    assert np.max(np.abs(r2.process(x) - want)) <= 1e-12


def test_reset_restores_state():
    x = np.zeros(128)
    x[0] = 1
    r = R.FDN(44100.0)
    out1 = r.process(x)
    r.Reset()
    assert np.max(np.abs(r.process(x) - out1)) <= 1e-12


def test_impulse_tail_exists():
    r = R.FDN(44100.0)
    r.SetDry(0)
    x = np.zeros(4096)
    x[0] = 1
    assert np.any(np.abs(r.process(x)[1:]) > 1e-10)


# ---- the dependency bound ---------------------------------------------------
@pytest.mark.parametrize("mod_depth", [0.0, 0.002])
def test_block_form_equals_serial_up_to_the_bound(mod_depth):
    """Reading max(1, P) samples ahead of their writes changes nothing; one
    more sample does (with mod depth 0 every read sits at floor(delay) = P
    exactly, so sample P of a block of P + 1 reads sample 0's write)."""
    x = noise(1500, 1)[0]

    def run(block):
        r = R.FDN(8000.0)
        r.SetModDepth(mod_depth)
        return r.process(x, block)

    P = R.FDN(8000.0).block_bound()
    assert P == 278
    serial = run(1)
    np.testing.assert_array_equal(run(P), serial)
    if mod_depth == 0.0:
        assert np.any(run(P + 1) != serial)


def test_block_bound_at_tiny_rates():
    assert R.FDN(20.0).block_bound() == 1    # P = 0
    assert R.FDN(28.6).block_bound() == 1
    assert R.FDN(300.0).block_bound() == 10
    assert R.FDN(48000.0).block_bound() == 1672


# ---- setter side effects ----------------------------------------------------
def _warm(fs=8000.0):
    r = R.FDN(fs)
    r.SetModRate(1.0)
    r.process(noise(700, 1)[0])
    assert any(r.filterState) and r.lfoPhase > 0
    return r


def test_line_lengths_and_clamp():
    r = R.FDN(8000.0)
    for i, ln in enumerate(r.lines):
        want = max(math.ceil(R.DELAY_SAMPLES[i] * (8000.0 / 44100.0) + 0.002 * 8000.0) + 3, 4)
        assert len(ln.buf) == want and ln.max_delay == want - 3
    assert len(r.preDelayLine.buf) == 80 + 3
    tiny = R.FDN(20.0)
    assert len(tiny.preDelayLine.buf) == 4 and tiny.preDelayLine.max_delay == 1


def test_reconfiguring_setters():
    """SetSampleRate / SetPreDelay / SetModDepth: filter states zeroed, a line
    replaced (zeroed, writePos 0) only when its length changes, gains
    recomputed, lfoPhase kept."""
    r = _warm()
    phase = r.lfoPhase
    bufs = [list(ln.buf) for ln in r.lines]
    pos = [ln.pos for ln in r.lines]
    r.SetModDepth(0.002 - 1e-9)  # 16 samples -> 15.99..: the same ceil, the same lengths
    assert r.filterState == [0.0] * 8 and r.lfoPhase == phase
    assert [list(ln.buf) for ln in r.lines] == bufs and [ln.pos for ln in r.lines] == pos
    r = _warm()
    pre = list(r.preDelayLine.buf)
    r.SetModDepth(0.004)  # longer lines
    assert r.filterState == [0.0] * 8 and r.lfoPhase == phase
    assert all(not any(ln.buf) and ln.pos == 0 for ln in r.lines)
    assert list(r.preDelayLine.buf) == pre
    r = _warm()
    bufs = [list(ln.buf) for ln in r.lines]
    r.SetPreDelay(0.02)
    assert r.filterState == [0.0] * 8 and [list(ln.buf) for ln in r.lines] == bufs
    assert len(r.preDelayLine.buf) == 163 and not any(r.preDelayLine.buf) and r.preDelayLine.pos == 0
    r = _warm()
    r.SetSampleRate(11025.0)
    assert r.filterState == [0.0] * 8 and r.lfoPhase == phase
    assert all(not any(ln.buf) and ln.pos == 0 for ln in r.lines)
    assert r.feedbackGain == [math.pow(10, -3 * ((d * (11025.0 / 44100.0)) / 11025.0) / 1.8) for d in R.DELAY_SAMPLES]
    assert r.modDepthSamples == 0.002 * 11025.0 and r.preDelaySamples == 0.01 * 11025.0


def test_storing_setters_and_reset():
    r = _warm()
    fs, phase = list(r.filterState), r.lfoPhase
    bufs = [list(ln.buf) for ln in r.lines]
    g = list(r.feedbackGain)
    r.SetRT60(0.9)
    assert r.feedbackGain != g and r.filterState == fs and [list(ln.buf) for ln in r.lines] == bufs
    g = list(r.feedbackGain)
    r.SetWet(0.5), r.SetDry(0.25), r.SetDamp(0.9), r.SetModRate(0.3)
    assert (r.wet, r.dry, r.damp, r.modRateHz) == (0.5, 0.25, 0.9, 0.3)
    assert r.feedbackGain == g and r.filterState == fs and r.lfoPhase == phase
    assert [list(ln.buf) for ln in r.lines] == bufs
    r.Reset()
    assert r.lfoPhase == 0 and r.filterState == [0.0] * 8 and not any(r.preDelayLine.buf)
    assert all(not any(ln.buf) and ln.pos == 0 for ln in r.lines)


BAD_FDN_VALUES = [
    ("sample_rate", 0.0), ("sample_rate", -1.0), ("sample_rate", float("nan")), ("sample_rate", float("inf")),
    ("wet", -0.1), ("wet", float("nan")), ("wet", float("inf")),
    ("dry", -0.1), ("dry", float("nan")), ("dry", float("inf")),
    ("rt60_seconds", 0.0), ("rt60_seconds", -1.0), ("rt60_seconds", float("nan")), ("rt60_seconds", float("inf")),
    ("damp", -0.01), ("damp", 1.01), ("damp", float("nan")), ("damp", float("inf")),
    ("pre_delay_seconds", -0.001), ("pre_delay_seconds", float("nan")), ("pre_delay_seconds", float("inf")),
    ("mod_depth_seconds", -0.001), ("mod_depth_seconds", float("nan")), ("mod_depth_seconds", float("inf")),
    ("mod_rate_hz", -0.1), ("mod_rate_hz", float("nan")), ("mod_rate_hz", float("inf")),
]
GOOD_FDN_EDGES = [
    ("sample_rate", 5e-324), ("wet", 0.0), ("dry", 0.0), ("rt60_seconds", 5e-324), ("damp", 0.0), ("damp", 1.0),
    ("pre_delay_seconds", 0.0), ("mod_depth_seconds", 0.0), ("mod_rate_hz", 0.0),
]
_SETTER = {"sample_rate": "SetSampleRate", "wet": "SetWet", "dry": "SetDry", "rt60_seconds": "SetRT60",
           "damp": "SetDamp", "pre_delay_seconds": "SetPreDelay", "mod_depth_seconds": "SetModDepth",
           "mod_rate_hz": "SetModRate"}


def _cfg(fs=48000.0, **kv):
    cfg = _lib.FdnConfig()
    _lib.lib().ad_fdn_default_config(C.byref(cfg), fs)
    for k, v in kv.items():
        setattr(cfg, k, v)
    return cfg


@pytest.mark.parametrize("field,value", BAD_FDN_VALUES)
def test_rejected_value_changes_nothing_and_fails_validation(field, value):
    r = _warm()
    before = (r.sampleRate, r.wet, r.dry, r.rt60Seconds, r.damp, r.preDelaySeconds, r.modDepthSeconds, r.modRateHz,
              r.lfoPhase, list(r.filterState), list(r.feedbackGain), [list(ln.buf) for ln in r.lines])
    with pytest.raises(ValueError):
        getattr(r, _SETTER[field])(value)
    assert before == (r.sampleRate, r.wet, r.dry, r.rt60Seconds, r.damp, r.preDelaySeconds, r.modDepthSeconds,
                      r.modRateHz, r.lfoPhase, list(r.filterState), list(r.feedbackGain),
                      [list(ln.buf) for ln in r.lines])
    assert _lib.lib().ad_fdn_validate(C.byref(_cfg(**{field: value}))) == _lib.AD_ERR_INVALID_ARGUMENT


@pytest.mark.parametrize("field,value", GOOD_FDN_EDGES)
def test_validation_accepts_range_edges(field, value):
    getattr(R.FDN(48000.0), _SETTER[field])(value)
    assert _lib.lib().ad_fdn_validate(C.byref(_cfg(**{field: value}))) == _lib.AD_OK


def test_validation_null_and_oversized():
    L = _lib.lib()
    assert L.ad_fdn_validate(None) == _lib.AD_ERR_INVALID_ARGUMENT
    assert L.ad_fdn_validate(C.byref(_cfg())) == _lib.AD_OK
    # a line of more than 2^27 samples is refused (the reference would allocate it)
    assert L.ad_fdn_validate(C.byref(_cfg(fs=3e9))) == _lib.AD_ERR_INVALID_ARGUMENT
    assert L.ad_fdn_validate(C.byref(_cfg(pre_delay_seconds=1e300))) == _lib.AD_ERR_INVALID_ARGUMENT


def test_default_config_is_new_fdn_reverb():
    c = _cfg(12345.0)
    assert [getattr(c, f) for f, _ in c._fields_] == [12345.0, 0.2, 1.0, 1.8, 0.3, 0.01, 0.002, 0.1]
    r = R.FDN(12345.0)
    assert (r.sampleRate, r.wet, r.dry, r.rt60Seconds, r.damp, r.preDelaySeconds, r.modDepthSeconds,
            r.modRateHz) == (12345.0, 0.2, 1.0, 1.8, 0.3, 0.01, 0.002, 0.1)


def test_create_validates_before_the_device():
    L = _lib.lib()
    h = C.c_void_p()
    assert L.ad_fdn_create(C.byref(_cfg(damp=1.5)), 2, 0, C.byref(h)) == _lib.AD_ERR_INVALID_ARGUMENT
    assert not h.value
    assert L.ad_fdn_create(C.byref(_cfg()), 0, 0, C.byref(h)) == _lib.AD_ERR_INVALID_ARGUMENT
    assert L.ad_fdn_create(None, 1, 0, C.byref(h)) == _lib.AD_ERR_INVALID_ARGUMENT
    rc = L.ad_fdn_create(C.byref(_cfg()), 2, 0, C.byref(h))
    if _lib.device_count() == 0:
        assert rc == _lib.AD_ERR_NO_DEVICE and not h.value  # no CPU path
    else:
        assert rc == _lib.AD_OK
        L.ad_fdn_destroy(h)
    assert L.ad_fdn_set_param(None, 1, 0.5) == _lib.AD_ERR_INVALID_ARGUMENT
    assert L.ad_fdn_process_device(None, None, 0, 0, None) == _lib.AD_ERR_INVALID_ARGUMENT


# ---- the graph compiler -----------------------------------------------------
def test_fdn_params_defaults_and_clamps():
    c = E.fdn_params(E.Params("r", "reverb-fdn"), 48000.0)
    assert [getattr(c, f) for f, _ in c._fields_] == [48000.0, 0.22, 1.0, 1.8, 0.45, 0.01, 0.002, 0.1]
    hi = E.fdn_params(E.Params("r", "reverb-fdn", num=dict(wet=9, dry=9, rt60=99, preDelay=9, damp=9, modDepth=9,
                                                          modRate=9)), 44100.0)
    assert [getattr(hi, f) for f, _ in hi._fields_] == [44100.0, 1.5, 1.5, 8, 0.99, 0.1, 0.01, 1]
    lo = E.fdn_params(E.Params("r", "reverb-fdn", num=dict(wet=-1, dry=-1, rt60=0, preDelay=-1, damp=-1, modDepth=-1,
                                                          modRate=-1)), 44100.0)
    assert [getattr(lo, f) for f, _ in lo._fields_] == [44100.0, 0, 0, 0.2, 0, 0, 0, 0]
    nan = E.fdn_params(E.Params("r", "reverb-fdn", num=dict(wet=float("nan"), rt60=float("inf"))), 44100.0)
    assert (nan.wet, nan.rt60_seconds) == (0.22, 1.8)
    assert _lib.lib().ad_fdn_validate(C.byref(hi)) == _lib.AD_OK and _lib.lib().ad_fdn_validate(C.byref(lo)) == _lib.AD_OK


def _graph(node):
    return E._graph_json([node], [(E.INPUT_NODE_ID, node["id"]), (node["id"], E.OUTPUT_NODE_ID)])


@pytest.mark.parametrize("node", [{"id": "r", "type": "reverb-fdn"},
                                  {"id": "r", "type": "reverb", "params": {"model": "fdn"}},
                                  {"id": "r", "type": "reverb"}])
def test_graph_compiler_knows_the_reverb_nodes(node):
    """reverb-fdn and reverb compile; without a device they fail at the device,
    not as an unknown effect."""
    ch = E.Chain(48000.0, 2)
    if _lib.device_count() == 0:
        with pytest.raises(_lib.ADError) as e:
            ch.LoadGraph(_graph(node))
        assert e.value.code == _lib.AD_ERR_NO_DEVICE
    else:
        ch.LoadGraph(_graph(node))
        assert ch.spec[1]["type"] == ("verb" if node == {"id": "r", "type": "reverb"} else "fdn")


@pytest.mark.parametrize("t", ["chorus", "dyn-lookahead", "filter-moog", "vocoder"])
def test_unknown_effect_still_raises(t):
    with pytest.raises(E.UnknownEffect):
        E.Chain(48000.0, 2).LoadGraph(_graph({"id": "n", "type": t}))


# ---- the sine spread --------------------------------------------------------
# (sample rate, mod rate, n): the modulated cases of tests/test_fdn_gpu.py
MODULATED = [(8000.0, 0.1, 4096), (8000.0, 1.0, 4096), (48000.0, 0.1, 12000)]


@pytest.mark.parametrize("fs,rate,n", MODULATED)
def test_sine_spread(fs, rate, n):
    """Every sine moved by a random -1 / 0 / +1 ulp moves the output by less
    than 1e-13 relative RMS, a tenth of the GPU tests' bar: a math library
    whose sine is good to an ulp stays far inside that bar."""
    x = noise(n)
    for c in range(x.shape[0]):
        plain, nudged = R.FDN(fs), R.FDN(fs, sin=R.nudged_sin(0x51E + c))
        plain.SetModRate(rate), nudged.SetModRate(rate)
        a, b = plain.process(x[c]), nudged.process(x[c])
        spread = rel_rms(b, a)
        print(f"fs {fs} mod rate {rate} channel {c}: sine spread {spread:.3g}")
        assert np.any(a != b)
        assert spread < 1e-13
