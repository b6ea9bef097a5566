"""The Python layer over the effect handles, pinned without a device: the ctypes
prototypes that algodsp._lib binds, the public surface of algodsp.processors, and
what a handle class's constructor does before it reaches a device.

The two snapshots under tests/golden/ were written by `prototypes()` and
`surface()` below at the commit before the handle classes were folded onto one
base (json.dump(..., indent=1, sort_keys=True)); they hold type names, member
names and constants, no code.
"""
import ctypes as C
import inspect
import json
import pathlib

import pytest

from algodsp import _lib
from algodsp import processors as P

GOLDEN = pathlib.Path(__file__).resolve().parent / "golden"


def _tname(t):
    return "None" if t is None else t.__name__


def prototypes():
    """{function: [restype, [argtypes]]} of every ad_* function the loader bound, and {structure: [[field,
    type]]} of every structure of _lib."""
    fns = {n: [_tname(f.restype), [_tname(a) for a in f.argtypes]] for n, f in vars(_lib.lib()).items()
           if n.startswith("ad_") and f.argtypes is not None}
    structs = {n: [[f[0], _tname(f[1])] for f in s._fields_] for n, s in vars(_lib).items()
               if isinstance(s, type) and issubclass(s, C.Structure) and s is not C.Structure}
    return {"functions": fns, "structures": structs}


def _jsonable(v):
    return [_jsonable(x) for x in v] if isinstance(v, (tuple, list)) else v


def _call_shape(fn):
    """What a caller can rely on: how many positional arguments it must pass, every parameter that has a
    default with its value, and whether *args / **kwargs are taken.  The names of required parameters are
    free."""
    ps = list(inspect.signature(fn).parameters.values())
    return {"required": sum(p.default is p.empty and p.kind in (p.POSITIONAL_ONLY, p.POSITIONAL_OR_KEYWORD)
                            for p in ps),
            "defaults": [[p.name, repr(p.default)] for p in ps if p.default is not p.empty],
            "star": [str(p.kind) for p in ps if p.kind in (p.VAR_POSITIONAL, p.VAR_KEYWORD)]}


def _class_surface(cls):
    names = sorted(n for n in dir(cls) if not n.startswith("_"))  # the base-class chain's names included
    members = {n: inspect.getattr_static(cls, n) for n in names}
    return {"bases": [b.__name__ for b in cls.__mro__[1:] if not b.__name__.startswith("_") and b is not object],
            "names": names,
            "constants": {n: _jsonable(getattr(cls, n)) for n, m in members.items()
                          if not callable(m) and not isinstance(m, (staticmethod, classmethod, property))},
            "init": str(inspect.signature(cls.__init__)),
            "methods": {n: _call_shape(getattr(cls, n)) for n, m in members.items() if callable(getattr(cls, n))}}


def surface():
    pub = {n: v for n, v in vars(P).items() if not n.startswith("_") and getattr(v, "__module__", None) == P.__name__}
    return {"classes": {n: _class_surface(c) for n, c in pub.items() if isinstance(c, type)},
            "functions": {n: {"signature": str(inspect.signature(f))} for n, f in pub.items()
                          if inspect.isfunction(f)},
            "constants": {n: _jsonable(v) for n, v in vars(P).items()
                          if not n.startswith(("_", "AD_")) and isinstance(v, (int, float, str, tuple))}}


def _load(name):
    return json.loads((GOLDEN / name).read_text())


# ---- 1. prototype identity --------------------------------------------------------
def test_every_bound_prototype_is_the_snapshot():
    want, got = _load("lib_prototypes.json"), prototypes()
    assert sorted(got["functions"]) == sorted(want["functions"])  # none missing, none new
    diff = {n: (got["functions"][n], w) for n, w in want["functions"].items() if got["functions"][n] != w}
    assert not diff
    assert got["structures"] == want["structures"]


def test_every_exported_symbol_has_a_prototype():
    assert set(_lib.exported_symbols()) <= set(prototypes()["functions"])


# ---- 2. public surface ------------------------------------------------------------
def test_public_surface_is_the_snapshot():
    want, got = _load("processors_surface.json"), surface()
    assert sorted(got["classes"]) == sorted(want["classes"])
    for name, w in want["classes"].items():
        g = got["classes"][name]
        for part in ("bases", "names", "constants", "init", "methods"):
            assert g[part] == w[part], (name, part)
    assert got["functions"] == want["functions"]
    assert got["constants"] == want["constants"]


# ---- 3. constructors without a device ---------------------------------------------
def _fdn_bad():
    cfg = _lib.FdnConfig()
    _lib.lib().ad_fdn_default_config(C.byref(cfg), 44100.0)
    cfg.damp = 2.0
    return {"config": cfg}


def _delay_bad():
    cfg = _lib.DelayConfig()
    _lib.lib().ad_delay_default_config(C.byref(cfg), 48000.0)
    cfg.feedback = 1.5
    return {"config": cfg}


# class, a keyword the validator rejects: the (field, value) of test_fx_handle.FAMILIES.  FDNReverb and Delay
# take no option keywords, so theirs arrives in `config`.
HANDLES = [
    (P.Phaser, lambda: {"stages": 0}),
    (P.Tremolo, lambda: {"depth": 2.0}),
    (P.RingModulator, lambda: {"mix": -1.0}),
    (P.TransientShaper, lambda: {"attack_ms": 0.0}),
    (P.DeEsser, lambda: {"q": 0.0}),
    (P.Distortion, lambda: {"drive": 0.0}),
    (P.BitCrusher, lambda: {"downsample": 0}),
    (P.SpectralFreeze, lambda: {"hop_size": 0}),
    (P.SpectralPitchShifter, lambda: {"pitch_ratio": 8.0}),
    (P.Delay, _delay_bad),
    (P.Flanger, lambda: {"mix": 2.0}),
    (P.FDNReverb, _fdn_bad),
    (P.LookaheadLimiter, lambda: {"release_ms": 0.0}),
    (P.Vocoder, lambda: {"synth_q": 0.0}),
]
HANDLE_IDS = [h[0].__name__ for h in HANDLES]


@pytest.mark.parametrize("cls,bad", HANDLES, ids=HANDLE_IDS)
def test_constructor_without_a_device(cls, bad):
    with pytest.raises(_lib.ADError) as e:
        cls(device=-1)
    assert e.value.code == _lib.AD_ERR_NO_DEVICE
    with pytest.raises(TypeError):
        cls(device=-1, no_such_option=1)
    with pytest.raises(_lib.ErrInvalidArgument):  # the config is checked before the device
        cls(device=-1, **bad())


# ---- the option keywords, through the config builder (no device) -------------------
# class: (options stored as floats, as whole numbers, as flags), as the class docstrings list them
OPTIONS = {
    P.FDNReverb: ((), (), ()),
    P.Delay: ((), (), ()),
    P.Flanger: (("rate_hz", "depth_seconds", "base_delay_seconds", "feedback", "mix"), (), ()),
    P.Phaser: (("rate_hz", "min_freq_hz", "max_freq_hz", "feedback", "mix"), ("stages",), ()),
    P.Tremolo: (("rate_hz", "depth", "smoothing_ms", "mix", "smoothing_coeff"), (), ()),
    P.RingModulator: (("carrier_hz", "mix"), (), ()),
    P.Distortion: (("drive", "mix", "output_level", "clip_level", "shape", "bias", "cheb_gain"),
                   ("mode", "approx", "cheb_order", "cheb_harmonic", "cheb_invert", "cheb_dc_bypass"), ()),
    P.BitCrusher: (("bit_depth", "mix"), ("downsample",), ()),
    P.TransientShaper: (("attack_amount", "sustain_amount", "attack_ms", "release_ms", "attack_coeff",
                         "release_coeff"), (), ()),
    P.DeEsser: (("freq_hz", "q", "threshold_db", "ratio", "knee_db", "attack_ms", "release_ms", "range_db",
                 "attack_coeff", "release_coeff"), ("mode", "detector", "listen", "filter_order"), ()),
    P.Vocoder: (("synth_q", "attack_ms", "release_ms", "input_level", "synth_level", "vocoder_level"), ("layout",),
                ("downsample",)),
    P.LookaheadLimiter: (("threshold_db", "release_ms", "lookahead_ms"), (), ()),
    P.SpectralFreeze: (("mix",), ("frame_size", "hop_size", "phase_mode", "frozen", "window_type"), ()),
    P.SpectralPitchShifter: (("pitch_ratio",), ("frame_size", "analysis_hop", "window_type", "resample_quality"), ()),
}
STFT = (P.SpectralFreeze, P.SpectralPitchShifter)


def _defaults(cls, fs=48000.0):
    cfg = cls._config()
    cls._fn("default_config")(C.byref(cfg), fs)
    return cfg


def _diff(a, b):
    """The names of the scalar fields that differ (the tables have tests of their own)."""
    return {n for n, t in a._fields_ if issubclass(t, C._SimpleCData) and getattr(a, n) != getattr(b, n)}


@pytest.mark.parametrize("cls", list(OPTIONS), ids=lambda c: c.__name__)
def test_every_option_reaches_its_field_alone(cls):
    floats, ints, flags = OPTIONS[cls]
    special = {"cheb_weights"} if cls is P.Distortion else set()
    assert set(cls._options + cls._int_options + cls._bool_options) == set(floats + ints + flags) | special
    base = _defaults(cls)
    assert not _diff(cls._make_config(48000.0), base)
    assert cls._make_config(44100.0).sample_rate == 44100.0
    for k in floats:  # a whole number arrives as a float
        v = int(getattr(base, k)) + 2
        cfg = cls._make_config(48000.0, **{k: v})
        assert (getattr(cfg, k), type(getattr(cfg, k))) == (float(v), float)
        assert _diff(cfg, base) == {k} | ({"synth_q_set"} if k == "synth_q" else set())
    for k in ints:  # a float is cut to a whole number; window type 1 + 2 is Blackman, frame 1026 makes a table
        v = getattr(base, k) + 2
        cfg = cls._make_config(48000.0, **{k: v + 0.75})
        assert (getattr(cfg, k), type(getattr(cfg, k))) == (v, int)
        assert _diff(cfg, base) == {k}
    for k in flags:  # any truth value is 0 or 1
        for v, want in (("yes", 1), (0.0, 0), (2, 1)):
            cfg = cls._make_config(48000.0, **{k: v})
            assert getattr(cfg, k) == want
            assert _diff(cfg, base) <= {k}
    if floats or ints or flags:
        with pytest.raises((TypeError, ValueError)):
            cls._make_config(48000.0, **{(floats + ints + flags)[0]: "loud"})


@pytest.mark.parametrize("cls", list(OPTIONS), ids=lambda c: c.__name__)
def test_unknown_option_raises_before_any_library_call(cls, monkeypatch):
    def no_library():
        raise AssertionError("the library was reached")

    monkeypatch.setattr(P, "lib", no_library)
    with pytest.raises(TypeError, match="no_such_option"):
        cls._make_config(48000.0, no_such_option=1)
    with pytest.raises(TypeError):
        cls(device=-1, no_such_option=1)


@pytest.mark.parametrize("cls", [c for c in OPTIONS if c not in STFT], ids=lambda c: c.__name__)
def test_config_is_copied_whole(cls):
    src = _defaults(cls, 32000.0)
    first = src._fields_[1][0]  # a double of every structure
    setattr(src, first, getattr(src, first) * 0.5)
    cfg = cls._make_config(48000.0, src)  # the sample rate argument is not used
    assert cfg is not src and bytes(cfg) == bytes(src)
    floats = OPTIONS[cls][0]
    if floats:  # an option lands on top of the copy
        k = floats[-1]
        cfg = cls._make_config(48000.0, src, **{k: getattr(src, k) + 1.0})
        assert _diff(cfg, src) == {k} | ({"synth_q_set"} if k == "synth_q" else set())


def test_vocoder_synth_q_keyword_marks_it_set():
    assert P.Vocoder._make_config(48000.0).synth_q_set == 0
    assert P.Vocoder._make_config(48000.0, attack_ms=1.0, layout=P.Vocoder.BARK).synth_q_set == 0
    cfg = P.Vocoder._make_config(48000.0, synth_q=2.5, layout=P.Vocoder.BARK)
    assert (cfg.synth_q, cfg.synth_q_set, cfg.layout) == (2.5, 1, P.Vocoder.BARK)


def test_distortion_chebyshev_weights_option():
    assert list(P.Distortion._make_config(48000.0).cheb_weights) == [0.0] * 16
    cfg = P.Distortion._make_config(48000.0, cheb_weights=(1, 0.5, -0.25), cheb_order=3)
    assert list(cfg.cheb_weights) == [1.0, 0.5, -0.25] + [0.0] * 13 and cfg.cheb_order == 3
    assert list(P.Distortion._make_config(48000.0, cheb_weights=range(16)).cheb_weights) == list(map(float, range(16)))
    with pytest.raises(TypeError):
        P.Distortion._make_config(48000.0, cheb_weights=[0.0] * 17)


@pytest.mark.parametrize("cls", STFT, ids=lambda c: c.__name__)
def test_stft_config_carries_its_window_table(cls):
    import numpy as np

    hop = "hop_size" if cls is P.SpectralFreeze else "analysis_hop"
    cfg = cls._make_config(48000.0, frame_size=128, window_type=P.WindowHamming, **{hop: 32})
    want = P.spectral_window(P.WindowHamming, 128)
    assert np.array_equal(np.ctypeslib.as_array(cfg.window, (128,)), want)
    assert cls._fn("validate")(C.byref(cfg)) == _lib.AD_OK
    cfg = cls._make_config(48000.0)  # the defaults: Hann, 1024
    assert np.array_equal(np.ctypeslib.as_array(cfg.window, (1024,)), P.spectral_window(P.WindowHann, 1024))
    with pytest.raises(ValueError):
        cls._make_config(48000.0, window_type=9)
    if cls is P.SpectralPitchShifter:
        assert not cfg.resample_taps and cfg.n_resample_taps == 0  # the taps follow create (_sync_taps)
