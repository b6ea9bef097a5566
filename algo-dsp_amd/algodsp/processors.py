"""Host-side mirror of the reference's per-sample processors on the HIP engine.

Names and argument meaning follow the Go packages so the parity tests read
like the reference's own tests:

  biquad.Chain / biquad.Section  dsp/filter/biquad/chain.go, section.go
  dynamics.Compressor            dsp/effects/dynamics/compressor.go
  reverb.Reverb (Freeverb)       dsp/effects/reverb/reverb.go
  reverb.FDNReverb               dsp/effects/reverb/fdn_reverb.go
  effects.Delay                  dsp/effects/delay.go
  modulation.Flanger             dsp/effects/modulation/flanger.go
  modulation.Phaser              dsp/effects/modulation/phaser.go
  modulation.Tremolo             dsp/effects/modulation/tremolo.go
  modulation.RingModulator       dsp/effects/modulation/ring_modulator.go
  effects.Distortion             dsp/effects/distortion.go
  effects.BitCrusher             dsp/effects/bit_crusher.go
  dynamics.TransientShaper       dsp/effects/dynamics/transient_shaper.go
  dynamics.DeEsser               dsp/effects/dynamics/deesser.go
  effects.Vocoder                dsp/effects/vocoder.go
  dynamics.LookaheadLimiter      dsp/effects/dynamics/lookahead_limiter.go
  crossover.MultiBand            dsp/filter/crossover/crossover.go
  dynamics.MultibandCompressor   dsp/effects/dynamics/multiband.go
  effects.SpectralFreeze         dsp/effects/spectral_freeze.go
  pitch.SpectralPitchShifter     dsp/effects/pitch/pitch_shift_spectral.go
  fir.Filter                     dsp/filter/fir/filter.go
  effectchain filter -> dyn-compressor -> reverb-freeverb (EffectChain)

Every instance can carry `channels` independent reference instances (one
lane each on the GPU); buffers are [channels][n] float64 (a 1-D buffer is
one channel).  All work runs in libalgodsp_hip.so; there is no CPU path.

Every class that owns a C handle derives from _Handle, which names the
entry points ad_<kind>_* and owns the handle's life.  The fourteen effects
whose create takes a config structure derive from _ConfigHandle: a class
there is its `_kind`, its `_config` structure, its option names, its P_*
parameter numbers and a table of setters and getters (_setter, _getter).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import (AD_ERR_INVALID_ARGUMENT, BitCrusherConfig, CompressorConfig, DeEsserConfig, DelayConfig,
                   DistortionConfig, ErrInvalidArgument, FdnConfig, FlangerConfig, LookaheadConfig, PhaserConfig,
                   PitchSpecConfig, RingModConfig, SpecFreezeConfig, TransientConfig, TremoloConfig, VocoderConfig,
                   VocoderTables, check, f64, lib, ptr)

DEVICE = 0
SEC_STRIDE = 6  # {pre_gain, b0, b1, b2, a1, a2}
_INT, _I64, _F64 = (C.c_int,), (C.c_int64,), (C.c_double,)  # the C types of by-reference outputs, for _outputs


def _as2d(buf, channels: int):
    if not isinstance(buf, np.ndarray) or buf.dtype != np.float64 or not buf.flags.c_contiguous:
        raise TypeError("buffer must be a C-contiguous float64 numpy array")
    b2 = buf.reshape(1, -1) if buf.ndim == 1 else buf
    if b2.shape[0] != channels:
        raise ValueError(f"buffer has {b2.shape[0]} channels, processor has {channels}")
    return b2


def section_table(coeffs, gain: float = 1.0) -> np.ndarray:
    """[sections][5] {b0,b1,b2,a1,a2} (+ chain gain) -> [sections][6] device table."""
    c = f64(coeffs).reshape(-1, 5)
    t = np.ones((c.shape[0], SEC_STRIDE))
    t[:, 1:] = c
    if c.shape[0]:
        t[0, 0] = gain
    return t


def _outputs(fn, types, *args):
    """fn(*args, out...) with one by-reference output of each C type in `types`: the values it wrote."""
    outs = [t() for t in types]
    check(fn(*args, *[C.byref(o) for o in outs]))
    return tuple(o.value for o in outs)


def _setter(param):
    """A method that forwards its value to set_param: `param` is the P_* number, or the constant's name in
    a base whose subclasses number it differently."""
    def set_(self, v):
        self._set(getattr(self, param) if isinstance(param, str) else param, v)
    return set_


def _getter(field: str, kind=None):
    """A method that returns `field` of config(), through `kind` (bool, for a flag) when given."""
    def get(self):
        v = getattr(self.config(), field)
        return v if kind is None else kind(v)
    return get


class _Handle:
    """A C handle whose entry points are named ad_<kind>_*: create (whatever comes before channels, device
    and the handle goes through _create), process, process_device, reset and destroy."""

    _kind = ""

    @classmethod
    def _fn(cls, name):
        return getattr(lib(), f"ad_{cls._kind}_{name}")

    def _create(self, channels: int, device: int, *head):
        self.channels = int(channels)
        self._h = C.c_void_p()
        self._device_fn = self._fn("process_device")  # bound once: the call that streaming callers repeat
        check(self._fn("create")(*head, self.channels, int(device), C.byref(self._h)))

    def _out(self, name, types, *args):
        """ad_<kind>_<name>(handle, *args, out...): the values of the by-reference outputs."""
        return _outputs(self._fn(name), types, self._h, *args)

    def _process(self, buf):
        b = _as2d(buf, self.channels)
        check(self._fn("process")(self._h, ptr(b), b.shape[1]))

    def process_device(self, d_buf: int, stride: int, n: int, stream: int | None = None):
        check(self._device_fn(self._h, C.c_void_p(d_buf), int(stride), int(n), C.c_void_p(stream or 0)))

    def Reset(self):
        check(self._fn("reset")(self._h))

    def close(self):
        if self._h:
            self._fn("destroy")(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _ConfigHandle(_Handle):
    """A handle whose create takes a config structure: the constructor, options as keywords, set_param and
    get_config, once for the fourteen effect classes.  A class names its structure (`_config`), the option
    keywords stored as floats (`_options`), whole numbers (`_int_options`) and flags (`_bool_options`), and
    what the "unknown option" error calls it (`_name`)."""

    _config = None
    _name = ""
    _options = ()
    _int_options = ()
    _bool_options = ()

    def __init__(self, sample_rate: float = 48000.0, channels: int = 1, device: int = DEVICE, config=None, **options):
        cfg = self._make_config(sample_rate, config, **options)
        self._create(channels, device, C.byref(cfg))

    @classmethod
    def _make_config(cls, sample_rate, config=None, **options):
        """The structure the constructor passes to create: default_config(sample_rate), or a copy of `config`,
        with the options stored.  An unknown option raises before any library call; nothing here needs a
        device."""
        unknown = set(options) - set(cls._options + cls._int_options + cls._bool_options)
        if unknown:
            raise TypeError(f"unknown {cls._name} option {min(unknown)!r}")
        cfg = cls._config()
        if config is None:
            cls._fn("default_config")(C.byref(cfg), float(sample_rate))
        else:
            C.memmove(C.byref(cfg), C.byref(config), C.sizeof(cfg))
        for k, v in options.items():
            cls._option(cfg, k, v)
        return cfg

    @classmethod
    def _option(cls, cfg, key, value):
        """Stores one option keyword; a class overrides it for an option that is more than one field."""
        if key in cls._bool_options:
            setattr(cfg, key, 1 if value else 0)
        else:
            setattr(cfg, key, int(value) if key in cls._int_options else float(value))

    def _set(self, which: int, v):
        check(self._fn("set_param")(self._h, which, float(v)))

    def config(self):
        cfg = self._config()
        check(self._fn("get_config")(self._h, C.byref(cfg)))
        return cfg

    def ProcessInPlace(self, buf):
        self._process(buf)

    SetSampleRate = _setter(0)  # parameter 0 of every kind
    SampleRate = _getter("sample_rate")


class _FxChain(_Handle):
    _kind = "fx_chain"

    def __init__(self, channels: int, device: int):
        self._create(channels, device)

    # engine selection (include/algodsp.h ad_fx_chain_set_engine); the fused
    # and staged engines give identical results, the time-parallel one within
    # 1e-12 relative RMS of them
    ENGINE_AUTO, ENGINE_FUSED, ENGINE_STAGED_NOSPLIT, ENGINE_STAGED, ENGINE_TIME_PARALLEL = 0, 1, 2, 3, 4

    def SetEngine(self, engine: int, chunk: int = 0):
        check(lib().ad_fx_chain_set_engine(self._h, int(engine), int(chunk)))

    def LastEngine(self) -> tuple[int, float]:
        """(engine that ran the last call, the EQ's round-off noise estimate)
        (ad_fx_chain_last_engine)."""
        return self._out("last_engine", _INT + _F64)


class Chain(_FxChain):
    """biquad.Chain (chain.go:6-138): optional gain, then sections in order."""

    def __init__(self, coeffs, gain: float = 1.0, channels: int = 1, device: int = DEVICE):
        super().__init__(channels, device)
        self._coeffs = f64(coeffs).reshape(-1, 5)
        self._gain = float(gain)
        self._load()

    def _load(self):
        t = section_table(self._coeffs, self._gain)
        check(lib().ad_fx_chain_set_eq(self._h, ptr(t), t.shape[0], 0))

    def NumSections(self) -> int:
        return self._coeffs.shape[0]

    def Gain(self) -> float:
        return self._gain

    def SetGain(self, g: float):  # chain.go:89-97
        self._gain = float(g)
        self._load()

    def UpdateCoefficients(self, coeffs, gain: float | None = None):  # chain.go:99-115
        self._coeffs = f64(coeffs).reshape(-1, 5)
        if gain is not None:
            self._gain = float(gain)
        self._load()

    def ProcessBlock(self, buf):  # chain.go:59-70
        self._process(buf)

    def State(self) -> np.ndarray:  # chain.go:122-130 -> [channels][sections][2]
        out = np.zeros((self.channels, self.NumSections(), 2))
        check(lib().ad_fx_chain_eq_state(self._h, ptr(out), out.size))
        return out

    def SetState(self, states):  # chain.go:130-138: [channels][sections][2] (a [sections][2] list for 1 channel)
        st = np.ascontiguousarray(np.asarray(states, dtype=np.float64))
        check(lib().ad_fx_chain_set_eq_state(self._h, ptr(st), st.size))


def Section(b0, b1, b2, a1, a2, channels: int = 1, device: int = DEVICE) -> Chain:
    """biquad.Section (section.go:26-155) = a one-section chain with unit gain."""
    return Chain([[b0, b1, b2, a1, a2]], 1.0, channels, device)


def _flag(on) -> int:
    return int(bool(on))


# The setters of a compressor's config, as Compressor.Set<name>(v) (compressor.go:130-305, core.go:106-250) and
# as MultibandCompressor.SetBand<name>(band, v) (multiband.go:190-329) and SetAllBands<name>(v) (:331-437):
# (name, config field, what the value goes through, the fields stored with it, has a SetAllBands form)
_DYNAMICS_SETTERS = (
    ("Threshold", "threshold_db", float, {}, True),
    ("Ratio", "ratio", float, {}, True),
    ("Knee", "knee_db", float, {}, True),
    ("Attack", "attack_ms", float, {}, True),
    ("Release", "release_ms", float, {}, True),
    ("RMSWindow", "rms_window_ms", float, {}, True),
    ("SidechainLowCut", "sidechain_low_cut_hz", float, {}, False),
    ("SidechainHighCut", "sidechain_high_cut_hz", float, {}, False),
    ("AutoMakeup", "auto_makeup", _flag, {}, False),
    ("MakeupGain", "makeup_db", float, {"auto_makeup": 0}, False),  # SetManualMakeupGain (core.go:201-210,
                                                                    # multiband.go:242-249) turns auto makeup off
    ("Topology", "topology", int, {}, True),  # core.go:106-114
    ("DetectorMode", "detector_mode", int, {}, True),  # core.go:116-124
    ("FeedbackRatioScale", "feedback_ratio_scale", _flag, {}, True),  # core.go:126-129
)


class Compressor(_FxChain):
    """dynamics.Compressor (compressor.go:39-431) on `channels` lanes.  Its setters are Set<name> for every
    name of _DYNAMICS_SETTERS."""

    def __init__(self, sample_rate: float = 48000.0, channels: int = 1, device: int = DEVICE, **cfg):
        super().__init__(channels, device)
        self.cfg = CompressorConfig()
        lib().ad_compressor_default_config(C.byref(self.cfg), float(sample_rate))
        for k, v in cfg.items():
            setattr(self.cfg, k, v)
        self._apply()

    def _apply(self):
        check(lib().ad_fx_chain_set_compressor(self._h, C.byref(self.cfg)))

    def _set(self, **kv):
        # a setter the reference rejects returns its error and leaves the
        # config as it was (core.go:131-198): restore the fields, then raise
        old = {k: getattr(self.cfg, k) for k in kv}
        for k, v in kv.items():
            setattr(self.cfg, k, v)
        try:
            self._apply()
        except Exception:
            for k, v in old.items():
                setattr(self.cfg, k, v)
            raise

    def ProcessInPlace(self, buf):  # compressor.go:362-366
        self._process(buf)

    def Metrics(self, channel: int = 0):
        return self._out("compressor_metrics", _F64 * 3, int(channel))


def _compressor_setter(field, kind, also):
    def set_(self, v):
        self._set(**{field: kind(v)}, **also)
    return set_


for _name, _field, _kind, _also, _ in _DYNAMICS_SETTERS:
    setattr(Compressor, "Set" + _name, _compressor_setter(_field, _kind, _also))


class Expander(Compressor):
    """dynamics.Expander (expander.go) on `channels` lanes: the compressor's
    detector core with the downward-expansion gain and a range floor.
    Defaults of NewExpander (expander.go:9-15)."""

    GATE = False

    def __init__(self, sample_rate: float = 48000.0, channels: int = 1, device: int = DEVICE, **cfg):
        _FxChain.__init__(self, channels, device)
        self.cfg = CompressorConfig()
        lib().ad_compressor_default_config(C.byref(self.cfg), float(sample_rate))
        defaults = dict(threshold_db=-40.0, ratio=10.0, knee_db=6.0, attack_ms=0.1, release_ms=100.0) \
            if self.GATE else dict(threshold_db=-35.0, ratio=2.0, knee_db=6.0, attack_ms=1.0, release_ms=100.0)
        self.range_db = cfg.pop("range_db", -80.0 if self.GATE else -60.0)
        self.hold_ms = cfg.pop("hold_ms", 50.0 if self.GATE else 0.0)
        for k, v in {**defaults, **cfg}.items():
            setattr(self.cfg, k, v)
        self._apply()

    def _apply(self):
        check(lib().ad_fx_chain_set_expander(self._h, C.byref(self.cfg), int(self.GATE), float(self.range_db),
                                             float(self.hold_ms)))

    def _set_attr(self, name, value):
        # a rejected value raises and leaves the stage as it was (like _set)
        old = getattr(self, name)
        setattr(self, name, value)
        try:
            self._apply()
        except Exception:
            setattr(self, name, old)
            raise

    def SetRange(self, db):  # expander.go / gate.go SetRange
        self._set_attr("range_db", db)


class Gate(Expander):
    """dynamics.Gate (gate.go): Expander gain plus a hold counter; defaults of
    NewGate (gate.go:9-17)."""

    GATE = True

    def SetHold(self, ms):  # gate.go:196-223
        self._set_attr("hold_ms", ms)


def _reverb_setter(attr):
    def set_(self, v):
        setattr(self, attr, float(v))
        self._apply()
    return set_


class Reverb(_FxChain):
    """reverb.Reverb (Freeverb, reverb.go:33-235) with NewReverb defaults."""

    def __init__(self, channels: int = 1, device: int = DEVICE):
        super().__init__(channels, device)
        self.wet, self.dry, self.room, self.damp, self.gain = 0.22, 1.0, 0.72, 0.45, 0.015
        self._apply()

    def _apply(self):
        check(lib().ad_fx_chain_set_freeverb(self._h, self.wet, self.dry, self.room, self.damp, self.gain))

    SetWet = _reverb_setter("wet")  # reverb.go:192-220
    SetDry = _reverb_setter("dry")
    SetRoomSize = _reverb_setter("room")
    SetDamp = _reverb_setter("damp")
    SetGain = _reverb_setter("gain")

    def ProcessInPlace(self, buf):  # reverb.go:185-189
        self._process(buf)


class FDNReverb(_ConfigHandle):
    """reverb.FDNReverb (fdn_reverb.go:37-391) for `channels` instances sharing
    one configuration: NewFDNReverb(sample_rate), or `config` (an FdnConfig)
    applied whole.  The setters are the reference's, side effects included
    (ad_fdn_set_param); a rejected value raises ErrInvalidArgument and changes
    nothing."""

    P_SAMPLE_RATE, P_WET, P_DRY, P_RT60, P_DAMP, P_PRE_DELAY, P_MOD_DEPTH, P_MOD_RATE = range(8)  # AD_FDN_*
    _kind = "fdn"
    _name = "fdn reverb"
    _config = FdnConfig

    def __init__(self, sample_rate: float = 44100.0, channels: int = 1, device: int = DEVICE, config=None):
        super().__init__(sample_rate, channels, device, config)

    SetSampleRate = _setter(P_SAMPLE_RATE)  # :95-106
    SetWet = _setter(P_WET)  # :109-117
    SetDry = _setter(P_DRY)  # :120-128
    SetRT60 = _setter(P_RT60)  # :131-140
    SetDamp = _setter(P_DAMP)  # :143-151
    SetPreDelay = _setter(P_PRE_DELAY)  # :154-163
    SetModDepth = _setter(P_MOD_DEPTH)  # :166-175
    SetModRate = _setter(P_MOD_RATE)  # :178-186
    SampleRate = _getter("sample_rate")  # :251-272
    Wet = _getter("wet")
    Dry = _getter("dry")
    RT60 = _getter("rt60_seconds")
    Damp = _getter("damp")
    PreDelay = _getter("pre_delay_seconds")
    ModDepth = _getter("mod_depth_seconds")
    ModRate = _getter("mod_rate_hz")

    def derived(self):
        """(feedback gains [8], line lengths [8], pre-delay line length, LFO
        phase): what reconfigureDelays / updateFeedbackGains derived, and the
        phase after the last call (ad_fdn_derived)."""
        g = np.zeros(8)
        ln = np.zeros(8, dtype=np.int64)
        return (g, ln) + self._out("derived", _I64 + _F64, ptr(g), ln.ctypes.data_as(C.POINTER(C.c_int64)))

    def kernel_info(self):
        """(block, sub_block, lds_bytes) of ad_fdn_kernel_info."""
        return self._out("kernel_info", _INT * 3)

    # ProcessInPlace :244-248, Reset :189-197


class Delay(_ConfigHandle):
    """effects.Delay (delay.go:25-257) for `channels` instances sharing one
    configuration: NewDelay(sample_rate), or `config` (a DelayConfig) as
    ad_delay_create applies it (NewDelay, then SetTargetTime, SetFeedback,
    SetMix; mode 1 is the graph's delay-simple).  The setters are the
    reference's; a rejected value raises ErrInvalidArgument and changes nothing."""

    P_SAMPLE_RATE, P_TIME, P_FEEDBACK, P_MIX, P_TARGET_TIME, P_SAMPLES, P_SMOOTH_COEFF = range(7)  # AD_DELAY_*
    _kind = "delay"
    _name = "delay"
    _config = DelayConfig

    def __init__(self, sample_rate: float = 48000.0, channels: int = 1, device: int = DEVICE, config=None):
        super().__init__(sample_rate, channels, device, config)

    SetSampleRate = _setter(P_SAMPLE_RATE)  # :63-72
    SetTime = _setter(P_TIME)  # :77-89
    SetTargetTime = _setter(P_TARGET_TIME)  # :95-106
    SetFeedback = _setter(P_FEEDBACK)  # :109-117
    SetMix = _setter(P_MIX)  # :120-128
    SetDelaySamples = _setter(P_SAMPLES)  # mode 1: simpleDelayRuntime.Configure
    SetSmoothCoeff = _setter(P_SMOOTH_COEFF)  # smoothCoeff, for a caller whose exp is not the C library's
    SampleRate = _getter("sample_rate")  # :176-185
    Time = _getter("time_seconds")
    Feedback = _getter("feedback")
    Mix = _getter("mix")

    def derived(self):
        """(currentSamples, targetSamples, ring length, write position) of ad_delay_derived."""
        return self._out("derived", _F64 * 2 + _I64 * 2)

    def CurrentDelaySamples(self) -> float:  # :189
        return self.derived()[0]

    def kernel_info(self):
        """(block, sub_block, regime of the last call, its launches) of ad_delay_kernel_info."""
        return self._out("kernel_info", _INT * 4)

    def set_regime(self, regime: int):
        """0: the library chooses; 1: one launch per block; 2: one persistent launch."""
        check(lib().ad_delay_set_regime(self._h, int(regime)))


class Flanger(_ConfigHandle):
    """modulation.Flanger (flanger.go:108-424) for `channels` instances sharing
    one configuration: NewFlanger(sample_rate, options...) with the options as
    keywords (rate_hz, depth_seconds, base_delay_seconds, feedback, mix), or
    `config` (a FlangerConfig) applied whole."""

    P_SAMPLE_RATE, P_RATE, P_DEPTH, P_BASE_DELAY, P_FEEDBACK, P_MIX = range(6)  # AD_FLANGER_*
    _kind = "flanger"
    _name = "flanger"
    _config = FlangerConfig
    _options = ("rate_hz", "depth_seconds", "base_delay_seconds", "feedback", "mix")

    SetSampleRate = _setter(P_SAMPLE_RATE)  # :165-173
    SetRateHz = _setter(P_RATE)  # :176-184
    SetDepthSeconds = _setter(P_DEPTH)  # :187-203
    SetBaseDelaySeconds = _setter(P_BASE_DELAY)  # :206-224
    SetFeedback = _setter(P_FEEDBACK)  # :227-235
    SetMix = _setter(P_MIX)  # :238-246
    SampleRate = _getter("sample_rate")  # :299-314
    RateHz = _getter("rate_hz")
    DepthSeconds = _getter("depth_seconds")
    BaseDelaySeconds = _getter("base_delay_seconds")
    Feedback = _getter("feedback")
    Mix = _getter("mix")

    def derived(self):
        """(ring length, maxDelay, write position, LFO phase after the last call) of ad_flanger_derived."""
        return self._out("derived", _I64 * 3 + _F64)

    def kernel_info(self):
        """(block, sub_block, channels per workgroup, lds_bytes) of ad_flanger_kernel_info."""
        return self._out("kernel_info", _INT * 4)


class _ModHandle(_ConfigHandle):
    """What Phaser, Tremolo and RingModulator share: a config structure whose
    field k is parameter k, a mix, and peek_lfo."""

    def peek_lfo(self, n: int):
        """(phases, table) of the next n samples as the kernels would take them:
        the table is the phaser's allpass coefficient, the tremolo's gain or the
        ring modulator's carrier.  Nothing advances; phases[0] is the phase state."""
        ph, tab = np.empty(int(n)), np.empty(int(n))
        check(self._fn("peek_lfo")(self._h, int(n), ptr(ph), ptr(tab)))
        return ph, tab

    SetMix = _setter("P_MIX")
    Mix = _getter("mix")


class Phaser(_ModHandle):
    """modulation.Phaser (phaser.go:130-379) for `channels` instances sharing one
    configuration: NewPhaser(sample_rate, options...) with the options as
    keywords (rate_hz, min_freq_hz, max_freq_hz, stages, feedback, mix), or
    `config` (a PhaserConfig) applied whole.  A rejected setter value raises
    ErrInvalidArgument and changes nothing."""

    P_SAMPLE_RATE, P_RATE, P_MIN_FREQ, P_MAX_FREQ, P_FEEDBACK, P_MIX, P_STAGES = range(7)  # AD_PHASER_*
    _kind = "phaser"
    _name = "phaser"
    _config = PhaserConfig
    _options = ("rate_hz", "min_freq_hz", "max_freq_hz", "feedback", "mix")
    _int_options = ("stages",)

    SetRateHz = _setter(P_RATE)  # :194-202
    SetStages = _setter(P_STAGES)  # :221-233
    SetFeedback = _setter(P_FEEDBACK)  # :236-244
    RateHz = _getter("rate_hz")  # :302-320
    MinFrequencyHz = _getter("min_freq_hz")
    MaxFrequencyHz = _getter("max_freq_hz")
    Stages = _getter("stages")
    Feedback = _getter("feedback")

    def SetFrequencyRangeHz(self, min_freq_hz, max_freq_hz):  # :205-218
        check(lib().ad_phaser_set_range(self._h, float(min_freq_hz), float(max_freq_hz)))

    def kernel_info(self):
        """(channels per workgroup, samples staged per chunk, lds_bytes) of ad_phaser_kernel_info."""
        return self._out("kernel_info", _INT * 3)


class Tremolo(_ModHandle):
    """modulation.Tremolo (tremolo.go:86-294): NewTremolo(sample_rate,
    options...) with the options as keywords (rate_hz, depth, smoothing_ms,
    mix, smoothing_coeff), or `config` (a TremoloConfig) applied whole."""

    P_SAMPLE_RATE, P_RATE, P_DEPTH, P_SMOOTHING, P_MIX, P_SMOOTHING_COEFF = range(6)  # AD_TREMOLO_*
    _kind = "tremolo"
    _name = "tremolo"
    _config = TremoloConfig
    _options = ("rate_hz", "depth", "smoothing_ms", "mix", "smoothing_coeff")

    SetRateHz = _setter(P_RATE)  # :150-158
    SetDepth = _setter(P_DEPTH)  # :161-169
    SetSmoothingMs = _setter(P_SMOOTHING)  # :172-181
    SetSmoothingCoeff = _setter(P_SMOOTHING_COEFF)  # smoothingCoef, for a caller whose exp is not the C library's
    RateHz = _getter("rate_hz")  # :233-246
    Depth = _getter("depth")
    SmoothingMs = _getter("smoothing_ms")

    def kernel_info(self):
        """(samples of a row per apply workgroup, the stepper lane's chunk, smoothed) of ad_tremolo_kernel_info."""
        return self._out("kernel_info", _INT * 3)


class RingModulator(_ModHandle):
    """modulation.RingModulator (ring_modulator.go:63-178):
    NewRingModulator(sample_rate, options...) with the options as keywords
    (carrier_hz, mix), or `config` (a RingModConfig) applied whole."""

    P_SAMPLE_RATE, P_CARRIER, P_MIX = range(3)  # AD_RINGMOD_*
    _kind = "ringmod"
    _name = "ringmod"
    _config = RingModConfig
    _options = ("carrier_hz", "mix")

    SetCarrierHz = _setter(P_CARRIER)  # :115-124
    CarrierHz = _getter("carrier_hz")  # :171

    def kernel_info(self):
        """(samples of a row per apply workgroup, table threads, phaseInc) of ad_ringmod_kernel_info."""
        return self._out("kernel_info", _INT * 2 + _F64)


class _ShaperHandle(_ConfigHandle):
    """What Distortion and BitCrusher share: a mix."""

    SetMix = _setter("P_MIX")
    Mix = _getter("mix")


class Distortion(_ShaperHandle):
    """effects.Distortion (distortion.go:296-797) for `channels` instances
    sharing one configuration: NewDistortion(sample_rate, options...) with the
    options as keywords (mode, approx, drive, mix, output_level, clip_level,
    shape, bias, cheb_order, cheb_harmonic, cheb_invert, cheb_gain,
    cheb_dc_bypass, cheb_weights), or `config` (a DistortionConfig) applied
    whole.  A rejected setter value raises ErrInvalidArgument and changes
    nothing."""

    (P_SAMPLE_RATE, P_DRIVE, P_MIX, P_OUTPUT_LEVEL, P_CLIP_LEVEL, P_SHAPE, P_BIAS, P_CHEB_GAIN, P_MODE, P_APPROX,
     P_CHEB_ORDER, P_CHEB_HARMONIC, P_CHEB_INVERT, P_CHEB_DC_BYPASS) = range(14)  # AD_DISTORTION_*
    # DistortionMode :36-52, DistortionApproxMode :57-60, ChebyshevHarmonicMode :65-69
    MODES = ("softclip", "hardclip", "tanh", "waveshaper1", "waveshaper2", "waveshaper3", "waveshaper4",
             "waveshaper5", "waveshaper6", "waveshaper7", "waveshaper8", "saturate", "saturate2", "softsat", "chebyshev")
    APPROX = ("exact", "polynomial")
    HARMONICS = ("all", "odd", "even")
    _kind = "distortion"
    _name = "distortion"
    _config = DistortionConfig
    _options = ("drive", "mix", "output_level", "clip_level", "shape", "bias", "cheb_gain", "cheb_weights")
    _int_options = ("mode", "approx", "cheb_order", "cheb_harmonic", "cheb_invert", "cheb_dc_bypass")

    @classmethod
    def _option(cls, cfg, key, value):
        if key != "cheb_weights":
            return super()._option(cfg, key, value)
        w = [float(x) for x in value]
        if len(w) > 16:
            raise TypeError("at most 16 chebyshev weights")
        cfg.cheb_weights = (C.c_double * 16)(*w)

    SetMode = _setter(P_MODE)  # :376-384
    SetApproxMode = _setter(P_APPROX)  # :387-395
    SetDrive = _setter(P_DRIVE)  # :398-406
    SetOutputLevel = _setter(P_OUTPUT_LEVEL)  # :420-429
    SetClipLevel = _setter(P_CLIP_LEVEL)  # :432-441
    SetShape = _setter(P_SHAPE)  # :444-452
    SetBias = _setter(P_BIAS)  # :455-463
    SetChebyshevOrder = _setter(P_CHEB_ORDER)  # :466-474
    SetChebyshevHarmonicMode = _setter(P_CHEB_HARMONIC)  # :477-485
    SetChebyshevGainLevel = _setter(P_CHEB_GAIN)  # :493-502
    Mode = _getter("mode")  # :567-588
    Drive = _getter("drive")
    OutputLevel = _getter("output_level")
    ClipLevel = _getter("clip_level")
    Shape = _getter("shape")
    Bias = _getter("bias")
    ChebyshevOrder = _getter("cheb_order")

    def SetChebyshevInvert(self, on: bool):  # :488-490
        self._set(self.P_CHEB_INVERT, 1 if on else 0)

    def SetChebyshevDCBypass(self, on: bool):  # :505-507
        self._set(self.P_CHEB_DC_BYPASS, 1 if on else 0)

    def SetChebyshevWeights(self, weights):  # :514-529
        w = f64(weights).reshape(-1)
        check(lib().ad_distortion_set_weights(self._h, ptr(w), int(w.size)))

    def derived(self):
        """dict(atan_scale=atan(1 + 4 shape), scale6=1 + 6 shape, scale2=1 + 2 shape, one_minus_mix,
        weights_active) of ad_distortion_derived: the constants the host computes for the kernels."""
        *v, w = self._out("derived", _F64 * 4 + _INT)
        return dict(atan_scale=v[0], scale6=v[1], scale2=v[2], one_minus_mix=v[3], weights_active=bool(w))

    def kernel_info(self):
        """(samples of a row per pointwise workgroup; channels per workgroup, samples staged per chunk and
        lds_bytes of the DC-bypass kernel) of ad_distortion_kernel_info."""
        return self._out("kernel_info", _INT * 4)

    def curve(self, x):
        """shapeSample(x) * outputLevel with the finite check, by the device
        code a call runs: the transfer curve.  Nothing advances."""
        xs = f64(x).reshape(-1)
        wet = np.empty_like(xs)
        check(lib().ad_distortion_curve(self._h, ptr(xs), int(xs.size), ptr(wet)))
        return wet.reshape(np.shape(x))


class BitCrusher(_ShaperHandle):
    """effects.BitCrusher (bit_crusher.go:92-230): NewBitCrusher(sample_rate,
    options...) with the options as keywords (bit_depth, downsample, mix), or
    `config` (a BitCrusherConfig) applied whole.  Every channel has its own
    hold value; the hold counter is one for all of them."""

    P_SAMPLE_RATE, P_BIT_DEPTH, P_MIX, P_DOWNSAMPLE = range(4)  # AD_BITCRUSHER_*
    _kind = "bitcrusher"
    _name = "bitcrusher"
    _config = BitCrusherConfig
    _options = ("bit_depth", "mix")
    _int_options = ("downsample",)

    SetBitDepth = _setter(P_BIT_DEPTH)  # :149-160
    SetDownsample = _setter(P_DOWNSAMPLE)  # :163-172
    BitDepth = _getter("bit_depth")  # :214-220
    Downsample = _getter("downsample")

    def derived(self, channel: int = 0):
        """dict(quant_levels, counter, hold_value) of ad_bitcrusher_derived: quantLevels = exp2(bitDepth - 1)
        as the host computed it, holdCounter, and holdValue of `channel`."""
        q, c, h = self._out("derived", _F64 + _INT + _F64, int(channel))
        return dict(quant_levels=q, counter=c, hold_value=h)

    def kernel_info(self):
        """(samples of a row per workgroup, the staged span of whole hold periods, lds_bytes) of
        ad_bitcrusher_kernel_info."""
        return self._out("kernel_info", _INT * 3)


class _DynHandle(_ConfigHandle):
    """What TransientShaper and DeEsser share: the attack and release times
    and their coefficients."""

    SetAttack = _setter("P_ATTACK")
    SetRelease = _setter("P_RELEASE")
    SetAttackCoeff = _setter("P_ATTACK_COEFF")  # attackCoeff, for a caller whose exp is not the C library's
    SetReleaseCoeff = _setter("P_RELEASE_COEFF")
    Attack = _getter("attack_ms")
    Release = _getter("release_ms")


def transient_derived(cfg: TransientConfig):
    """(attack_coeff, release_coeff) in use for a config, of ad_transient_derived: host only."""
    return _outputs(lib().ad_transient_derived, _F64 * 2, C.byref(cfg))


def deesser_derived(cfg: DeEsserConfig) -> dict:
    """dict(section=(b0, b1, b2, a1, a2), band_norm, threshold_log2, knee_width_log2, range_lin, attack_coeff,
    release_coeff) for a config, of ad_deesser_derived: what the reference caches, host only."""
    sec = (C.c_double * 5)()
    v = _outputs(lib().ad_deesser_derived, _F64 * 6, C.byref(cfg), sec)
    return dict(section=tuple(sec), band_norm=v[0], threshold_log2=v[1], knee_width_log2=v[2], range_lin=v[3],
                attack_coeff=v[4], release_coeff=v[5])


class TransientShaper(_DynHandle):
    """dynamics.TransientShaper (transient_shaper.go:25-200) for `channels`
    instances sharing one configuration: NewTransientShaper(sample_rate) with
    options as keywords (attack_amount, sustain_amount, attack_ms, release_ms,
    attack_coeff, release_coeff), or `config` (a TransientConfig) applied
    whole.  A rejected setter value raises ErrInvalidArgument and changes
    nothing."""

    (P_SAMPLE_RATE, P_ATTACK_AMOUNT, P_SUSTAIN_AMOUNT, P_ATTACK, P_RELEASE, P_ATTACK_COEFF,
     P_RELEASE_COEFF) = range(7)  # AD_TRANSIENT_*
    _kind = "transient"
    _name = "transient"
    _config = TransientConfig
    _options = ("attack_amount", "sustain_amount", "attack_ms", "release_ms", "attack_coeff", "release_coeff")

    SetAttackAmount = _setter(P_ATTACK_AMOUNT)  # :57-66
    SetSustainAmount = _setter(P_SUSTAIN_AMOUNT)  # :69-78
    AttackAmount = _getter("attack_amount")  # :120-132
    SustainAmount = _getter("sustain_amount")

    def derived(self):
        return transient_derived(self.config())

    def kernel_info(self):
        """(channels per workgroup, samples staged per chunk, lds_bytes) of the walk, of ad_transient_kernel_info."""
        return self._out("kernel_info", _INT * 3)

    def get_state(self, channel: int = 0) -> float:
        """The envelope of `channel`."""
        return self._out("get_state", _F64, int(channel))[0]

    def set_state(self, channel: int, envelope: float):
        check(lib().ad_transient_set_state(self._h, int(channel), float(envelope)))


class DeEsser(_DynHandle):
    """dynamics.DeEsser (deesser.go:100-622) for `channels` instances sharing
    one configuration: NewDeEsser(sample_rate) with options as keywords
    (freq_hz, q, threshold_db, ratio, knee_db, attack_ms, release_ms, range_db,
    attack_coeff, release_coeff, mode, detector, listen, filter_order), or
    `config` (a DeEsserConfig) applied whole.  A rejected setter value raises
    ErrInvalidArgument and changes nothing."""

    (P_SAMPLE_RATE, P_FREQ, P_Q, P_THRESHOLD, P_RATIO, P_KNEE, P_ATTACK, P_RELEASE, P_RANGE, P_ATTACK_COEFF,
     P_RELEASE_COEFF, P_MODE, P_DETECTOR, P_LISTEN, P_FILTER_ORDER) = range(15)  # AD_DEESSER_*
    SPLIT_BAND, WIDEBAND = 0, 1  # DeEsserMode :15-25
    DETECT_BANDPASS, DETECT_HIGHPASS = 0, 1  # DeEsserDetector :30-39
    _kind = "deesser"
    _name = "deesser"
    _config = DeEsserConfig
    _options = ("freq_hz", "q", "threshold_db", "ratio", "knee_db", "attack_ms", "release_ms", "range_db",
                "attack_coeff", "release_coeff")
    _int_options = ("mode", "detector", "listen", "filter_order")

    SetFrequency = _setter(P_FREQ)  # :228-244
    SetQ = _setter(P_Q)  # :248-259
    SetThreshold = _setter(P_THRESHOLD)  # :263-272
    SetRatio = _setter(P_RATIO)  # :276-287
    SetKnee = _setter(P_KNEE)  # :291-302
    SetRange = _setter(P_RANGE)  # :336-347
    SetMode = _setter(P_MODE)  # :350-358
    SetDetector = _setter(P_DETECTOR)  # :361-370
    SetFilterOrder = _setter(P_FILTER_ORDER)  # :381-391
    Frequency = _getter("freq_hz")  # :186-222
    Q = _getter("q")
    Threshold = _getter("threshold_db")
    Ratio = _getter("ratio")
    Knee = _getter("knee_db")
    Range = _getter("range_db")
    Mode = _getter("mode")
    Detector = _getter("detector")
    Listen = _getter("listen", bool)
    FilterOrder = _getter("filter_order")

    def SetListen(self, on: bool):  # :375-377
        self._set(self.P_LISTEN, 1 if on else 0)

    def GetMetrics(self, channel: int = 0):  # :499-501 -> (DetectionLevel, GainReduction)
        return self._out("metrics", _F64 * 2, int(channel))

    def ResetMetrics(self):  # :504-506
        check(lib().ad_deesser_reset_metrics(self._h))

    def derived(self) -> dict:
        return deesser_derived(self.config())

    def kernel_info(self):
        """(channels per workgroup, samples staged per chunk, lds_bytes, cascades walked) of the walk the next
        call runs, of ad_deesser_kernel_info."""
        return self._out("kernel_info", _INT * 4)

    def get_state(self, channel: int = 0):
        """(envelope, detect [4][2], band [4][2]) of `channel`: {d0, d1} of each section."""
        e = C.c_double()
        det, band = np.zeros((4, 2)), np.zeros((4, 2))
        check(lib().ad_deesser_get_state(self._h, int(channel), C.byref(e), ptr(det), ptr(band)))
        return e.value, det, band

    def set_state(self, channel: int, envelope: float, detect, band):
        det, bnd = f64(detect).reshape(4, 2), f64(band).reshape(4, 2)
        check(lib().ad_deesser_set_state(self._h, int(channel), float(envelope), ptr(det), ptr(bnd)))

    def gain(self, levels):
        """calculateGain(level) by the device code a call runs.  Nothing advances."""
        lv = f64(levels).reshape(-1)
        out = np.empty_like(lv)
        check(lib().ad_deesser_gain(self._h, ptr(lv), ptr(out), int(lv.size)))
        return out.reshape(np.shape(levels))


def _rows(t, channels: int):
    """(device pointer, row stride, n) of device rows [channels][stride]: anything with torch's data_ptr(),
    stride() and shape."""
    if t.dim() != 2 or t.shape[0] != channels or (t.shape[1] > 1 and t.stride(1) != 1):
        raise ValueError(f"device rows must be [{channels}][n] with unit sample stride")
    if t.element_size() != 8 or not t.is_floating_point():
        raise TypeError("device rows must be float64")
    n = int(t.shape[1])
    return t.data_ptr(), max(int(t.stride(0)), n) if channels == 1 else int(t.stride(0)), n  # one row: any stride


def vocoder_derived(cfg: VocoderConfig) -> dict:
    """What the reference caches for a config, of ad_vocoder_derived: host only.  dict(num_bands, factors,
    group_factors, group_of_band, downsample_max, analysis, synthesis, decimated [bands][5], antialias
    [groups][5], attack_coeff, release_coeff, ds_attack, ds_release [bands]); sections are {b0, b1, b2, a1, a2}."""
    t = VocoderTables()
    check(lib().ad_vocoder_derived(C.byref(cfg), C.byref(t)))
    nb, ng = t.num_bands, t.num_groups
    sec = lambda a, n: np.array([list(a[i]) for i in range(n)], dtype=np.float64).reshape(n, 5)  # noqa: E731
    on = ng > 0
    return dict(num_bands=nb, downsample_max=t.downsample_max, factors=list(t.factors[:nb]) if on else None,
                group_factors=list(t.group_factors[:ng]), group_of_band=list(t.group_of_band[:nb]) if on else None,
                analysis=sec(t.analysis, nb), synthesis=sec(t.synthesis, nb), decimated=sec(t.decimated, nb if on else 0),
                antialias=sec(t.antialias, ng), attack_coeff=t.attack_coeff, release_coeff=t.release_coeff,
                ds_attack=np.array(t.ds_attack[:nb if on else 0]), ds_release=np.array(t.ds_release[:nb if on else 0]))


class Vocoder(_ConfigHandle):
    """effects.Vocoder (vocoder.go:199-833) for `channels` instances sharing one
    configuration: NewVocoder(sample_rate, options...) with the options as
    keywords (layout, synth_q, attack_ms, release_ms, input_level, synth_level,
    vocoder_level, downsample), or `config` (a VocoderConfig) applied whole.
    synth_q given as a keyword is WithVocoderSynthesisQ: it overrides Bark's
    per-band default too.  Each channel has its own modulator row, carrier row
    and state.  A rejected value raises ErrInvalidArgument and changes nothing."""

    (P_SAMPLE_RATE, _P_SYNTH_Q, P_ATTACK, P_RELEASE, P_INPUT_LEVEL, P_SYNTH_LEVEL, P_VOCODER_LEVEL,
     P_DOWNSAMPLING) = range(8)  # AD_VOCODER_*
    THIRD_OCTAVE, BARK = 0, 1  # BandLayout :15-25
    _kind = "vocoder"
    _name = "vocoder"
    _config = VocoderConfig
    _options = ("synth_q", "attack_ms", "release_ms", "input_level", "synth_level", "vocoder_level")
    _int_options = ("layout",)
    _bool_options = ("downsample",)

    @classmethod
    def _option(cls, cfg, key, value):
        super()._option(cfg, key, value)
        if key == "synth_q":
            cfg.synth_q_set = 1

    SetSampleRate = _setter(P_SAMPLE_RATE)  # :673-683
    SetAttack = _setter(P_ATTACK)  # :772-783
    SetRelease = _setter(P_RELEASE)  # :786-797
    SetInputLevel = _setter(P_INPUT_LEVEL)  # :800-809
    SetSynthLevel = _setter(P_SYNTH_LEVEL)  # :812-821
    SetVocoderLevel = _setter(P_VOCODER_LEVEL)  # :824-833
    SampleRate = _getter("sample_rate")  # :688-717
    Layout = _getter("layout")
    SynthesisQ = _getter("synth_q")
    Attack = _getter("attack_ms")
    Release = _getter("release_ms")
    InputLevel = _getter("input_level")
    SynthLevel = _getter("synth_level")
    VocoderLevel = _getter("vocoder_level")
    Downsampling = _getter("downsample", bool)

    def SetDownsampling(self, on: bool):  # :737-769
        self._set(self.P_DOWNSAMPLING, 1 if on else 0)

    def NumBands(self) -> int:
        return self._out("num_bands", _INT)[0]

    def DownsampleFactors(self):  # :722-731: None with downsampling off
        f, n = (C.c_int * 32)(), C.c_int()
        check(lib().ad_vocoder_downsample_factors(self._h, f, 32, C.byref(n)))
        return list(f[:n.value]) if n.value else None

    def derived(self) -> dict:
        return vocoder_derived(self.config())

    def kernel_info(self):
        """(lanes per channel, samples per chunk, lds_bytes of a workgroup) of ad_vocoder_kernel_info."""
        return self._out("kernel_info", _INT * 3)

    def get_state(self, channel: int = 0):
        """(state [9][32], downsampleCount) of `channel`: rows {analysis s0, s1, synthesis s0, s1, decimated s0,
        s1, envelope} by band, then the anti-alias {s0, s1} by group."""
        st = np.zeros((9, 32))
        return (st,) + self._out("get_state", _INT, int(channel), ptr(st))

    def ProcessBlock(self, modulator, carrier) -> np.ndarray:  # :634-645 on host rows [channels][n]
        m = _as2d(np.ascontiguousarray(modulator, dtype=np.float64), self.channels)
        c = _as2d(np.ascontiguousarray(carrier, dtype=np.float64), self.channels)
        if m.shape != c.shape:
            raise ErrInvalidArgument(AD_ERR_INVALID_ARGUMENT, "vocoder: buffer length mismatch")
        out = np.empty_like(m)
        check(lib().ad_vocoder_process(self._h, ptr(m), ptr(c), ptr(out), m.shape[1]))
        return out.reshape(np.shape(modulator))

    def ProcessInPlace(self, buf):
        raise TypeError("a vocoder takes a modulator and a carrier: use ProcessBlock or process")

    def process(self, modulator, carrier, out=None, stream: int | None = None):
        """ProcessBlock on device rows [channels][stride] (torch tensors, or anything with their data_ptr(),
        stride() and shape), asynchronous on `stream`.  `out` may be the modulator or the carrier; None: the
        modulator, as the graph's node runs.  Returns out."""
        out = modulator if out is None else out
        (mp, ms, n), (cp, cs, cn), (op, os_, on) = (_rows(t, self.channels) for t in (modulator, carrier, out))
        if n != cn or n != on:  # :635-638
            raise ErrInvalidArgument(AD_ERR_INVALID_ARGUMENT, "vocoder: buffer length mismatch")
        self.process_device(mp, ms, cp, cs, op, os_, n, stream)
        return out

    def process_device(self, d_mod: int, mod_stride: int, d_car: int, car_stride: int, d_out: int, out_stride: int,
                       n: int, stream: int | None = None):
        check(self._device_fn(self._h, C.c_void_p(d_mod), int(mod_stride), C.c_void_p(d_car), int(car_stride),
                              C.c_void_p(d_out), int(out_stride), int(n), C.c_void_p(stream or 0)))


def lookahead_derived(cfg: LookaheadConfig) -> dict:
    """dict(attack_coeff, release_coeff, threshold_log2, delay_samples) for a config, of ad_lookahead_derived:
    what the limiter's Compressor core caches and the delay D, host only."""
    a, r, th, d = _outputs(lib().ad_lookahead_derived, _F64 * 3 + _I64, C.byref(cfg))
    return dict(attack_coeff=a, release_coeff=r, threshold_log2=th, delay_samples=d)


class LookaheadLimiter(_ConfigHandle):
    """dynamics.LookaheadLimiter (lookahead_limiter.go:23-239) for `channels`
    instances sharing one configuration: NewLookaheadLimiter(sample_rate) with
    options as keywords (threshold_db, release_ms, lookahead_ms), or `config`
    (a LookaheadConfig) applied whole.  A rejected setter value raises
    ErrInvalidArgument and changes nothing."""

    P_SAMPLE_RATE, P_THRESHOLD, P_RELEASE, P_LOOKAHEAD = range(4)  # AD_LOOKAHEAD_*
    _kind = "lookahead"
    _name = "lookahead limiter"
    _config = LookaheadConfig
    _options = ("threshold_db", "release_ms", "lookahead_ms")

    SetSampleRate = _setter(P_SAMPLE_RATE)  # :146-161
    SetThreshold = _setter(P_THRESHOLD)  # :99-113
    SetRelease = _setter(P_RELEASE)  # :116-130
    SetLookahead = _setter(P_LOOKAHEAD)  # :133-143
    SampleRate = _getter("sample_rate")  # :164-173
    Threshold = _getter("threshold_db")
    Release = _getter("release_ms")
    Lookahead = _getter("lookahead_ms")

    def derived(self) -> dict:
        return lookahead_derived(self.config())

    def DelaySamples(self) -> int:
        return self.derived()["delay_samples"]

    def get_state(self, channel: int = 0) -> float:
        """The detector envelope of `channel`."""
        return self._out("get_state", _F64, int(channel))[0]

    def gain(self, levels):
        """GainForLevel(level) by the device code a call runs.  Nothing advances."""
        lv = f64(levels).reshape(-1)
        out = np.empty_like(lv)
        check(lib().ad_lookahead_gain(self._h, ptr(lv), ptr(out), int(lv.size)))
        return out.reshape(np.shape(levels))

    def last_envelope(self, n: int) -> np.ndarray:
        """The detector envelope of every sample of the last call, [channels][n]."""
        out = np.zeros((self.channels, int(n)))
        check(lib().ad_lookahead_last_envelope(self._h, ptr(out), int(n)))
        return out

    def ProcessInPlace(self, buf):  # :213-217
        self.ProcessInPlaceSidechain(buf, None)

    def ProcessInPlaceSidechain(self, program, sidechain):  # :221-230 on host rows; a short sidechain reads as 0
        b = _as2d(program, self.channels)
        if sidechain is None:
            check(lib().ad_lookahead_process(self._h, ptr(b), None, 0, b.shape[1]))
            return
        s = _as2d(np.ascontiguousarray(sidechain, dtype=np.float64), self.channels)
        sp = ptr(s) if s.size else ptr(np.zeros(1))  # an empty sidechain is still a sidechain: all zeros
        check(lib().ad_lookahead_process(self._h, ptr(b), sp, s.shape[1], b.shape[1]))

    def process(self, program, sidechain=None, stream: int | None = None):
        """ProcessInPlace / ProcessInPlaceSidechain on device rows [channels][stride] (torch tensors, or anything
        with their data_ptr(), stride() and shape), asynchronous on `stream`.  Returns program."""
        pp, ps, n = _rows(program, self.channels)
        sp, ss, sn = (0, 0, 0) if sidechain is None else _rows(sidechain, self.channels)
        if sidechain is not None and sn == 0:
            sp, ss = pp, 0  # an empty sidechain is still a sidechain, all zeros: any address, never read
        self.process_device(pp, ps, n, stream, sp, ss, sn)
        return program

    def process_device(self, d_buf: int, stride: int, n: int, stream: int | None = None, d_side: int = 0,
                       side_stride: int = 0, side_n: int = 0):
        check(self._device_fn(self._h, C.c_void_p(d_buf), int(stride), C.c_void_p(d_side or None), int(side_stride),
                              int(side_n), int(n), C.c_void_p(stream or 0)))


def _freq_args(freqs):
    f = f64(list(freqs)).reshape(-1)
    return f, ptr(f), int(f.size)


def crossover_sections(freqs, order: int, sample_rate: float) -> np.ndarray:
    """The sections an ad_xover runs, [len(freqs)][2 (LP, HP)][S][5] {b0, b1, b2, a1, a2} (ad_xover_sections);
    host only."""
    f, fp, nf = _freq_args(freqs)
    s = C.c_int()
    check(lib().ad_xover_sections(fp, nf, int(order), float(sample_rate), None, 0, C.byref(s)))
    tab = np.zeros((nf, 2, s.value, 5))
    check(lib().ad_xover_sections(fp, nf, int(order), float(sample_rate), ptr(tab), int(tab.size), C.byref(s)))
    return tab


class MultiBandCrossover(_Handle):
    """crossover.MultiBand (dsp/filter/crossover/crossover.go:113-222) on `channels` lanes: len(freqs) cascaded
    two-way Linkwitz-Riley stages of one order, len(freqs) + 1 bands, every band bit for bit the reference's."""

    _kind = "xover"

    def __init__(self, freqs, order: int, sample_rate: float = 48000.0, channels: int = 1, device: int = DEVICE):
        f, fp, nf = _freq_args(freqs)
        self._create(channels, device, fp, nf, int(order), float(sample_rate))
        self._freqs, self._order, self._fs = f.copy(), int(order), float(sample_rate)
        self._sections = crossover_sections(f, order, sample_rate)

    def NumBands(self) -> int:  # :163
        return int(self._freqs.size) + 1

    def sections(self) -> np.ndarray:
        """[stages][2 (LP, HP)][S][5] {b0, b1, b2, a1, a2}: the sections in use."""
        return self._sections.copy()

    def ProcessBlock(self, x) -> np.ndarray:  # :194-215 -> [bands][channels][n]
        b = _as2d(np.ascontiguousarray(x, dtype=np.float64), self.channels)
        out = np.zeros((self.NumBands(), self.channels, b.shape[1]))
        check(lib().ad_xover_process(self._h, ptr(b), ptr(out), b.shape[1]))
        return out

    def ProcessInPlace(self, buf):
        raise TypeError("a crossover has no in-place form: use ProcessBlock")

    def process_device(self, d_in: int, in_stride: int, d_bands: int, row_stride: int, band_stride: int, n: int,
                       stream: int | None = None):
        check(self._device_fn(self._h, C.c_void_p(d_in), int(in_stride), C.c_void_p(d_bands), int(row_stride),
                              int(band_stride), int(n), C.c_void_p(stream or 0)))

    def get_state(self, channel: int = 0) -> np.ndarray:
        """[stages][2][S][2] {s0, s1} of `channel`."""
        st = np.zeros(self._sections.shape[:3] + (2,))
        check(lib().ad_xover_get_state(self._h, int(channel), ptr(st), int(st.size)))
        return st

    def set_state(self, channel: int, state):
        st = f64(state).reshape(self._sections.shape[:3] + (2,))
        check(lib().ad_xover_set_state(self._h, int(channel), ptr(st), int(st.size)))

    def kernel_info(self):
        """(waves per workgroup, samples per tile, lds_bytes) of ad_xover_kernel_info."""
        return self._out("kernel_info", _INT * 3)

    def set_pipelined(self, on: bool):
        """All stages in one launch as a pipeline over time tiles (True, the default), or one stage per launch;
        the same bits either way."""
        check(lib().ad_xover_set_pipelined(self._h, int(bool(on))))


class BandView:
    """Read-only view of one band's compressor (MultibandCompressor.Band): the reference's getters."""

    _GETTERS = {"Threshold": "threshold_db", "Ratio": "ratio", "Knee": "knee_db", "Attack": "attack_ms",
                "Release": "release_ms", "MakeupGain": "makeup_db", "RMSWindow": "rms_window_ms",
                "SidechainLowCut": "sidechain_low_cut_hz", "SidechainHighCut": "sidechain_high_cut_hz",
                "Topology": "topology", "DetectorMode": "detector_mode", "SampleRate": "sample_rate"}

    def __init__(self, cfg: CompressorConfig):
        object.__setattr__(self, "_cfg", cfg)

    def __getattr__(self, name):
        if name in BandView._GETTERS:
            return lambda: getattr(self._cfg, BandView._GETTERS[name])
        if name == "AutoMakeup":
            return lambda: bool(self._cfg.auto_makeup)
        if name == "FeedbackRatioScale":
            return lambda: bool(self._cfg.feedback_ratio_scale)
        return getattr(self._cfg, name)  # the config's own field names

    def __setattr__(self, name, value):
        raise AttributeError("a band view is read-only: use the MultibandCompressor setters")


# BandConfig fields (multiband.go:27-41) in applyBandConfig's order -> (setter, keep value)
_BAND_CONFIG = (("ThresholdDB", "SetBandThreshold", None), ("Ratio", "SetBandRatio", 0), ("KneeDB", "SetBandKnee", None),
                ("AttackMs", "SetBandAttack", 0), ("ReleaseMs", "SetBandRelease", 0),
                ("MakeupGainDB", "SetBandMakeupGain", None), ("AutoMakeup", "SetBandAutoMakeup", None),
                ("Topology", "SetBandTopology", None), ("DetectorMode", "SetBandDetectorMode", None),
                ("FeedbackRatioScale", "SetBandFeedbackRatioScale", None), ("RMSWindowMs", "SetBandRMSWindow", None),
                ("SidechainLowCutHz", "SetBandSidechainLowCut", None),
                ("SidechainHighCutHz", "SetBandSidechainHighCut", None))


class MultibandCompressor(_Handle):
    """dynamics.MultibandCompressor (dsp/effects/dynamics/multiband.go) on `channels` lanes: the crossover, one
    compressor per band, the bands summed in band order.  `configs`: one BandConfig-like dict per band
    (NewMultibandCompressorWithConfig :130-150); a key left out, None, or 0 for Ratio / AttackMs / ReleaseMs
    keeps the default.  Its per-band setters are SetBand<name>(band, v) for every name of _DYNAMICS_SETTERS,
    with SetAllBands<name>(v) where the reference has one."""

    _kind = "multiband"

    def __init__(self, freqs, order: int, sample_rate: float = 48000.0, channels: int = 1, device: int = DEVICE,
                 configs=None):
        f, fp, nf = _freq_args(freqs)
        if configs is not None and len(configs) != nf + 1:  # :131-135
            raise ErrInvalidArgument(AD_ERR_INVALID_ARGUMENT, f"expected {nf + 1} band configs, got {len(configs)}")
        self._create(channels, device, fp, nf, int(order), float(sample_rate))
        self._freqs, self._order, self._fs = f.copy(), int(order), float(sample_rate)
        for i, cfg in enumerate(configs or ()):
            self.SetBandConfig(i, cfg)

    def NumBands(self) -> int:  # :153-155
        return int(self._freqs.size) + 1

    def CrossoverFreqs(self) -> list:  # :158-163
        return [float(v) for v in self._freqs]

    def CrossoverOrder(self) -> int:  # :166-168
        return self._order

    def SampleRate(self) -> float:  # :171-173
        return self._fs

    def _band(self, band: int) -> CompressorConfig:
        cfg = CompressorConfig()
        check(lib().ad_multiband_get_band(self._h, int(band), C.byref(cfg)))
        return cfg

    def Band(self, i: int) -> BandView:  # :178-180
        return BandView(self._band(i))

    def _set(self, band: int, **kv):
        cfg = self._band(band)  # a bad band index raises here, checkBand :555-561
        for k, v in kv.items():
            setattr(cfg, k, v)
        check(lib().ad_multiband_set_band(self._h, int(band), C.byref(cfg)))  # rejected: nothing changes

    def SetBandConfig(self, band, cfg):  # :322-329, applyBandConfig :563-658: stops at the first rejected field
        self._band(band)
        unknown = set(cfg) - {k for k, _, _ in _BAND_CONFIG}
        if unknown:
            raise KeyError(f"unknown BandConfig field(s): {sorted(unknown)}")
        for key, setter, keep in _BAND_CONFIG:
            v = cfg.get(key)
            if v is None or (keep is not None and v == keep):
                continue
            getattr(self, setter)(band, v)

    def _all(self, setter, v):  # :331-437: stops at the first band that rejects; earlier bands stay changed
        for b in range(self.NumBands()):
            getattr(self, setter)(b, v)

    def ProcessInPlace(self, buf):  # :476-490
        self._process(buf)

    def ProcessInPlaceMulti(self, x) -> np.ndarray:  # :507-523 -> [bands][channels][n]; x is not written
        b = _as2d(np.ascontiguousarray(x, dtype=np.float64), self.channels)
        out = np.zeros((self.NumBands(), self.channels, b.shape[1]))
        check(lib().ad_multiband_process_multi(self._h, ptr(b), ptr(out), b.shape[1]))
        return out

    def ProcessStereoInPlace(self, left, right):  # :493-502 on a handle of two channels, one per side
        if self.channels != 2:
            raise ValueError("ProcessStereoInPlace needs a processor of two channels")
        if len(left) != len(right):
            raise ValueError(f"stereo buffers must have equal length, got {len(left)} and {len(right)}")
        both = np.stack([f64(left), f64(right)])
        self.ProcessInPlace(both)
        left[:], right[:] = both[0], both[1]

    def process_multi_device(self, d_in: int, in_stride: int, d_bands: int, row_stride: int, band_stride: int, n: int,
                             stream: int | None = None):
        check(lib().ad_multiband_process_multi_device(self._h, C.c_void_p(d_in), int(in_stride), C.c_void_p(d_bands),
                                                      int(row_stride), int(band_stride), int(n),
                                                      C.c_void_p(stream or 0)))

    def GetMetrics(self, channel: int = 0) -> list:  # :537-544 -> per band (InputPeak, OutputPeak, GainReduction)
        return [self._out("metrics", _F64 * 3, b, int(channel)) for b in range(self.NumBands())]

    def ResetMetrics(self):  # :547-551
        check(lib().ad_multiband_reset_metrics(self._h))

    def xover_state(self, channel: int = 0) -> np.ndarray:
        """The crossover's [stages][2][S][2] {s0, s1} of `channel`."""
        s = crossover_sections(self._freqs, self._order, self._fs).shape
        st = np.zeros(s[:3] + (2,))
        check(lib().ad_multiband_xover_state(self._h, int(channel), ptr(st), int(st.size)))
        return st

    def SetChunk(self, samples: int):
        """Runs every call in passes of at most `samples` samples (0: as many as the scratch cap allows)."""
        check(lib().ad_multiband_set_chunk(self._h, int(samples)))


def _band_setter(field, kind, also):
    def set_(self, band, v):
        self._set(band, **{field: kind(v)}, **also)
    return set_


def _all_bands_setter(setter):
    def set_(self, v):
        self._all(setter, v)
    return set_


for _name, _field, _kind, _also, _all_bands in _DYNAMICS_SETTERS:
    setattr(MultibandCompressor, "SetBand" + _name, _band_setter(_field, _kind, _also))
    if _all_bands:
        setattr(MultibandCompressor, "SetAllBands" + _name, _all_bands_setter("SetBand" + _name))
del _name, _field, _kind, _also, _all_bands


# window.Type (dsp/window/window.go:12-16) of the windows the STFT processors take
WindowRectangular, WindowHann, WindowHamming, WindowBlackman = range(4)
_WINDOW_COEFFS = {  # fixedCosineWindowCoeffs (window.go:283-286, tables.go:4-6)
    WindowHann: (0.5, -0.5),
    WindowHamming: (0.54, -0.46),
    WindowBlackman: (0.42, -0.5, 0.08),
}


def spectral_window(window_type: int, n: int) -> np.ndarray:
    """window.Generate(t, n, WithPeriodic()) (window.go:140-162) for the
    rectangular, Hann, Hamming and Blackman types: samplePosition i / n
    (:404-415), cosineFromCoeffs (:393-402).  Any other type raises."""
    t = int(window_type)
    if t == WindowRectangular:
        return np.ones(n)
    if t not in _WINDOW_COEFFS:
        raise ValueError(f"window type {window_type} is not supported by the STFT processors")
    x = np.arange(n, dtype=np.float64) / float(n) if n > 1 else np.zeros(n)
    phase = 2 * np.pi * x
    s = np.zeros(n)
    for k, c in enumerate(_WINDOW_COEFFS[t]):
        s = s + c * np.cos(float(k) * phase)
    return s


class _StftHandle(_ConfigHandle):
    """What SpectralFreeze and SpectralPitchShifter share: the frame size and
    the window, whose table this layer computes, and the Process forms.  The
    constructors take no `config`: a config's window table is this layer's."""

    def __init__(self, sample_rate: float = 48000.0, channels: int = 1, device: int = DEVICE, **options):
        super().__init__(sample_rate, channels, device, None, **options)

    @classmethod
    def _make_config(cls, sample_rate, config=None, **options):
        cfg = super()._make_config(sample_rate, config, **options)
        cfg._window = spectral_window(cfg.window_type, max(cfg.frame_size, 0))  # the table lives with the structure
        cfg.window = ptr(cfg._window)
        return cfg

    def SetFrameSize(self, size: int):
        size = int(size)
        if size < 64 or size & (size - 1):  # the table needs a valid size; the library repeats the check
            raise ErrInvalidArgument(AD_ERR_INVALID_ARGUMENT, f"frame size must be power-of-two and >= 64: {size}")
        w = spectral_window(self.WindowType(), size)
        check(self._fn("set_frame")(self._h, size, ptr(w)))

    def SetWindowType(self, window_type: int):
        w = spectral_window(window_type, self.FrameSize())
        check(self._fn("set_window")(self._h, int(window_type), ptr(w)))

    FrameSize = _getter("frame_size")
    WindowType = _getter("window_type")

    def Process(self, x) -> np.ndarray:
        out = f64(x).copy()
        if out.size:
            self.ProcessInPlace(out)
        return out

    PASSES = ("analysis", "walk", "synthesis", "overlap_add", "resample", "fused_frames")  # AD_STFT_PASS_*

    def profile(self, enable: bool, read: bool = False):
        """ad_*_profile: switch the per-pass event timing on or off; with `read`, the milliseconds per pass
        of the calls made while it was on."""
        ms = np.zeros(len(self.PASSES))
        check(self._fn("profile")(self._h, 1 if enable else 0, ptr(ms) if read else None))
        return dict(zip(self.PASSES, ms.tolist())) if read else None


class SpectralFreeze(_StftHandle):
    """effects.SpectralFreeze (spectral_freeze.go:36-414) for `channels`
    instances sharing one configuration: NewSpectralFreeze(sample_rate) with
    options as keywords (frame_size, hop_size, mix, phase_mode, frozen,
    window_type).  One call handles a whole buffer.  A rejected setter value
    raises ErrInvalidArgument and changes nothing."""

    PhaseHold, PhaseAdvance = 0, 1  # SpectralFreezePhaseMode :23-28
    P_SAMPLE_RATE, P_HOP, P_MIX, P_PHASE_MODE, P_FROZEN = range(5)  # AD_SPECFREEZE_*
    _kind = "specfreeze"
    _name = "spectral freeze"
    _config = SpecFreezeConfig
    _options = ("mix",)
    _int_options = ("frame_size", "hop_size", "phase_mode", "frozen", "window_type")

    SetHopSize = _setter(P_HOP)
    SetMix = _setter(P_MIX)
    SetPhaseMode = _setter(P_PHASE_MODE)
    HopSize = _getter("hop_size")
    Mix = _getter("mix")
    PhaseMode = _getter("phase_mode")
    Frozen = _getter("frozen", bool)

    def SetFrozen(self, frozen: bool):
        self._set(self.P_FROZEN, 1 if frozen else 0)

    def Freeze(self):
        self.SetFrozen(True)

    def Unfreeze(self):
        self.SetFrozen(False)

    def state(self):
        """(heldMagnitude [channels][N/2+1], phaseAcc [channels][N/2+1], hasFrozenFrame) of ad_specfreeze_state."""
        bins = self.FrameSize() // 2 + 1
        held, acc = np.zeros((self.channels, bins)), np.zeros((self.channels, bins))
        return held, acc, bool(self._out("state", _INT, ptr(held), ptr(acc))[0])

    def norm(self, n: int) -> np.ndarray:
        """The overlap-add norm (sum of w^2 in ascending frame order) of a call of n samples, by the device code."""
        out = np.zeros(int(n))
        check(lib().ad_specfreeze_norm(self._h, ptr(out), int(n)))
        return out


def pitchspec_resample_taps(analysis_hop: int, synthesis_hop: int, quality: int) -> np.ndarray:
    """The prototype resample.Resample(x, analysisHop, synthesisHop, WithQuality(q))
    designs (resample.go:153-187): the hops reduced by their gcd, the quality's profile."""
    from . import resample as rs

    g = rs._gcd(int(analysis_hop), int(synthesis_hop))
    p = rs.QualityProfile(int(quality))
    return rs.design_polyphase_fir(int(analysis_hop) // g, int(synthesis_hop) // g, p.TapsPerPhase, p.CutoffScale,
                                   p.KaiserBeta)


class SpectralPitchShifter(_StftHandle):
    """pitch.SpectralPitchShifter (pitch_shift_spectral.go:36-646) for `channels`
    instances sharing one configuration: NewSpectralPitchShifter(sample_rate)
    with options as keywords (pitch_ratio, frame_size, analysis_hop,
    window_type, resample_quality).  Stateless between calls.  The prototype
    of the time stretch's resampling is designed here whenever the hops or the
    quality change.  A rejected setter value raises and changes nothing."""

    P_SAMPLE_RATE, P_RATIO, P_HOP, P_RESAMPLE_QUALITY = range(4)  # AD_PITCHSPEC_*
    _kind = "pitchspec"
    _name = "spectral pitch shifter"
    _config = PitchSpecConfig
    _options = ("pitch_ratio",)
    _int_options = ("frame_size", "analysis_hop", "window_type", "resample_quality")

    def __init__(self, sample_rate: float = 48000.0, channels: int = 1, device: int = DEVICE, **options):
        super().__init__(sample_rate, channels, device, **options)
        self._sync_taps()

    def _sync_taps(self):
        c = self.config()
        hop, shop = c.analysis_hop, self.SynthesisHop()
        if c.n_resample_taps == 0 and self.path() == 2 and shop != hop:
            t = pitchspec_resample_taps(hop, shop, c.resample_quality)
            check(lib().ad_pitchspec_set_resample_taps(self._h, ptr(t), t.size))

    def _set(self, which: int, v):
        super()._set(which, v)
        self._sync_taps()

    def SetFrameSize(self, size: int):
        super().SetFrameSize(size)
        self._sync_taps()

    SetPitchRatio = _setter(P_RATIO)
    SetAnalysisHop = _setter(P_HOP)
    SetResampleQuality = _setter(P_RESAMPLE_QUALITY)
    PitchRatio = _getter("pitch_ratio")
    AnalysisHop = _getter("analysis_hop")
    ResampleQuality = _getter("resample_quality")

    def SetPitchSemitones(self, semitones: float):  # :164-177
        s = float(semitones)
        if not np.isfinite(s):
            raise ErrInvalidArgument(AD_ERR_INVALID_ARGUMENT, f"spectral pitch shifter semitones must be finite: {s}")
        self.SetPitchRatio(2.0 ** (s / 12.0))

    def PitchSemitones(self) -> float:  # :103
        return 12.0 * float(np.log2(self.PitchRatio()))

    def EffectivePitchRatio(self) -> float:
        return self._out("effective_ratio", _F64)[0]

    def SynthesisHop(self) -> int:
        return self._out("synthesis_hop", _INT)[0]

    def path(self) -> int:
        """0: the identity shortcut, 1: bin shifting, 2: time stretch (ad_pitchspec_path)."""
        return self._out("path", _INT)[0]


class EffectChain(_FxChain):
    """effectchain `_input -> filter-* -> dyn-compressor -> reverb-freeverb ->
    _output` for `channels` chains, fused per sample (chain_process.go:11-33).

    eq: list of (coeffs [sections][5], gain) biquad chains (filter nodes, in
    order); compressor: dict of ad_compressor_config fields or None;
    freeverb: (wet, dry, room, damp, gain) or None."""

    def __init__(self, channels: int, eq=(), compressor=None, freeverb=None, sample_rate: float = 48000.0,
                 device: int = DEVICE):
        super().__init__(channels, device)
        tabs = [section_table(c, g) for c, g in eq]
        t = np.concatenate(tabs) if tabs else np.zeros((0, SEC_STRIDE))
        check(lib().ad_fx_chain_set_eq(self._h, ptr(f64(t)), t.shape[0], 0))
        if compressor is not None:
            cfg = CompressorConfig()
            lib().ad_compressor_default_config(C.byref(cfg), float(sample_rate))
            for k, v in compressor.items():
                setattr(cfg, k, v)
            self.cfg = cfg
            check(lib().ad_fx_chain_set_compressor(self._h, C.byref(cfg)))
        if freeverb is not None:
            check(lib().ad_fx_chain_set_freeverb(self._h, *map(float, freeverb)))

    def Process(self, buf):
        self._process(buf)


class Filter(_Handle):
    """fir.Filter (filter.go:11-172) for `channels` lanes sharing the taps."""

    _kind = "fir"

    def __init__(self, coeffs, channels: int = 1, device: int = DEVICE):
        self.coeffs = f64(coeffs).ravel()
        self._create(channels, device, ptr(self.coeffs), self.coeffs.size)

    def ProcessBlock(self, buf):  # :74-114
        b = _as2d(buf, self.channels)
        check(lib().ad_fir_process_block(self._h, ptr(b), b.shape[1]))

    def ProcessBlockTo(self, dst, src):  # :119-159
        d, s = _as2d(dst, self.channels), _as2d(f64(src), self.channels)
        if d.shape != s.shape:
            raise ValueError("dst/src length mismatch")
        check(lib().ad_fir_process_block_to(self._h, ptr(d), ptr(s), s.shape[1]))

    def ProcessSample(self, x: float) -> float:  # :46-69 (one channel)
        b = np.array([[x]] * self.channels, dtype=np.float64)
        self.ProcessBlock(b)
        return float(b[0, 0])

    def process_device(self, d_src: int, src_stride: int, d_dst: int, dst_stride: int, n: int,
                       stream: int | None = None):
        check(self._device_fn(self._h, C.c_void_p(d_src), int(src_stride), C.c_void_p(d_dst), int(dst_stride), int(n),
                              C.c_void_p(stream or 0)))


def chain_process(coeffs, state, gain, buf):
    """ad_biquad_chain_process: one-shot Chain.ProcessBlock, state in/out."""
    c = f64(coeffs).reshape(-1, 5)
    b = _as2d(buf, buf.shape[0] if buf.ndim == 2 else 1)
    st = state
    if not (isinstance(st, np.ndarray) and st.dtype == np.float64 and st.flags.c_contiguous
            and st.size == b.shape[0] * c.shape[0] * 2):
        raise TypeError("state must be a C-contiguous float64 array [channels][sections][2]")
    check(lib().ad_biquad_chain_process(ptr(c), ptr(st), float(gain), ptr(b), b.shape[0], c.shape[0], b.shape[1],
                                        DEVICE))
