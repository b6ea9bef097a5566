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


class _FxChain:
    def __init__(self, channels: int, device: int):
        self.channels = int(channels)
        self._h = C.c_void_p()
        check(lib().ad_fx_chain_create(self.channels, int(device), C.byref(self._h)))

    def _process(self, buf):
        b = _as2d(buf, self.channels)
        check(lib().ad_fx_chain_process(self._h, ptr(b), b.shape[1]))

    def process_device(self, d_buf: int, stride: int, n: int, stream: int | None = None):
        check(lib().ad_fx_chain_process_device(self._h, C.c_void_p(d_buf), int(stride), int(n),
                                               C.c_void_p(stream or 0)))

    def Reset(self):
        check(lib().ad_fx_chain_reset(self._h))

    # engine selection (include/algodsp.h ad_fx_chain_set_engine); the fused
    # and staged engines give identical results, the time-parallel one within
    # 1e-12 relative RMS of them
    ENGINE_AUTO, ENGINE_FUSED, ENGINE_STAGED_NOSPLIT, ENGINE_STAGED, ENGINE_TIME_PARALLEL = 0, 1, 2, 3, 4

    def SetEngine(self, engine: int, chunk: int = 0):
        check(lib().ad_fx_chain_set_engine(self._h, int(engine), int(chunk)))

    def LastEngine(self) -> tuple[int, float]:
        """(engine that ran the last call, the EQ's round-off noise estimate)
        (ad_fx_chain_last_engine)."""
        e, ng = C.c_int(), C.c_double()
        check(lib().ad_fx_chain_last_engine(self._h, C.byref(e), C.byref(ng)))
        return e.value, ng.value

    def close(self):
        if self._h:
            lib().ad_fx_chain_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


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


class Compressor(_FxChain):
    """dynamics.Compressor (compressor.go:39-431) on `channels` lanes."""

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

    # setters (compressor.go:130-305, core.go:131-250)
    def SetThreshold(self, db):
        self._set(threshold_db=db)

    def SetRatio(self, r):
        self._set(ratio=r)

    def SetKnee(self, db):
        self._set(knee_db=db)

    def SetAttack(self, ms):
        self._set(attack_ms=ms)

    def SetRelease(self, ms):
        self._set(release_ms=ms)

    def SetRMSWindow(self, ms):
        self._set(rms_window_ms=ms)

    def SetSidechainLowCut(self, hz):
        self._set(sidechain_low_cut_hz=hz)

    def SetSidechainHighCut(self, hz):
        self._set(sidechain_high_cut_hz=hz)

    def SetAutoMakeup(self, on: bool):
        self._set(auto_makeup=int(bool(on)))

    def SetMakeupGain(self, db):  # SetManualMakeupGain (core.go:201-210) turns auto makeup off
        self._set(makeup_db=db, auto_makeup=0)

    def SetTopology(self, topology: int):  # core.go:106-114
        self._set(topology=int(topology))

    def SetDetectorMode(self, mode: int):  # core.go:116-124
        self._set(detector_mode=int(mode))

    def SetFeedbackRatioScale(self, on: bool):  # core.go:126-129
        self._set(feedback_ratio_scale=int(bool(on)))

    def ProcessInPlace(self, buf):  # compressor.go:362-366
        self._process(buf)

    def Metrics(self, channel: int = 0):
        ip, op, gr = C.c_double(), C.c_double(), C.c_double()
        check(lib().ad_fx_chain_compressor_metrics(self._h, int(channel), C.byref(ip), C.byref(op), C.byref(gr)))
        return ip.value, op.value, gr.value


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


class Reverb(_FxChain):
    """reverb.Reverb (Freeverb, reverb.go:33-235) with NewReverb defaults."""

    def __init__(self, channels: int = 1, device: int = DEVICE):
        super().__init__(channels, device)
        self.wet, self.dry, self.room, self.damp, self.gain = 0.22, 1.0, 0.72, 0.45, 0.015
        self._apply()

    def _apply(self):
        check(lib().ad_fx_chain_set_freeverb(self._h, self.wet, self.dry, self.room, self.damp, self.gain))

    def SetWet(self, v):
        self.wet = float(v)
        self._apply()

    def SetDry(self, v):
        self.dry = float(v)
        self._apply()

    def SetRoomSize(self, v):
        self.room = float(v)
        self._apply()

    def SetDamp(self, v):
        self.damp = float(v)
        self._apply()

    def SetGain(self, v):
        self.gain = float(v)
        self._apply()

    def ProcessInPlace(self, buf):  # reverb.go:185-189
        self._process(buf)


class FDNReverb:
    """reverb.FDNReverb (fdn_reverb.go:37-391) for `channels` instances sharing
    one configuration: NewFDNReverb(sample_rate), or `config` (an FdnConfig)
    applied whole.  The setters are the reference's, side effects included
    (ad_fdn_set_param); a rejected value raises ErrInvalidArgument and changes
    nothing."""

    P_SAMPLE_RATE, P_WET, P_DRY, P_RT60, P_DAMP, P_PRE_DELAY, P_MOD_DEPTH, P_MOD_RATE = range(8)  # AD_FDN_*

    def __init__(self, sample_rate: float = 44100.0, channels: int = 1, device: int = DEVICE, config=None):
        self.channels = int(channels)
        self._h = C.c_void_p()
        cfg = FdnConfig()
        if config is None:
            lib().ad_fdn_default_config(C.byref(cfg), float(sample_rate))
        else:
            C.memmove(C.byref(cfg), C.byref(config), C.sizeof(cfg))
        check(lib().ad_fdn_create(C.byref(cfg), self.channels, int(device), C.byref(self._h)))

    def _set(self, which: int, v):
        check(lib().ad_fdn_set_param(self._h, which, float(v)))

    def config(self) -> FdnConfig:
        cfg = FdnConfig()
        check(lib().ad_fdn_get_config(self._h, C.byref(cfg)))
        return cfg

    def SetSampleRate(self, v):  # :95-106
        self._set(self.P_SAMPLE_RATE, v)

    def SetWet(self, v):  # :109-117
        self._set(self.P_WET, v)

    def SetDry(self, v):  # :120-128
        self._set(self.P_DRY, v)

    def SetRT60(self, v):  # :131-140
        self._set(self.P_RT60, v)

    def SetDamp(self, v):  # :143-151
        self._set(self.P_DAMP, v)

    def SetPreDelay(self, v):  # :154-163
        self._set(self.P_PRE_DELAY, v)

    def SetModDepth(self, v):  # :166-175
        self._set(self.P_MOD_DEPTH, v)

    def SetModRate(self, v):  # :178-186
        self._set(self.P_MOD_RATE, v)

    def SampleRate(self) -> float:  # :251-272
        return self.config().sample_rate

    def Wet(self) -> float:
        return self.config().wet

    def Dry(self) -> float:
        return self.config().dry

    def RT60(self) -> float:
        return self.config().rt60_seconds

    def Damp(self) -> float:
        return self.config().damp

    def PreDelay(self) -> float:
        return self.config().pre_delay_seconds

    def ModDepth(self) -> float:
        return self.config().mod_depth_seconds

    def ModRate(self) -> float:
        return self.config().mod_rate_hz

    def derived(self):
        """(feedback gains [8], line lengths [8], pre-delay line length, LFO
        phase): what reconfigureDelays / updateFeedbackGains derived, and the
        phase after the last call (ad_fdn_derived)."""
        g = np.zeros(8)
        ln = np.zeros(8, dtype=np.int64)
        pl, ph = C.c_int64(), C.c_double()
        check(lib().ad_fdn_derived(self._h, ptr(g), ln.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(pl),
                                   C.byref(ph)))
        return g, ln, pl.value, ph.value

    def kernel_info(self):
        """(block, sub_block, lds_bytes) of ad_fdn_kernel_info."""
        a, b, c = C.c_int(), C.c_int(), C.c_int()
        check(lib().ad_fdn_kernel_info(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def ProcessInPlace(self, buf):  # :244-248
        b = _as2d(buf, self.channels)
        check(lib().ad_fdn_process(self._h, ptr(b), b.shape[1]))

    def process_device(self, d_buf: int, stride: int, n: int, stream: int | None = None):
        check(lib().ad_fdn_process_device(self._h, C.c_void_p(d_buf), int(stride), int(n), C.c_void_p(stream or 0)))

    def Reset(self):  # :189-197
        check(lib().ad_fdn_reset(self._h))

    def close(self):
        if self._h:
            lib().ad_fdn_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _Handle:
    """A C handle with process / process_device / reset / destroy named ad_<kind>_*."""

    _kind = ""

    def _fn(self, name):
        return getattr(lib(), f"ad_{self._kind}_{name}")

    def ProcessInPlace(self, buf):
        b = _as2d(buf, self.channels)
        check(self._fn("process")(self._h, ptr(b), b.shape[1]))

    def process_device(self, d_buf: int, stride: int, n: int, stream: int | None = None):
        check(self._fn("process_device")(self._h, C.c_void_p(d_buf), int(stride), int(n), C.c_void_p(stream or 0)))

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


class Delay(_Handle):
    """effects.Delay (delay.go:25-257) for `channels` instances sharing one
    configuration: NewDelay(sample_rate), or `config` (a DelayConfig) as
    ad_delay_create applies it (NewDelay, then SetTargetTime, SetFeedback,
    SetMix; mode 1 is the graph's delay-simple).  The setters are the
    reference's; a rejected value raises ErrInvalidArgument and changes nothing."""

    P_SAMPLE_RATE, P_TIME, P_FEEDBACK, P_MIX, P_TARGET_TIME, P_SAMPLES, P_SMOOTH_COEFF = range(7)  # AD_DELAY_*
    _kind = "delay"

    def __init__(self, sample_rate: float = 48000.0, channels: int = 1, device: int = DEVICE, config=None):
        self.channels = int(channels)
        self._h = C.c_void_p()
        cfg = DelayConfig()
        if config is None:
            lib().ad_delay_default_config(C.byref(cfg), float(sample_rate))
        else:
            C.memmove(C.byref(cfg), C.byref(config), C.sizeof(cfg))
        check(lib().ad_delay_create(C.byref(cfg), self.channels, int(device), C.byref(self._h)))

    def _set(self, which: int, v):
        check(lib().ad_delay_set_param(self._h, which, float(v)))

    def config(self) -> DelayConfig:
        cfg = DelayConfig()
        check(lib().ad_delay_get_config(self._h, C.byref(cfg)))
        return cfg

    def SetSampleRate(self, v):  # :63-72
        self._set(self.P_SAMPLE_RATE, v)

    def SetTime(self, v):  # :77-89
        self._set(self.P_TIME, v)

    def SetTargetTime(self, v):  # :95-106
        self._set(self.P_TARGET_TIME, v)

    def SetFeedback(self, v):  # :109-117
        self._set(self.P_FEEDBACK, v)

    def SetMix(self, v):  # :120-128
        self._set(self.P_MIX, v)

    def SetDelaySamples(self, v):  # mode 1: simpleDelayRuntime.Configure
        self._set(self.P_SAMPLES, v)

    def SetSmoothCoeff(self, v):  # smoothCoeff, for a caller whose exp is not the C library's
        self._set(self.P_SMOOTH_COEFF, v)

    def SampleRate(self) -> float:  # :176-185
        return self.config().sample_rate

    def Time(self) -> float:
        return self.config().time_seconds

    def Feedback(self) -> float:
        return self.config().feedback

    def Mix(self) -> float:
        return self.config().mix

    def derived(self):
        """(currentSamples, targetSamples, ring length, write position) of ad_delay_derived."""
        c, t, ln, wp = C.c_double(), C.c_double(), C.c_int64(), C.c_int64()
        check(lib().ad_delay_derived(self._h, C.byref(c), C.byref(t), C.byref(ln), C.byref(wp)))
        return c.value, t.value, ln.value, wp.value

    def CurrentDelaySamples(self) -> float:  # :189
        return self.derived()[0]

    def kernel_info(self):
        """(block, sub_block, regime of the last call, its launches) of ad_delay_kernel_info."""
        v = [C.c_int() for _ in range(4)]
        check(lib().ad_delay_kernel_info(self._h, *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def set_regime(self, regime: int):
        """0: the library chooses; 1: one launch per block; 2: one persistent launch."""
        check(lib().ad_delay_set_regime(self._h, int(regime)))


class Flanger(_Handle):
    """modulation.Flanger (flanger.go:108-424) for `channels` instances sharing
    one configuration: NewFlanger(sample_rate, options...) with the options as
    keywords (rate_hz, depth_seconds, base_delay_seconds, feedback, mix), or
    `config` (a FlangerConfig) applied whole."""

    P_SAMPLE_RATE, P_RATE, P_DEPTH, P_BASE_DELAY, P_FEEDBACK, P_MIX = range(6)  # AD_FLANGER_*
    _kind = "flanger"

    def __init__(self, sample_rate: float = 48000.0, channels: int = 1, device: int = DEVICE, config=None, **options):
        self.channels = int(channels)
        self._h = C.c_void_p()
        cfg = FlangerConfig()
        if config is None:
            lib().ad_flanger_default_config(C.byref(cfg), float(sample_rate))
        else:
            C.memmove(C.byref(cfg), C.byref(config), C.sizeof(cfg))
        for k, v in options.items():
            if k not in ("rate_hz", "depth_seconds", "base_delay_seconds", "feedback", "mix"):
                raise TypeError(f"unknown flanger option {k!r}")
            setattr(cfg, k, float(v))
        check(lib().ad_flanger_create(C.byref(cfg), self.channels, int(device), C.byref(self._h)))

    def _set(self, which: int, v):
        check(lib().ad_flanger_set_param(self._h, which, float(v)))

    def config(self) -> FlangerConfig:
        cfg = FlangerConfig()
        check(lib().ad_flanger_get_config(self._h, C.byref(cfg)))
        return cfg

    def SetSampleRate(self, v):  # :165-173
        self._set(self.P_SAMPLE_RATE, v)

    def SetRateHz(self, v):  # :176-184
        self._set(self.P_RATE, v)

    def SetDepthSeconds(self, v):  # :187-203
        self._set(self.P_DEPTH, v)

    def SetBaseDelaySeconds(self, v):  # :206-224
        self._set(self.P_BASE_DELAY, v)

    def SetFeedback(self, v):  # :227-235
        self._set(self.P_FEEDBACK, v)

    def SetMix(self, v):  # :238-246
        self._set(self.P_MIX, v)

    def SampleRate(self) -> float:  # :299-314
        return self.config().sample_rate

    def RateHz(self) -> float:
        return self.config().rate_hz

    def DepthSeconds(self) -> float:
        return self.config().depth_seconds

    def BaseDelaySeconds(self) -> float:
        return self.config().base_delay_seconds

    def Feedback(self) -> float:
        return self.config().feedback

    def Mix(self) -> float:
        return self.config().mix

    def derived(self):
        """(ring length, maxDelay, write position, LFO phase after the last call) of ad_flanger_derived."""
        ln, md, wp, ph = C.c_int64(), C.c_int64(), C.c_int64(), C.c_double()
        check(lib().ad_flanger_derived(self._h, C.byref(ln), C.byref(md), C.byref(wp), C.byref(ph)))
        return ln.value, md.value, wp.value, ph.value

    def kernel_info(self):
        """(block, sub_block, channels per workgroup, lds_bytes) of ad_flanger_kernel_info."""
        v = [C.c_int() for _ in range(4)]
        check(lib().ad_flanger_kernel_info(self._h, *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)


class _ModHandle(_Handle):
    """What Phaser, Tremolo and RingModulator share: a config structure whose
    field k is parameter k, options as keywords, and peek_lfo."""

    _config = None
    _options = ()

    def __init__(self, sample_rate: float = 48000.0, channels: int = 1, device: int = DEVICE, config=None, **options):
        self.channels = int(channels)
        self._h = C.c_void_p()
        cfg = self._config()
        if config is None:
            self._fn("default_config")(C.byref(cfg), float(sample_rate))
        else:
            C.memmove(C.byref(cfg), C.byref(config), C.sizeof(cfg))
        for k, v in options.items():
            if k not in self._options:
                raise TypeError(f"unknown {self._kind} option {k!r}")
            setattr(cfg, k, int(v) if k == "stages" else float(v))
        check(self._fn("create")(C.byref(cfg), self.channels, int(device), C.byref(self._h)))

    def _set(self, which: int, v):
        check(self._fn("set_param")(self._h, which, float(v)))

    def config(self):
        cfg = self._config()
        check(self._fn("get_config")(self._h, C.byref(cfg)))
        return cfg

    def peek_lfo(self, n: int):
        """(phases, table) of the next n samples as the kernels would take them:
        the table is the phaser's allpass coefficient, the tremolo's gain or the
        ring modulator's carrier.  Nothing advances; phases[0] is the phase state."""
        ph, tab = np.empty(int(n)), np.empty(int(n))
        check(self._fn("peek_lfo")(self._h, int(n), ptr(ph), ptr(tab)))
        return ph, tab

    def SetSampleRate(self, v):
        self._set(0, v)

    def SetMix(self, v):
        self._set(self.P_MIX, v)

    def SampleRate(self) -> float:
        return self.config().sample_rate

    def Mix(self) -> float:
        return self.config().mix


class Phaser(_ModHandle):
    """modulation.Phaser (phaser.go:130-379) for `channels` instances sharing one
    configuration: NewPhaser(sample_rate, options...) with the options as
    keywords (rate_hz, min_freq_hz, max_freq_hz, stages, feedback, mix), or
    `config` (a PhaserConfig) applied whole.  A rejected setter value raises
    ErrInvalidArgument and changes nothing."""

    P_SAMPLE_RATE, P_RATE, P_MIN_FREQ, P_MAX_FREQ, P_FEEDBACK, P_MIX, P_STAGES = range(7)  # AD_PHASER_*
    _kind = "phaser"
    _config = PhaserConfig
    _options = ("rate_hz", "min_freq_hz", "max_freq_hz", "stages", "feedback", "mix")

    def SetRateHz(self, v):  # :194-202
        self._set(self.P_RATE, v)

    def SetFrequencyRangeHz(self, min_freq_hz, max_freq_hz):  # :205-218
        check(lib().ad_phaser_set_range(self._h, float(min_freq_hz), float(max_freq_hz)))

    def SetStages(self, v):  # :221-233
        self._set(self.P_STAGES, v)

    def SetFeedback(self, v):  # :236-244
        self._set(self.P_FEEDBACK, v)

    def RateHz(self) -> float:  # :302-320
        return self.config().rate_hz

    def MinFrequencyHz(self) -> float:
        return self.config().min_freq_hz

    def MaxFrequencyHz(self) -> float:
        return self.config().max_freq_hz

    def Stages(self) -> int:
        return self.config().stages

    def Feedback(self) -> float:
        return self.config().feedback

    def kernel_info(self):
        """(channels per workgroup, samples staged per chunk, lds_bytes) of ad_phaser_kernel_info."""
        v = [C.c_int() for _ in range(3)]
        check(lib().ad_phaser_kernel_info(self._h, *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)


class Tremolo(_ModHandle):
    """modulation.Tremolo (tremolo.go:86-294): NewTremolo(sample_rate,
    options...) with the options as keywords (rate_hz, depth, smoothing_ms,
    mix), or `config` (a TremoloConfig) applied whole."""

    P_SAMPLE_RATE, P_RATE, P_DEPTH, P_SMOOTHING, P_MIX, P_SMOOTHING_COEFF = range(6)  # AD_TREMOLO_*
    _kind = "tremolo"
    _config = TremoloConfig
    _options = ("rate_hz", "depth", "smoothing_ms", "mix", "smoothing_coeff")

    def SetRateHz(self, v):  # :150-158
        self._set(self.P_RATE, v)

    def SetDepth(self, v):  # :161-169
        self._set(self.P_DEPTH, v)

    def SetSmoothingMs(self, v):  # :172-181
        self._set(self.P_SMOOTHING, v)

    def SetSmoothingCoeff(self, v):  # smoothingCoef, for a caller whose exp is not the C library's
        self._set(self.P_SMOOTHING_COEFF, v)

    def RateHz(self) -> float:  # :233-246
        return self.config().rate_hz

    def Depth(self) -> float:
        return self.config().depth

    def SmoothingMs(self) -> float:
        return self.config().smoothing_ms

    def kernel_info(self):
        """(samples of a row per apply workgroup, the stepper lane's chunk, smoothed) of ad_tremolo_kernel_info."""
        v = [C.c_int() for _ in range(3)]
        check(lib().ad_tremolo_kernel_info(self._h, *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)


class RingModulator(_ModHandle):
    """modulation.RingModulator (ring_modulator.go:63-178):
    NewRingModulator(sample_rate, options...) with the options as keywords
    (carrier_hz, mix), or `config` (a RingModConfig) applied whole."""

    P_SAMPLE_RATE, P_CARRIER, P_MIX = range(3)  # AD_RINGMOD_*
    _kind = "ringmod"
    _config = RingModConfig
    _options = ("carrier_hz", "mix")

    def SetCarrierHz(self, v):  # :115-124
        self._set(self.P_CARRIER, v)

    def CarrierHz(self) -> float:  # :171
        return self.config().carrier_hz

    def kernel_info(self):
        """(samples of a row per apply workgroup, table threads, phaseInc) of ad_ringmod_kernel_info."""
        a, b, inc = C.c_int(), C.c_int(), C.c_double()
        check(lib().ad_ringmod_kernel_info(self._h, C.byref(a), C.byref(b), C.byref(inc)))
        return a.value, b.value, inc.value


class _ShaperHandle(_Handle):
    """What Distortion and BitCrusher share: a config structure, options as
    keywords, set_param with the int parameters as whole numbers."""

    _config = None
    _options = ()
    _int_options = ()

    def __init__(self, sample_rate: float = 48000.0, channels: int = 1, device: int = DEVICE, config=None, **options):
        self.channels = int(channels)
        self._h = C.c_void_p()
        cfg = self._config()
        if config is None:
            self._fn("default_config")(C.byref(cfg), float(sample_rate))
        else:
            C.memmove(C.byref(cfg), C.byref(config), C.sizeof(cfg))
        for k, v in options.items():
            if k == "cheb_weights":
                w = [float(x) for x in v]
                if len(w) > 16:
                    raise TypeError("at most 16 chebyshev weights")
                cfg.cheb_weights = (C.c_double * 16)(*w)
            elif k in self._int_options:
                setattr(cfg, k, int(v))
            elif k in self._options:
                setattr(cfg, k, float(v))
            else:
                raise TypeError(f"unknown {self._kind} option {k!r}")
        check(self._fn("create")(C.byref(cfg), self.channels, int(device), C.byref(self._h)))

    def _set(self, which: int, v):
        check(self._fn("set_param")(self._h, which, float(v)))

    def config(self):
        cfg = self._config()
        check(self._fn("get_config")(self._h, C.byref(cfg)))
        return cfg

    def SetSampleRate(self, v):
        self._set(0, v)

    def SetMix(self, v):
        self._set(self.P_MIX, v)

    def SampleRate(self) -> float:
        return self.config().sample_rate

    def Mix(self) -> float:
        return self.config().mix


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
    _config = DistortionConfig
    _options = ("drive", "mix", "output_level", "clip_level", "shape", "bias", "cheb_gain")
    _int_options = ("mode", "approx", "cheb_order", "cheb_harmonic", "cheb_invert", "cheb_dc_bypass")

    def SetMode(self, v):  # :376-384
        self._set(self.P_MODE, v)

    def SetApproxMode(self, v):  # :387-395
        self._set(self.P_APPROX, v)

    def SetDrive(self, v):  # :398-406
        self._set(self.P_DRIVE, v)

    def SetOutputLevel(self, v):  # :420-429
        self._set(self.P_OUTPUT_LEVEL, v)

    def SetClipLevel(self, v):  # :432-441
        self._set(self.P_CLIP_LEVEL, v)

    def SetShape(self, v):  # :444-452
        self._set(self.P_SHAPE, v)

    def SetBias(self, v):  # :455-463
        self._set(self.P_BIAS, v)

    def SetChebyshevOrder(self, v):  # :466-474
        self._set(self.P_CHEB_ORDER, v)

    def SetChebyshevHarmonicMode(self, v):  # :477-485
        self._set(self.P_CHEB_HARMONIC, v)

    def SetChebyshevInvert(self, on: bool):  # :488-490
        self._set(self.P_CHEB_INVERT, 1 if on else 0)

    def SetChebyshevGainLevel(self, v):  # :493-502
        self._set(self.P_CHEB_GAIN, v)

    def SetChebyshevDCBypass(self, on: bool):  # :505-507
        self._set(self.P_CHEB_DC_BYPASS, 1 if on else 0)

    def SetChebyshevWeights(self, weights):  # :514-529
        w = f64(weights).reshape(-1)
        check(lib().ad_distortion_set_weights(self._h, ptr(w), int(w.size)))

    def Mode(self) -> int:  # :567-588
        return self.config().mode

    def Drive(self) -> float:
        return self.config().drive

    def OutputLevel(self) -> float:
        return self.config().output_level

    def ClipLevel(self) -> float:
        return self.config().clip_level

    def Shape(self) -> float:
        return self.config().shape

    def Bias(self) -> float:
        return self.config().bias

    def ChebyshevOrder(self) -> int:
        return self.config().cheb_order

    def derived(self):
        """dict(atan_scale=atan(1 + 4 shape), scale6=1 + 6 shape, scale2=1 + 2 shape, one_minus_mix,
        weights_active) of ad_distortion_derived: the constants the host computes for the kernels."""
        v = [C.c_double() for _ in range(4)]
        w = C.c_int()
        check(lib().ad_distortion_derived(self._h, *[C.byref(x) for x in v], C.byref(w)))
        return dict(atan_scale=v[0].value, scale6=v[1].value, scale2=v[2].value, one_minus_mix=v[3].value,
                    weights_active=bool(w.value))

    def kernel_info(self):
        """(samples of a row per pointwise workgroup; channels per workgroup, samples staged per chunk and
        lds_bytes of the DC-bypass kernel) of ad_distortion_kernel_info."""
        v = [C.c_int() for _ in range(4)]
        check(lib().ad_distortion_kernel_info(self._h, *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)

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
    _config = BitCrusherConfig
    _options = ("bit_depth", "mix")
    _int_options = ("downsample",)

    def SetBitDepth(self, v):  # :149-160
        self._set(self.P_BIT_DEPTH, v)

    def SetDownsample(self, v):  # :163-172
        self._set(self.P_DOWNSAMPLE, v)

    def BitDepth(self) -> float:  # :214-220
        return self.config().bit_depth

    def Downsample(self) -> int:
        return self.config().downsample

    def derived(self, channel: int = 0):
        """dict(quant_levels, counter, hold_value) of ad_bitcrusher_derived: quantLevels = exp2(bitDepth - 1)
        as the host computed it, holdCounter, and holdValue of `channel`."""
        q, c, h = C.c_double(), C.c_int(), C.c_double()
        check(lib().ad_bitcrusher_derived(self._h, int(channel), C.byref(q), C.byref(c), C.byref(h)))
        return dict(quant_levels=q.value, counter=c.value, hold_value=h.value)

    def kernel_info(self):
        """(samples of a row per workgroup, the staged span of whole hold periods, lds_bytes) of
        ad_bitcrusher_kernel_info."""
        v = [C.c_int() for _ in range(3)]
        check(lib().ad_bitcrusher_kernel_info(self._h, *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)


class _DynHandle(_Handle):
    """What TransientShaper and DeEsser share: a config structure, options as
    keywords, set_param with the int parameters as whole numbers, and the
    host-only derived values of a config."""

    _config = None
    _options = ()
    _int_options = ()

    def __init__(self, sample_rate: float = 48000.0, channels: int = 1, device: int = DEVICE, config=None, **options):
        self.channels = int(channels)
        self._h = C.c_void_p()
        cfg = self._config()
        if config is None:
            self._fn("default_config")(C.byref(cfg), float(sample_rate))
        else:
            C.memmove(C.byref(cfg), C.byref(config), C.sizeof(cfg))
        for k, v in options.items():
            if k in self._int_options:
                setattr(cfg, k, int(v))
            elif k in self._options:
                setattr(cfg, k, float(v))
            else:
                raise TypeError(f"unknown {self._kind} option {k!r}")
        check(self._fn("create")(C.byref(cfg), self.channels, int(device), C.byref(self._h)))

    def _set(self, which: int, v):
        check(self._fn("set_param")(self._h, which, float(v)))

    def config(self):
        cfg = self._config()
        check(self._fn("get_config")(self._h, C.byref(cfg)))
        return cfg

    def SetSampleRate(self, v):
        self._set(0, v)

    def SetAttack(self, v):
        self._set(self.P_ATTACK, v)

    def SetRelease(self, v):
        self._set(self.P_RELEASE, v)

    def SetAttackCoeff(self, v):  # attackCoeff, for a caller whose exp is not the C library's
        self._set(self.P_ATTACK_COEFF, v)

    def SetReleaseCoeff(self, v):
        self._set(self.P_RELEASE_COEFF, v)

    def SampleRate(self) -> float:
        return self.config().sample_rate

    def Attack(self) -> float:
        return self.config().attack_ms

    def Release(self) -> float:
        return self.config().release_ms


def transient_derived(cfg: TransientConfig):
    """(attack_coeff, release_coeff) in use for a config, of ad_transient_derived: host only."""
    a, r = C.c_double(), C.c_double()
    check(lib().ad_transient_derived(C.byref(cfg), C.byref(a), C.byref(r)))
    return a.value, r.value


def deesser_derived(cfg: DeEsserConfig) -> dict:
    """dict(section=(b0, b1, b2, a1, a2), band_norm, threshold_log2, knee_width_log2, range_lin, attack_coeff,
    release_coeff) for a config, of ad_deesser_derived: what the reference caches, host only."""
    sec = (C.c_double * 5)()
    v = [C.c_double() for _ in range(6)]
    check(lib().ad_deesser_derived(C.byref(cfg), sec, *[C.byref(x) for x in v]))
    return dict(section=tuple(sec), band_norm=v[0].value, threshold_log2=v[1].value, knee_width_log2=v[2].value,
                range_lin=v[3].value, attack_coeff=v[4].value, release_coeff=v[5].value)


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
    _config = TransientConfig
    _options = ("attack_amount", "sustain_amount", "attack_ms", "release_ms", "attack_coeff", "release_coeff")

    def SetAttackAmount(self, v):  # :57-66
        self._set(self.P_ATTACK_AMOUNT, v)

    def SetSustainAmount(self, v):  # :69-78
        self._set(self.P_SUSTAIN_AMOUNT, v)

    def AttackAmount(self) -> float:  # :120-132
        return self.config().attack_amount

    def SustainAmount(self) -> float:
        return self.config().sustain_amount

    def derived(self):
        return transient_derived(self.config())

    def kernel_info(self):
        """(channels per workgroup, samples staged per chunk, lds_bytes) of the walk, of ad_transient_kernel_info."""
        v = [C.c_int() for _ in range(3)]
        check(lib().ad_transient_kernel_info(self._h, *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def get_state(self, channel: int = 0) -> float:
        """The envelope of `channel`."""
        e = C.c_double()
        check(lib().ad_transient_get_state(self._h, int(channel), C.byref(e)))
        return e.value

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
    _config = DeEsserConfig
    _options = ("freq_hz", "q", "threshold_db", "ratio", "knee_db", "attack_ms", "release_ms", "range_db",
                "attack_coeff", "release_coeff")
    _int_options = ("mode", "detector", "listen", "filter_order")

    def SetFrequency(self, v):  # :228-244
        self._set(self.P_FREQ, v)

    def SetQ(self, v):  # :248-259
        self._set(self.P_Q, v)

    def SetThreshold(self, v):  # :263-272
        self._set(self.P_THRESHOLD, v)

    def SetRatio(self, v):  # :276-287
        self._set(self.P_RATIO, v)

    def SetKnee(self, v):  # :291-302
        self._set(self.P_KNEE, v)

    def SetRange(self, v):  # :336-347
        self._set(self.P_RANGE, v)

    def SetMode(self, v):  # :350-358
        self._set(self.P_MODE, v)

    def SetDetector(self, v):  # :361-370
        self._set(self.P_DETECTOR, v)

    def SetListen(self, on: bool):  # :375-377
        self._set(self.P_LISTEN, 1 if on else 0)

    def SetFilterOrder(self, v):  # :381-391
        self._set(self.P_FILTER_ORDER, v)

    def Frequency(self) -> float:  # :186-222
        return self.config().freq_hz

    def Q(self) -> float:
        return self.config().q

    def Threshold(self) -> float:
        return self.config().threshold_db

    def Ratio(self) -> float:
        return self.config().ratio

    def Knee(self) -> float:
        return self.config().knee_db

    def Range(self) -> float:
        return self.config().range_db

    def Mode(self) -> int:
        return self.config().mode

    def Detector(self) -> int:
        return self.config().detector

    def Listen(self) -> bool:
        return bool(self.config().listen)

    def FilterOrder(self) -> int:
        return self.config().filter_order

    def GetMetrics(self, channel: int = 0):  # :499-501 -> (DetectionLevel, GainReduction)
        d, g = C.c_double(), C.c_double()
        check(lib().ad_deesser_metrics(self._h, int(channel), C.byref(d), C.byref(g)))
        return d.value, g.value

    def ResetMetrics(self):  # :504-506
        check(lib().ad_deesser_reset_metrics(self._h))

    def derived(self) -> dict:
        return deesser_derived(self.config())

    def kernel_info(self):
        """(channels per workgroup, samples staged per chunk, lds_bytes, cascades walked) of the walk the next
        call runs, of ad_deesser_kernel_info."""
        v = [C.c_int() for _ in range(4)]
        check(lib().ad_deesser_kernel_info(self._h, *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)

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


class Vocoder(_Handle):
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
    _options = ("synth_q", "attack_ms", "release_ms", "input_level", "synth_level", "vocoder_level")

    def __init__(self, sample_rate: float = 48000.0, channels: int = 1, device: int = DEVICE, config=None, **options):
        self.channels = int(channels)
        self._h = C.c_void_p()
        cfg = VocoderConfig()
        if config is None:
            lib().ad_vocoder_default_config(C.byref(cfg), float(sample_rate))
        else:
            C.memmove(C.byref(cfg), C.byref(config), C.sizeof(cfg))
        for k, v in options.items():
            if k == "layout":
                cfg.layout = int(v)
            elif k == "downsample":
                cfg.downsample = 1 if v else 0
            elif k in self._options:
                setattr(cfg, k, float(v))
                if k == "synth_q":
                    cfg.synth_q_set = 1
            else:
                raise TypeError(f"unknown vocoder option {k!r}")
        check(lib().ad_vocoder_create(C.byref(cfg), self.channels, int(device), C.byref(self._h)))

    def _set(self, which: int, v):
        check(lib().ad_vocoder_set_param(self._h, which, float(v)))

    def config(self) -> VocoderConfig:
        cfg = VocoderConfig()
        check(lib().ad_vocoder_get_config(self._h, C.byref(cfg)))
        return cfg

    def SetSampleRate(self, v):  # :673-683
        self._set(self.P_SAMPLE_RATE, v)

    def SetAttack(self, v):  # :772-783
        self._set(self.P_ATTACK, v)

    def SetRelease(self, v):  # :786-797
        self._set(self.P_RELEASE, v)

    def SetInputLevel(self, v):  # :800-809
        self._set(self.P_INPUT_LEVEL, v)

    def SetSynthLevel(self, v):  # :812-821
        self._set(self.P_SYNTH_LEVEL, v)

    def SetVocoderLevel(self, v):  # :824-833
        self._set(self.P_VOCODER_LEVEL, v)

    def SetDownsampling(self, on: bool):  # :737-769
        self._set(self.P_DOWNSAMPLING, 1 if on else 0)

    def SampleRate(self) -> float:  # :688-717
        return self.config().sample_rate

    def Layout(self) -> int:
        return self.config().layout

    def NumBands(self) -> int:
        n = C.c_int()
        check(lib().ad_vocoder_num_bands(self._h, C.byref(n)))
        return n.value

    def SynthesisQ(self) -> float:
        return self.config().synth_q

    def Attack(self) -> float:
        return self.config().attack_ms

    def Release(self) -> float:
        return self.config().release_ms

    def InputLevel(self) -> float:
        return self.config().input_level

    def SynthLevel(self) -> float:
        return self.config().synth_level

    def VocoderLevel(self) -> float:
        return self.config().vocoder_level

    def Downsampling(self) -> bool:
        return bool(self.config().downsample)

    def DownsampleFactors(self):  # :722-731: None with downsampling off
        f, n = (C.c_int * 32)(), C.c_int()
        check(lib().ad_vocoder_downsample_factors(self._h, f, 32, C.byref(n)))
        return list(f[:n.value]) if n.value else None

    def derived(self) -> dict:
        return vocoder_derived(self.config())

    def kernel_info(self):
        """(lanes per channel, samples per chunk, lds_bytes of a workgroup) of ad_vocoder_kernel_info."""
        v = [C.c_int() for _ in range(3)]
        check(lib().ad_vocoder_kernel_info(self._h, *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def get_state(self, channel: int = 0):
        """(state [9][32], downsampleCount) of `channel`: rows {analysis s0, s1, synthesis s0, s1, decimated s0,
        s1, envelope} by band, then the anti-alias {s0, s1} by group."""
        st, cnt = np.zeros((9, 32)), C.c_int()
        check(lib().ad_vocoder_get_state(self._h, int(channel), ptr(st), C.byref(cnt)))
        return st, cnt.value

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
        check(lib().ad_vocoder_process_device(self._h, C.c_void_p(d_mod), int(mod_stride), C.c_void_p(d_car),
                                              int(car_stride), C.c_void_p(d_out), int(out_stride), int(n),
                                              C.c_void_p(stream or 0)))


def lookahead_derived(cfg: LookaheadConfig) -> dict:
    """dict(attack_coeff, release_coeff, threshold_log2, delay_samples) for a config, of ad_lookahead_derived:
    what the limiter's Compressor core caches and the delay D, host only."""
    a, r, th, d = C.c_double(), C.c_double(), C.c_double(), C.c_int64()
    check(lib().ad_lookahead_derived(C.byref(cfg), C.byref(a), C.byref(r), C.byref(th), C.byref(d)))
    return dict(attack_coeff=a.value, release_coeff=r.value, threshold_log2=th.value, delay_samples=d.value)


class LookaheadLimiter(_Handle):
    """dynamics.LookaheadLimiter (lookahead_limiter.go:23-239) for `channels`
    instances sharing one configuration: NewLookaheadLimiter(sample_rate) with
    options as keywords (threshold_db, release_ms, lookahead_ms), or `config`
    (a LookaheadConfig) applied whole.  A rejected setter value raises
    ErrInvalidArgument and changes nothing."""

    P_SAMPLE_RATE, P_THRESHOLD, P_RELEASE, P_LOOKAHEAD = range(4)  # AD_LOOKAHEAD_*
    _kind = "lookahead"
    _options = ("threshold_db", "release_ms", "lookahead_ms")

    def __init__(self, sample_rate: float = 48000.0, channels: int = 1, device: int = DEVICE, config=None, **options):
        self.channels = int(channels)
        self._h = C.c_void_p()
        cfg = LookaheadConfig()
        if config is None:
            lib().ad_lookahead_default_config(C.byref(cfg), float(sample_rate))
        else:
            C.memmove(C.byref(cfg), C.byref(config), C.sizeof(cfg))
        for k, v in options.items():
            if k not in self._options:
                raise TypeError(f"unknown lookahead limiter option {k!r}")
            setattr(cfg, k, float(v))
        check(lib().ad_lookahead_create(C.byref(cfg), self.channels, int(device), C.byref(self._h)))

    def _set(self, which: int, v):
        check(lib().ad_lookahead_set_param(self._h, which, float(v)))

    def config(self) -> LookaheadConfig:
        cfg = LookaheadConfig()
        check(lib().ad_lookahead_get_config(self._h, C.byref(cfg)))
        return cfg

    def SetSampleRate(self, v):  # :146-161
        self._set(self.P_SAMPLE_RATE, v)

    def SetThreshold(self, v):  # :99-113
        self._set(self.P_THRESHOLD, v)

    def SetRelease(self, v):  # :116-130
        self._set(self.P_RELEASE, v)

    def SetLookahead(self, v):  # :133-143
        self._set(self.P_LOOKAHEAD, v)

    def SampleRate(self) -> float:  # :164-173
        return self.config().sample_rate

    def Threshold(self) -> float:
        return self.config().threshold_db

    def Release(self) -> float:
        return self.config().release_ms

    def Lookahead(self) -> float:
        return self.config().lookahead_ms

    def derived(self) -> dict:
        return lookahead_derived(self.config())

    def DelaySamples(self) -> int:
        return self.derived()["delay_samples"]

    def get_state(self, channel: int = 0) -> float:
        """The detector envelope of `channel`."""
        e = C.c_double()
        check(lib().ad_lookahead_get_state(self._h, int(channel), C.byref(e)))
        return e.value

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
        check(lib().ad_lookahead_process_device(self._h, C.c_void_p(d_buf), int(stride), C.c_void_p(d_side or None),
                                                int(side_stride), int(side_n), int(n), C.c_void_p(stream or 0)))


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
        self.channels = int(channels)
        self._h = C.c_void_p()
        f, fp, nf = _freq_args(freqs)
        check(lib().ad_xover_create(fp, nf, int(order), float(sample_rate), self.channels, int(device),
                                    C.byref(self._h)))
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
        check(lib().ad_xover_process_device(self._h, C.c_void_p(d_in), int(in_stride), C.c_void_p(d_bands),
                                            int(row_stride), int(band_stride), int(n), C.c_void_p(stream or 0)))

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
        v = [C.c_int() for _ in range(3)]
        check(lib().ad_xover_kernel_info(self._h, *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)

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
    keeps the default."""

    _kind = "multiband"

    def __init__(self, freqs, order: int, sample_rate: float = 48000.0, channels: int = 1, device: int = DEVICE,
                 configs=None):
        self.channels = int(channels)
        self._h = C.c_void_p()
        f, fp, nf = _freq_args(freqs)
        if configs is not None and len(configs) != nf + 1:  # :131-135
            raise ErrInvalidArgument(AD_ERR_INVALID_ARGUMENT, f"expected {nf + 1} band configs, got {len(configs)}")
        check(lib().ad_multiband_create(fp, nf, int(order), float(sample_rate), self.channels, int(device),
                                        C.byref(self._h)))
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

    # per-band setters :190-329
    def SetBandThreshold(self, band, db):
        self._set(band, threshold_db=float(db))

    def SetBandRatio(self, band, ratio):
        self._set(band, ratio=float(ratio))

    def SetBandKnee(self, band, db):
        self._set(band, knee_db=float(db))

    def SetBandAttack(self, band, ms):
        self._set(band, attack_ms=float(ms))

    def SetBandRelease(self, band, ms):
        self._set(band, release_ms=float(ms))

    def SetBandMakeupGain(self, band, db):  # :242-249: turns auto makeup off
        self._set(band, makeup_db=float(db), auto_makeup=0)

    def SetBandAutoMakeup(self, band, on):
        self._set(band, auto_makeup=int(bool(on)))

    def SetBandTopology(self, band, topology):
        self._set(band, topology=int(topology))

    def SetBandDetectorMode(self, band, mode):
        self._set(band, detector_mode=int(mode))

    def SetBandFeedbackRatioScale(self, band, on):
        self._set(band, feedback_ratio_scale=int(bool(on)))

    def SetBandRMSWindow(self, band, ms):
        self._set(band, rms_window_ms=float(ms))

    def SetBandSidechainLowCut(self, band, hz):
        self._set(band, sidechain_low_cut_hz=float(hz))

    def SetBandSidechainHighCut(self, band, hz):
        self._set(band, sidechain_high_cut_hz=float(hz))

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

    def SetAllBandsThreshold(self, db):
        self._all("SetBandThreshold", db)

    def SetAllBandsRatio(self, ratio):
        self._all("SetBandRatio", ratio)

    def SetAllBandsKnee(self, db):
        self._all("SetBandKnee", db)

    def SetAllBandsAttack(self, ms):
        self._all("SetBandAttack", ms)

    def SetAllBandsRelease(self, ms):
        self._all("SetBandRelease", ms)

    def SetAllBandsTopology(self, topology):
        self._all("SetBandTopology", topology)

    def SetAllBandsDetectorMode(self, mode):
        self._all("SetBandDetectorMode", mode)

    def SetAllBandsFeedbackRatioScale(self, on):
        self._all("SetBandFeedbackRatioScale", on)

    def SetAllBandsRMSWindow(self, ms):
        self._all("SetBandRMSWindow", ms)

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
        out = []
        for b in range(self.NumBands()):
            v = [C.c_double() for _ in range(3)]
            check(lib().ad_multiband_metrics(self._h, b, int(channel), *[C.byref(x) for x in v]))
            out.append(tuple(x.value for x in v))
        return out

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


class _StftHandle(_Handle):
    """What SpectralFreeze and SpectralPitchShifter share: the frame size and
    the window, whose table this layer computes, and the Process forms."""

    _config = None

    def _set(self, which: int, v):
        check(self._fn("set_param")(self._h, which, float(v)))

    def config(self):
        cfg = self._config()
        check(self._fn("get_config")(self._h, C.byref(cfg)))
        return cfg

    def SetSampleRate(self, v):
        self._set(0, v)

    def SetFrameSize(self, size: int):
        size = int(size)
        if size < 64 or size & (size - 1):  # the table needs a valid size; the library repeats the check
            raise ErrInvalidArgument(AD_ERR_INVALID_ARGUMENT, f"frame size must be power-of-two and >= 64: {size}")
        w = spectral_window(self.WindowType(), size)
        check(self._fn("set_frame")(self._h, size, ptr(w)))

    def SetWindowType(self, window_type: int):
        w = spectral_window(window_type, self.FrameSize())
        check(self._fn("set_window")(self._h, int(window_type), ptr(w)))

    def SampleRate(self) -> float:
        return self.config().sample_rate

    def FrameSize(self) -> int:
        return self.config().frame_size

    def WindowType(self) -> int:
        return self.config().window_type

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
    _config = SpecFreezeConfig

    def __init__(self, sample_rate: float = 48000.0, channels: int = 1, device: int = DEVICE, **options):
        self.channels = int(channels)
        self._h = C.c_void_p()
        cfg = SpecFreezeConfig()
        lib().ad_specfreeze_default_config(C.byref(cfg), float(sample_rate))
        for k, v in options.items():
            if k in ("frame_size", "hop_size", "phase_mode", "frozen", "window_type"):
                setattr(cfg, k, int(v))
            elif k == "mix":
                cfg.mix = float(v)
            else:
                raise TypeError(f"unknown spectral freeze option {k!r}")
        w = spectral_window(cfg.window_type, max(cfg.frame_size, 0))
        cfg.window = ptr(w)
        check(lib().ad_specfreeze_create(C.byref(cfg), self.channels, int(device), C.byref(self._h)))

    def SetHopSize(self, hop: int):
        self._set(self.P_HOP, hop)

    def SetMix(self, mix: float):
        self._set(self.P_MIX, mix)

    def SetPhaseMode(self, mode: int):
        self._set(self.P_PHASE_MODE, mode)

    def SetFrozen(self, frozen: bool):
        self._set(self.P_FROZEN, 1 if frozen else 0)

    def Freeze(self):
        self.SetFrozen(True)

    def Unfreeze(self):
        self.SetFrozen(False)

    def HopSize(self) -> int:
        return self.config().hop_size

    def Mix(self) -> float:
        return self.config().mix

    def PhaseMode(self) -> int:
        return self.config().phase_mode

    def Frozen(self) -> bool:
        return bool(self.config().frozen)

    def state(self):
        """(heldMagnitude [channels][N/2+1], phaseAcc [channels][N/2+1], hasFrozenFrame) of ad_specfreeze_state."""
        bins = self.FrameSize() // 2 + 1
        held, acc = np.zeros((self.channels, bins)), np.zeros((self.channels, bins))
        has = C.c_int()
        check(lib().ad_specfreeze_state(self._h, ptr(held), ptr(acc), C.byref(has)))
        return held, acc, bool(has.value)

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
    _config = PitchSpecConfig

    def __init__(self, sample_rate: float = 48000.0, channels: int = 1, device: int = DEVICE, **options):
        self.channels = int(channels)
        self._h = C.c_void_p()
        cfg = PitchSpecConfig()
        lib().ad_pitchspec_default_config(C.byref(cfg), float(sample_rate))
        for k, v in options.items():
            if k in ("frame_size", "analysis_hop", "window_type", "resample_quality"):
                setattr(cfg, k, int(v))
            elif k == "pitch_ratio":
                cfg.pitch_ratio = float(v)
            else:
                raise TypeError(f"unknown spectral pitch shifter option {k!r}")
        w = spectral_window(cfg.window_type, max(cfg.frame_size, 0))
        cfg.window = ptr(w)
        check(lib().ad_pitchspec_create(C.byref(cfg), self.channels, int(device), C.byref(self._h)))
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

    def SetPitchRatio(self, ratio: float):
        self._set(self.P_RATIO, ratio)

    def SetPitchSemitones(self, semitones: float):  # :164-177
        s = float(semitones)
        if not np.isfinite(s):
            raise ErrInvalidArgument(AD_ERR_INVALID_ARGUMENT, f"spectral pitch shifter semitones must be finite: {s}")
        self.SetPitchRatio(2.0 ** (s / 12.0))

    def SetAnalysisHop(self, hop: int):
        self._set(self.P_HOP, hop)

    def SetResampleQuality(self, q: int):
        self._set(self.P_RESAMPLE_QUALITY, q)

    def PitchRatio(self) -> float:
        return self.config().pitch_ratio

    def PitchSemitones(self) -> float:  # :103
        return 12.0 * float(np.log2(self.PitchRatio()))

    def AnalysisHop(self) -> int:
        return self.config().analysis_hop

    def ResampleQuality(self) -> int:
        return self.config().resample_quality

    def EffectivePitchRatio(self) -> float:
        r = C.c_double()
        check(lib().ad_pitchspec_effective_ratio(self._h, C.byref(r)))
        return r.value

    def SynthesisHop(self) -> int:
        h = C.c_int()
        check(lib().ad_pitchspec_synthesis_hop(self._h, C.byref(h)))
        return h.value

    def path(self) -> int:
        """0: the identity shortcut, 1: bin shifting, 2: time stretch (ad_pitchspec_path)."""
        v = C.c_int()
        check(lib().ad_pitchspec_path(self._h, C.byref(v)))
        return v.value


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


class Filter:
    """fir.Filter (filter.go:11-172) for `channels` lanes sharing the taps."""

    def __init__(self, coeffs, channels: int = 1, device: int = DEVICE):
        self.coeffs = f64(coeffs).ravel()
        self.channels = int(channels)
        self._h = C.c_void_p()
        check(lib().ad_fir_create(ptr(self.coeffs), self.coeffs.size, self.channels, int(device),
                                  C.byref(self._h)))

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
        check(lib().ad_fir_process_device(self._h, C.c_void_p(d_src), int(src_stride), C.c_void_p(d_dst),
                                          int(dst_stride), int(n), C.c_void_p(stream or 0)))

    def Reset(self):
        check(lib().ad_fir_reset(self._h))

    def close(self):
        if self._h:
            lib().ad_fir_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


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
