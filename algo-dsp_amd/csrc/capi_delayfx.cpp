// C ABI of the feedback delay (dsp/effects/delay.go), the graph's delay-simple
// (dsp/effectchain/runtime_modulation.go:322-362) and the flanger
// (dsp/effects/modulation/flanger.go).  A handle keeps the reference's
// configuration, the write position and the delay-time ramp on the host, in
// plain IEEE double as the setters and ProcessSample compute them, and every
// channel's ring (and the flanger's LFO phase) on the device.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <utility>
#include <vector>

#include "delayfx_kernels.hpp"
#include "fx_handle.hpp"

using namespace adsp;

namespace {

constexpr double kDefaultTime = 0.25, kDefaultFeedback = 0.35, kDefaultMix = 0.25;  // delay.go:9-11
constexpr double kMaxTime = 2.0, kMinTime = 0.001, kSmoothSeconds = 0.010;          // :12-19
constexpr double kMinFlangerDelay = 0.0001, kMaxFlangerDelay = 0.0100;              // flanger.go:15-16
// The reference allocates whatever a sample rate asks for; a ring is bounded
// here so that every length and index fits an int.
constexpr double kMaxRing = 134217728.0;  // 2^27 samples
// A call whose hazard-free block is at least this long runs as one launch per
// block (regime 1); below it a persistent workgroup walks the call (regime 2).
// From the sweep in profiles/delayfx_bench.json (48 kHz): at 256 channels the
// two regimes meet at a block of 191 (18.2 against 18.7 ms per 2^20 samples)
// and regime 1 is 1.7x as fast at 383; at 4096 channels regime 2 still leads
// by 6 % at 383 and regime 1 by 22 % at 767.  256 costs the many-channel case
// less than the 22 % it measured at 191; 512 would cost the other one 1.7x.
constexpr int kDelayCrossover = 256;

const double kTwoPi = 2.0 * M_PI;

double smooth_coeff(double fs) { return 1 - std::exp(-1 / (fs * kSmoothSeconds)); }  // computeSmoothCoeff :255-257

void validate_time(double v) {  // validateTime :191-199
  if (!(v >= kMinTime && v <= kMaxTime)) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "delay time must be in [0.001, 2]");
}
void validate_delay_rate(double v) {
  if (!(v > 0) || !is_finite(v)) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "delay sample rate must be > 0");
  if (!(std::ceil(kMaxTime * v) + 1 <= kMaxRing)) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "delay: a ring longer than 2^27 samples");
}
void validate_feedback(double v) {  // SetFeedback :109-117
  if (!(v >= 0 && v <= 0.99)) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "delay feedback must be in [0, 0.99]");
}
void validate_mix(double v, const char* what) {  // SetMix :120-128, flanger.go:238-246
  if (!(v >= 0 && v <= 1)) AD_FAIL(AD_ERR_INVALID_ARGUMENT, what);
}

void validate(const ad_delay_config& c) {
  if (c.mode == 1) {
    if (c.delay_samples < 0 || (double)c.delay_samples > kMaxRing)
      AD_FAIL(AD_ERR_INVALID_ARGUMENT, "delay-simple: delay must be in [0, 2^27] samples");
    return;
  }
  if (c.mode != 0) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "delay mode must be 0 (Delay) or 1 (delay-simple)");
  validate_delay_rate(c.sample_rate);
  validate_time(c.time_seconds);
  validate_feedback(c.feedback);
  validate_mix(c.mix, "delay mix must be in [0, 1]");
  if (!(c.smooth_coeff == 0 || (c.smooth_coeff > 0 && c.smooth_coeff <= 1)))
    AD_FAIL(AD_ERR_INVALID_ARGUMENT, "delay smoothing coefficient must be 0 (derive it) or in (0, 1]");
}

int flanger_needed(const ad_flanger_config& c) {  // reconfigureDelayLine :358
  return std::max((int)std::ceil((c.base_delay_seconds + c.depth_seconds) * c.sample_rate) + 3, 4);
}

void validate(const ad_flanger_config& c) {  // validateParams :317-350
  if (!(c.sample_rate > 0) || !is_finite(c.sample_rate))
    AD_FAIL(AD_ERR_INVALID_ARGUMENT, "flanger sample rate must be > 0 and finite");
  if (!(c.rate_hz > 0) || !is_finite(c.rate_hz)) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "flanger rate must be > 0 and finite");
  if (!(c.depth_seconds >= 0) || !is_finite(c.depth_seconds))
    AD_FAIL(AD_ERR_INVALID_ARGUMENT, "flanger depth must be >= 0 and finite");
  if (!(c.base_delay_seconds >= kMinFlangerDelay && c.base_delay_seconds <= kMaxFlangerDelay))
    AD_FAIL(AD_ERR_INVALID_ARGUMENT, "flanger base delay must be in [0.0001, 0.01]");
  if (c.base_delay_seconds + c.depth_seconds > kMaxFlangerDelay)
    AD_FAIL(AD_ERR_INVALID_ARGUMENT, "flanger max delay exceeds 0.01 seconds");
  if (!(c.feedback >= -0.99 && c.feedback <= 0.99))
    AD_FAIL(AD_ERR_INVALID_ARGUMENT, "flanger feedback must be in [-0.99, 0.99]");
  validate_mix(c.mix, "flanger mix must be in [0, 1]");
  // the reference allocates any length; here a channel's ring has to fit the kernel's share of LDS
  const double need = std::ceil((c.base_delay_seconds + c.depth_seconds) * c.sample_rate) + 3;
  if (!((need + 31) * sizeof(double) <= kFlangerRingLdsBytes))
    AD_FAIL(AD_ERR_INVALID_ARGUMENT, "flanger: a delay line longer than the kernel's LDS share (4065 samples)");
}

// a zeroed [channels][new_len] ring holding the newest min(old, new) samples of `ring`, write position 0
void resize_ring(DevBuf<double>& ring, int channels, int old_len, int old_wp, int new_len, hipStream_t s) {
  DevBuf<double> fresh;
  fresh.alloc((size_t)channels * new_len);
  AD_HIP(hipMemsetAsync(fresh.p, 0, fresh.n * sizeof(double), s));
  if (ring.p) {
    launch_ring_resize(ring.p, old_len, old_wp, fresh.p, new_len, std::min(old_len, new_len), channels, s);
    AD_HIP(hipGetLastError());
  }
  AD_HIP(hipStreamSynchronize(s));
  std::swap(ring.p, fresh.p);
  std::swap(ring.n, fresh.n);
}

}  // namespace

struct ad_delay : HandleCore {
  ad_delay_config cfg{};             // time_seconds: delaySeconds; smooth_coeff: the coefficient in use
  double target = 0, current = 0;    // targetSamples, currentSamples
  int len = 0, wp = 0;               // ring length (mode 1: D slots), write position of every channel
  DevBuf<double> ring;               // [channels][len]
  PinnedUpload traj;                 // the call's ramp
  int force_regime = 0, last_regime = 0, last_launches = 0;
};

struct ad_flanger : HandleCore {
  ad_flanger_config cfg{};
  int len = 0, wp = 0;
  DevBuf<double> ring;   // [channels][len]
  DevBuf<double> phase;  // [2]: lfoPhase, ping-pong (cur = phase[ph_cur])
  int ph_cur = 0;
};

namespace {

// ---- delay ------------------------------------------------------------------
double snapped(const ad_delay* f) {  // reconfigureBuffer :209-215, :244-250
  const double samples = std::round(f->cfg.time_seconds * f->cfg.sample_rate);
  return samples < 1 ? 1 : samples;
}

// reconfigureBuffer (:201-253) for f->cfg.sample_rate
void reconfigure_buffer(ad_delay* f) {
  const int want = (int)std::ceil(kMaxTime * f->cfg.sample_rate) + 1;
  if (want != f->len || !f->ring.p) {
    f->order.wait_host();
    resize_ring(f->ring, f->channels, f->len, f->wp, want, f->stream);
    f->len = want;
    f->wp = 0;
  }
  f->target = f->current = snapped(f);
}

// The blocks a call may use: `raw` consecutive samples read none of each
// other's writes, `both` of them also overwrite nothing another still reads.
struct Blocks {
  int raw, both;
};
Blocks blocks_of(const ad_delay* f) {
  if (f->cfg.mode == 1) return {f->len, f->len};
  const double lo = std::min(f->current, f->target), hi = std::max(f->current, f->target);
  const int raw = std::max(1, (int)std::floor(lo) - 1);
  const int war = std::max(1, f->len - (int)std::ceil(hi));
  return {raw, std::min(raw, war)};
}

void delay_run(ad_delay* f, double* d_buf, int64_t stride, int64_t n, hipStream_t s) {
#pragma clang fp contract(off)
  if (f->cfg.mode == 1 && f->cfg.delay_samples == 0) return;  // Process returns at once (:347-349)
  CallScope call(f->order, s);
  const Blocks b = blocks_of(f);  // before the ramp moves `current`
  // the ramp (:142), one rounded subtraction, product and sum per sample, up to its fixed point
  std::vector<double> ramp;
  double c = f->current;
  if (f->cfg.mode == 0 && c != f->target) {
    const double k = f->cfg.smooth_coeff;
    while ((int64_t)ramp.size() < n) {
      const double nc = c + (f->target - c) * k;
      if (nc == c) break;  // the same inputs give the same sum for ever
      c = nc;
      ramp.push_back(c);
    }
  }
  if (!ramp.empty()) {
    std::memcpy(f->traj.stage(ramp.size()), ramp.data(), ramp.size() * sizeof(double));
    f->traj.send(ramp.size(), s);
  }
  DelayArgs a{};
  a.buf = d_buf;
  a.stride = stride;
  a.n = n;
  a.ring = f->ring.p;
  a.len = f->len;
  a.wp = f->wp;
  a.traj = f->traj.dev.p;
  a.ntraj = (int64_t)ramp.size();
  a.c_rest = c;
  a.feedback = f->cfg.feedback;
  a.mix = f->cfg.mix;
  a.one_minus_mix = 1 - f->cfg.mix;
  a.pure = f->cfg.mode == 1;
  a.channels = f->channels;
  const int regime = f->force_regime ? f->force_regime : (b.both >= kDelayCrossover || n <= b.both ? 1 : 2);
  int launches = 0;
  if (regime == 1) {
    for (int64_t t0 = 0; t0 < n; t0 += b.both, ++launches)
      launch_delay_tile(a, t0, (int)std::min<int64_t>(b.both, n - t0), s);
  } else {
    launch_delay_walk(a, pow2_sub(b.raw), s);
    launches = 1;
  }
  AD_HIP(hipGetLastError());
  f->wp = (int)((f->wp + n) % f->len);
  f->current = c;
  f->last_regime = regime;
  f->last_launches = launches;
}

// ---- flanger ----------------------------------------------------------------
int flanger_block(const ad_flanger* f) {  // max(1, P - 1), P = floor(max(1, base * fs))
  const double p = std::floor(std::max(1.0, f->cfg.base_delay_seconds * f->cfg.sample_rate));
  return std::max(1, (int)std::min(p, 1e6) - 1);
}

// reconfigureDelayLine (:352-390) for f->cfg
void reconfigure_line(ad_flanger* f) {
  const int want = flanger_needed(f->cfg);
  if (want == f->len && f->ring.p) return;
  f->order.wait_host();
  resize_ring(f->ring, f->channels, f->len, f->wp, want, f->stream);
  f->len = want;
  f->wp = 0;
}

void flanger_run(ad_flanger* f, double* d_buf, int64_t stride, int64_t n, hipStream_t s) {
  CallScope call(f->order, s);
  FlangerArgs a{};
  a.buf = d_buf;
  a.stride = stride;
  a.n = n;
  a.ring = f->ring.p;
  a.len = f->len;
  a.wp = f->wp;
  a.phase_in = f->phase.p + f->ph_cur;
  a.phase_out = f->phase.p + (f->ph_cur ^ 1);
  a.base = f->cfg.base_delay_seconds;
  a.depth = f->cfg.depth_seconds;
  a.sample_rate = f->cfg.sample_rate;
  a.max_delay = (double)(f->len - 3);
  a.lfo_inc = kTwoPi * f->cfg.rate_hz / f->cfg.sample_rate;  // :276
  a.two_pi = kTwoPi;
  a.feedback = f->cfg.feedback;
  a.mix = f->cfg.mix;
  a.one_minus_mix = 1 - f->cfg.mix;
  a.channels = f->channels;
  launch_flanger(a, flanger_shape(flanger_block(f), f->len, f->channels), s);
  AD_HIP(hipGetLastError());
  f->wp = (int)((f->wp + n) % f->len);
  f->ph_cur ^= 1;
}

double* field(ad_flanger_config& c, int which) {
  switch (which) {
    case AD_FLANGER_SAMPLE_RATE: return &c.sample_rate;
    case AD_FLANGER_RATE: return &c.rate_hz;
    case AD_FLANGER_DEPTH: return &c.depth_seconds;
    case AD_FLANGER_BASE_DELAY: return &c.base_delay_seconds;
    case AD_FLANGER_FEEDBACK: return &c.feedback;
    case AD_FLANGER_MIX: return &c.mix;
  }
  return nullptr;
}

}  // namespace

extern "C" {

// ---- ad_delay ---------------------------------------------------------------
void ad_delay_default_config(ad_delay_config* cfg, double sample_rate) {
  if (!cfg) return;
  *cfg = ad_delay_config{};
  cfg->sample_rate = sample_rate;  // NewDelay :40-60
  cfg->time_seconds = kDefaultTime;
  cfg->feedback = kDefaultFeedback;
  cfg->mix = kDefaultMix;
}

int ad_delay_validate(const ad_delay_config* cfg) { return validate_config(cfg, validate); }

int ad_delay_create(const ad_delay_config* cfg, int channels, int device, ad_delay** out) {
  return create_handle(cfg, channels, device, out, validate, [](ad_delay* f, const ad_delay_config& c) {
    if (c.mode == 1) {
      if (c.delay_samples > 0) {
        f->len = (int)c.delay_samples;
        f->ring.alloc((size_t)f->channels * f->len);
        zero(f->ring, f->stream);
      }
      f->target = f->current = (double)c.delay_samples;
    } else {
      // NewDelay(sample_rate), then SetTargetTime(time_seconds) as configureDelay does
      if (f->cfg.smooth_coeff == 0) f->cfg.smooth_coeff = smooth_coeff(f->cfg.sample_rate);
      f->cfg.time_seconds = kDefaultTime;
      reconfigure_buffer(f);
      f->cfg.time_seconds = c.time_seconds;
      f->target = std::round(c.time_seconds * c.sample_rate);
    }
  });
}

int ad_delay_set_param(ad_delay* f, int which, double value) {
  return with_handle(f, [&] {
    if (f->cfg.mode == 1) {
      // simpleDelayRuntime.Configure (:330-344): another length is a zeroed ring
      if (which != AD_DELAY_SAMPLES) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "delay-simple has one parameter, its delay in samples");
      if (!(value >= 0 && value <= kMaxRing) || value != std::floor(value))
        AD_FAIL(AD_ERR_INVALID_ARGUMENT, "delay-simple: delay must be a whole number of samples in [0, 2^27]");
      const int d = (int)value;
      if (d == f->cfg.delay_samples) return;
      f->order.wait_host();
      DevBuf<double> fresh;
      fresh.alloc((size_t)f->channels * d);
      if (fresh.p) {
        AD_HIP(hipMemsetAsync(fresh.p, 0, fresh.n * sizeof(double), f->stream));
        AD_HIP(hipStreamSynchronize(f->stream));
      }
      std::swap(f->ring.p, fresh.p);
      std::swap(f->ring.n, fresh.n);
      f->len = d;
      f->wp = 0;
      f->cfg.delay_samples = d;
      f->target = f->current = value;
      return;
    }
    switch (which) {
      case AD_DELAY_SAMPLE_RATE: {  // SetSampleRate :63-72
        validate_delay_rate(value);
        const double old_rate = f->cfg.sample_rate, old_k = f->cfg.smooth_coeff;
        f->cfg.sample_rate = value;
        f->cfg.smooth_coeff = smooth_coeff(value);
        try {
          reconfigure_buffer(f);
        } catch (...) {
          f->cfg.sample_rate = old_rate;
          f->cfg.smooth_coeff = old_k;
          throw;
        }
        break;
      }
      case AD_DELAY_TIME:  // SetTime :77-89: no clamp to one sample
        validate_time(value);
        f->cfg.time_seconds = value;
        f->target = f->current = std::round(value * f->cfg.sample_rate);
        break;
      case AD_DELAY_TARGET_TIME:  // SetTargetTime :95-106
        validate_time(value);
        f->cfg.time_seconds = value;
        f->target = std::round(value * f->cfg.sample_rate);
        break;
      case AD_DELAY_FEEDBACK:
        validate_feedback(value);
        f->cfg.feedback = value;
        break;
      case AD_DELAY_MIX:
        validate_mix(value, "delay mix must be in [0, 1]");
        f->cfg.mix = value;
        break;
      case AD_DELAY_SMOOTH_COEFF:  // a caller's own 1 - exp(-1/(fs * 0.010))
        if (!(value > 0 && value <= 1)) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "delay smoothing coefficient must be in (0, 1]");
        f->cfg.smooth_coeff = value;
        break;
      default:
        AD_FAIL(AD_ERR_INVALID_ARGUMENT, "unknown delay parameter");
    }
  });
}

int ad_delay_get_config(const ad_delay* f, ad_delay_config* cfg) {
  return guard([&] {
    if (!f || !cfg) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "null delay handle or config");
    *cfg = f->cfg;
  });
}

int ad_delay_derived(const ad_delay* f, double* current_samples, double* target_samples, int64_t* ring_len,
                     int64_t* write_pos) {
  return with_handle(f, [&] {
    if (current_samples) *current_samples = f->current;
    if (target_samples) *target_samples = f->target;
    if (ring_len) *ring_len = f->len;
    if (write_pos) *write_pos = f->wp;
  });
}

int ad_delay_kernel_info(const ad_delay* f, int* block, int* sub_block, int* regime, int* launches) {
  return with_handle(f, [&] {
    const Blocks b = f->len > 0 ? blocks_of(f) : Blocks{1, 1};
    if (block) *block = b.both;
    if (sub_block) *sub_block = pow2_sub(b.raw);
    if (regime) *regime = f->last_regime;
    if (launches) *launches = f->last_launches;
  });
}

int ad_delay_set_regime(ad_delay* f, int regime) {
  return with_handle(f, [&] {
    if (regime < 0 || regime > 2) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "delay regime must be 0 (choose), 1 or 2");
    f->force_regime = regime;
  });
}

int ad_delay_process(ad_delay* f, double* buf, int64_t n) { return process_host(f, buf, n, delay_run); }

int ad_delay_process_device(ad_delay* f, double* d_buf, int64_t stride, int64_t n, void* stream) {
  return process_device(f, d_buf, stride, n, stream, delay_run);
}

int ad_delay_reset(ad_delay* f) {
  // Reset :131-137 (currentSamples stays); ordered after the last call, whatever stream it used
  return with_handle(f, [&] {
    f->order.wait_host();
    zero(f->ring, f->stream);
    AD_HIP(hipStreamSynchronize(f->stream));
    f->wp = 0;
  });
}

void ad_delay_destroy(ad_delay* f) { destroy_handle(f); }

// ---- ad_flanger -------------------------------------------------------------
void ad_flanger_default_config(ad_flanger_config* cfg, double sample_rate) {
  if (!cfg) return;
  cfg->sample_rate = sample_rate;  // defaultFlangerConfig flanger.go:9-13
  cfg->rate_hz = 0.25;
  cfg->depth_seconds = 0.0015;
  cfg->base_delay_seconds = 0.001;
  cfg->feedback = 0.25;
  cfg->mix = 0.5;
}

int ad_flanger_validate(const ad_flanger_config* cfg) { return validate_config(cfg, validate); }

int ad_flanger_create(const ad_flanger_config* cfg, int channels, int device, ad_flanger** out) {
  return create_handle(cfg, channels, device, out, validate, [](ad_flanger* f, const ad_flanger_config&) {
    f->phase.alloc(2);
    zero(f->phase, f->stream);
    reconfigure_line(f);
  });
}

int ad_flanger_set_param(ad_flanger* f, int which, double value) {
  return with_handle(f, [&] {
    ad_flanger_config c = f->cfg;
    double* v = field(c, which);
    if (!v) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "unknown flanger parameter");
    *v = value;
    // every field but the new one is valid already, so this is the setter's own
    // check plus, for depth and base delay, reconfigureDelayLine's (:187-224)
    validate(c);
    const ad_flanger_config old = f->cfg;
    f->cfg = c;
    if (which == AD_FLANGER_SAMPLE_RATE || which == AD_FLANGER_DEPTH || which == AD_FLANGER_BASE_DELAY) {
      try {
        reconfigure_line(f);
      } catch (...) {
        f->cfg = old;
        throw;
      }
    }
  });
}

int ad_flanger_get_config(const ad_flanger* f, ad_flanger_config* cfg) {
  return guard([&] {
    if (!f || !cfg) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "null flanger handle or config");
    *cfg = f->cfg;
  });
}

int ad_flanger_derived(const ad_flanger* f, int64_t* ring_len, int64_t* max_delay, int64_t* write_pos,
                       double* lfo_phase) {
  return with_handle(f, [&] {
    if (ring_len) *ring_len = f->len;
    if (max_delay) *max_delay = f->len - 3;
    if (write_pos) *write_pos = f->wp;
    if (lfo_phase) {
      f->order.wait_host();
      AD_HIP(hipMemcpy(lfo_phase, f->phase.p + f->ph_cur, sizeof(double), hipMemcpyDeviceToHost));
    }
  });
}

int ad_flanger_kernel_info(const ad_flanger* f, int* block, int* sub_block, int* channels_per_workgroup,
                           int* lds_bytes) {
  return with_handle(f, [&] {
    const FlangerShape sh = flanger_shape(flanger_block(f), f->len, f->channels);
    if (block) *block = flanger_block(f);
    if (sub_block) *sub_block = sh.sub;
    if (channels_per_workgroup) *channels_per_workgroup = sh.group();
    if (lds_bytes) *lds_bytes = sh.lds_bytes();
  });
}

int ad_flanger_process(ad_flanger* f, double* buf, int64_t n) { return process_host(f, buf, n, flanger_run); }

int ad_flanger_process_device(ad_flanger* f, double* d_buf, int64_t stride, int64_t n, void* stream) {
  return process_device(f, d_buf, stride, n, stream, flanger_run);
}

int ad_flanger_reset(ad_flanger* f) {
  // Reset :249-256: the line, the write position and the LFO phase
  return with_handle(f, [&] {
    f->order.wait_host();
    zero(f->ring, f->stream);
    zero(f->phase, f->stream);
    AD_HIP(hipStreamSynchronize(f->stream));
    f->wp = 0;
  });
}

void ad_flanger_destroy(ad_flanger* f) { destroy_handle(f); }

}  // extern "C"
