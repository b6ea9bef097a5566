// C ABI of the phaser (dsp/effects/modulation/phaser.go), the tremolo
// (tremolo.go) and the ring modulator (ring_modulator.go).  A handle keeps the
// reference's configuration and the LFO phase on the host, in plain IEEE double
// as the setters and Process compute them: the phase is one sequence for every
// channel, so a call steps it on the host, uploads the call's phases and lets
// the kernels take the sine (and what follows from it) once per sample.  The
// phaser's stage states and feedback samples and the tremolo's smoothed gain
// live on the device.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>

#include "fx_handle.hpp"
#include "modfx_kernels.hpp"

using namespace adsp;

namespace {

const double kTwoPi = 2.0 * M_PI;
constexpr double kNyquistSafety = 0.49;  // phaserNyquistSafetyRatio phaser.go:16

void validate(const ad_phaser_config& c) {  // validateParams phaser.go:323-358
  if (!positive(c.sample_rate)) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "phaser sample rate must be > 0 and finite");
  if (!positive(c.rate_hz)) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "phaser rate must be > 0 and finite");
  if (!positive(c.min_freq_hz)) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "phaser min frequency must be > 0 and finite");
  if (!(c.max_freq_hz > c.min_freq_hz) || !is_finite(c.max_freq_hz))
    AD_FAIL(AD_ERR_INVALID_ARGUMENT, "phaser max frequency must be > min frequency and finite");
  if (c.max_freq_hz >= kNyquistSafety * c.sample_rate)
    AD_FAIL(AD_ERR_INVALID_ARGUMENT, "phaser max frequency must be < 0.49 of the sample rate");
  if (c.stages < 1 || c.stages > kPhaserMaxStages) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "phaser stages must be in [1, 12]");
  if (!in_range(c.feedback, -0.99, 0.99)) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "phaser feedback must be in [-0.99, 0.99]");
  if (!in_range(c.mix, 0, 1)) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "phaser mix must be in [0, 1]");
}

void validate(const ad_tremolo_config& c) {  // validateParams tremolo.go:249-271
  if (!positive(c.sample_rate)) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "tremolo sample rate must be > 0 and finite");
  if (!positive(c.rate_hz)) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "tremolo rate must be > 0 and finite");
  if (!in_range(c.depth, 0, 1)) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "tremolo depth must be in [0, 1]");
  if (!(c.smoothing_ms >= 0) || !is_finite(c.smoothing_ms))
    AD_FAIL(AD_ERR_INVALID_ARGUMENT, "tremolo smoothing must be >= 0 and finite");
  if (!in_range(c.mix, 0, 1)) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "tremolo mix must be in [0, 1]");
  if (!in_range(c.smoothing_coeff, 0, 1))
    AD_FAIL(AD_ERR_INVALID_ARGUMENT, "tremolo smoothing coefficient must be 0 (derive it) or in (0, 1]");
}

void validate(const ad_ringmod_config& c) {  // NewRingModulator :74-77, the options :29-52
  if (!positive(c.sample_rate)) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "ring modulator sample rate must be > 0 and finite");
  if (!positive(c.carrier_hz)) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "ring modulator carrier frequency must be > 0 and finite");
  if (!in_range(c.mix, 0, 1)) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "ring modulator mix must be in [0, 1]");
}

double smoothing_coeff(double ms, double fs) {  // updateSmoothingCoefficient tremolo.go:273-289
  if (ms <= 0) return 1;
  const double tau = ms / 1000;
  const double k = 1 - std::exp(-1 / (tau * fs));
  return k < 0 ? 0 : (k > 1 ? 1 : k);
}

// phase += inc with the wrap of phaser.go:279-282, tremolo.go:211-214 and
// ring_modulator.go:147-150: out[i] is the phase sample i sees; returns the one after sample n - 1
double step_phases(double phase, double inc, double* out, int64_t n) {
#pragma clang fp contract(off)
  for (int64_t i = 0; i < n; ++i) {
    out[i] = phase;
    phase = phase + inc;
    if (phase >= kTwoPi) phase = phase - kTwoPi;
  }
  return phase;
}

// What the three handles share: the phase and the call's tables.
struct ModCore : HandleCore {
  double phase = 0;    // lfoPhase / phase before the next sample
  PinnedUpload ph;     // the call's phases
  DevBuf<double> tab;  // what the kernels take from them
  // the phases of the next n samples into ph on s; returns the phase after them
  double upload(double inc, int64_t n, hipStream_t s) {
    const double end = step_phases(phase, inc, ph.stage((size_t)n), n);
    tab.reserve(ph.cap);  // hipFree waits for the device, so no earlier call still reads the old one
    ph.send((size_t)n, s);
    return end;
  }
};

}  // namespace

struct ad_phaser : ModCore {
  ad_phaser_config cfg{};
  DevBuf<double> stage;  // [channels][12][2]
  DevBuf<double> fb;     // [channels] feedbackSample
};

struct ad_tremolo : ModCore {
  ad_tremolo_config cfg{};  // smoothing_coeff: the coefficient in use
  DevBuf<double> cur;       // [1] currentMod
};

struct ad_ringmod : ModCore {
  ad_ringmod_config cfg{};
  double inc = 0;  // phaseInc, updatePhaseIncrement :176-178
};

namespace {

double lfo_inc(double rate_hz, double fs) { return kTwoPi * rate_hz / fs; }

// ---- the device work of a call: the table from the uploaded phases ----------
void phaser_table(ad_phaser* f, int64_t n, hipStream_t s) {
  ModTableArgs t{};
  t.phase = f->ph.dev.p;
  t.out = f->tab.p;
  t.n = n;
  t.kind = MOD_COEF;
  t.min_hz = f->cfg.min_freq_hz;
  t.span_hz = f->cfg.max_freq_hz - f->cfg.min_freq_hz;
  t.sample_rate = f->cfg.sample_rate;
  t.max_allowed = kNyquistSafety * f->cfg.sample_rate;
  t.pi = M_PI;
  launch_mod_table(t, s);
}

void tremolo_table(ad_tremolo* f, int64_t n, bool commit, hipStream_t s) {
  ModTableArgs t{};
  t.phase = f->ph.dev.p;
  t.out = f->tab.p;
  t.n = n;
  t.kind = MOD_TARGET;
  t.depth = f->cfg.depth;
  t.one_minus_depth = 1 - f->cfg.depth;
  launch_mod_table(t, s);
  if (f->cfg.smoothing_coeff < 1)
    launch_tremolo_smooth(f->tab.p, n, f->cfg.smoothing_coeff, f->cur.p, commit ? 1 : 0, s);
  else if (commit)  // currentMod = targetMod (:204)
    AD_HIP(hipMemcpyAsync(f->cur.p, f->tab.p + (n - 1), sizeof(double), hipMemcpyDeviceToDevice, s));
}

void ringmod_table(ad_ringmod* f, int64_t n, hipStream_t s) {
  ModTableArgs t{};
  t.phase = f->ph.dev.p;
  t.out = f->tab.p;
  t.n = n;
  t.kind = MOD_CARRIER;
  launch_mod_table(t, s);
}

void apply(ModCore* f, double* d_buf, int64_t stride, int64_t n, double mix, hipStream_t s) {
  ModApplyArgs a{};
  a.buf = d_buf;
  a.stride = stride;
  a.n = n;
  a.tab = f->tab.p;
  a.mix = mix;
  a.one_minus_mix = 1 - mix;
  a.channels = f->channels;
  launch_mod_apply(a, s);
}

void phaser_run(ad_phaser* f, double* d_buf, int64_t stride, int64_t n, hipStream_t s) {
  CallScope call(f->order, s);
  const double end = f->upload(lfo_inc(f->cfg.rate_hz, f->cfg.sample_rate), n, s);
  phaser_table(f, n, s);
  PhaserArgs a{};
  a.buf = d_buf;
  a.stride = stride;
  a.n = n;
  a.coef = f->tab.p;
  a.stage = f->stage.p;
  a.fb = f->fb.p;
  a.feedback = f->cfg.feedback;
  a.mix = f->cfg.mix;
  a.one_minus_mix = 1 - f->cfg.mix;
  a.stages = f->cfg.stages;
  a.channels = f->channels;
  launch_phaser(a, s);
  AD_HIP(hipGetLastError());
  f->phase = end;
}

void tremolo_run(ad_tremolo* f, double* d_buf, int64_t stride, int64_t n, hipStream_t s) {
  CallScope call(f->order, s);
  const double end = f->upload(lfo_inc(f->cfg.rate_hz, f->cfg.sample_rate), n, s);
  tremolo_table(f, n, true, s);
  apply(f, d_buf, stride, n, f->cfg.mix, s);
  AD_HIP(hipGetLastError());
  f->phase = end;
}

void ringmod_run(ad_ringmod* f, double* d_buf, int64_t stride, int64_t n, hipStream_t s) {
  CallScope call(f->order, s);
  const double end = f->upload(f->inc, n, s);
  ringmod_table(f, n, s);
  apply(f, d_buf, stride, n, f->cfg.mix, s);
  AD_HIP(hipGetLastError());
  f->phase = end;
}

// The next n phases and table values, by the code a call runs; nothing advances.
template <class H, class Table>
int peek(H* f, int64_t n, double inc, double* phase_out, double* second_out, Table table) {
  return with_handle(f, [&] {
    if (n < 0 || (n > 0 && (!phase_out || !second_out))) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "bad peek buffers");
    if (n == 0) return;
    f->order.wait_host();
    (void)f->upload(inc, n, f->stream);
    table(f, n, f->stream);
    AD_HIP(hipGetLastError());
    AD_HIP(hipMemcpyAsync(second_out, f->tab.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, f->stream));
    AD_HIP(hipStreamSynchronize(f->stream));
    std::memcpy(phase_out, f->ph.host, (size_t)n * sizeof(double));
  });
}

void phaser_clear_stages(ad_phaser* f) {
  f->order.wait_host();
  zero(f->stage, f->stream);
  AD_HIP(hipStreamSynchronize(f->stream));
}

void tremolo_set_cur(ad_tremolo* f, double v) {
  f->order.wait_host();
  AD_HIP(hipMemcpy(f->cur.p, &v, sizeof(double), hipMemcpyHostToDevice));
}

// a candidate configuration replaces the handle's only when it is valid as a whole
void phaser_commit(ad_phaser* f, const ad_phaser_config& c) {
  validate(c);
  const bool restage = c.stages != f->cfg.stages;  // SetStages :226-230: the same count keeps the states
  if (restage) phaser_clear_stages(f);
  f->cfg = c;
}

}  // namespace

extern "C" {

// ---- ad_phaser --------------------------------------------------------------
void ad_phaser_default_config(ad_phaser_config* cfg, double sample_rate) {
  if (!cfg) return;
  *cfg = ad_phaser_config{};
  cfg->sample_rate = sample_rate;  // defaultPhaserConfig phaser.go:8-14
  cfg->rate_hz = 0.4;
  cfg->min_freq_hz = 300.0;
  cfg->max_freq_hz = 1600.0;
  cfg->feedback = 0.2;
  cfg->mix = 0.5;
  cfg->stages = 6;
}

int ad_phaser_validate(const ad_phaser_config* cfg) { return validate_config(cfg, validate); }

int ad_phaser_create(const ad_phaser_config* cfg, int channels, int device, ad_phaser** out) {
  return create_handle(cfg, channels, device, out, validate, [](ad_phaser* f, const ad_phaser_config&) {
    f->stage.alloc((size_t)f->channels * 2 * kPhaserMaxStages);
    f->fb.alloc((size_t)f->channels);
    zero(f->stage, f->stream);
    zero(f->fb, f->stream);
  });
}

int ad_phaser_set_param(ad_phaser* f, int which, double value) {
  return with_handle(f, [&] {
    ad_phaser_config c = f->cfg;
    switch (which) {
      case AD_PHASER_SAMPLE_RATE: c.sample_rate = value; break;  // SetSampleRate :183-191
      case AD_PHASER_RATE: c.rate_hz = value; break;             // SetRateHz :194-202
      case AD_PHASER_MIN_FREQ: c.min_freq_hz = value; break;     // SetFrequencyRangeHz(value, max) :205-218
      case AD_PHASER_MAX_FREQ: c.max_freq_hz = value; break;     // SetFrequencyRangeHz(min, value)
      case AD_PHASER_FEEDBACK: c.feedback = value; break;        // SetFeedback :236-244
      case AD_PHASER_MIX: c.mix = value; break;                  // SetMix :247-255
      case AD_PHASER_STAGES:                                     // SetStages :221-233
        if (!in_range(value, 1, kPhaserMaxStages) || value != std::floor(value))
          AD_FAIL(AD_ERR_INVALID_ARGUMENT, "phaser stages must be a whole number in [1, 12]");
        c.stages = (int)value;
        break;
      default: AD_FAIL(AD_ERR_INVALID_ARGUMENT, "unknown phaser parameter");
    }
    // every other field is valid already, so this is the setter's own check plus, for the
    // sample rate and the range, validateParams
    phaser_commit(f, c);
  });
}

int ad_phaser_set_range(ad_phaser* f, double min_freq_hz, double max_freq_hz) {
  return with_handle(f, [&] {
    ad_phaser_config c = f->cfg;
    c.min_freq_hz = min_freq_hz;
    c.max_freq_hz = max_freq_hz;
    phaser_commit(f, c);
  });
}

int ad_phaser_get_config(const ad_phaser* f, ad_phaser_config* cfg) {
  return guard([&] {
    if (!f || !cfg) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "null phaser handle or config");
    *cfg = f->cfg;
  });
}

int ad_phaser_kernel_info(const ad_phaser* f, int* channels_per_workgroup, int* tile, int* lds_bytes) {
  return with_handle(f, [&] {
    if (channels_per_workgroup) *channels_per_workgroup = 64;
    if (tile) *tile = kPhaserTile;
    if (lds_bytes) *lds_bytes = (2 * 64 * kPhaserPitch + kPhaserTile) * (int)sizeof(double);
  });
}

int ad_phaser_peek_lfo(ad_phaser* f, int64_t n, double* phase_out, double* coef_out) {
  return peek(f, n, f ? lfo_inc(f->cfg.rate_hz, f->cfg.sample_rate) : 0.0, phase_out, coef_out, phaser_table);
}

int ad_phaser_process(ad_phaser* f, double* buf, int64_t n) { return process_host(f, buf, n, phaser_run); }

int ad_phaser_process_device(ad_phaser* f, double* d_buf, int64_t stride, int64_t n, void* stream) {
  return process_device(f, d_buf, stride, n, stream, phaser_run);
}

int ad_phaser_reset(ad_phaser* f) {
  // Reset :258-265: the stages, feedbackSample and lfoPhase; ordered after the last call
  return with_handle(f, [&] {
    f->order.wait_host();
    zero(f->stage, f->stream);
    zero(f->fb, f->stream);
    AD_HIP(hipStreamSynchronize(f->stream));
    f->phase = 0;
  });
}

void ad_phaser_destroy(ad_phaser* f) { destroy_handle(f); }

// ---- ad_tremolo -------------------------------------------------------------
void ad_tremolo_default_config(ad_tremolo_config* cfg, double sample_rate) {
  if (!cfg) return;
  *cfg = ad_tremolo_config{};
  cfg->sample_rate = sample_rate;  // defaultTremoloConfig tremolo.go:8-13
  cfg->rate_hz = 4.0;
  cfg->depth = 0.6;
  cfg->smoothing_ms = 5.0;
  cfg->mix = 1.0;
}

int ad_tremolo_validate(const ad_tremolo_config* cfg) { return validate_config(cfg, validate); }

int ad_tremolo_create(const ad_tremolo_config* cfg, int channels, int device, ad_tremolo** out) {
  return create_handle(cfg, channels, device, out, validate, [](ad_tremolo* f, const ad_tremolo_config&) {
    if (f->cfg.smoothing_coeff == 0) f->cfg.smoothing_coeff = smoothing_coeff(f->cfg.smoothing_ms, f->cfg.sample_rate);
    f->cur.alloc(1);
    tremolo_set_cur(f, 1.0);  // NewTremolo :124
  });
}

int ad_tremolo_set_param(ad_tremolo* f, int which, double value) {
  return with_handle(f, [&] {
    ad_tremolo_config c = f->cfg;
    switch (which) {
      case AD_TREMOLO_SAMPLE_RATE: c.sample_rate = value; break;    // SetSampleRate :138-147
      case AD_TREMOLO_RATE: c.rate_hz = value; break;               // SetRateHz :150-158
      case AD_TREMOLO_DEPTH: c.depth = value; break;                // SetDepth :161-169
      case AD_TREMOLO_SMOOTHING: c.smoothing_ms = value; break;     // SetSmoothingMs :172-181
      case AD_TREMOLO_MIX: c.mix = value; break;                    // SetMix :184-192
      case AD_TREMOLO_SMOOTHING_COEFF:                              // a caller's own 1 - exp(...)
        if (!(value > 0 && value <= 1)) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "tremolo smoothing coefficient must be in (0, 1]");
        c.smoothing_coeff = value;
        break;
      default: AD_FAIL(AD_ERR_INVALID_ARGUMENT, "unknown tremolo parameter");
    }
    validate(c);  // every other field is valid already: the setter's own check
    if (which == AD_TREMOLO_SAMPLE_RATE || which == AD_TREMOLO_SMOOTHING)
      c.smoothing_coeff = smoothing_coeff(c.smoothing_ms, c.sample_rate);
    f->cfg = c;
  });
}

int ad_tremolo_get_config(const ad_tremolo* f, ad_tremolo_config* cfg) {
  return guard([&] {
    if (!f || !cfg) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "null tremolo handle or config");
    *cfg = f->cfg;
  });
}

int ad_tremolo_kernel_info(const ad_tremolo* f, int* samples_per_workgroup, int* smooth_chunk, int* smoothed) {
  return with_handle(f, [&] {
    if (samples_per_workgroup) *samples_per_workgroup = 2 * kModApplyThreads * kModApplySteps;
    if (smooth_chunk) *smooth_chunk = kModSmoothChunk;
    if (smoothed) *smoothed = f->cfg.smoothing_coeff < 1 ? 1 : 0;
  });
}

int ad_tremolo_peek_lfo(ad_tremolo* f, int64_t n, double* phase_out, double* gain_out) {
  return peek(f, n, f ? lfo_inc(f->cfg.rate_hz, f->cfg.sample_rate) : 0.0, phase_out, gain_out,
              [](ad_tremolo* h, int64_t m, hipStream_t s) { tremolo_table(h, m, false, s); });
}

int ad_tremolo_process(ad_tremolo* f, double* buf, int64_t n) { return process_host(f, buf, n, tremolo_run); }

int ad_tremolo_process_device(ad_tremolo* f, double* d_buf, int64_t stride, int64_t n, void* stream) {
  return process_device(f, d_buf, stride, n, stream, tremolo_run);
}

int ad_tremolo_reset(ad_tremolo* f) {
  // Reset :195-198: lfoPhase = 0, currentMod = 1
  return with_handle(f, [&] {
    tremolo_set_cur(f, 1.0);
    f->phase = 0;
  });
}

void ad_tremolo_destroy(ad_tremolo* f) { destroy_handle(f); }

// ---- ad_ringmod -------------------------------------------------------------
void ad_ringmod_default_config(ad_ringmod_config* cfg, double sample_rate) {
  if (!cfg) return;
  cfg->sample_rate = sample_rate;  // defaultRingModConfig ring_modulator.go:8-11
  cfg->carrier_hz = 440.0;
  cfg->mix = 1.0;
}

int ad_ringmod_validate(const ad_ringmod_config* cfg) { return validate_config(cfg, validate); }

int ad_ringmod_create(const ad_ringmod_config* cfg, int channels, int device, ad_ringmod** out) {
  return create_handle(cfg, channels, device, out, validate, [](ad_ringmod* f, const ad_ringmod_config& c) {
    f->inc = lfo_inc(c.carrier_hz, c.sample_rate);
  });
}

int ad_ringmod_set_param(ad_ringmod* f, int which, double value) {
  return with_handle(f, [&] {
    ad_ringmod_config c = f->cfg;
    switch (which) {
      case AD_RINGMOD_SAMPLE_RATE: c.sample_rate = value; break;  // SetSampleRate :103-112
      case AD_RINGMOD_CARRIER: c.carrier_hz = value; break;       // SetCarrierHz :115-124
      case AD_RINGMOD_MIX: c.mix = value; break;                  // SetMix :127-135
      default: AD_FAIL(AD_ERR_INVALID_ARGUMENT, "unknown ring modulator parameter");
    }
    validate(c);
    f->cfg = c;
    if (which != AD_RINGMOD_MIX) f->inc = lfo_inc(c.carrier_hz, c.sample_rate);
  });
}

int ad_ringmod_get_config(const ad_ringmod* f, ad_ringmod_config* cfg) {
  return guard([&] {
    if (!f || !cfg) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "null ring modulator handle or config");
    *cfg = f->cfg;
  });
}

int ad_ringmod_kernel_info(const ad_ringmod* f, int* samples_per_workgroup, int* table_threads, double* phase_inc) {
  return with_handle(f, [&] {
    if (samples_per_workgroup) *samples_per_workgroup = 2 * kModApplyThreads * kModApplySteps;
    if (table_threads) *table_threads = kModTableThreads;
    if (phase_inc) *phase_inc = f->inc;
  });
}

int ad_ringmod_peek_lfo(ad_ringmod* f, int64_t n, double* phase_out, double* carrier_out) {
  return peek(f, n, f ? f->inc : 0.0, phase_out, carrier_out, ringmod_table);
}

int ad_ringmod_process(ad_ringmod* f, double* buf, int64_t n) { return process_host(f, buf, n, ringmod_run); }

int ad_ringmod_process_device(ad_ringmod* f, double* d_buf, int64_t stride, int64_t n, void* stream) {
  return process_device(f, d_buf, stride, n, stream, ringmod_run);
}

int ad_ringmod_reset(ad_ringmod* f) {
  // Reset :138-140; ordered after the last call, which took its phases when it was enqueued
  return with_handle(f, [&] {
    f->phase = 0;
  });
}

void ad_ringmod_destroy(ad_ringmod* f) { destroy_handle(f); }

}  // extern "C"
