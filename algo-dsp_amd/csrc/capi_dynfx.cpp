// C ABI of the transient shaper (dsp/effects/dynamics/transient_shaper.go) and
// the de-esser (deesser.go).  A handle keeps the reference's configuration on
// the host and derives what the reference caches (the envelope coefficients,
// the detection section, bandNorm, the gain computer's log2-domain constants)
// there with the C library, as the setters do.  The envelope, the two cascades'
// states and the metrics live on the device, one set per channel.
//
// The de-esser's two cascades have equal sections and see the same input, so
// while their states are equal one walk stands for both.  They stop being
// equal when a call runs that advances detectFilters alone: listen mode
// (:422-424) or wideband mode (:448-449).  The handle tracks that; from then on
// split-band calls run both cascades until a rebuild or Reset makes them equal
// again.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <vector>

#include "dynfx_kernels.hpp"
#include "fx_handle.hpp"

using namespace adsp;

namespace {

constexpr double kLog2Of10Div20 = 0.166096404744;  // compressor.go:27 (truncated literal, kept)

void validate(const ad_transient_config& c) {
  if (!positive(c.sample_rate)) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "transient shaper sample rate must be positive and finite");
  if (!in_range(c.attack_amount, -1, 1)) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "transient shaper attack amount must be in [-1, 1]");
  if (!in_range(c.sustain_amount, -1, 1)) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "transient shaper sustain amount must be in [-1, 1]");
  if (!in_range(c.attack_ms, 0.1, 200)) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "transient shaper attack must be in [0.1, 200]");
  if (!in_range(c.release_ms, 1, 2000)) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "transient shaper release must be in [1, 2000]");
  if (!in_range(c.attack_coeff, 0, 1) || !in_range(c.release_coeff, 0, 1))
    AD_FAIL(AD_ERR_INVALID_ARGUMENT, "transient shaper coefficients must be 0 (derive them) or in (0, 1]");
}

void validate(const ad_deesser_config& c) {
  if (!positive(c.sample_rate)) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "de-esser sample rate must be positive and finite");
  if (!in_range(c.freq_hz, 1000, 20000)) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "de-esser frequency must be in [1000, 20000]");
  if (c.freq_hz >= c.sample_rate / 2) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "de-esser frequency must be < Nyquist");
  if (!in_range(c.q, 0.1, 10)) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "de-esser Q must be in [0.1, 10]");
  if (!is_finite(c.threshold_db)) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "de-esser threshold must be finite");
  if (!in_range(c.ratio, 1, 100)) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "de-esser ratio must be in [1, 100]");
  if (!in_range(c.knee_db, 0, 12)) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "de-esser knee must be in [0, 12]");
  if (!in_range(c.attack_ms, 0.01, 50)) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "de-esser attack must be in [0.01, 50]");
  if (!in_range(c.release_ms, 1, 500)) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "de-esser release must be in [1, 500]");
  if (!in_range(c.range_db, -60, 0)) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "de-esser range must be in [-60, 0]");
  if (!in_range(c.attack_coeff, 0, 1) || !in_range(c.release_coeff, 0, 1))
    AD_FAIL(AD_ERR_INVALID_ARGUMENT, "de-esser coefficients must be 0 (derive them) or in (0, 1]");
  if (!flag(c.mode)) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "de-esser mode invalid");
  if (!flag(c.detector)) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "de-esser detector invalid");
  if (!flag(c.listen)) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "de-esser listen must be 0 or 1");
  if (c.filter_order < 1 || c.filter_order > kDynMaxOrder) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "de-esser filter order must be in [1, 4]");
}

double time_ms_to_coeff(double ms, double fs) {  // timeMsToCoeff transient_shaper.go:184-200
  const double seconds = ms / 1000.0;
  if (seconds <= 0) return 1;
  const double coeff = 1.0 - std::exp(-1.0 / (seconds * fs));
  return coeff < 0 ? 0 : (coeff > 1 ? 1 : coeff);
}

// the coefficients in use: the caller's own where the config carries one, else updateCoefficients :179-182
void transient_coeffs(const ad_transient_config& c, double* attack, double* release) {
  *attack = c.attack_coeff != 0 ? c.attack_coeff : time_ms_to_coeff(c.attack_ms, c.sample_rate);
  *release = c.release_coeff != 0 ? c.release_coeff : time_ms_to_coeff(c.release_ms, c.sample_rate);
}

void deesser_coeffs(const ad_deesser_config& c, double* attack, double* release) {  // updateTimeConstants :573-576
  *attack = c.attack_coeff != 0 ? c.attack_coeff : 1.0 - std::exp(-M_LN2 / (c.attack_ms * 0.001 * c.sample_rate));
  *release = c.release_coeff != 0 ? c.release_coeff : std::exp(-M_LN2 / (c.release_ms * 0.001 * c.sample_rate));
}

// design.Bandpass design.go:47-66 and design.Highpass (pass.HighpassRBJ butterworth.go:91-123) -> {b0, b1, b2, a1, a2}
void deesser_section(const ad_deesser_config& c, double* sec) {
  const double fs = c.sample_rate, freq = c.freq_hz;
  for (int i = 0; i < 5; ++i) sec[i] = 0;
  if (!positive(fs) || !(freq > 0) || freq >= fs / 2 || !is_finite(freq)) return;
  double q = c.q;
  if (q <= 0 || !is_finite(q)) q = 1 / std::sqrt(2.0);
  const double w0 = 2 * M_PI * freq / fs;
  const double cw = std::cos(w0), sw = std::sin(w0);
  const double alpha = sw / (2 * q);
  double b0, b1, b2;
  if (c.detector == 1) {
    b0 = (1 + cw) / 2, b1 = -(1 + cw), b2 = (1 + cw) / 2;
  } else {
    b0 = sw / 2, b1 = 0.0, b2 = -sw / 2;
  }
  const double a0 = 1 + alpha, a1 = -2 * cw, a2 = 1 - alpha;
  if (a0 == 0 || !is_finite(a0)) return;
  sec[0] = b0 / a0, sec[1] = b1 / a0, sec[2] = b2 / a0, sec[3] = a1 / a0, sec[4] = a2 / a0;
}

struct DeessDerived {
  double sec[5], band_norm, threshold_log2, knee_width_log2, range_lin, attack, release;
  DeessGainParams gain;
};

DeessDerived deesser_derive(const ad_deesser_config& c) {
  DeessDerived d{};
  deesser_section(c, d.sec);
  d.band_norm = 1.0 / std::pow(c.q, (double)c.filter_order);  // rebuildFilters :621
  d.threshold_log2 = c.threshold_db * kLog2Of10Div20;         // updateCoefficients :559-571
  d.knee_width_log2 = c.knee_db * kLog2Of10Div20;
  d.range_lin = std::pow(10.0, c.range_db / 20.0);
  deesser_coeffs(c, &d.attack, &d.release);
  d.gain.threshold_log2 = d.threshold_log2;
  d.gain.knee_on = c.knee_db > 0 ? 1 : 0;
  d.gain.half_knee = d.knee_width_log2 * 0.5;  // calculateGain :536
  d.gain.inv_knee_width_log2 = c.knee_db > 0 ? 1.0 / d.knee_width_log2 : 0.0;
  d.gain.cf = 1.0 - 1.0 / c.ratio;  // :526, :549
  d.gain.range_lin = d.range_lin;
  return d;
}

// What the two handles share: the envelope and the scratch rows.
struct DynCore : HandleCore {
  DevBuf<double> env;            // [channels]
  DevBuf<double> env_s, band_s;  // [channels][pitch] of one pass
  void init_env() {
    env.alloc((size_t)channels);
    zero(env, stream);
  }
};

}  // namespace

struct ad_transient : DynCore {
  ad_transient_config cfg{};  // attack_coeff, release_coeff: the coefficients in use
};

struct ad_deesser : DynCore {
  ad_deesser_config cfg{};  // attack_coeff, release_coeff: the coefficients in use
  DeessDerived d{};
  DevBuf<double> det, band;  // [channels][kDynMaxOrder][2]
  DevBuf<double> peak, gr;   // [channels] metrics
  DevBuf<double> part;       // [channels][tiles][2]
  DevBuf<double> curve;      // ad_deesser_gain
  bool diverged = false;     // a call has advanced detectFilters alone since the two cascades were last equal
};

namespace {

void transient_run(ad_transient* f, double* d_buf, int64_t stride, int64_t n, hipStream_t s) {
  CallScope call(f->order, s);
  const int64_t seg = scratch_segment(n, f->channels, 1);
  f->env_s.reserve((size_t)f->channels * (seg + 1));  // hipFree waits for the device, so no earlier call still reads the old one
  for (int64_t off = 0; off < n; off += seg) {
    const int64_t m = std::min(seg, n - off);
    DynWalkArgs w{};
    w.buf = d_buf + off;
    w.stride = stride;
    w.n = m;
    w.env_s = f->env_s.p;
    w.pitch = seg + 1;
    w.env = f->env.p;
    w.attack = f->cfg.attack_coeff;
    w.release = f->cfg.release_coeff;
    w.channels = f->channels;
    launch_transient_walk(w, s);
    TransientPointArgs p{};
    p.buf = d_buf + off;
    p.stride = stride;
    p.n = m;
    p.env_s = f->env_s.p;
    p.pitch = seg + 1;
    p.attack_amount = f->cfg.attack_amount;
    p.sustain_amount = f->cfg.sustain_amount;
    p.channels = f->channels;
    launch_transient_point(p, s);
  }
  AD_HIP(hipGetLastError());
}

int deesser_walk_mode(const ad_deesser* f) {
  if (f->cfg.listen) return DEESS_LISTEN;
  if (f->cfg.mode == 1) return DEESS_WIDE;
  return f->diverged ? DEESS_SPLIT_TWO : DEESS_SPLIT_ONE;
}

void deesser_run(ad_deesser* f, double* d_buf, int64_t stride, int64_t n, hipStream_t s) {
  CallScope call(f->order, s);
  const int mode = deesser_walk_mode(f);
  const bool split = mode == DEESS_SPLIT_ONE || mode == DEESS_SPLIT_TWO;
  const int64_t seg = scratch_segment(n, f->channels, 2);
  if (mode != DEESS_LISTEN) {
    f->env_s.reserve((size_t)f->channels * (seg + 1));
    if (split) f->band_s.reserve((size_t)f->channels * (seg + 1));
    f->part.reserve((size_t)f->channels * deess_point_tiles(seg) * 2);
  }
  for (int64_t off = 0; off < n; off += seg) {
    const int64_t m = std::min(seg, n - off);
    DynWalkArgs w{};
    w.buf = d_buf + off;
    w.stride = stride;
    w.n = m;
    w.env_s = f->env_s.p;
    w.band_s = f->band_s.p;
    w.pitch = seg + 1;
    w.env = f->env.p;
    w.det_state = f->det.p;
    w.band_state = f->band.p;
    w.peak = f->peak.p;
    w.attack = f->d.attack;
    w.release = f->d.release;
    w.b0 = f->d.sec[0], w.b1 = f->d.sec[1], w.b2 = f->d.sec[2], w.a1 = f->d.sec[3], w.a2 = f->d.sec[4];
    w.order = f->cfg.filter_order;
    w.mode = mode;
    w.channels = f->channels;
    launch_deesser_walk(w, s);
    if (mode == DEESS_LISTEN) continue;
    DeessPointArgs p{};
    p.buf = d_buf + off;
    p.stride = stride;
    p.n = m;
    p.env_s = f->env_s.p;
    p.band_s = split ? f->band_s.p : nullptr;
    p.pitch = seg + 1;
    p.g = f->d.gain;
    p.band_norm = f->d.band_norm;
    p.part = f->part.p;
    p.gr = f->gr.p;
    p.channels = f->channels;
    launch_deesser_point(p, s);
  }
  AD_HIP(hipGetLastError());
  if (!split) f->diverged = true;  // detectFilters moved, bandFilters did not
}

// rebuildFilters :578-622: new sections, so both cascades start from zero; the envelope and the metrics stay
void deesser_rebuild(ad_deesser* f) {
  f->order.wait_host();
  zero(f->det, f->stream);
  zero(f->band, f->stream);
  AD_HIP(hipStreamSynchronize(f->stream));
  f->diverged = false;
}

void deesser_reset_metrics(ad_deesser* f) {
  f->order.wait_host();
  fill(f->peak, 0.0, f->stream);
  fill(f->gr, 1.0, f->stream);
  AD_HIP(hipStreamSynchronize(f->stream));
}

constexpr int walk_lds_bytes(int tile, int rows) { return 2 * rows * 64 * (tile + 1) * (int)sizeof(double); }

}  // namespace

extern "C" {

// ---- ad_transient -----------------------------------------------------------
void ad_transient_default_config(ad_transient_config* cfg, double sample_rate) {
  if (!cfg) return;
  *cfg = ad_transient_config{};
  cfg->sample_rate = sample_rate;  // transient_shaper.go:9-12
  cfg->attack_amount = 0.0;
  cfg->sustain_amount = 0.0;
  cfg->attack_ms = 10.0;
  cfg->release_ms = 120.0;
}

int ad_transient_validate(const ad_transient_config* cfg) { return validate_config(cfg, validate); }

int ad_transient_derived(const ad_transient_config* cfg, double* attack_coeff, double* release_coeff) {
  return guard([&] {
    if (!cfg) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "null transient shaper config");
    validate(*cfg);
    double a, r;
    transient_coeffs(*cfg, &a, &r);
    if (attack_coeff) *attack_coeff = a;
    if (release_coeff) *release_coeff = r;
  });
}

int ad_transient_create(const ad_transient_config* cfg, int channels, int device, ad_transient** out) {
  return create_handle(cfg, channels, device, out, validate, [](ad_transient* f, const ad_transient_config&) {
    f->init_env();
    transient_coeffs(f->cfg, &f->cfg.attack_coeff, &f->cfg.release_coeff);
  });
}

int ad_transient_set_param(ad_transient* f, int which, double value) {
  return with_handle(f, [&] {
    ad_transient_config c = f->cfg;
    switch (which) {
      case AD_TRANSIENT_SAMPLE_RATE: c.sample_rate = value; break;        // SetSampleRate :107-117
      case AD_TRANSIENT_ATTACK_AMOUNT: c.attack_amount = value; break;    // SetAttackAmount :57-66
      case AD_TRANSIENT_SUSTAIN_AMOUNT: c.sustain_amount = value; break;  // SetSustainAmount :69-78
      case AD_TRANSIENT_ATTACK: c.attack_ms = value; break;               // SetAttack :81-91
      case AD_TRANSIENT_RELEASE: c.release_ms = value; break;             // SetRelease :94-104
      case AD_TRANSIENT_ATTACK_COEFF:                                     // a caller's own 1 - exp(...)
      case AD_TRANSIENT_RELEASE_COEFF:
        if (!(value > 0 && value <= 1)) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "transient shaper coefficient must be in (0, 1]");
        (which == AD_TRANSIENT_ATTACK_COEFF ? c.attack_coeff : c.release_coeff) = value;
        break;
      default: AD_FAIL(AD_ERR_INVALID_ARGUMENT, "unknown transient shaper parameter");
    }
    validate(c);  // every other field is valid already: the setter's own check
    if (which == AD_TRANSIENT_SAMPLE_RATE || which == AD_TRANSIENT_ATTACK || which == AD_TRANSIENT_RELEASE) {
      c.attack_coeff = c.release_coeff = 0;  // updateCoefficients :179-182 derives both
      transient_coeffs(c, &c.attack_coeff, &c.release_coeff);
    }
    f->cfg = c;
  });
}

int ad_transient_get_config(const ad_transient* f, ad_transient_config* cfg) {
  return guard([&] {
    if (!f || !cfg) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "null transient shaper handle or config");
    *cfg = f->cfg;
  });
}

int ad_transient_kernel_info(const ad_transient* f, int* channels_per_workgroup, int* tile, int* lds_bytes) {
  return with_handle(f, [&] {
    if (channels_per_workgroup) *channels_per_workgroup = 64;
    if (tile) *tile = kDynWalkTile;
    if (lds_bytes) *lds_bytes = walk_lds_bytes(kDynWalkTile, 1);
  });
}

int ad_transient_get_state(ad_transient* f, int channel, double* envelope) {
  return guard([&] {
    check_channel(f, channel);
    if (!envelope) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "null state output");
    DeviceScope ds(f->device);
    f->order.wait_host();
    AD_HIP(hipMemcpy(envelope, f->env.p + channel, sizeof(double), hipMemcpyDeviceToHost));
  });
}

int ad_transient_set_state(ad_transient* f, int channel, double envelope) {
  return guard([&] {
    check_channel(f, channel);
    DeviceScope ds(f->device);
    f->order.wait_host();
    AD_HIP(hipMemcpy(f->env.p + channel, &envelope, sizeof(double), hipMemcpyHostToDevice));
  });
}

int ad_transient_process(ad_transient* f, double* buf, int64_t n) { return process_host(f, buf, n, transient_run); }

int ad_transient_process_device(ad_transient* f, double* d_buf, int64_t stride, int64_t n, void* stream) {
  return process_device(f, d_buf, stride, n, stream, transient_run);
}

int ad_transient_reset(ad_transient* f) {
  // Reset :135-137: the envelope; ordered after the last call
  return with_handle(f, [&] {
    f->order.wait_host();
    zero(f->env, f->stream);
    AD_HIP(hipStreamSynchronize(f->stream));
  });
}

void ad_transient_destroy(ad_transient* f) { destroy_handle(f); }

// ---- ad_deesser -------------------------------------------------------------
void ad_deesser_default_config(ad_deesser_config* cfg, double sample_rate) {
  if (!cfg) return;
  *cfg = ad_deesser_config{};
  cfg->sample_rate = sample_rate;  // deesser.go:43-54
  cfg->freq_hz = 6000.0;
  cfg->q = 1.5;
  cfg->threshold_db = -20.0;
  cfg->ratio = 4.0;
  cfg->knee_db = 3.0;
  cfg->attack_ms = 0.5;
  cfg->release_ms = 20.0;
  cfg->range_db = -24.0;
  cfg->mode = 0;
  cfg->detector = 0;
  cfg->listen = 0;
  cfg->filter_order = 2;
}

int ad_deesser_validate(const ad_deesser_config* cfg) { return validate_config(cfg, validate); }

int ad_deesser_derived(const ad_deesser_config* cfg, double* section, double* band_norm, double* threshold_log2,
                       double* knee_width_log2, double* range_lin, double* attack_coeff, double* release_coeff) {
  return guard([&] {
    if (!cfg) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "null de-esser config");
    validate(*cfg);
    const DeessDerived d = deesser_derive(*cfg);
    if (section) std::memcpy(section, d.sec, sizeof(d.sec));
    if (band_norm) *band_norm = d.band_norm;
    if (threshold_log2) *threshold_log2 = d.threshold_log2;
    if (knee_width_log2) *knee_width_log2 = d.knee_width_log2;
    if (range_lin) *range_lin = d.range_lin;
    if (attack_coeff) *attack_coeff = d.attack;
    if (release_coeff) *release_coeff = d.release;
  });
}

int ad_deesser_create(const ad_deesser_config* cfg, int channels, int device, ad_deesser** out) {
  return create_handle(cfg, channels, device, out, validate, [](ad_deesser* f, const ad_deesser_config&) {
    f->init_env();
    f->d = deesser_derive(f->cfg);
    f->cfg.attack_coeff = f->d.attack;
    f->cfg.release_coeff = f->d.release;
    const size_t states = (size_t)f->channels * kDynMaxOrder * 2;
    f->det.alloc(states);
    f->band.alloc(states);
    f->peak.alloc((size_t)f->channels);
    f->gr.alloc((size_t)f->channels);
    fill(f->det, 0.0, f->stream);
    fill(f->band, 0.0, f->stream);
    fill(f->peak, 0.0, f->stream);
    fill(f->gr, 1.0, f->stream);  // NewDeEsser :174
  });
}

int ad_deesser_set_param(ad_deesser* f, int which, double value) {
  return with_handle(f, [&] {
    ad_deesser_config c = f->cfg;
    bool rebuild = false, times = false;
    switch (which) {
      case AD_DEESSER_SAMPLE_RATE: c.sample_rate = value; rebuild = times = true; break;  // SetSampleRate :394-409
      case AD_DEESSER_FREQ: c.freq_hz = value; rebuild = true; break;                     // SetFrequency :228-244
      case AD_DEESSER_Q: c.q = value; rebuild = true; break;                              // SetQ :248-259
      case AD_DEESSER_THRESHOLD: c.threshold_db = value; times = true; break;             // SetThreshold :263-272
      case AD_DEESSER_RATIO: c.ratio = value; times = true; break;                        // SetRatio :276-287
      case AD_DEESSER_KNEE: c.knee_db = value; times = true; break;                       // SetKnee :291-302
      case AD_DEESSER_ATTACK: c.attack_ms = value; times = true; break;                   // SetAttack :306-317
      case AD_DEESSER_RELEASE: c.release_ms = value; times = true; break;                 // SetRelease :321-332
      case AD_DEESSER_RANGE: c.range_db = value; times = true; break;                     // SetRange :336-347
      case AD_DEESSER_ATTACK_COEFF:                                                       // a caller's own exp(...)
      case AD_DEESSER_RELEASE_COEFF:
        if (!(value > 0 && value <= 1)) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "de-esser coefficient must be in (0, 1]");
        (which == AD_DEESSER_ATTACK_COEFF ? c.attack_coeff : c.release_coeff) = value;
        break;
      case AD_DEESSER_MODE: c.mode = whole(value, 0, 1, "de-esser mode invalid"); break;  // SetMode :350-358
      case AD_DEESSER_DETECTOR:                                                           // SetDetector :361-370
        c.detector = whole(value, 0, 1, "de-esser detector invalid");
        rebuild = true;
        break;
      case AD_DEESSER_LISTEN: c.listen = whole(value, 0, 1, "de-esser listen must be 0 or 1"); break;  // SetListen :375
      case AD_DEESSER_FILTER_ORDER:                                                       // SetFilterOrder :381-391
        c.filter_order = whole(value, 1, kDynMaxOrder, "de-esser filter order must be a whole number in [1, 4]");
        rebuild = true;
        break;
      default: AD_FAIL(AD_ERR_INVALID_ARGUMENT, "unknown de-esser parameter");
    }
    validate(c);  // every other field is valid already: the setter's own check, and the Nyquist rule of :235 and :399
    if (times) c.attack_coeff = c.release_coeff = 0;  // updateTimeConstants :573-576 derives both
    const DeessDerived d = deesser_derive(c);
    c.attack_coeff = d.attack;
    c.release_coeff = d.release;
    if (rebuild) deesser_rebuild(f);
    f->cfg = c;
    f->d = d;
  });
}

int ad_deesser_get_config(const ad_deesser* f, ad_deesser_config* cfg) {
  return guard([&] {
    if (!f || !cfg) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "null de-esser handle or config");
    *cfg = f->cfg;
  });
}

int ad_deesser_kernel_info(const ad_deesser* f, int* channels_per_workgroup, int* tile, int* lds_bytes, int* cascades) {
  return with_handle(f, [&] {
    const int mode = deesser_walk_mode(f);
    const bool split = mode == DEESS_SPLIT_ONE || mode == DEESS_SPLIT_TWO;
    const int t = split ? kDynWalkTileMulti : kDynWalkTile;
    if (channels_per_workgroup) *channels_per_workgroup = 64;
    if (tile) *tile = t;
    if (lds_bytes) *lds_bytes = walk_lds_bytes(t, split ? 2 : 1);
    if (cascades) *cascades = mode == DEESS_SPLIT_TWO ? 2 : 1;
  });
}

int ad_deesser_get_state(ad_deesser* f, int channel, double* envelope, double* detect, double* band) {
  return guard([&] {
    check_channel(f, channel);
    DeviceScope ds(f->device);
    f->order.wait_host();
    const size_t per = kDynMaxOrder * 2;
    if (envelope) AD_HIP(hipMemcpy(envelope, f->env.p + channel, sizeof(double), hipMemcpyDeviceToHost));
    if (detect) AD_HIP(hipMemcpy(detect, f->det.p + channel * per, per * sizeof(double), hipMemcpyDeviceToHost));
    if (band) AD_HIP(hipMemcpy(band, f->band.p + channel * per, per * sizeof(double), hipMemcpyDeviceToHost));
  });
}

int ad_deesser_set_state(ad_deesser* f, int channel, double envelope, const double* detect, const double* band) {
  return guard([&] {
    check_channel(f, channel);
    if (!detect || !band) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "null cascade states");
    DeviceScope ds(f->device);
    f->order.wait_host();
    const size_t per = kDynMaxOrder * 2;
    AD_HIP(hipMemcpy(f->env.p + channel, &envelope, sizeof(double), hipMemcpyHostToDevice));
    AD_HIP(hipMemcpy(f->det.p + channel * per, detect, per * sizeof(double), hipMemcpyHostToDevice));
    AD_HIP(hipMemcpy(f->band.p + channel * per, band, per * sizeof(double), hipMemcpyHostToDevice));
    if (std::memcmp(detect, band, per * sizeof(double)) != 0) f->diverged = true;
  });
}

int ad_deesser_metrics(ad_deesser* f, int channel, double* detection_level, double* gain_reduction) {
  return guard([&] {
    check_channel(f, channel);
    DeviceScope ds(f->device);
    f->order.wait_host();
    if (detection_level) AD_HIP(hipMemcpy(detection_level, f->peak.p + channel, sizeof(double), hipMemcpyDeviceToHost));
    if (gain_reduction) AD_HIP(hipMemcpy(gain_reduction, f->gr.p + channel, sizeof(double), hipMemcpyDeviceToHost));
  });
}

int ad_deesser_reset_metrics(ad_deesser* f) {
  // ResetMetrics :504-506
  return with_handle(f, [&] {
    deesser_reset_metrics(f);
  });
}

int ad_deesser_gain(ad_deesser* f, const double* levels, double* gains, int64_t n) {
  return with_handle(f, [&] {
    if (n < 0 || (n > 0 && (!levels || !gains))) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "bad gain buffers");
    if (n == 0) return;
    f->curve.reserve((size_t)n);
    AD_HIP(hipMemcpyAsync(f->curve.p, levels, (size_t)n * sizeof(double), hipMemcpyHostToDevice, f->stream));
    launch_deesser_gain(f->d.gain, f->curve.p, f->curve.p, n, f->stream);
    AD_HIP(hipGetLastError());
    AD_HIP(hipMemcpyAsync(gains, f->curve.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, f->stream));
    AD_HIP(hipStreamSynchronize(f->stream));
  });
}

int ad_deesser_process(ad_deesser* f, double* buf, int64_t n) { return process_host(f, buf, n, deesser_run); }

int ad_deesser_process_device(ad_deesser* f, double* d_buf, int64_t stride, int64_t n, void* stream) {
  return process_device(f, d_buf, stride, n, stream, deesser_run);
}

int ad_deesser_reset(ad_deesser* f) {
  // Reset :485-496: the envelope, both cascades, the metrics; ordered after the last call
  return with_handle(f, [&] {
    f->order.wait_host();
    zero(f->env, f->stream);
    deesser_rebuild(f);
    deesser_reset_metrics(f);
  });
}

void ad_deesser_destroy(ad_deesser* f) { destroy_handle(f); }

}  // extern "C"
