// C ABI of the FDN reverb (dsp/effects/reverb/fdn_reverb.go).  The handle keeps
// the reference's configuration and derived constants on the host, in plain
// IEEE double as reconfigureDelays / updateFeedbackGains compute them, and
// every channel's delay lines, damping states and the LFO phase on the device.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <memory>
#include <utility>

#include "fdn_kernels.hpp"
#include "fx_handle.hpp"

using namespace adsp;

namespace {

constexpr double kFdnDelaySamples[kFdnLines] = {1537, 1753, 1999, 2251, 2473, 2689, 2851, 3067};  // :24
constexpr double kFdnReferenceRate = 44100.0;                                                      // :21
constexpr int kMinLine = 4;                                                                        // :20
// The reference allocates whatever a sample rate asks for; a line is bounded
// here so that every length and ring index fits an int.
constexpr double kMaxLine = 134217728.0;  // 2^27 samples

const double kTwoPi = 2.0 * M_PI;

double* field(ad_fdn_config& c, int which) {
  switch (which) {
    case AD_FDN_SAMPLE_RATE: return &c.sample_rate;
    case AD_FDN_WET: return &c.wet;
    case AD_FDN_DRY: return &c.dry;
    case AD_FDN_RT60: return &c.rt60_seconds;
    case AD_FDN_DAMP: return &c.damp;
    case AD_FDN_PRE_DELAY: return &c.pre_delay_seconds;
    case AD_FDN_MOD_DEPTH: return &c.mod_depth_seconds;
    case AD_FDN_MOD_RATE: return &c.mod_rate_hz;
  }
  return nullptr;
}

// What SetSampleRate / SetPreDelay / SetModDepth and reconfigureDelays derive (:95-106, :274-301).
struct Derived {
  double base[kFdnLines];  // baseDelaySamples[i] * lineDelayScale
  double mod_depth, pre_delay;  // samples
  int len[kFdnLines], pre_len;
};

// false: a line would be longer than kMaxLine
bool derive(const ad_fdn_config& c, Derived& d) {
  const double scale = c.sample_rate / kFdnReferenceRate;
  d.mod_depth = c.mod_depth_seconds * c.sample_rate;
  d.pre_delay = c.pre_delay_seconds * c.sample_rate;
  for (int i = 0; i < kFdnLines; ++i) {
    d.base[i] = kFdnDelaySamples[i] * scale;
    const double m = std::ceil(d.base[i] + d.mod_depth);
    if (!(m + 3 <= kMaxLine)) return false;
    d.len[i] = std::max((int)m + 3, kMinLine);
  }
  const double m = std::ceil(d.pre_delay);
  if (!(m + 3 <= kMaxLine)) return false;
  d.pre_len = std::max((int)m + 3, kMinLine);
  return true;
}

void validate(const ad_fdn_config& c) {
  // the setters' own checks (:95-186)
  if (!(c.sample_rate > 0) || !is_finite(c.sample_rate)) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "fdn reverb sample rate must be > 0");
  if (!(c.wet >= 0) || !is_finite(c.wet)) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "fdn reverb wet must be >= 0");
  if (!(c.dry >= 0) || !is_finite(c.dry)) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "fdn reverb dry must be >= 0");
  if (!(c.rt60_seconds > 0) || !is_finite(c.rt60_seconds)) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "fdn reverb RT60 must be > 0");
  if (!(c.damp >= 0 && c.damp <= 1)) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "fdn reverb damp must be in [0,1]");
  if (!(c.pre_delay_seconds >= 0) || !is_finite(c.pre_delay_seconds))
    AD_FAIL(AD_ERR_INVALID_ARGUMENT, "fdn reverb pre-delay must be >= 0");
  if (!(c.mod_depth_seconds >= 0) || !is_finite(c.mod_depth_seconds))
    AD_FAIL(AD_ERR_INVALID_ARGUMENT, "fdn reverb mod depth must be >= 0");
  if (!(c.mod_rate_hz >= 0) || !is_finite(c.mod_rate_hz)) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "fdn reverb mod rate must be >= 0");
  Derived d;
  if (!derive(c, d)) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "fdn reverb: a delay line longer than 2^27 samples");
}

void swap_buf(DevBuf<double>& a, DevBuf<double>& b) {
  std::swap(a.p, b.p);
  std::swap(a.n, b.n);
}

}  // namespace

struct ad_fdn : HandleCore {
  ad_fdn_config cfg{};
  Derived d{};
  double fb_gain[kFdnLines] = {};
  int wp[kFdnLines] = {}, pre_wp = 0;  // writePos of every channel's lines (all channels see the same lengths)
  DevBuf<double> line[kFdnLines], pre;  // [channels][len]
  DevBuf<double> fstate;                // [channels][8]
  DevBuf<double> phase;                 // [2]: lfoPhase, ping-pong (cur = phase[ph_cur])
  int ph_cur = 0;
};

namespace {

void update_gains(ad_fdn* f) {  // updateFeedbackGains :303-312
  for (int i = 0; i < kFdnLines; ++i) {
    const double delay_seconds = f->d.base[i] / f->cfg.sample_rate;
    f->fb_gain[i] = std::pow(10.0, -3 * delay_seconds / f->cfg.rt60_seconds);
  }
}

// reconfigureDelays (:274-301) for f->cfg: a line whose length changes is
// replaced by a zeroed one with writePos 0 (resize :320-332), the others keep
// their contents; every filterState is zeroed; the gains are recomputed.  The
// new lines are allocated before anything is replaced.
void reconfigure(ad_fdn* f, const Derived& nd) {
  f->order.wait_host();
  const size_t C = (size_t)f->channels;
  DevBuf<double> fresh[kFdnLines + 1];
  for (int i = 0; i <= kFdnLines; ++i) {
    const int have = i < kFdnLines ? f->d.len[i] : f->d.pre_len;
    const int want = i < kFdnLines ? nd.len[i] : nd.pre_len;
    if (want != have || !(i < kFdnLines ? f->line[i].p : f->pre.p)) fresh[i].alloc(C * want);
  }
  for (int i = 0; i <= kFdnLines; ++i) {
    if (!fresh[i].p) continue;
    swap_buf(i < kFdnLines ? f->line[i] : f->pre, fresh[i]);
    zero(i < kFdnLines ? f->line[i] : f->pre, f->stream);
    (i < kFdnLines ? f->wp[i] : f->pre_wp) = 0;
  }
  zero(f->fstate, f->stream);
  AD_HIP(hipStreamSynchronize(f->stream));
  f->d = nd;
  update_gains(f);
}

int block_of(const ad_fdn* f) {  // max(1, P): consecutive samples whose reads see none of their writes
  const double p = std::floor(f->d.base[0]);
  return p >= 1 ? (int)p : 1;
}
int sub_of(const ad_fdn* f) { return std::min(block_of(f), kFdnMaxSub); }

void fdn_run(ad_fdn* f, double* d_buf, int64_t stride, int64_t n, hipStream_t s) {
  CallScope call(f->order, s);
  FdnArgs a{};
  a.buf = d_buf;
  a.stride = stride;
  a.n = n;
  for (int i = 0; i < kFdnLines; ++i) {
    a.line[i] = f->line[i].p;
    a.len[i] = f->d.len[i];
    a.wp[i] = f->wp[i];
    a.base[i] = f->d.base[i];
    a.offset[i] = (kTwoPi * (double)i) / (double)kFdnLines;  // :209
    a.fb_gain[i] = f->fb_gain[i];
  }
  a.pre = f->pre.p;
  a.pre_len = f->d.pre_len;
  a.pre_wp = f->pre_wp;
  a.fstate = f->fstate.p;
  a.phase_in = f->phase.p + f->ph_cur;
  a.phase_out = f->phase.p + (f->ph_cur ^ 1);
  a.mod_depth = f->d.mod_depth;
  a.pre_delay = f->d.pre_delay;
  a.lfo_inc = kTwoPi * f->cfg.mod_rate_hz / f->cfg.sample_rate;  // :215
  a.two_pi = kTwoPi;
  a.gain = 1 / std::sqrt((double)kFdnLines);  // :81
  a.damp = f->cfg.damp;
  a.one_minus_damp = 1 - f->cfg.damp;
  a.wet = f->cfg.wet;
  a.dry = f->cfg.dry;
  a.sub = sub_of(f);
  launch_fdn(a, f->channels, s);
  AD_HIP(hipGetLastError());
  for (int i = 0; i < kFdnLines; ++i) f->wp[i] = (int)((f->wp[i] + n) % f->d.len[i]);
  if (f->d.pre_delay > 0) f->pre_wp = (int)((f->pre_wp + n) % f->d.pre_len);  // written only then (:202-205)
  f->ph_cur ^= 1;
}

}  // namespace

extern "C" {

void ad_fdn_default_config(ad_fdn_config* cfg, double sample_rate) {
  if (!cfg) return;
  // NewFDNReverb :12-19, :66-92
  cfg->sample_rate = sample_rate;
  cfg->wet = 0.2;
  cfg->dry = 1.0;
  cfg->rt60_seconds = 1.8;
  cfg->damp = 0.3;
  cfg->pre_delay_seconds = 0.01;
  cfg->mod_depth_seconds = 0.002;
  cfg->mod_rate_hz = 0.1;
}

int ad_fdn_validate(const ad_fdn_config* cfg) { return validate_config(cfg, validate); }

int ad_fdn_create(const ad_fdn_config* cfg, int channels, int device, ad_fdn** out) {
  return create_handle(cfg, channels, device, out, validate, [](ad_fdn* f, const ad_fdn_config& c) {
    f->fstate.alloc((size_t)f->channels * kFdnLines);
    f->phase.alloc(2);
    zero(f->phase, f->stream);
    Derived nd;
    derive(c, nd);
    reconfigure(f, nd);
  });
}

int ad_fdn_set_param(ad_fdn* f, int which, double value) {
  return with_handle(f, [&] {
    ad_fdn_config c = f->cfg;
    double* v = field(c, which);
    if (!v) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "unknown fdn reverb parameter");
    *v = value;
    validate(c);
    switch (which) {
      case AD_FDN_SAMPLE_RATE:
      case AD_FDN_PRE_DELAY:
      case AD_FDN_MOD_DEPTH: {  // :95-106, :154-175
        const ad_fdn_config old = f->cfg;
        Derived nd;
        derive(c, nd);
        f->cfg = c;
        try {
          reconfigure(f, nd);
        } catch (...) {
          f->cfg = old;
          throw;
        }
        break;
      }
      case AD_FDN_RT60:  // :131-140
        f->cfg = c;
        update_gains(f);
        break;
      default:  // SetWet, SetDry, SetDamp, SetModRate only store
        f->cfg = c;
    }
  });
}

int ad_fdn_get_config(const ad_fdn* f, ad_fdn_config* cfg) {
  return guard([&] {
    if (!f || !cfg) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "null fdn reverb handle or config");
    *cfg = f->cfg;
  });
}

int ad_fdn_derived(const ad_fdn* f, double feedback_gain[8], int64_t line_len[8], int64_t* pre_len,
                   double* lfo_phase) {
  return with_handle(f, [&] {
    for (int i = 0; i < kFdnLines; ++i) {
      if (feedback_gain) feedback_gain[i] = f->fb_gain[i];
      if (line_len) line_len[i] = f->d.len[i];
    }
    if (pre_len) *pre_len = f->d.pre_len;
    if (lfo_phase) {
      f->order.wait_host();
      AD_HIP(hipMemcpy(lfo_phase, f->phase.p + f->ph_cur, sizeof(double), hipMemcpyDeviceToHost));
    }
  });
}

int ad_fdn_kernel_info(const ad_fdn* f, int* block, int* sub_block, int* lds_bytes) {
  return with_handle(f, [&] {
    if (block) *block = block_of(f);
    if (sub_block) *sub_block = sub_of(f);
    if (lds_bytes) *lds_bytes = fdn_lds_bytes(sub_of(f));
  });
}

int ad_fdn_process(ad_fdn* f, double* buf, int64_t n) { return process_host(f, buf, n, fdn_run); }

int ad_fdn_process_device(ad_fdn* f, double* d_buf, int64_t stride, int64_t n, void* stream) {
  return process_device(f, d_buf, stride, n, stream, fdn_run);
}

int ad_fdn_reset(ad_fdn* f) {
  // Reset :189-197; ordered after the last call, whatever stream it used
  return with_handle(f, [&] {
    f->order.wait_host();
    for (auto& l : f->line) zero(l, f->stream);
    zero(f->pre, f->stream);
    zero(f->fstate, f->stream);
    zero(f->phase, f->stream);
    AD_HIP(hipStreamSynchronize(f->stream));
    for (int& w : f->wp) w = 0;
    f->pre_wp = 0;
  });
}

void ad_fdn_destroy(ad_fdn* f) { destroy_handle(f); }

}  // extern "C"
