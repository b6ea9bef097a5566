// C ABI of the lookahead limiter (dsp/effects/dynamics/lookahead_limiter.go).
// A handle keeps the reference's configuration on the host and derives what
// the Compressor core caches (the detector coefficients core.go:486-487, the
// gain computer's log2-domain threshold :521) there with the C library.  The
// envelope and the delay line's history live on the device, one per channel.
//
// Processing is in place, and the delayed multiply of sample t reads the
// program at t - D: a thread writing out[t] would race the thread that reads
// in[t] for sample t + D.  So a call first copies its program samples to a
// scratch row (prog_s); the pointwise pass reads only that copy and the
// history, and writes only the caller's rows.  The history of the next call,
// the last D samples of [history | prog_s], goes to the other buffer of a
// ping-pong pair (delay_line_next), so nothing a kernel of the call reads is
// written by it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <memory>

#include "dynfx_kernels.hpp"
#include "fx_handle.hpp"

using namespace adsp;

namespace {

constexpr double kLog2Of10Div20 = 0.166096404744;    // compressor.go:27 (truncated literal, kept)
constexpr int kScratchRows = 3;  // env_s, prog_s, side_s

void validate(const ad_lookahead_config& c) {
  if (!(c.sample_rate > 0) || !is_finite(c.sample_rate))
    AD_FAIL(AD_ERR_INVALID_ARGUMENT, "lookahead limiter sample rate must be positive and finite");
  if (!in_range(c.threshold_db, -24, 0)) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "lookahead limiter threshold must be in [-24, 0]");
  if (!in_range(c.release_ms, 1, 5000)) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "lookahead limiter release must be in [1, 5000]");
  if (!in_range(c.lookahead_ms, 0, 200)) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "lookahead limiter lookahead must be in [0, 200]");
}

struct Derived {
  double attack, release;
  DeessGainParams gain;
  int64_t delay;
};

Derived derive(const ad_lookahead_config& c) {
  Derived d{};
  d.attack = 1.0 - std::exp(-M_LN2 / (0.1 * 0.001 * c.sample_rate));         // SetAttack(0.1) :52, core.go:486
  d.release = std::exp(-M_LN2 / (c.release_ms * 0.001 * c.sample_rate));     // core.go:487
  d.gain.threshold_log2 = c.threshold_db * kLog2Of10Div20;                   // core.go:521
  d.gain.knee_on = 0;                                                        // SetKnee(0) :57
  d.gain.cf = 1.0 - 1.0 / 100.0;                                             // SetRatio(100) :47, core.go:296
  d.gain.range_lin = 0.0;                                                    // no floor: a gain is never below 0
  d.delay = std::max<int64_t>((int64_t)std::round(c.lookahead_ms * c.sample_rate / 1000.0), 0);  // :233, halves away from 0
  return d;
}

}  // namespace

struct ad_lookahead : HandleCore {
  ad_lookahead_config cfg{};
  Derived d{};
  DevBuf<double> env;             // [channels]
  DevBuf<double> hist[2];         // [channels][delay]: the ping-pong pair; hist[cur] holds the history
  int cur = 0;
  DevBuf<double> env_s, prog_s, side_s;  // [channels][pitch] of one pass
  int64_t last_n = -1, last_pitch = 0;   // the last call, where one pass took it
  DevBuf<double> curve;                  // ad_lookahead_gain
};

namespace {

// rebuildDelayBuffer :232-239: a new zeroed line, whatever the length was
void rebuild_delay(ad_lookahead* f, int64_t delay) {
  f->order.wait_host();
  const size_t count = (size_t)f->channels * (size_t)delay;
  for (auto& h : f->hist) {
    h.alloc(count);
    zero(h, f->stream);
  }
  AD_HIP(hipStreamSynchronize(f->stream));
  f->cur = 0;
}

void run(ad_lookahead* f, double* d_buf, int64_t stride, const double* d_side, int64_t side_stride, int64_t side_n,
         int64_t n, hipStream_t s) {
  CallScope call(f->order, s);
  const int64_t D = f->d.delay, C = f->channels;
  const int64_t seg = scratch_segment(n, f->channels, kScratchRows);
  f->env_s.reserve((size_t)C * (seg + 1));  // hipFree waits for the device, so no earlier call still reads the old one
  f->prog_s.reserve((size_t)C * seg);
  for (int64_t off = 0; off < n; off += seg) {
    const int64_t m = std::min(seg, n - off);
    // the detector's input: the program itself, the sidechain rows, or those padded with zeros in scratch
    const double* det = d_buf + off;
    int64_t det_stride = stride;
    if (d_side) {
      const int64_t have = std::max<int64_t>(0, std::min(m, side_n - off));
      if (have == m) {
        det = d_side + off;
        det_stride = side_stride;
      } else {  // :223-226
        f->side_s.reserve((size_t)C * seg);
        AD_HIP(hipMemsetAsync(f->side_s.p, 0, (size_t)C * seg * sizeof(double), s));
        if (have > 0)
          AD_HIP(hipMemcpy2DAsync(f->side_s.p, seg * sizeof(double), d_side + off, side_stride * sizeof(double),
                                  have * sizeof(double), (size_t)C, hipMemcpyDeviceToDevice, s));
        det = f->side_s.p;
        det_stride = seg;
      }
    }
    DynWalkArgs w{};
    w.buf = const_cast<double*>(det);  // the limiter's walk reads it only
    w.stride = det_stride;
    w.n = m;
    w.env_s = f->env_s.p;
    w.pitch = seg + 1;
    w.env = f->env.p;
    w.attack = f->d.attack;
    w.release = f->d.release;
    w.channels = f->channels;
    launch_limiter_walk(w, s);
    AD_HIP(hipMemcpy2DAsync(f->prog_s.p, seg * sizeof(double), d_buf + off, stride * sizeof(double), m * sizeof(double),
                            (size_t)C, hipMemcpyDeviceToDevice, s));
    LookaheadPointArgs p{};
    p.buf = d_buf + off;
    p.stride = stride;
    p.n = m;
    p.prog_s = f->prog_s.p;
    p.prog_pitch = seg;
    p.hist = f->hist[f->cur].p;
    p.delay = D;
    p.env_s = f->env_s.p;
    p.pitch = seg + 1;
    p.g = f->d.gain;
    p.channels = f->channels;
    launch_lookahead_point(p, s);
    delay_line_next(f->hist[f->cur ^ 1].p, f->hist[f->cur].p, D, f->prog_s.p, seg, m, (size_t)C, s);
    if (D > 0) f->cur ^= 1;
  }
  AD_HIP(hipGetLastError());
  f->last_n = n <= seg ? n : -1;
  f->last_pitch = seg + 1;
}

}  // namespace

extern "C" {

void ad_lookahead_default_config(ad_lookahead_config* cfg, double sample_rate) {
  if (!cfg) return;
  *cfg = ad_lookahead_config{};
  cfg->sample_rate = sample_rate;  // lookahead_limiter.go:9-11
  cfg->threshold_db = -0.1;
  cfg->release_ms = 100.0;
  cfg->lookahead_ms = 3.0;
}

int ad_lookahead_validate(const ad_lookahead_config* cfg) { return validate_config(cfg, validate); }

int ad_lookahead_derived(const ad_lookahead_config* cfg, double* attack_coeff, double* release_coeff,
                         double* threshold_log2, int64_t* delay_samples) {
  return guard([&] {
    if (!cfg) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "null lookahead limiter config");
    validate(*cfg);
    const Derived d = derive(*cfg);
    if (attack_coeff) *attack_coeff = d.attack;
    if (release_coeff) *release_coeff = d.release;
    if (threshold_log2) *threshold_log2 = d.gain.threshold_log2;
    if (delay_samples) *delay_samples = d.delay;
  });
}

int ad_lookahead_create(const ad_lookahead_config* cfg, int channels, int device, ad_lookahead** out) {
  return create_handle(cfg, channels, device, out, validate, [](ad_lookahead* f, const ad_lookahead_config& c) {
    f->d = derive(c);
    f->env.alloc((size_t)f->channels);
    zero(f->env, f->stream);
    rebuild_delay(f, f->d.delay);
  });
}

int ad_lookahead_set_param(ad_lookahead* f, int which, double value) {
  return with_handle(f, [&] {
    ad_lookahead_config c = f->cfg;
    switch (which) {
      case AD_LOOKAHEAD_SAMPLE_RATE: c.sample_rate = value; break;  // SetSampleRate :146-161
      case AD_LOOKAHEAD_THRESHOLD: c.threshold_db = value; break;   // SetThreshold :99-113
      case AD_LOOKAHEAD_RELEASE: c.release_ms = value; break;       // SetRelease :116-130
      case AD_LOOKAHEAD_LOOKAHEAD: c.lookahead_ms = value; break;   // SetLookahead :133-143
      default: AD_FAIL(AD_ERR_INVALID_ARGUMENT, "unknown lookahead limiter parameter");
    }
    validate(c);  // every other field is valid already: the setter's own check
    const Derived d = derive(c);
    if (which == AD_LOOKAHEAD_SAMPLE_RATE || which == AD_LOOKAHEAD_LOOKAHEAD) rebuild_delay(f, d.delay);
    f->cfg = c;
    f->d = d;
  });
}

int ad_lookahead_get_config(const ad_lookahead* f, ad_lookahead_config* cfg) {
  return guard([&] {
    if (!f || !cfg) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "null lookahead limiter handle or config");
    *cfg = f->cfg;
  });
}

int ad_lookahead_get_state(ad_lookahead* f, int channel, double* envelope) {
  return guard([&] {
    check_channel(f, channel);
    if (!envelope) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "null state output");
    DeviceScope ds(f->device);
    f->order.wait_host();
    AD_HIP(hipMemcpy(envelope, f->env.p + channel, sizeof(double), hipMemcpyDeviceToHost));
  });
}

int ad_lookahead_gain(ad_lookahead* f, const double* levels, double* gains, int64_t n) {
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

int ad_lookahead_last_envelope(ad_lookahead* f, double* envelope, int64_t n) {
  return guard([&] {
    if (!f || !envelope) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "null lookahead limiter handle or output");
    if (f->last_n < 0 || n != f->last_n) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "no call of that length to report");
    if (n == 0) return;
    DeviceScope ds(f->device);
    f->order.wait_host();
    AD_HIP(hipMemcpy2D(envelope, n * sizeof(double), f->env_s.p + 1, f->last_pitch * sizeof(double), n * sizeof(double),
                       (size_t)f->channels, hipMemcpyDeviceToHost));
  });
}

int ad_lookahead_process(ad_lookahead* f, double* program, const double* sidechain, int64_t side_n, int64_t n) {
  return with_handle(f, [&] {
    if (n < 0 || (n > 0 && !program) || side_n < 0) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "bad buffer");
    if (n == 0) return;
    const size_t count = (size_t)f->channels * n, side_count = sidechain ? (size_t)f->channels * side_n : 0;
    f->order.wait_host();
    f->io.reserve(count + side_count + 1);
    AD_HIP(hipMemcpyAsync(f->io.p, program, count * sizeof(double), hipMemcpyHostToDevice, f->stream));
    const double* d_side = nullptr;
    if (sidechain) {
      d_side = f->io.p + count;  // never null, also for an empty sidechain: it reads as zeros
      if (side_count)
        AD_HIP(hipMemcpyAsync(f->io.p + count, sidechain, side_count * sizeof(double), hipMemcpyHostToDevice, f->stream));
    }
    run(f, f->io.p, n, d_side, side_n, side_n, n, f->stream);
    AD_HIP(hipMemcpyAsync(program, f->io.p, count * sizeof(double), hipMemcpyDeviceToHost, f->stream));
    AD_HIP(hipStreamSynchronize(f->stream));
  });
}

int ad_lookahead_process_device(ad_lookahead* f, double* d_buf, int64_t stride, const double* d_side, int64_t side_stride,
                                int64_t side_n, int64_t n, void* stream) {
  return with_handle(f, [&] {
    if (n < 0 || (n > 0 && (!d_buf || stride < n))) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "bad buffer geometry");
    if (d_side && (side_n < 0 || side_stride < side_n)) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "bad sidechain geometry");
    if (n == 0) return;
    if (d_side && side_n > 0) {
      const double* a_end = d_buf + (int64_t)(f->channels - 1) * stride + n;
      const double* b_end = d_side + (int64_t)(f->channels - 1) * side_stride + side_n;
      if (d_buf < b_end && d_side < a_end)
        AD_FAIL(AD_ERR_INVALID_ARGUMENT, "lookahead limiter: the sidechain rows overlap the program rows");
    }
    run(f, d_buf, stride, d_side, side_stride, side_n, n, reinterpret_cast<hipStream_t>(stream));
  });
}

int ad_lookahead_reset(ad_lookahead* f) {
  // Reset :176-183: the core's envelope and the delay line; ordered after the last call
  return with_handle(f, [&] {
    f->order.wait_host();
    zero(f->env, f->stream);
    rebuild_delay(f, f->d.delay);
  });
}

void ad_lookahead_destroy(ad_lookahead* f) { destroy_handle(f); }

}  // extern "C"
