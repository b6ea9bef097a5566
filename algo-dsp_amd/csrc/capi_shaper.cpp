// C ABI of the distortion (dsp/effects/distortion.go) and the bit crusher
// (bit_crusher.go).  A handle keeps the reference's configuration on the host
// and hands the kernels an argument block per call: the constants the
// reference recomputes per sample (atan(1 + 4 shape), 1 + 6 shape, 1 + 2 shape,
// 1 - mix, exp2(bitDepth - 1)) are computed here once, with the C library.
// The distortion's two DC-bypass states per channel and the bit crusher's hold
// value per channel live on the device; the bit crusher's hold counter is the
// same for every channel and does not depend on the input, so the host keeps it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>

#include "fx_handle.hpp"
#include "shaper_kernels.hpp"

using namespace adsp;

namespace {

void validate(const ad_distortion_config& c) {  // the setters :364-529, validate :590-605
  if (!(c.sample_rate > 0) || !is_finite(c.sample_rate))
    AD_FAIL(AD_ERR_INVALID_ARGUMENT, "distortion sample rate must be > 0 and finite");
  if (c.mode < 0 || c.mode >= SHAPE_MODES) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "distortion mode is invalid");
  if (c.approx < 0 || c.approx > 1) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "distortion approximation mode is invalid");
  if (!in_range(c.drive, 0.01, 20)) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "distortion drive must be in [0.01, 20]");
  if (!in_range(c.mix, 0, 1)) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "distortion mix must be in [0, 1]");
  if (!in_range(c.output_level, 0, 4)) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "distortion output level must be in [0, 4]");
  if (!in_range(c.clip_level, 0.05, 1)) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "distortion clip level must be in [0.05, 1]");
  if (!in_range(c.shape, 0, 1)) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "distortion shape must be in [0, 1]");
  if (!in_range(c.bias, -1, 1)) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "distortion bias must be in [-1, 1]");
  if (!in_range(c.cheb_gain, 0, 4)) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "chebyshev gain level must be in [0, 4]");
  if (c.cheb_order < 1 || c.cheb_order > kChebMaxOrder)
    AD_FAIL(AD_ERR_INVALID_ARGUMENT, "chebyshev order must be in [1, 16]");
  if (c.cheb_harmonic < 0 || c.cheb_harmonic > 2) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "chebyshev harmonic mode is invalid");
  // validateChebyshevParity :750-767
  if (c.cheb_harmonic == 1 && c.cheb_order % 2 == 0)
    AD_FAIL(AD_ERR_INVALID_ARGUMENT, "chebyshev odd harmonic mode requires odd order");
  if (c.cheb_harmonic == 2 && c.cheb_order % 2 != 0)
    AD_FAIL(AD_ERR_INVALID_ARGUMENT, "chebyshev even harmonic mode requires even order");
  if ((c.cheb_invert != 0 && c.cheb_invert != 1) || (c.cheb_dc_bypass != 0 && c.cheb_dc_bypass != 1))
    AD_FAIL(AD_ERR_INVALID_ARGUMENT, "chebyshev invert and DC bypass are 0 or 1");
  for (int k = 0; k < kChebMaxOrder; ++k)
    if (!is_finite(c.cheb_weights[k])) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "chebyshev weights must be finite");
}

void validate(const ad_bitcrusher_config& c) {  // NewBitCrusher :108-111, the setters :137-183
  if (!(c.sample_rate > 0) || !is_finite(c.sample_rate))
    AD_FAIL(AD_ERR_INVALID_ARGUMENT, "bit crusher sample rate must be > 0 and finite");
  if (!in_range(c.bit_depth, 1, 32)) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "bit crusher bit depth must be in [1, 32]");
  if (c.downsample < 1 || c.downsample > 256)
    AD_FAIL(AD_ERR_INVALID_ARGUMENT, "bit crusher downsample factor must be in [1, 256]");
  if (!in_range(c.mix, 0, 1)) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "bit crusher mix must be in [0, 1]");
}

// What the kernels read, from a valid configuration
ShapeParams shape_params(const ad_distortion_config& c) {
#pragma clang fp contract(off)
  ShapeParams p{};
  p.mode = c.mode;
  p.poly = c.approx == 1;
  p.order = c.cheb_order;
  p.invert = c.cheb_invert;
  p.has_weights = 0;
  for (int k = 0; k < c.cheb_order; ++k)  // :690-695: the first `order` slots only
    if (c.cheb_weights[k] != 0) p.has_weights = 1;
  p.bias = c.bias;
  p.drive = c.drive;
  p.output_level = c.output_level;
  p.mix = c.mix;
  p.one_minus_mix = 1 - c.mix;
  p.clip_level = c.clip_level;
  p.shape = c.shape;
  p.cheb_gain = c.cheb_gain;
  p.scale4 = 1 + 4 * c.shape;
  p.atan_scale4 = std::atan(p.scale4);
  p.scale6 = 1 + 6 * c.shape;
  p.scale2 = 1 + 2 * c.shape;
  std::memcpy(p.w, c.cheb_weights, sizeof(p.w));
  return p;
}

}  // namespace

struct ad_distortion : HandleCore {
  ad_distortion_config cfg{};
  DevBuf<double> dc;  // [channels][2] dcPrevIn, dcPrevOut
};

struct ad_bitcrusher : HandleCore {
  ad_bitcrusher_config cfg{};
  double q = 0;          // quantLevels, updateQuantLevels :222-224
  int counter = 0;       // holdCounter
  DevBuf<double> hold;   // [2][channels] holdValue: a call with an update reads one half and writes the other
  int cur = 0;           // the half that holds holdValue now
};

namespace {

void distortion_run(ad_distortion* f, double* d_buf, int64_t stride, int64_t n, hipStream_t s) {
  CallScope call(f->order, s);
  const ShapeParams p = shape_params(f->cfg);
  if (f->cfg.mode == SHAPE_CHEBYSHEV && f->cfg.cheb_dc_bypass) {  // :545-547
    ShapeDcArgs a{};
    a.buf = d_buf;
    a.stride = stride;
    a.n = n;
    a.channels = f->channels;
    a.dc = f->dc.p;
    a.p = p;
    launch_shape_dc(a, s);
  } else {
    ShapeArgs a{};
    a.buf = d_buf;
    a.stride = stride;
    a.n = n;
    a.channels = f->channels;
    a.p = p;
    launch_shape(a, s);
  }
  AD_HIP(hipGetLastError());
}

// the first update sample of a call that starts with the counter at c0
int64_t first_update(int downsample, int c0) { return std::max(downsample - 1 - c0, 0); }

void bitcrusher_run(ad_bitcrusher* f, double* d_buf, int64_t stride, int64_t n, hipStream_t s) {
  CallScope call(f->order, s);
  const int ds = f->cfg.downsample;
  const int64_t t0 = first_update(ds, f->counter);
  CrushArgs a{};
  a.buf = d_buf;
  a.stride = stride;
  a.n = n;
  a.t0 = t0;
  a.channels = f->channels;
  a.downsample = ds;
  a.q = f->q;
  a.mix = f->cfg.mix;
  a.one_minus_mix = 1 - f->cfg.mix;
  a.hold_in = f->hold.p + (size_t)f->cur * f->channels;
  a.hold_out = f->hold.p + (size_t)(f->cur ^ 1) * f->channels;
  launch_crush(a, s);
  AD_HIP(hipGetLastError());
  if (n > t0) {  // the call holds an update: its last one left holdValue in the other half
    f->cur ^= 1;
    f->counter = (int)((n - 1 - t0) % ds);
  } else {
    f->counter += (int)n;
  }
}

}  // namespace

extern "C" {

// ---- ad_distortion ----------------------------------------------------------
void ad_distortion_default_config(ad_distortion_config* cfg, double sample_rate) {
  if (!cfg) return;
  *cfg = ad_distortion_config{};  // defaultDistortionConfig :91-107: soft clip, exact, no weights
  cfg->sample_rate = sample_rate;
  cfg->drive = 1.0;
  cfg->mix = 1.0;
  cfg->output_level = 1.0;
  cfg->clip_level = 1.0;
  cfg->shape = 0.5;
  cfg->bias = 0.0;
  cfg->cheb_gain = 1.0;
  cfg->cheb_order = 3;
}

int ad_distortion_validate(const ad_distortion_config* cfg) { return validate_config(cfg, validate); }

int ad_distortion_create(const ad_distortion_config* cfg, int channels, int device, ad_distortion** out) {
  return create_handle(cfg, channels, device, out, validate, [](ad_distortion* f, const ad_distortion_config&) {
    f->dc.alloc((size_t)f->channels * 2);
    zero(f->dc, f->stream);
  });
}

int ad_distortion_set_param(ad_distortion* f, int which, double value) {
  return with_handle(f, [&] {
    ad_distortion_config c = f->cfg;
    switch (which) {
      case AD_DISTORTION_SAMPLE_RATE: c.sample_rate = value; break;    // SetSampleRate :365-373
      case AD_DISTORTION_DRIVE: c.drive = value; break;                // SetDrive :398-406
      case AD_DISTORTION_MIX: c.mix = value; break;                    // SetMix :409-417
      case AD_DISTORTION_OUTPUT_LEVEL: c.output_level = value; break;  // SetOutputLevel :420-429
      case AD_DISTORTION_CLIP_LEVEL: c.clip_level = value; break;      // SetClipLevel :432-441
      case AD_DISTORTION_SHAPE: c.shape = value; break;                // SetShape :444-452
      case AD_DISTORTION_BIAS: c.bias = value; break;                  // SetBias :455-463
      case AD_DISTORTION_CHEB_GAIN: c.cheb_gain = value; break;        // SetChebyshevGainLevel :493-502
      case AD_DISTORTION_MODE:                                         // SetMode :376-384
        c.mode = whole(value, 0, SHAPE_MODES - 1, "distortion mode is invalid");
        break;
      case AD_DISTORTION_APPROX:  // SetApproxMode :387-395
        c.approx = whole(value, 0, 1, "distortion approximation mode is invalid");
        break;
      case AD_DISTORTION_CHEB_ORDER:  // SetChebyshevOrder :466-474
        c.cheb_order = whole(value, 1, kChebMaxOrder, "chebyshev order must be a whole number in [1, 16]");
        break;
      case AD_DISTORTION_CHEB_HARMONIC:  // SetChebyshevHarmonicMode :477-485
        c.cheb_harmonic = whole(value, 0, 2, "chebyshev harmonic mode is invalid");
        break;
      case AD_DISTORTION_CHEB_INVERT:  // SetChebyshevInvert :488-490
        c.cheb_invert = whole(value, 0, 1, "chebyshev invert is 0 or 1");
        break;
      case AD_DISTORTION_CHEB_DC_BYPASS:  // SetChebyshevDCBypass :505-507
        c.cheb_dc_bypass = whole(value, 0, 1, "chebyshev DC bypass is 0 or 1");
        break;
      default: AD_FAIL(AD_ERR_INVALID_ARGUMENT, "unknown distortion parameter");
    }
    validate(c);  // every other field is valid already: the setter's own check and the parity rule
    f->cfg = c;
  });
}

int ad_distortion_set_weights(ad_distortion* f, const double* w, int n) {
  return with_handle(f, [&] {  // SetChebyshevWeights :514-529
    if (n < 0 || n > kChebMaxOrder || (n > 0 && !w))
      AD_FAIL(AD_ERR_INVALID_ARGUMENT, "chebyshev weights length must be <= 16");
    for (int k = 0; k < n; ++k)
      if (!is_finite(w[k])) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "chebyshev weights must be finite");
    std::memset(f->cfg.cheb_weights, 0, sizeof(f->cfg.cheb_weights));
    if (n > 0) std::memcpy(f->cfg.cheb_weights, w, (size_t)n * sizeof(double));
  });
}

int ad_distortion_get_config(const ad_distortion* f, ad_distortion_config* cfg) {
  return guard([&] {
    if (!f || !cfg) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "null distortion handle or config");
    *cfg = f->cfg;
  });
}

int ad_distortion_derived(const ad_distortion* f, double* atan_scale, double* scale6, double* scale2,
                          double* one_minus_mix, int* weights_active) {
  return with_handle(f, [&] {
    const ShapeParams p = shape_params(f->cfg);
    if (atan_scale) *atan_scale = p.atan_scale4;
    if (scale6) *scale6 = p.scale6;
    if (scale2) *scale2 = p.scale2;
    if (one_minus_mix) *one_minus_mix = p.one_minus_mix;
    if (weights_active) *weights_active = p.has_weights;
  });
}

int ad_distortion_kernel_info(const ad_distortion* f, int* samples_per_workgroup, int* dc_channels_per_workgroup,
                              int* dc_tile, int* dc_lds_bytes) {
  return with_handle(f, [&] {
    if (samples_per_workgroup) *samples_per_workgroup = 2 * kShapeThreads * kShapeSteps;
    if (dc_channels_per_workgroup) *dc_channels_per_workgroup = 64;
    if (dc_tile) *dc_tile = kDcTile;
    if (dc_lds_bytes) *dc_lds_bytes = 3 * 64 * kDcPitch * (int)sizeof(double);
  });
}

int ad_distortion_curve(ad_distortion* f, const double* x, int64_t n, double* wet) {
  return with_handle(f, [&] {
    if (n < 0 || (n > 0 && (!x || !wet))) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "bad curve buffers");
    if (n == 0) return;
    DevBuf<double> dx, dw;  // a plot, not a hot path: buffers of its own, so no call's staging is touched
    dx.alloc((size_t)n);
    dw.alloc((size_t)n);
    AD_HIP(hipMemcpyAsync(dx.p, x, (size_t)n * sizeof(double), hipMemcpyHostToDevice, f->stream));
    launch_shape_curve(shape_params(f->cfg), dx.p, dw.p, n, f->stream);
    AD_HIP(hipGetLastError());
    AD_HIP(hipMemcpyAsync(wet, dw.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, f->stream));
    AD_HIP(hipStreamSynchronize(f->stream));
  });
}

int ad_distortion_process(ad_distortion* f, double* buf, int64_t n) { return process_host(f, buf, n, distortion_run); }

int ad_distortion_process_device(ad_distortion* f, double* d_buf, int64_t stride, int64_t n, void* stream) {
  return process_device(f, d_buf, stride, n, stream, distortion_run);
}

int ad_distortion_reset(ad_distortion* f) {
  // Reset :532-535: dcPrevIn, dcPrevOut; ordered after the last call
  return with_handle(f, [&] {
    f->order.wait_host();
    zero(f->dc, f->stream);
    AD_HIP(hipStreamSynchronize(f->stream));
  });
}

void ad_distortion_destroy(ad_distortion* f) { destroy_handle(f); }

// ---- ad_bitcrusher ----------------------------------------------------------
void ad_bitcrusher_default_config(ad_bitcrusher_config* cfg, double sample_rate) {
  if (!cfg) return;
  *cfg = ad_bitcrusher_config{};
  cfg->sample_rate = sample_rate;  // defaultBitCrusherConfig :26-32
  cfg->bit_depth = 8.0;
  cfg->mix = 1.0;
  cfg->downsample = 1;
}

int ad_bitcrusher_validate(const ad_bitcrusher_config* cfg) { return validate_config(cfg, validate); }

int ad_bitcrusher_create(const ad_bitcrusher_config* cfg, int channels, int device, ad_bitcrusher** out) {
  return create_handle(cfg, channels, device, out, validate, [](ad_bitcrusher* f, const ad_bitcrusher_config& c) {
    f->q = std::exp2(c.bit_depth - 1);
    f->hold.alloc((size_t)f->channels * 2);
    zero(f->hold, f->stream);
  });
}

int ad_bitcrusher_set_param(ad_bitcrusher* f, int which, double value) {
  return with_handle(f, [&] {
    ad_bitcrusher_config c = f->cfg;
    switch (which) {
      case AD_BITCRUSHER_SAMPLE_RATE: c.sample_rate = value; break;  // SetSampleRate :138-146
      case AD_BITCRUSHER_BIT_DEPTH: c.bit_depth = value; break;      // SetBitDepth :149-160
      case AD_BITCRUSHER_MIX: c.mix = value; break;                  // SetMix :175-183
      case AD_BITCRUSHER_DOWNSAMPLE:                                 // SetDownsample :163-172
        c.downsample = whole(value, 1, 256, "bit crusher downsample factor must be a whole number in [1, 256]");
        break;
      default: AD_FAIL(AD_ERR_INVALID_ARGUMENT, "unknown bit crusher parameter");
    }
    validate(c);
    f->cfg = c;
    if (which == AD_BITCRUSHER_BIT_DEPTH) f->q = std::exp2(c.bit_depth - 1);
  });
}

int ad_bitcrusher_get_config(const ad_bitcrusher* f, ad_bitcrusher_config* cfg) {
  return guard([&] {
    if (!f || !cfg) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "null bit crusher handle or config");
    *cfg = f->cfg;
  });
}

int ad_bitcrusher_derived(ad_bitcrusher* f, int channel, double* quant_levels, int* counter, double* hold_value) {
  return guard([&] {
    check_channel(f, channel);
    if (quant_levels) *quant_levels = f->q;
    if (counter) *counter = f->counter;
    if (hold_value) {
      DeviceScope ds(f->device);
      f->order.wait_host();
      AD_HIP(hipMemcpy(hold_value, f->hold.p + (size_t)f->cur * f->channels + channel, sizeof(double),
                       hipMemcpyDeviceToHost));
    }
  });
}

int ad_bitcrusher_kernel_info(const ad_bitcrusher* f, int* samples_per_workgroup, int* span, int* lds_bytes) {
  return with_handle(f, [&] {
    const bool pointwise = f->cfg.downsample == 1;
    if (samples_per_workgroup)
      *samples_per_workgroup = pointwise ? 2 * kShapeThreads * kShapeSteps : (int)crush_span(f->cfg.downsample);
    if (span) *span = pointwise ? 0 : (int)crush_span(f->cfg.downsample);
    if (lds_bytes) *lds_bytes = pointwise ? 0 : kCrushSpan * (int)sizeof(double);
  });
}

int ad_bitcrusher_process(ad_bitcrusher* f, double* buf, int64_t n) { return process_host(f, buf, n, bitcrusher_run); }

int ad_bitcrusher_process_device(ad_bitcrusher* f, double* d_buf, int64_t stride, int64_t n, void* stream) {
  return process_device(f, d_buf, stride, n, stream, bitcrusher_run);
}

int ad_bitcrusher_reset(ad_bitcrusher* f) {
  // Reset :186-189: holdCounter = 0, holdValue = 0; ordered after the last call
  return with_handle(f, [&] {
    f->order.wait_host();
    zero(f->hold, f->stream);
    AD_HIP(hipStreamSynchronize(f->stream));
    f->counter = 0;
  });
}

void ad_bitcrusher_destroy(ad_bitcrusher* f) { destroy_handle(f); }

}  // extern "C"
