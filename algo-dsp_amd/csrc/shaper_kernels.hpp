// Distortion (dsp/effects/distortion.go:538-797) and bit crusher
// (bit_crusher.go:192-230): launch layouts and argument blocks.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace adsp {

constexpr int kShapeThreads = 256;  // a 16-byte pair per thread and step
constexpr int kShapeSteps = 4;      // pairs per thread
constexpr int kDcTile = 32;         // samples a DC-bypass workgroup stages per chunk
constexpr int kDcPitch = kDcTile + 1;  // odd: the 32 lanes of an LDS access group meet no bank twice
constexpr int kCrushThreads = 256;
constexpr int kCrushSpan = 2048;    // most samples of a row a span workgroup holds in LDS
constexpr int kChebMaxOrder = 16;   // maxChebyshevOrder distortion.go:27

// DistortionMode distortion.go:36-52
enum ShapeMode {
  SHAPE_SOFTCLIP = 0, SHAPE_HARDCLIP, SHAPE_TANH, SHAPE_WS1, SHAPE_WS2, SHAPE_WS3, SHAPE_WS4, SHAPE_WS5, SHAPE_WS6,
  SHAPE_WS7, SHAPE_WS8, SHAPE_SATURATE, SHAPE_SATURATE2, SHAPE_SOFTSAT, SHAPE_CHEBYSHEV,
  SHAPE_MODES
};

// What shapeSample reads, uniform over a launch.  The kernels are instantiated
// per (mode, polynomial, weights active); the rest is data.
struct ShapeParams {
  int mode, poly, has_weights;  // has_weights: a nonzero weight among the first `order` (:690-695)
  int order, invert;
  double bias, drive, output_level, mix, one_minus_mix;
  double clip_level, shape, cheb_gain;
  double scale4, atan_scale4;  // 1 + 4 shape and its atan (Waveshaper5 :625-626)
  double scale6, scale2;       // 1 + 6 shape (Waveshaper7, 8), 1 + 2 shape (Saturate2)
  double w[kChebMaxOrder];
};

// Distortion.ProcessInPlace without DC bypass over [channels][stride], n samples a row, in place.
struct ShapeArgs {
  double* buf;
  int64_t stride, n;
  int channels;
  ShapeParams p;
};
void launch_shape(const ShapeArgs& a, hipStream_t s);

// wet[i] = finite(shapeSample(x[i]) * outputLevel) for device arrays [n]
void launch_shape_curve(const ShapeParams& p, const double* x, double* wet, int64_t n, hipStream_t s);

// Chebyshev mode with dcBypass (:545-547, 730-736): one channel per lane, dc [channels][2] = {dcPrevIn, dcPrevOut}.
struct ShapeDcArgs {
  double* buf;
  int64_t stride, n;
  int channels;
  double* dc;
  ShapeParams p;
};
void launch_shape_dc(const ShapeDcArgs& a, hipStream_t s);

// BitCrusher.ProcessInPlace over [channels][stride], n samples a row, in place.
// The hold counter is the host's: t0 is the call's first update sample
// (max(downsample - 1 - counter, 0)), later ones follow every `downsample`.
// hold_in [channels] is holdValue before the call; a call with an update
// (n > t0) writes the value after it to hold_out, which is another array.
struct CrushArgs {
  double* buf;
  int64_t stride, n, t0;
  int channels, downsample;
  double q, mix, one_minus_mix;
  const double* hold_in;
  double* hold_out;
};
void launch_crush(const CrushArgs& a, hipStream_t s);
// samples of a row a span workgroup owns at this factor: whole hold periods, at most kCrushSpan
inline int64_t crush_span(int downsample) { return (int64_t)(kCrushSpan / downsample) * downsample; }

}  // namespace adsp
