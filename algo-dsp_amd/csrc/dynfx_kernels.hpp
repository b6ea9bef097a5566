// Transient shaper (dsp/effects/dynamics/transient_shaper.go:139-170) and
// de-esser (deesser.go:413-475, 513-557): launch layouts and argument blocks.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace adsp {

constexpr int kDynWalkTile = 32;      // samples a walk workgroup stages per chunk with one output row
constexpr int kDynWalkTileMulti = 16; // ... with two or three output rows (the LDS of a workgroup stays under 64 KiB)
constexpr int kDynMaxOrder = 4;       // maxDeEsserFilterOrder deesser.go:72
constexpr int kDynPointThreads = 256; // the pointwise kernels: one sample per thread and step
constexpr int kDynPointSteps = 8;     // samples per thread
constexpr int kDynPointSpan = kDynPointThreads * kDynPointSteps;  // samples of a row a pointwise workgroup covers

// What the de-esser's walk has to run (deesser.go:414-475).
enum DeessWalkMode {
  DEESS_LISTEN = 0,     // the detection cascade alone, written in place (:416-424)
  DEESS_WIDE = 1,       // detection cascade and envelope; bandFilters do not run (:448-449)
  DEESS_SPLIT_ONE = 2,  // split band while both cascades hold equal states: one cascade stands for both
  DEESS_SPLIT_TWO = 3,  // split band with cascades that have diverged: both run
};

// The serial part of both processors over n samples of every channel, one
// channel per lane.  The envelope of sample t goes to env_s[ch][t + 1] and the
// envelope before the call's first sample to env_s[ch][0]; the pointwise
// kernels take everything else from there.
struct DynWalkArgs {
  double* buf;  // [channels][stride]; read only, except DEESS_LISTEN: in place
  int64_t stride, n;
  double* env_s;   // [channels][pitch], pitch >= n + 1
  double* band_s;  // [channels][pitch]: what the band cascade gives at sample t (DEESS_SPLIT_*)
  int64_t pitch;
  double* env;         // [channels] envelope / envLevel
  double* det_state;   // [channels][kDynMaxOrder][2]: d0, d1 of each detection section
  double* band_state;  // [channels][kDynMaxOrder][2]: of each band section
  double* peak;        // [channels] metrics.DetectionLevel
  double attack, release;      // the two envelope coefficients
  double b0, b1, b2, a1, a2;   // the section every stage of both cascades shares
  int order, mode, channels;
};
void launch_transient_walk(const DynWalkArgs& a, hipStream_t s);
void launch_deesser_walk(const DynWalkArgs& a, hipStream_t s);

// transient_shaper.go:151-169 from env_s, in place on buf.
struct TransientPointArgs {
  double* buf;
  int64_t stride, n;
  const double* env_s;
  int64_t pitch;
  double attack_amount, sustain_amount;
  int channels;
};
void launch_transient_point(const TransientPointArgs& a, hipStream_t s);

// calculateGain deesser.go:513-557 with the constants updateCoefficients :559-571 caches.
struct DeessGainParams {
  double threshold_log2, half_knee, inv_knee_width_log2, cf, range_lin;  // cf = 1 - 1/ratio
  int knee_on;                                                           // kneeDB > 0
};

// deesser.go:435-474 from env_s (and band_s), in place on buf; the
// minimum gain of the call goes through part[channels][tiles][2] into gr.
struct DeessPointArgs {
  double* buf;
  int64_t stride, n;
  const double* env_s;
  const double* band_s;  // what the band cascade gave; null in wideband mode
  int64_t pitch;
  DeessGainParams g;
  double band_norm;
  double* part;  // [channels][tiles][2]: the least finite gain, and 1 where a gain was NaN
  double* gr;    // [channels] metrics.GainReduction
  int channels;
};
int deess_point_tiles(int64_t n);
void launch_deesser_point(const DeessPointArgs& a, hipStream_t s);

// The lookahead limiter (lookahead_limiter.go:191-210): the detector's envelope of n samples of buf (the
// sidechain rows, read only) into env_s as the other walks leave it, then the gain times the delayed program.
void launch_limiter_walk(const DynWalkArgs& a, hipStream_t s);
struct LookaheadPointArgs {
  double* buf;  // [channels][stride]: the program, rewritten
  int64_t stride, n;
  const double* prog_s;  // [channels][prog_pitch]: the call's program samples, copied before
  int64_t prog_pitch;
  const double* hist;  // [channels][delay]: the program's last `delay` samples of the calls before
  int64_t delay;       // D = round(lookaheadMs * fs / 1000)
  const double* env_s;
  int64_t pitch;
  DeessGainParams g;  // knee off, range_lin 0: GainForLevel core.go:288-309
  int channels;
};
void launch_lookahead_point(const LookaheadPointArgs& a, hipStream_t s);

// gains[i] = calculateGain(levels[i]) over device arrays [n].
void launch_deesser_gain(const DeessGainParams& g, const double* levels, double* gains, int64_t n, hipStream_t s);

}  // namespace adsp
