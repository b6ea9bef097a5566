// Phaser (dsp/effects/modulation/phaser.go:268-285, 360-379), tremolo
// (tremolo.go:201-217, 291-294) and ring modulator (ring_modulator.go:143-153):
// launch layouts and argument blocks.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace adsp {

constexpr int kModTableThreads = 256;  // one sample per thread
constexpr int kModApplyThreads = 256;  // a 16-byte pair per thread and step
constexpr int kModApplySteps = 4;      // pairs per thread
constexpr int kModSmoothChunk = 1024;  // samples the stepper lane walks between two barriers
constexpr int kPhaserTile = 32;        // samples a phaser workgroup stages per chunk
constexpr int kPhaserPitch = kPhaserTile + 1;  // odd: the 32 lanes of an LDS access group meet no bank twice
constexpr int kPhaserMaxStages = 12;   // maxPhaserStages phaser.go:15

// What the kernels take from a call's phases, one value per sample.
enum ModTableKind {
  MOD_CARRIER = 0,  // sin(phase)                                      ring_modulator.go:144
  MOD_TARGET = 1,   // (1 - depth) + depth * (0.5 * (1 + sin(phase)))  tremolo.go:291-294
  MOD_COEF = 2,     // phaserAllpassCoefficient(modulatedFrequency())  phaser.go:360-379
};
struct ModTableArgs {
  const double* phase;  // [n] the phase of each sample, stepped on the host
  double* out;          // [n]
  int64_t n;
  int kind;
  double depth, one_minus_depth;        // MOD_TARGET
  double min_hz, span_hz, sample_rate;  // MOD_COEF: span = max - min
  double max_allowed, pi;               // MOD_COEF: 0.49 * fs, M_PI
};
void launch_mod_table(const ModTableArgs& a, hipStream_t s);

// tremolo.go:203-207 with a coefficient below 1: tab[t] (the targets) becomes
// currentMod after sample t.  *cur is currentMod before sample 0; it is replaced
// by the value after sample n - 1 when `commit` is set.  One workgroup.
void launch_tremolo_smooth(double* tab, int64_t n, double coef, double* cur, int commit, hipStream_t s);

// out = s * (1 - mix) + (s * tab[t]) * mix over [channels][n], in place
// (tremolo.go:209-216, ring_modulator.go:145-152).
struct ModApplyArgs {
  double* buf;  // [channels][stride]
  int64_t stride, n;
  const double* tab;  // [n]
  double mix, one_minus_mix;
  int channels;
};
void launch_mod_apply(const ModApplyArgs& a, hipStream_t s);

// Phaser.Process over n samples of every channel, in place, one channel per lane.
struct PhaserArgs {
  double* buf;  // [channels][stride]
  int64_t stride, n;
  const double* coef;  // [n]
  double* stage;       // [channels][kPhaserMaxStages][2]: x1, y1 of each stage
  double* fb;          // [channels] feedbackSample
  double feedback, mix, one_minus_mix;
  int stages, channels;
};
void launch_phaser(const PhaserArgs& a, hipStream_t s);

}  // namespace adsp
