// Feedback delay (dsp/effects/delay.go:139-166), the graph's delay-simple
// (dsp/effectchain/runtime_modulation.go:346-362) and the flanger
// (dsp/effects/modulation/flanger.go:258-282): launch layouts and argument blocks.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace adsp {

constexpr int kDelayTileThreads = 256;  // regime 1: one sample per thread
constexpr int kDelayWalkWaves = 4;      // regime 2: waves per workgroup
constexpr int kFlangerMaxWaves = 4;
constexpr int kFlangerChunkSubs = 8;          // sub-blocks per staged chunk of input
constexpr int kFlangerRingLdsBytes = 32768;   // budget for a workgroup's rings

// largest power of two <= min(b, 64), b >= 1
inline int pow2_sub(int b) {
  int s = 1;
  while (s * 2 <= b && s < 64) s *= 2;
  return s;
}

// One call of the feedback delay: n samples of every channel, in place.  All
// channels share the write position and the delay.  0 <= wp < len.
struct DelayArgs {
  double* buf;  // [channels][stride]
  int64_t stride, n;
  double* ring;        // [channels][len]
  int len, wp;         // wp: the slot sample 0 of the call writes
  const double* traj;  // currentSamples of samples 0 .. ntraj-1 (after their ramp step)
  int64_t ntraj;
  double c_rest;       // currentSamples of every later sample (the ramp's fixed point)
  double feedback, mix, one_minus_mix;
  int pure;            // delay-simple: out = ring[slot], ring[slot] = in (len = D)
  int channels;
};
// Regime 1: samples [t0, t0 + m) of every channel, no sample reading what another writes.
void launch_delay_tile(const DelayArgs& a, int64_t t0, int m, hipStream_t s);
// Regime 2: the whole call, walked in sub-blocks of `sub` samples (a power of two <= 64).
void launch_delay_walk(const DelayArgs& a, int sub, hipStream_t s);

// Rings after a length change (reconfigureBuffer delay.go:220-242,
// reconfigureDelayLine flanger.go:365-387): the newest `keep` samples ending at
// old_wp - 1 go to the end of the new ring, whose write position is 0.  The new
// ring is zeroed by the caller.
void launch_ring_resize(const double* old_ring, int old_len, int old_wp, double* new_ring, int new_len, int keep,
                        int channels, hipStream_t s);

// How a flanger call is laid out: a wave is a tile of `ch_per_wave` channels x
// `sub` samples, a workgroup has `waves` of them and keeps its channels' rings
// in LDS at row pitch `pitch`.
struct FlangerShape {
  int sub, ch_per_wave, waves, pitch, chunk;
  int group() const { return ch_per_wave * waves; }  // channels per workgroup
  int lds_bytes() const { return (group() * pitch + group() * chunk + 3 * chunk) * (int)sizeof(double); }
};
FlangerShape flanger_shape(int block, int len, int channels);

struct FlangerArgs {
  double* buf;  // [channels][stride]
  int64_t stride, n;
  double* ring;  // [channels][len]
  int len, wp;
  const double* phase_in;  // lfoPhase at the call's first sample
  double* phase_out;       // lfoPhase after its last one (another word)
  double base, depth, sample_rate, max_delay;
  double lfo_inc, two_pi;
  double feedback, mix, one_minus_mix;
  int channels;
};
void launch_flanger(const FlangerArgs& a, const FlangerShape& sh, hipStream_t s);

}  // namespace adsp
