// FDN reverb (dsp/effects/reverb/fdn_reverb.go:199-241): the launch layout and
// the kernel's argument block.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace adsp {

constexpr int kFdnLines = 8;       // fdnSize
constexpr int kFdnThreads = 512;   // one wave per delay line
constexpr int kFdnMaxSub = 240;    // samples per sub-block, at most (38.5 KB of LDS: four workgroups per CU)

// Row pitch of the [line][sample] LDS arrays: odd, so that the eight lanes of
// the serial damping loop (one line each, same sample) read eight different banks.
__host__ __device__ inline int fdn_pitch(int sub) { return sub | 1; }
inline int fdn_lds_bytes(int sub) { return (4 * sub + 2 * kFdnLines * fdn_pitch(sub)) * (int)sizeof(double); }

// One call: n samples of every channel, in place.  Everything that
// reconfigureDelays / updateFeedbackGains derive (fdn_reverb.go:274-312) comes
// from the host as data.  Ring positions are already reduced: 0 <= wp[i] < len[i].
struct FdnArgs {
  double* buf;        // [channels][stride]
  int64_t stride, n;
  double* line[kFdnLines];  // [channels][len[i]]: the delay lines' rings
  int len[kFdnLines];       // buffer lengths; the read clamp is len - 3
  int wp[kFdnLines];        // writePos of each line at the call's first sample
  double* pre;        // [channels][pre_len]: the pre-delay line's ring
  int pre_len, pre_wp;
  double* fstate;     // [channels][8] filterState
  const double* phase_in;  // lfoPhase at the call's first sample
  double* phase_out;       // lfoPhase after the call's last sample (another word: workgroups start at different times)
  double base[kFdnLines];    // baseDelaySamples[i] * lineDelayScale
  double offset[kFdnLines];  // 2 pi i / 8
  double fb_gain[kFdnLines];
  double mod_depth, pre_delay;  // in samples
  double lfo_inc, two_pi;
  double gain;                  // 1/sqrt(8): input, output and matrix scale
  double damp, one_minus_damp, wet, dry;
  int sub;                      // samples per sub-block, <= min(kFdnMaxSub, every len[i])
};
void launch_fdn(const FdnArgs& a, int channels, hipStream_t s);

}  // namespace adsp
