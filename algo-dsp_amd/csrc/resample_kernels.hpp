// Rational polyphase resampler (dsp/resample/resample.go:249-292): the launch
// plan fixed at create and the kernel's argument block.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace adsp {

constexpr int kRsR = 4;                   // outputs per lane, W apart
constexpr int kRsLanes = 256;             // workgroup size when any size fits the ratio
constexpr int kRsMaxLanes = 512;          // workgroup size, at most
constexpr int kRsPF = 8;                  // window samples a lane can hold ahead in registers
constexpr int64_t kRsLdsBudget = 65536;   // bytes of LDS a workgroup may take (table + window)
constexpr int64_t kRsWinReserve = 8192;   // of those, kept for the window when the table is placed

// Row pitch of the phase-major table: odd, so that lanes on different phases
// read different LDS banks (a pitch of 32 doubles would put every row on bank 0).
inline int64_t rs_pitch(int64_t T) { return T | 1; }

// Everything about a launch that depends on (up, down, T) alone.
struct ResamplePlan {
  int lanes = 0;          // W: a multiple of `up` (resample_plan), or 256 when up > 256
  int share = 0;          // W % up == 0: a lane's kRsR outputs share one phase
  int tab_lds = 0;        // coefficient table staged in LDS (else read from global / L2)
  int win_lds = 0;        // input window staged in LDS (else read from global)
  int tiles_per_wg = 1;   // consecutive tiles one workgroup walks (amortises the table staging)
  int prefetch = 0;       // the next tile's window is loaded while the current tile computes
  int64_t wlen = 0;       // window capacity in samples
  int64_t lds_bytes = 0;  // dynamic LDS per workgroup
  int64_t tile() const { return (int64_t)lanes * kRsR; }
};
ResamplePlan resample_plan(int64_t up, int64_t down, int64_t T);

// One call over X = [hist (T-1) | block (n_in)] per channel.  Output j reads
// X[ii0 + (phase0 + j*down) / up - k], k = 0 .. T-1, against row
// (phase0 + j*down) % up of the table.
struct ResampleArgs {
  const double* tab;   // [up][pitch]
  int64_t up, down;
  int T, pitch;
  const double* hist;  // [channels][T-1]: the delay line before this block
  const double* src;   // [channels][sstride]: the new samples
  int64_t sstride;
  double* y;           // [channels][ystride]: n_out outputs
  int64_t ystride, n_out;
  int64_t phase0, ii0;  // of output 0: phase, and index into X of its newest sample
  int channels;
};
void launch_resample(const ResamplePlan& p, const ResampleArgs& a, hipStream_t s);

}  // namespace adsp
