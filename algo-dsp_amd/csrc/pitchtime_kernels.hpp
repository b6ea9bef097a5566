// Kernels of the time-domain pitch shifter (dsp/effects/pitch/pitch_shifter.go):
// a WSOLA stretch (timeStretch :298-357, findBestOverlap :359-389) into scratch
// rows and a 4-point Hermite resample (pitchResampleHermite :391-419) back into
// the caller's rows.  See pitchtime_kernels.hip for the decomposition.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "ad_common.hpp"

namespace adsp {

// ---- the handle (capi_pitchtime.cpp) -------------------------------------------
// The effect reaches a caller as the AD_FXN_PITCHTIME node of an fx graph, so its create / process / reset /
// destroy are the graph's to call and no entry points of the C ABI.
struct PitchTime;
int pitchtime_validate(const ad_pitchtime_config* cfg);
int pitchtime_create(const ad_pitchtime_config* cfg, int channels, int device, PitchTime** out);
int pitchtime_process_device(PitchTime* p, double* d_buf, int64_t stride, int64_t n, void* stream);
int pitchtime_reset(PitchTime* p);
void pitchtime_destroy(PitchTime* p);

// ---- the kernels ---------------------------------------------------------------

constexpr int kPtThreads = 256;                    // threads of a search workgroup
constexpr int kPtR = 4;                            // candidates a lane owns (blocked_dot.hpp's R)
constexpr int kPtTile = kPtThreads * kPtR;         // candidates of a workgroup: one tile of the search range
constexpr int kPtTerms = 1024;                     // overlap terms the LDS window holds at a time
constexpr int kPtWindow = kPtTile + kPtTerms + 4 * kPtR;  // LDS doubles: the window, its lead element, the over-read
constexpr int kPtNone = 0x7fffffff;                // "no candidate has won" (every score NaN or -Inf)

// One group of channels of one call.  Rows are per channel; `state` holds what a frame hands to the next.
struct PtArgs {
  const double* in;   // [channels][stride]: the caller's rows (read by the stretch, written by the resample)
  int64_t stride, n;
  double* out;        // [channels][out_pitch]: the stretched rows; the frames write all of [0, targetLen)
  int64_t out_pitch;
  double* ref;        // [channels][ref_pitch]: the reference segment of the coming frame
  int64_t ref_pitch;
  double* ref_energy;   // [channels]
  int64_t* prev_start;  // [channels]
  int* done;            // [channels]: the loop's break (:344) was taken
  double* tile_score;   // [channels][tiles]: a tile's winner, kPtNone where it has none
  int* tile_cand;       // [channels][tiles]: relative to the frame's searchStart
  const double* fade_in;  // [overlap]
  int sequence, overlap, search, tiles, channels;
};

// frame 0: out[0 .. sequence) = the input's first samples, prevStart = 0, and the first reference segment
void launch_pt_first(const PtArgs& a, hipStream_t s);
// findBestOverlap of one frame for every channel: one workgroup per (channel, tile)
void launch_pt_search(const PtArgs& a, int64_t predicted, hipStream_t s);
// the rest of the frame: the winner across tiles, the cross-fade at out_start, the body, the exit test
// (`may_break`: outLen >= targetLen holds after this frame) and the next reference segment
void launch_pt_assemble(const PtArgs& a, int64_t predicted, int64_t out_start, int may_break, hipStream_t s);

// mode 0: out[i] = Hermite4 at pos[i] of src[0 .. len) with clamped reads; mode 1: out[i] = src[0] (len(input) == 1,
// :397-402, and outLen == 1, :405-408, where n is 1)
void launch_pt_resample(const double* src, int64_t src_pitch, int64_t len, const double* pos, double* out, int64_t stride,
                        int64_t n, int channels, int mode, hipStream_t s);

}  // namespace adsp
