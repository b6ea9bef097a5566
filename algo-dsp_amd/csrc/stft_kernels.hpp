// Short-frame STFT overlap-add for many channels (effects.SpectralFreeze,
// pitch.SpectralPitchShifter): launchers of stft_kernels.hip.
//
// One scratch row per (channel, frame) of kStftPitch(N) = N + 2 doubles holds
// the frame's magnitudes [0, N/2] and phases [N/2 + 1, N + 1] between the
// analysis and the synthesis, and the windowed time frame [0, N) after it:
// the synthesis reads its own row whole before it writes it.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace adsp {

constexpr int kStftMinFrame = 64;
constexpr int kStftMaxFrame = 4096;
constexpr double kStftNormFloor = 1e-12;  // spectral_freeze.go:17, pitch_shift_spectral.go:19

inline int64_t stft_pitch(int frame) { return (int64_t)frame + 2; }

enum StftFrameMode {
  STFT_ANALYSIS = 0,  // x -> window -> FFT -> pinned DC/Nyquist -> hypot, atan2 -> mag, phase
  STFT_SYNTH = 1,     // mag, phase -> mag cos, mag sin -> mirror -> IFFT -> window -> row
  STFT_FUSED = 2      // analysis and synthesis of a frame with nothing written in between
};

struct StftFrameArgs {
  const double* x;   // [channels] rows of n samples (ANALYSIS, FUSED)
  int64_t x_stride;
  int64_t n;
  const double* win;  // [N]
  int hop;            // frame j starts at j * hop
  int channels;
  int64_t frames;     // frames per channel
  // ANALYSIS writes, SYNTH reads: bin k of (c, j) at mag[c * mag_ch + j * mag_fr + k], phase likewise
  double* mag;
  int64_t mag_ch, mag_fr;
  double* phase;
  int64_t ph_ch, ph_fr;
  // SYNTH, FUSED write: sample i of (c, j) at rows[c * row_ch + j * row_fr + i]
  double* rows;
  int64_t row_ch, row_fr;
};
void launch_stft_frames(int frame, int mode, const StftFrameArgs& a, hipStream_t s);

enum StftWalkMode { STFT_WALK_BINSHIFT = 0, STFT_WALK_STRETCH = 1 };

// The phase vocoder's walk over the frames of each channel, in place on the
// scratch rows: magnitudes become shiftedMag (bin shift; unchanged for the
// stretch), phases become sumPhase.
struct StftWalkArgs {
  double* rows;  // [channels][frames][pitch]
  int64_t row_ch, row_fr;
  const double* omega;  // [N/2 + 1], 2*math.Pi*float64(k)/float64(N) from the host
  int channels;
  int64_t frames;
  double hop_f;        // float64(analysisHop)
  double syn_hop_f;    // float64(synthesisHop) (stretch)
  double ratio;        // pitchRatio (bin shift)
};
void launch_stft_walk(int frame, int mode, const StftWalkArgs& a, hipStream_t s);

// The frozen frames' phases: phaseAcc += omega * hop once per frame (Advance)
// but the first frame of a call that has just captured, written per frame.
struct StftFreezeWalkArgs {
  double* rows;  // phases at rows[c * row_ch + j * row_fr + bins + k]
  int64_t row_ch, row_fr;
  double* phase_acc;    // [channels][bins]
  const double* omega;  // [bins]
  int bins;
  int channels;
  int64_t frames;
  double hop_f;
  int advance;        // SpectralFreezePhaseAdvance
  int just_captured;  // frame 0 of this call is the captured frame
};
void launch_stft_freeze_walk(const StftFreezeWalkArgs& a, hipStream_t s);

// Overlap-add as a gather: out[c][i] = sum over the frames that cover i, in
// ascending frame order, of rows[c][j][i - j * hop]; norm the same way from
// win^2; the floor test; then the mix with the dry sample (mix_dry) or the sum
// alone.
struct StftOlaArgs {
  const double* rows;
  int64_t row_ch, row_fr;
  const double* win;
  int frame;  // N
  int hop;    // synthesis hop
  int64_t frames;
  double* out;  // [channels] rows of out_n samples
  int64_t out_stride;
  int64_t out_n;
  int channels;
  int mix_dry;  // out = out * (1 - mix) + wet * mix
  double mix;
  int norm_only;  // out = norm (a test entry)
};
void launch_stft_ola(const StftOlaArgs& a, hipStream_t s);

}  // namespace adsp
