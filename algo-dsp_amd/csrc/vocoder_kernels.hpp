// Vocoder (dsp/effects/vocoder.go:578-630): launch layout, device tables and
// the argument block.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace adsp {

constexpr int kVocBands = 32;           // AD_VOCODER_MAX_BANDS: a band per lane of a half wave
constexpr int kVocTile = 64;            // samples per chunk: the sum phase gives every lane of the wave one
constexpr int kVocPitch = kVocTile + 1; // odd row pitch of the product tiles
// LDS of a workgroup (one wave, one channel): the modulator and carrier chunk, and the env / syn product tiles
constexpr int kVocLdsBytes = (2 * kVocTile + 2 * kVocBands * kVocPitch) * (int)sizeof(double);

// Device tables of a handle, by band: rows of kVocBands doubles.
enum VocTabRow {
  VOC_ANALYSIS = 0,    // 5 rows {b0, b1, b2, a1, a2}: analysisFilters
  VOC_SYNTHESIS = 5,   // synthesisFilters
  VOC_DECIMATED = 10,  // downsampleAnalysisFilters
  VOC_ANTIALIAS = 15,  // downsampleGroupAAFilters of the band's group
  VOC_DS_ATTACK = 20,  // downsampleAttackCoeffs
  VOC_DS_RELEASE = 21, // downsampleReleaseCoeffs
  VOC_TAB_ROWS = 22,
};
// Integer tables by band: rows of kVocBands ints.
enum VocIntRow {
  VOC_MASK = 0,   // downsampleGroupMasks of the band's group
  VOC_GROUP = 1,  // the band's group
  VOC_FIRST = 2,  // 1 on the first band of its group: the lane that saves the group's anti-alias state
  VOC_INT_ROWS = 3,
};
// State of a channel: rows of kVocBands doubles.
enum VocStateRow {
  VOC_S_ANALYSIS = 0,   // s0, s1 by band
  VOC_S_SYNTHESIS = 2,
  VOC_S_DECIMATED = 4,
  VOC_S_ENV = 6,
  VOC_S_ANTIALIAS = 7,  // s0, s1 by group
  VOC_STATE_ROWS = 9,
};

struct VocArgs {
  const double* mod;  // [channels][mod_stride]
  const double* car;  // [channels][car_stride]
  double* out;        // [channels][out_stride]; may be mod or car exactly
  int64_t mod_stride, car_stride, out_stride, n;
  double* state;      // [channels][VOC_STATE_ROWS][kVocBands]
  const double* tab;  // [VOC_TAB_ROWS][kVocBands]
  const int* itab;    // [VOC_INT_ROWS][kVocBands]
  double attack, release;                          // attackCoeff, releaseCoeff (full rate)
  double vocoder_level, synth_level, input_level;  // :629
  int num_bands, channels;
  int cnt0, cnt_mask;  // downsampleCount at the call's first sample; downsampleMax - 1
};
void launch_vocoder(const VocArgs& a, bool downsample, hipStream_t s);

}  // namespace adsp
