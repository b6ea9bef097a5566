// N-way Linkwitz-Riley crossover (crossover.MultiBand, dsp/filter/crossover/
// crossover.go:113-222) and the band sum of dynamics.MultibandCompressor
// (dsp/effects/dynamics/multiband.go:482-488): launch layouts and argument blocks.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace adsp {

constexpr int kXoverMaxStages = 7;     // two-way stages of a network (maxMultibandBands - 1, multiband.go:16)
constexpr int kXoverMaxSections = 12;  // sections per side of a stage: LR24 (maxMultibandOrder, multiband.go:15)
constexpr int kXoverTile = 8;          // samples of every channel a wave stages per step
constexpr int kXoverTileDoubles = 64 * (kXoverTile + 1);  // one tile: 64 rows at the odd pitch
// LDS of a workgroup of `waves` stages, sized by the launch: per stage a
// double-buffered input tile and an LP output tile, and the last stage's HP
// tile.  A tile is 64 * 9 * 8 = 4608 bytes; one stage per launch takes 4 tiles =
// 18432 bytes, the worst case of 7 stages (3 * 7 + 1) tiles = 101376 bytes.
constexpr int xover_lds_bytes(int waves) { return (3 * waves + 1) * kXoverTileDoubles * (int)sizeof(double); }
static_assert(xover_lds_bytes(kXoverMaxStages) <= 160 * 1024,
              "the crossover walk's tiles must fit the 160 KiB of a CU's LDS");
static_assert(64 % kXoverTile == 0, "a staging step covers whole rows");

// Stages [stage_begin, stage_end) of the network over n samples of every
// channel: wave w of a workgroup runs stage stage_begin + w on 64 channels, one
// channel per lane.  The first stage of the launch reads `in` when it is stage
// 0 and band row stage_begin otherwise (in place: its LP goes back there).  LP
// of stage i goes to band row i, the HP of the last stage of the launch to band
// row stage_end.  Band b of channel c starts at bands + b * band_stride +
// c * row_stride.  `in` must not overlap the band rows.
struct XoverWalkArgs {
  const double* in;  // [channels][in_stride]
  int64_t in_stride;
  double* bands;
  int64_t row_stride, band_stride;
  int64_t n;
  const double* coef;  // device [stages][2 (LP, HP)][sections][5] {b0, b1, b2, a1, a2}
  double* state;       // device [channels][stages][2][sections][2] {s0, s1}
  int stages, sections, stage_begin, stage_end, channels;
};
void launch_xover_walk(const XoverWalkArgs& a, hipStream_t s);

// dst = band 0; dst += band 1; ... in band order (multiband.go:482-488), every
// add rounded on its own.  Band 0 is copied, so its -0.0 survives where nothing
// is added.  dst may be anything but a band row.
struct BandSumArgs {
  double* dst;  // [channels][dst_stride]
  int64_t dst_stride;
  const double* bands;
  int64_t row_stride, band_stride;
  int64_t n;
  int nbands, channels;
};
void launch_band_sum(const BandSumArgs& a, hipStream_t s);

}  // namespace adsp
