// Long-block overlap-save plan: one real FFT of N = N1 x N2
// points per block and hop N - K + 1, instead of UPOLS's 2L-point spectra per
// hop L.  With n = N2 n1 + n2 and k = k1 + N1 k2:
//   A  columns: real N1-point FFT over n1 for each n2; rows k1 = 0 .. N1/2 of
//      the intermediate T[k1][n2] are kept (the rest is their mirror);
//   B  rows: T[k1][.] *= W_N^(n2 k1), complex N2-point FFT over n2 (bins
//      X[k1 + N1 k2]), times the IR's row, inverse FFT, conjugate twiddle;
//   C  columns: complex-to-real inverse N1-point FFT per column, the block's
//      last `hop` samples stored.
// H (the IR's spectrum in the same layout, scaled by 1/N) is built by A and
// the forward half of B.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace adsp {

constexpr int kLongN1 = 512;    // column transform
constexpr int kLongN2 = 4096;   // row transform
constexpr int kLongW = 16;      // columns per A / C item
constexpr int64_t kLongN = (int64_t)kLongN1 * kLongN2;
constexpr int kLongRows = kLongN1 / 2 + 1;
constexpr int kLongPitch = kLongN2 + 8;  // row pitch of T and H, off the power of two

// Bounds of the tile I/O of A and C.  Point e of a block, 0 <= e < kLongN, is
// element origin + e of the signal (A) or of the output (C), valid in [lo, hi).
// long_block_range() turns that into the block's own terms once per item:
// valid <=> r.lo <= e < r.hi, in 32 bits.
//
// One global load or store instruction of a tile covers kLongTileRows rows of
// kLongW columns: instruction i of tile `tile` holds the points first + kLongN2
// r + col, r < kLongTileRows, col < kLongW, first = kLongW tile + kLongTileStep
// i.  It is wholly inside the range (no per-lane test) iff first >= r.lo and
// first + kLongTileSpan < r.hi, wholly outside (no access) iff first +
// kLongTileSpan < r.lo or first >= r.hi, and takes the per-lane test otherwise.
// Both conditions are runs of i, which long_tile_bounds() works out once per
// item from scalars; long_tile_class() is then one unsigned compare per run.
// kLongTileStep > kLongTileSpan, so the spans of an item's instructions are
// disjoint and each end of the range makes at most one of them straddle.
constexpr int kLongTileRows = 256 / kLongW;
constexpr int kLongTileStepLog2 = 16;
constexpr int kLongTileStep = kLongTileRows * kLongN2;                     // from one instruction's first point to the next's
constexpr int kLongTileSpan = (kLongTileRows - 1) * kLongN2 + kLongW - 1;  // from its first point to its last
static_assert(kLongTileStep == 1 << kLongTileStepLog2, "long_tile_bounds divides by shifting");
struct LongBlockRange {
  int lo, hi;
};
__host__ __device__ constexpr LongBlockRange long_block_range(int64_t origin, int64_t lo, int64_t hi) {
  const int64_t a = lo - origin, b = hi - origin;
  const int l = (int)(a < 0 ? 0 : a > kLongN ? kLongN : a);
  const int h = (int)(b < 0 ? 0 : b > kLongN ? kLongN : b);
  return h > l ? LongBlockRange{l, h} : LongBlockRange{0, 0};
}
__host__ __device__ constexpr bool long_point_valid(int e, LongBlockRange r) {
  return (unsigned)(e - r.lo) < (unsigned)(r.hi - r.lo);
}
// instructions in_first .. + in_count - 1 are inside, those of any_first .. +
// any_count - 1 touch the range at all (the arithmetic shift is a floor)
struct LongTileBounds {
  int in_first, in_count, any_first, any_count;
};
__host__ __device__ constexpr LongTileBounds long_tile_bounds(int tile, LongBlockRange r) {
  const int t = tile * kLongW;
  const int in_first = (r.lo - t + kLongTileStep - 1) >> kLongTileStepLog2;
  const int in_last = (r.hi - 1 - kLongTileSpan - t) >> kLongTileStepLog2;
  const int any_first = (r.lo - kLongTileSpan - t + kLongTileStep - 1) >> kLongTileStepLog2;
  const int any_last = (r.hi - 1 - t) >> kLongTileStepLog2;
  const int in_count = in_last - in_first + 1, any_count = any_last - any_first + 1;
  return {in_first, in_count > 0 ? in_count : 0, any_first, any_count > 0 ? any_count : 0};
}
__host__ __device__ constexpr bool long_tile_inside(int i, LongTileBounds b) {
  return (unsigned)(i - b.in_first) < (unsigned)b.in_count;
}
__host__ __device__ constexpr bool long_tile_touched(int i, LongTileBounds b) {
  return (unsigned)(i - b.any_first) < (unsigned)b.any_count;
}
// the touched instructions that are not inside, in rising order: the one after i
// (start from any_first - 1, stop at any_first + any_count)
__host__ __device__ constexpr int long_tile_next_straddling(int i, LongTileBounds b) {
  ++i;
  return b.in_count > 0 && i == b.in_first ? i + b.in_count : i;
}
enum LongTileClass : int { kLongTileInside = 0, kLongTileOutside = 1, kLongTileStraddle = 2 };
__host__ __device__ constexpr LongTileClass long_tile_class(int i, LongTileBounds b) {
  return long_tile_inside(i, b) ? kLongTileInside : long_tile_touched(i, b) ? kLongTileStraddle : kLongTileOutside;
}
__host__ __device__ constexpr int long_tile_first(int tile, int i) { return tile * kLongW + i * kLongTileStep; }
// C at K = 131072 (skip = 31 rows and 4095 columns), a full block: the first
// stored point is the last element of instruction 1 of the last tile
static_assert(long_tile_class(1, long_tile_bounds(kLongN2 / kLongW - 1, long_block_range(-131071, 0, kLongN - 131071))) ==
                      kLongTileStraddle &&
                  long_tile_class(1, long_tile_bounds(kLongN2 / kLongW - 2, long_block_range(-131071, 0, kLongN - 131071))) ==
                      kLongTileOutside &&
                  long_tile_class(2, long_tile_bounds(0, long_block_range(-131071, 0, kLongN - 131071))) == kLongTileInside,
              "tile bounds at the bench's own skip");

struct LongColArgs {
  // A: block j of row c reads x[c][start + j hop + i], i < N; indices outside [0, n) are zeros
  const double* x;
  int64_t x_stride, n, start, hop;
  int blocks, channels;
  double2* T;  // [channels * blocks][kLongRows][kLongPitch]
  // C: point i >= skip of block j goes to y[c][j hop + i - skip], below out_len
  double* y;
  int64_t y_stride, out_len, skip;
};

struct LongRowArgs {
  double2* T;
  int blocks, channels;
  const double2* H;      // [n_ir][kLongRows][kLongPitch]
  const int* ir_index;   // [channels]
  double2* Hout;         // build mode: the scaled forward spectrum goes here
  double scale;
};

void launch_long_cols_fwd(const LongColArgs& a, hipStream_t s);
void launch_long_rows(const LongRowArgs& a, bool build_h, hipStream_t s);
void launch_long_cols_inv(const LongColArgs& a, hipStream_t s);

}  // namespace adsp
