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
