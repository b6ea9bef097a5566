// crossover.MultiBand.ProcessBlock (dsp/filter/crossover/crossover.go:194-215)
// for many channels that share one network, in the reference's operation order
// (every product and sum rounded on its own, no FMA), and the band sum of
// dynamics.MultibandCompressor.ProcessInPlace (multiband.go:482-488).
//
// Stage i filters its input with an LP and an HP cascade of S sections each
// (biquad.Section.ProcessSample section.go:47-53); the LP output is band i, the
// HP output is the input of stage i + 1.  The chain of stages is serial per
// channel, so the walk is a pipeline over time tiles:
//   k_xover_walk     a workgroup is 64 channels by (stage_end - stage_begin)
//                    waves.  Wave w runs stage stage_begin + w, one channel per
//                    lane with its 4 S state doubles in registers, on tile
//                    k - w at step k.  Wave 0 stages its input through an LDS
//                    tile at an odd row pitch as k_dyn_walk does, so that
//                    consecutive lanes read consecutive samples of a row; every
//                    wave stores its LP tile the same way; the HP tile goes to
//                    the next wave through an LDS ring of two tiles and never
//                    to global memory, except the last stage's, which is the
//                    top band.  Two LDS barriers per step: before the walk
//                    (the inputs are whole) and after it (the outputs are).
//                    A launch of one stage is the sequential form: stage i > 0
//                    reads band row i, where stage i - 1 left its HP, and
//                    overwrites it with its LP; a lane stores the elements it
//                    loaded itself, one tile after loading them.
//   k_band_sum       pointwise, 16-byte accesses where every row allows them.
//
// Every global index is guarded by the row's length and the channel count.
#include "xover_kernels.hpp"

#include <algorithm>

#include "ad_common.hpp"

namespace adsp {
namespace {

// A workgroup barrier that orders the LDS accesses only: global loads and stores in flight stay in flight.
__device__ __forceinline__ void lds_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// The coefficient table is written before the launch and only read by it: through the constant address
// space a wave-uniform read of it is a scalar load, and the table takes no vector registers.
typedef const double __attribute__((address_space(4))) * ConstTable;

// biquad.Section.ProcessSample section.go:47-53 through a cascade of S sections.  First-order sections
// (b2 = a2 = 0) run the same recurrence: their zero products carry the sign of zero and an infinity's NaN.
template <int S>
__device__ __forceinline__ double cascade(ConstTable c, double x, double (&s0)[S], double (&s1)[S]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int i = 0; i < S; ++i) {
    const double b0 = c[i * 5], b1 = c[i * 5 + 1], b2 = c[i * 5 + 2], a1 = c[i * 5 + 3], a2 = c[i * 5 + 4];
    const double y = b0 * x + s0[i];
    s0[i] = b1 * x - a1 * y + s1[i];
    s1[i] = b2 * x - a2 * y;
    x = y;
  }
  return x;
}

template <int S>
__global__ __launch_bounds__(64 * kXoverMaxStages) void k_xover_walk(XoverWalkArgs a) {
#pragma clang fp contract(off)
  constexpr int T = kXoverTile, P = T + 1;  // P odd: the lanes of an LDS access group meet no bank twice
  constexpr int kRows = 64 / T;             // rows a staging step of a wave covers
  constexpr int kSteps = 64 / kRows;        // staging steps per tile
  // sized by the launch (xover_lds_bytes): per wave two input tiles and an LP tile, then the last wave's HP tile
  extern __shared__ __attribute__((aligned(16))) double tiles[];
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int nw = a.stage_end - a.stage_begin;
  typedef double Tile[kXoverTileDoubles];
  Tile(*in_t)[2] = reinterpret_cast<Tile(*)[2]>(tiles);             // [nw][2]
  Tile* lp_t = reinterpret_cast<Tile*>(tiles) + 2 * nw;             // [nw]
  double* hp_t = tiles + (int64_t)3 * nw * kXoverTileDoubles;       // the last wave's
  const int stage = a.stage_begin + w;
  const bool first = w == 0, last = w == nw - 1;
  const int64_t ch0 = (int64_t)blockIdx.x * 64;
  const int count = (int)(a.channels - ch0 < 64 ? a.channels - ch0 : 64);
  const bool active = lane < count;
  const int64_t ch = ch0 + (active ? lane : 0);

  const ConstTable coef = (ConstTable)(uintptr_t)(a.coef + (int64_t)stage * 2 * S * 5);  // uniform over the wave
  double* st = a.state + ((ch * a.stages + stage) * 2) * S * 2;
  double l0[S], l1[S], h0[S], h1[S];
#pragma unroll
  for (int i = 0; i < S; ++i) {
    l0[i] = st[i * 2], l1[i] = st[i * 2 + 1];
    h0[i] = st[(S + i) * 2], h1[i] = st[(S + i) * 2 + 1];
  }

  // staging: consecutive lanes take consecutive samples of a row; step k covers rows k * kRows + rl
  const int tl = lane % T, rl = lane / T;
  const double* src = a.stage_begin == 0 ? a.in : a.bands + (int64_t)a.stage_begin * a.band_stride;
  const int64_t src_stride = a.stage_begin == 0 ? a.in_stride : a.row_stride;
  src += (ch0 + rl) * src_stride + tl;
  double* lp_g = a.bands + (int64_t)stage * a.band_stride + (ch0 + rl) * a.row_stride + tl;
  double* hp_g = a.bands + (int64_t)(stage + 1) * a.band_stride + (ch0 + rl) * a.row_stride + tl;

  const int64_t ntiles = (a.n + T - 1) / T;
  const int64_t nsteps = ntiles + nw - 1;
  double v[kSteps];
  if (first) {
    const int m = (int)(a.n < T ? a.n : T);
#pragma unroll
    for (int k = 0; k < kSteps; ++k)
      v[k] = (k * kRows + rl < count && tl < m) ? src[(int64_t)k * kRows * src_stride] : 0.0;
  }
  for (int64_t step = 0; step < nsteps; ++step) {
    const int64_t j = step - w;  // this wave's tile
    const bool work = j >= 0 && j < ntiles;
    if (first && work) {
#pragma unroll
      for (int k = 0; k < kSteps; ++k) in_t[0][j & 1][(k * kRows + rl) * P + tl] = v[k];
    }
    lds_barrier();  // every wave's input tile is whole
    if (first && j + 1 < ntiles) {  // the next tile's loads fly during the walk
      const int64_t t1 = (j + 1) * T;
      const int m1 = (int)(a.n - t1 < T ? a.n - t1 : T);
#pragma unroll
      for (int k = 0; k < kSteps; ++k)
        v[k] = (k * kRows + rl < count && tl < m1) ? src[(int64_t)k * kRows * src_stride + t1] : 0.0;
    }
    const int64_t t0 = j * T;
    const int m = work ? (int)(a.n - t0 < T ? a.n - t0 : T) : 0;
    if (work) {
      const double* x_t = in_t[w][j & 1] + lane * P;
      double* lo_t = lp_t[w] + lane * P;
      double* hi_t = (last ? hp_t : in_t[last ? 0 : w + 1][j & 1]) + lane * P;
      double sv[T];
#pragma unroll
      for (int t = 0; t < T; ++t) sv[t] = x_t[t];
#pragma unroll
      for (int t = 0; t < T; ++t) {
        if (t >= m) break;
        lo_t[t] = cascade<S>(coef, sv[t], l0, l1);           // crossover.go:70
        hi_t[t] = cascade<S>(coef + S * 5, sv[t], h0, h1);
      }
    }
    lds_barrier();  // every wave's output tiles are whole
    if (work) {
#pragma unroll
      for (int k = 0; k < kSteps; ++k)
        if (k * kRows + rl < count && tl < m)
          lp_g[(int64_t)k * kRows * a.row_stride + t0] = lp_t[w][(k * kRows + rl) * P + tl];
      if (last) {
#pragma unroll
        for (int k = 0; k < kSteps; ++k)
          if (k * kRows + rl < count && tl < m)
            hp_g[(int64_t)k * kRows * a.row_stride + t0] = hp_t[(k * kRows + rl) * P + tl];
      }
    }
  }
  if (active) {
#pragma unroll
    for (int i = 0; i < S; ++i) {
      st[i * 2] = l0[i], st[i * 2 + 1] = l1[i];
      st[(S + i) * 2] = h0[i], st[(S + i) * 2 + 1] = h1[i];
    }
  }
}

constexpr int kSumThreads = 256;

template <bool VEC>
__global__ __launch_bounds__(kSumThreads) void k_band_sum(BandSumArgs a, int tiles) {
#pragma clang fp contract(off)
  const int64_t c = blockIdx.x / tiles;
  const int64_t t = ((int64_t)(blockIdx.x % tiles) * kSumThreads + threadIdx.x) * 2;
  if (t >= a.n) return;
  const double* b = a.bands + c * a.row_stride + t;
  double* d = a.dst + c * a.dst_stride + t;
  if (VEC && t + 1 < a.n) {
    double2 acc = *reinterpret_cast<const double2*>(b);  // copy(buf, bandBlocks[0]) :482
    for (int k = 1; k < a.nbands; ++k) {
      const double2 x = *reinterpret_cast<const double2*>(b + (int64_t)k * a.band_stride);
      acc.x = acc.x + x.x;  // buf[j] += v :484-488
      acc.y = acc.y + x.y;
    }
    *reinterpret_cast<double2*>(d) = acc;
    return;
  }
  const int m = t + 1 < a.n ? 2 : 1;
  for (int q = 0; q < m; ++q) {
    double acc = b[q];
    for (int k = 1; k < a.nbands; ++k) acc = acc + b[(int64_t)k * a.band_stride + q];
    d[q] = acc;
  }
}

}  // namespace

void launch_xover_walk(const XoverWalkArgs& a, hipStream_t s) {
  const int nw = a.stage_end - a.stage_begin;
  if (a.n <= 0 || a.channels <= 0 || nw <= 0) return;
  const dim3 grid((unsigned)((a.channels + 63) / 64)), block((unsigned)(64 * nw));
  const int lds = xover_lds_bytes(nw);
  switch (a.sections) {
    // more than 64 KiB of dynamic LDS (5 waves and up) has to be allowed per kernel first
#define ADSP_XOVER_CASE(S)                                                                                  \
  case S:                                                                                                   \
    if (lds > 64 * 1024)                                                                                    \
      AD_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_xover_walk<S>),                           \
                                 hipFuncAttributeMaxDynamicSharedMemorySize, lds));                         \
    k_xover_walk<S><<<grid, block, lds, s>>>(a);                                                            \
    break;
    ADSP_XOVER_CASE(1)
    ADSP_XOVER_CASE(2)
    ADSP_XOVER_CASE(3)
    ADSP_XOVER_CASE(4)
    ADSP_XOVER_CASE(5)
    ADSP_XOVER_CASE(6)
    ADSP_XOVER_CASE(7)
    ADSP_XOVER_CASE(8)
    ADSP_XOVER_CASE(9)
    ADSP_XOVER_CASE(10)
    ADSP_XOVER_CASE(11)
    ADSP_XOVER_CASE(12)
#undef ADSP_XOVER_CASE
  }
}

void launch_band_sum(const BandSumArgs& a, hipStream_t s) {
  if (a.n <= 0 || a.channels <= 0 || a.nbands <= 0) return;
  const int tiles = (int)((a.n + 2 * kSumThreads - 1) / (2 * kSumThreads));
  const dim3 grid((unsigned)((int64_t)a.channels * tiles));
  const bool vec = ((reinterpret_cast<uintptr_t>(a.dst) | reinterpret_cast<uintptr_t>(a.bands)) & 15) == 0 &&
                   ((a.dst_stride | a.row_stride | a.band_stride) & 1) == 0;
  if (vec)
    k_band_sum<true><<<grid, dim3(kSumThreads), 0, s>>>(a, tiles);
  else
    k_band_sum<false><<<grid, dim3(kSumThreads), 0, s>>>(a, tiles);
}

}  // namespace adsp
