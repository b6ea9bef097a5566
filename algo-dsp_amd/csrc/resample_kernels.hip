// HIP kernel of the rational polyphase resampler for gfx950.
//
// Reference semantics (dsp/resample/resample.go:249-292, Process): with the
// state (phase, inputIndex) the loop emits
//   y = sum_k phases[phase][k] * x[inputIndex - k]        k ascending from y = 0
// (a rounded product, then a rounded add; terms before the stream start are
// skipped) and advances phase += down; inputIndex += phase / up; phase %= up.
// In closed form the j-th output of a call has num = phase0 + j*down, input
// index inputIndex0 + num / up and phase num % up, which makes the loop
// output-parallel.  A zero-filled T-1 delay line stands for the skipped terms:
// +0 + (c * 0) is +0, so the bits are the same.
//
// Layout.  A workgroup of W lanes owns tiles of 4 W consecutive outputs of one
// channel (blockIdx.y); lane t computes outputs j0 + t + r W, r = 0 .. 3.  W
// is a multiple of `up` (the largest within 256 lanes, or one within 512 that
// fills its waves: resample_plan), so the four outputs of a lane share one
// phase: a coefficient is read once for four products, and consecutive lanes
// store consecutive outputs.  With up > 256 W = 256 and every output reads
// its own row (SHARE = false).
//
// The phase-major table [up][pitch] is staged in LDS once per workgroup when
// it fits (TAB_LDS) and the workgroup then walks several tiles; otherwise the
// rows are read from global memory (the table is shared by every workgroup, so
// it stays in L2).  The input window of a tile, ceil((4W-1) down / up) + T
// samples of [delay line | block], is staged in LDS when it fits (WIN_LDS);
// for steep decimation, where consecutive outputs share no input, it is read
// from global memory directly.  A large table leaves room for few workgroups
// per CU, too few to hide the window's load latency behind other workgroups'
// arithmetic, so a workgroup that walks several tiles loads the next tile's
// window into registers before it computes the current one (PF).  All index
// arithmetic is int64.
#include "resample_kernels.hpp"

namespace adsp {
namespace {

template <bool SHARE, bool TAB_LDS, bool WIN_LDS, bool PF>
__global__ __launch_bounds__(kRsMaxLanes) void k_resample(ResampleArgs a, int tiles_per_wg) {
#pragma clang fp contract(off)
  static_assert(WIN_LDS || !PF, "the prefetch feeds the LDS window");
  extern __shared__ __attribute__((aligned(16))) double rs_lds[];
  double* stab = rs_lds;
  double* win = rs_lds + (TAB_LDS ? a.up * a.pitch : 0);
  const int t = threadIdx.x;
  const int W = blockDim.x;
  const int c = blockIdx.y;
  const int T = a.T;
  const int64_t hn = T - 1;
  const double* hc = a.hist + (int64_t)c * hn;
  const double* xc = a.src + (int64_t)c * a.sstride;
  double* yc = a.y + (int64_t)c * a.ystride;
  const double* tab = TAB_LDS ? stab : a.tab;
  const int64_t tile = (int64_t)W * kRsR;
  const int64_t jbase = (int64_t)blockIdx.x * tiles_per_wg * tile;  // < n_out: the grid covers no empty workgroup

  // window of the tile at j0: X[wlo, wlo + cnt), every index inside [0, hn + n_in)
  // because the last output's newest sample is the window's last element
  auto window = [&](int64_t j0, int64_t& wlo, int64_t& cnt) {
    const int64_t jl = (j0 + tile < a.n_out ? j0 + tile : a.n_out) - 1;
    wlo = a.ii0 + (a.phase0 + j0 * a.down) / a.up - hn;                 // >= 0
    cnt = a.ii0 + (a.phase0 + jl * a.down) / a.up - wlo + 1;            // <= plan.wlen
  };
  auto xat = [&](int64_t p) { return p < hn ? hc[p] : xc[p - hn]; };

  double pre[kRsPF];  // PF: this lane's part of the next window, elements t + i W
  if (PF) {
    int64_t wlo, cnt;
    window(jbase, wlo, cnt);
#pragma unroll
    for (int i = 0; i < kRsPF; ++i) {
      const int64_t v = t + (int64_t)i * W;
      pre[i] = v < cnt ? xat(wlo + v) : 0.0;
    }
  }
  if (TAB_LDS) {
    // eight loads in flight per lane, then their stores
    const int64_t cnt = a.up * a.pitch;
    for (int64_t v0 = t; v0 < cnt; v0 += 8 * (int64_t)W) {
      double g[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int64_t v = v0 + (int64_t)i * W;
        g[i] = v < cnt ? a.tab[v] : 0.0;
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int64_t v = v0 + (int64_t)i * W;
        if (v < cnt) stab[v] = g[i];
      }
    }
  }
  for (int it = 0; it < tiles_per_wg; ++it) {
    const int64_t j0 = jbase + it * tile;
    if (j0 >= a.n_out) break;  // the same for every lane of the workgroup
    const int64_t jl = (j0 + tile < a.n_out ? j0 + tile : a.n_out) - 1;  // last output of this tile
    int64_t wlo, cnt;
    window(j0, wlo, cnt);
    const int64_t p0 = wlo + hn;  // newest sample of output j0
    __syncthreads();              // the previous tile's window reads are done
    if (WIN_LDS) {
      if (PF) {
#pragma unroll
        for (int i = 0; i < kRsPF; ++i) {
          const int64_t v = t + (int64_t)i * W;
          if (v < cnt) win[v] = pre[i];
        }
      } else {
        for (int64_t v = t; v < cnt; v += W) win[v] = xat(wlo + v);
      }
    }
    __syncthreads();  // window and table staged
    if (PF && it + 1 < tiles_per_wg && j0 + tile < a.n_out) {
      int64_t nlo, ncnt;
      window(j0 + tile, nlo, ncnt);
#pragma unroll
      for (int i = 0; i < kRsPF; ++i) {
        const int64_t v = t + (int64_t)i * W;
        pre[i] = v < ncnt ? xat(nlo + v) : 0.0;
      }
    }

    // Outputs past jl read output j0's samples (in range) and store nothing.
    int64_t pos[kRsR];        // newest sample of output r: into win (WIN_LDS) or into X
    const double* row[kRsR];  // its coefficient row (SHARE: row[0] for all)
    double acc[kRsR];
#pragma unroll
    for (int r = 0; r < kRsR; ++r) {
      const int64_t j = j0 + t + (int64_t)r * W;
      acc[r] = 0.0;
      if (SHARE && r > 0) {
        // W = m up: num grows by m up down, so the phase stays and the index moves m down
        pos[r] = j <= jl ? pos[0] + (int64_t)r * (W / a.up) * a.down : (WIN_LDS ? hn : p0);
        row[r] = row[0];
        continue;
      }
      const int64_t num = a.phase0 + (j <= jl ? j : j0) * a.down;
      const int64_t q = num / a.up;
      pos[r] = a.ii0 + q - (WIN_LDS ? wlo : 0);
      row[r] = tab + (num - q * a.up) * a.pitch;
    }
    const double* wr[kRsR];  // WIN_LDS: the newest sample itself
#pragma unroll
    for (int r = 0; r < kRsR; ++r) wr[r] = win + (WIN_LDS ? pos[r] : 0);
#pragma unroll 8
    for (int k = 0; k < T; ++k) {
      double cf[kRsR];
#pragma unroll
      for (int r = 0; r < kRsR; ++r) cf[r] = (SHARE && r > 0) ? cf[0] : row[r][k];
#pragma unroll
      for (int r = 0; r < kRsR; ++r) {
        const double x = WIN_LDS ? wr[r][-k] : xat(pos[r] - k);
        const double pr = cf[r] * x;
        acc[r] = acc[r] + pr;
      }
    }
#pragma unroll
    for (int r = 0; r < kRsR; ++r) {
      const int64_t j = j0 + t + (int64_t)r * W;
      if (j <= jl) yc[j] = acc[r];
    }
  }
}

template <bool SHARE, bool TAB_LDS, bool WIN_LDS, bool PF>
void go(const ResamplePlan& p, const ResampleArgs& a, hipStream_t s) {
  const int64_t tiles = (a.n_out + p.tile() - 1) / p.tile();
  const int64_t wgs = (tiles + p.tiles_per_wg - 1) / p.tiles_per_wg;
  hipLaunchKernelGGL((k_resample<SHARE, TAB_LDS, WIN_LDS, PF>), dim3((unsigned)wgs, (unsigned)a.channels),
                     dim3((unsigned)p.lanes), (size_t)p.lds_bytes, s, a, p.tiles_per_wg);
}

template <bool SHARE, bool TAB_LDS>
void go_win(const ResamplePlan& p, const ResampleArgs& a, hipStream_t s) {
  if (!p.win_lds)
    go<SHARE, TAB_LDS, false, false>(p, a, s);
  else if (p.prefetch)
    go<SHARE, TAB_LDS, true, true>(p, a, s);
  else
    go<SHARE, TAB_LDS, true, false>(p, a, s);
}

}  // namespace

ResamplePlan resample_plan(int64_t up, int64_t down, int64_t T) {
  ResamplePlan p;
  p.share = up <= kRsLanes;
  p.lanes = kRsLanes;
  if (p.share) {
    // the largest multiple of up within 256 lanes, unless it leaves more than a
    // tenth of its waves' lanes idle (160 -> 2.5 waves): then the multiple
    // within kRsMaxLanes that fills its waves best (320 -> 5 waves)
    auto slots = [](int64_t w) { return (w + 63) / 64 * 64; };
    int64_t w = (kRsLanes / up) * up;
    if (10 * w < 9 * slots(w))
      for (int64_t m = up; m <= kRsMaxLanes; m += up)
        if (m * slots(w) > w * slots(m)) w = m;
    p.lanes = (int)w;
  }
  const int64_t tile = p.tile();
  p.wlen = ((tile - 1) * down + up - 1) / up + T;
  const int64_t tab_bytes = up * rs_pitch(T) * (int64_t)sizeof(double);
  p.tab_lds = tab_bytes <= kRsLdsBudget - kRsWinReserve;
  const int64_t left = kRsLdsBudget - (p.tab_lds ? tab_bytes : 0);
  p.win_lds = p.wlen <= left / (int64_t)sizeof(double);
  p.lds_bytes = (p.tab_lds ? tab_bytes : 0) + (p.win_lds ? p.wlen * (int64_t)sizeof(double) : 0);
  if (p.tab_lds) {
    // staging reads up*pitch coefficients: walk enough tiles that it stays a small part of the work
    const int64_t n = (64 * up + tile - 1) / tile;
    p.tiles_per_wg = (int)(n < 1 ? 1 : (n > 64 ? 64 : n));
  }
  p.prefetch = p.win_lds && p.tiles_per_wg > 1 && p.wlen <= (int64_t)kRsPF * p.lanes;
  return p;
}

void launch_resample(const ResamplePlan& p, const ResampleArgs& a, hipStream_t s) {
  if (a.channels <= 0 || a.n_out <= 0) return;
  switch (p.share * 2 + p.tab_lds) {
    case 0: go_win<false, false>(p, a, s); break;
    case 1: go_win<false, true>(p, a, s); break;
    case 2: go_win<true, false>(p, a, s); break;
    default: go_win<true, true>(p, a, s); break;
  }
}

}  // namespace adsp
