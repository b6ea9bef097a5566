// The time-domain pitch shifter's kernels (dsp/effects/pitch/pitch_shifter.go).
//
// The stretch.  The frames of one channel depend on each other (the next
// reference segment starts at the chosen candStart + stepOut), so a call walks
// the frames in order, two launches per frame, and runs channels x candidates
// side by side within a frame:
//
//   k_pt_search    findBestOverlap :359-389.  A workgroup takes one tile of
//                  kPtTile consecutive candidates of one channel; a lane owns
//                  kPtR of them.  Candidate c's dot and candEnergy are summed
//                  over i = 0 ... overlapLen-1 in that order, product and add
//                  rounded separately, as blocked_dot.hpp sums a FIR output:
//                  the reference segment is the wave-uniform vector (scalar
//                  loads from the row k_pt_assemble left), the input around the
//                  candidates the sliding window in LDS, one aligned kPtR-wide
//                  LDS read per kPtR x kPtR products of each sum.  The window
//                  holds kPtTerms terms at a time, so the LDS a workgroup takes
//                  (kPtWindow doubles, 16.5 KB) depends on no parameter: a longer
//                  overlap refills it, the sums stay in registers.  The tile's
//                  winner is the highest score, the lowest candidate among equal
//                  ones, NaN never: what the reference's ascending scan with a
//                  strict > selects.
//   k_pt_assemble  the winner across the tiles in ascending order (none: the
//                  predicted start, as `best := predicted` stands), the
//                  cross-fade :329-333, the body :335-338, the exit test :344 and
//                  the next frame's reference segment with its energy :366-369.
//
// The reference segment is not in LDS: k_pt_search reads it with scalar loads
// through the constant address space, which is right only because the row was
// written by an earlier launch (k_pt_assemble of the frame before).  That
// coherence rests on the kernel boundary: a kernel that fused assembly and
// search would have to read the segment some other way.
//
// The loop's other exit (:319) depends on the lengths alone and is the host's.
// Reads outside [0, n) are zeros (pitchSampleZero :432-438).
//
// The resample.  pos is the same for every channel (the host accumulates it as
// :412-416 do), so every output of every channel is independent:
// interp.Hermite4 (dsp/interp/interp.go:51-58) on clamped reads
// (pitchSampleClamp :440-454).
#include <hip/hip_runtime.h>

#include <cmath>

#include "blocked_dot.hpp"
#include "pitchtime_kernels.hpp"

namespace adsp {

namespace {

constexpr double kTiny = 1e-12;  // pitchShifterTiny :30

__device__ __forceinline__ double sample_zero(const double* x, int64_t n, int64_t idx) {  // :432-438
  return (idx >= 0 && idx < n) ? x[idx] : 0.0;
}

// blocked_dot.hpp's bd_block with the window's own square summed beside the dot
template <int R>
__device__ __forceinline__ void pt_block(const double (&c0)[R], const double (&c1)[R], const double (&hv)[R],
                                         double (&dot)[R], double (&en)[R]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int j = 0; j < R; ++j) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int x = j + r + 1;
      const double w = x < R ? c0[x] : c1[x - R];
      const double p = hv[j] * w;
      dot[r] = dot[r] + p;
      const double q = w * w;
      en[r] = en[r] + q;
    }
  }
}

// terms 0 .. cnt-1 of the lane's R candidates: dot[r] += hs[u] * wt[u + r], en[r] += wt[u + r]^2, u ascending.
// wt follows blocked_dot.hpp's alignment contract; chunk reads run up to R past the last term's window.
template <int R>
__device__ __forceinline__ void pt_accumulate(const double* __restrict__ hs, const double* wt, int cnt, double (&dot)[R],
                                              double (&en)[R]) {
#pragma clang fp contract(off)
  const int nb = cnt / R;
  int k = 0;
  if (nb > 0) {
    double c0[R], c1[R];
    bd_chunk<R>(wt, 0, c0);
    for (; k + 2 <= nb; k += 2) {
      double hv[2][R];
      bd_taps<R, 1, 2>(hs, k, hv);
      bd_chunk<R>(wt, k + 1, c1);
      pt_block<R>(c0, c1, hv[0], dot, en);
      bd_chunk<R>(wt, k + 2, c0);
      pt_block<R>(c1, c0, hv[1], dot, en);
    }
    if (k < nb) {  // c0 = chunk k
      double hv[1][R];
      bd_taps<R, 1, 1>(hs, k, hv);
      bd_chunk<R>(wt, k + 1, c1);
      pt_block<R>(c0, c1, hv[0], dot, en);
      ++k;
    }
  }
  for (int u = k * R; u < cnt; ++u) {
    const double h = hs[u];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const double w = wt[u + r];
      const double p = h * w;
      dot[r] = dot[r] + p;
      const double q = w * w;
      en[r] = en[r] + q;
    }
  }
}

// the better of two winners: the higher score, the lower candidate among equal scores
__device__ __forceinline__ void pt_better(double& score, int& cand, double other_score, int other_cand) {
  if (other_score > score || (other_score == score && other_cand < cand)) {
    score = other_score;
    cand = other_cand;
  }
}

__global__ __launch_bounds__(kPtThreads) void k_pt_search(PtArgs a, int64_t predicted) {
#pragma clang fp contract(off)
  constexpr int R = kPtR;
  __shared__ __attribute__((aligned(32))) double win[kPtWindow];
  __shared__ double wave_score[kPtThreads / 64];
  __shared__ int wave_cand[kPtThreads / 64];
  const int ch = blockIdx.x / a.tiles, tile = blockIdx.x - ch * a.tiles;
  if (a.done[ch]) return;  // the whole workgroup
  const int t = threadIdx.x;
  const double* x = a.in + (int64_t)ch * a.stride;
  const double* ref = a.ref + (int64_t)ch * a.ref_pitch;
  const int rel0 = tile * kPtTile;                      // the tile's first candidate, from searchStart
  const int64_t first = predicted - a.search + rel0;   // its start in the input; may be negative
  double dot[R], en[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    dot[r] = 0.0;
    en[r] = kTiny;
  }
  const double* wt = win + 1 + t * R;  // window value j of the tile lies at win[1 + j]
  for (int u0 = 0; u0 < a.overlap; u0 += kPtTerms) {
    if (u0) __syncthreads();
    for (int j = t; j < kPtWindow; j += kPtThreads) win[j] = sample_zero(x, a.n, first + u0 + j - 1);
    __syncthreads();
    pt_accumulate<R>(ref + u0, wt, min(kPtTerms, a.overlap - u0), dot, en);
  }
  const double ref_energy = a.ref_energy[ch];
  double best = -INFINITY;
  int cand = kPtNone;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int rel = rel0 + t * R + r;
    if (rel <= 2 * a.search) {
      const double score = dot[r] / sqrt(ref_energy * en[r]);  // :381
      if (score > best) {                                       // :382, false for NaN
        best = score;
        cand = rel;
      }
    }
  }
  for (int off = 1; off < 64; off <<= 1) {
    const double os = __shfl_xor(best, off);
    const int oc = __shfl_xor(cand, off);
    pt_better(best, cand, os, oc);
  }
  if ((t & 63) == 0) {
    wave_score[t >> 6] = best;
    wave_cand[t >> 6] = cand;
  }
  __syncthreads();
  if (t == 0) {
    for (int w = 1; w < kPtThreads / 64; ++w) pt_better(best, cand, wave_score[w], wave_cand[w]);
    a.tile_score[(int64_t)ch * a.tiles + tile] = best;
    a.tile_cand[(int64_t)ch * a.tiles + tile] = cand;
  }
}

// first != 0: frame 0 (cand = 0, no cross-fade, nothing to pick)
__global__ __launch_bounds__(kPtThreads) void k_pt_assemble(PtArgs a, int64_t predicted, int64_t out_start, int may_break,
                                                            int first) {
#pragma clang fp contract(off)
  __shared__ int64_t s_cand;
  __shared__ double seg[kPtTerms];
  const int ch = blockIdx.x, t = threadIdx.x;
  if (!first && a.done[ch]) return;  // every thread reads it before the barrier; thread 0 writes it after
  if (t == 0) {
    int64_t cand = 0;
    if (!first) {
      double best = -INFINITY;
      int rel = kPtNone;
      for (int tile = 0; tile < a.tiles; ++tile)
        pt_better(best, rel, a.tile_score[(int64_t)ch * a.tiles + tile], a.tile_cand[(int64_t)ch * a.tiles + tile]);
      cand = rel == kPtNone ? predicted : predicted - a.search + rel;  // :360
    }
    s_cand = cand;
  }
  __syncthreads();
  const int64_t cand = s_cand;
  const double* x = a.in + (int64_t)ch * a.stride;
  double* o = a.out + (int64_t)ch * a.out_pitch + out_start;
  for (int i = t; i < a.sequence; i += kPtThreads) {
    double v = sample_zero(x, a.n, cand + i);
    if (!first && i < a.overlap) {  // :329-333
      const double fi = a.fade_in[i];
      const double fo = 1.0 - fi;  // fadeOut :292
      const double p = o[i] * fo;
      const double q = v * fi;
      v = p + q;
    }
    o[i] = v;
  }
  const int64_t ref_start = cand + (a.sequence - a.overlap);  // :320
  double* r = a.ref + (int64_t)ch * a.ref_pitch;
  // the segment goes to its row and, a run of kPtTerms at a time, through LDS, where one lane sums its energy
  // in the reference's order (:366-369) without a chain of global loads
  double e = kTiny;
  for (int u0 = 0; u0 < a.overlap; u0 += kPtTerms) {
    const int cnt = min(kPtTerms, a.overlap - u0);
    if (u0) __syncthreads();
    for (int i = t; i < cnt; i += kPtThreads) {
      const double v = sample_zero(x, a.n, ref_start + u0 + i);
      seg[i] = v;
      r[u0 + i] = v;
    }
    __syncthreads();
    if (t == 0) {
      for (int i = 0; i < cnt; ++i) {
        const double q = seg[i] * seg[i];
        e = e + q;
      }
    }
  }
  if (t == 0) {
    a.prev_start[ch] = cand;
    a.done[ch] = (!first && may_break && cand > a.n + a.sequence) ? 1 : 0;  // :344
    a.ref_energy[ch] = e;
  }
}

__device__ __forceinline__ double hermite4(double t, double xm1, double x0, double x1, double x2) {  // interp.go:51-58
#pragma clang fp contract(off)
  const double c0 = x0;
  const double c1 = 0.5 * (x1 - xm1);
  const double c2 = ((xm1 - 2.5 * x0) + 2 * x1) - 0.5 * x2;
  const double c3 = 0.5 * (x2 - xm1) + 1.5 * (x0 - x1);
  return ((c3 * t + c2) * t + c1) * t + c0;
}

__global__ __launch_bounds__(256) void k_pt_resample(const double* __restrict__ src, int64_t src_pitch, int64_t len,
                                                     const double* __restrict__ pos, double* __restrict__ out,
                                                     int64_t stride, int64_t n, int blocks_per_row, int mode) {
#pragma clang fp contract(off)
  const int ch = blockIdx.x / blocks_per_row;
  const int64_t i = (int64_t)(blockIdx.x - ch * blocks_per_row) * 256 + threadIdx.x;
  if (i >= n) return;
  const double* s = src + (int64_t)ch * src_pitch;
  double v;
  if (mode) {
    v = s[0];
  } else {
    const double p = pos[i];
    const int64_t idx = (int64_t)floor(p);  // :422
    const double frac = p - (double)idx;
    const int64_t last = len - 1;
    const double xm1 = s[min(max(idx - 1, (int64_t)0), last)];  // pitchSampleClamp :440-454
    const double x0 = s[min(max(idx, (int64_t)0), last)];
    const double x1 = s[min(max(idx + 1, (int64_t)0), last)];
    const double x2 = s[min(max(idx + 2, (int64_t)0), last)];
    v = hermite4(frac, xm1, x0, x1, x2);
  }
  out[(int64_t)ch * stride + i] = v;
}

}  // namespace

void launch_pt_first(const PtArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_pt_assemble, dim3(a.channels), dim3(kPtThreads), 0, s, a, (int64_t)0, (int64_t)0, 0, 1);
}

void launch_pt_search(const PtArgs& a, int64_t predicted, hipStream_t s) {
  hipLaunchKernelGGL(k_pt_search, dim3((unsigned)(a.channels * a.tiles)), dim3(kPtThreads), 0, s, a, predicted);
}

void launch_pt_assemble(const PtArgs& a, int64_t predicted, int64_t out_start, int may_break, hipStream_t s) {
  hipLaunchKernelGGL(k_pt_assemble, dim3(a.channels), dim3(kPtThreads), 0, s, a, predicted, out_start, may_break, 0);
}

void launch_pt_resample(const double* src, int64_t src_pitch, int64_t len, const double* pos, double* out, int64_t stride,
                        int64_t n, int channels, int mode, hipStream_t s) {
  const int blocks_per_row = (int)((n + 255) / 256);
  hipLaunchKernelGGL(k_pt_resample, dim3((unsigned)(channels * blocks_per_row)), dim3(256), 0, s, src, src_pitch, len, pos,
                     out, stride, n, blocks_per_row, mode);
}

}  // namespace adsp
