// effects.Distortion.ProcessInPlace (dsp/effects/distortion.go:538-797) and
// effects.BitCrusher.ProcessInPlace (bit_crusher.go:192-230) for many channels
// that share one configuration, in the reference's operation order (every
// product, sum and quotient rounded on its own, no FMA, the comparisons of
// clamp as written).
//
//   k_shape     out = in (1 - mix) + finite(shapeSample((in + bias) drive) outputLevel) mix,
//               pointwise over [channels][n], a 16-byte pair per thread and
//               step.  A row 8 bytes off 16-byte alignment takes its first
//               sample alone and its pairs from the second one on.  The mode,
//               the approximation and "weights active" are template
//               parameters: a launch runs one transfer function and the
//               per-sample path does not ask which.
//   k_shape_curve  the same shapeSample(x) outputLevel with the finite check,
//               over a plain array: the transfer curve as the device computes it.
//   k_shape_dc  Chebyshev with dcBypass: y = (w - prevIn) + 0.995 prevOut is
//               serial along time, so one channel per lane walks the row; a
//               workgroup is one wave of 64 channels that stages kDcTile
//               samples of each through LDS (consecutive lanes, consecutive
//               samples of a row in global memory; lane = channel at an odd
//               pitch for the walk), loads of the next chunk and stores of
//               the last one in flight during the walk, as k_phaser.  The
//               shaped value w does not depend on the filter: it is computed
//               in the staging layout, kDcTile independent samples per lane,
//               and the walk is left with the recurrence, the finite check
//               and the mix.
//   k_crush1    downsample 1: hold = round(in q) / q of the sample itself, pointwise
//               like k_shape; the thread of the row's last sample keeps its hold.
//   k_crush     downsample >= 2, in place: sample t needs the input at the
//               latest update u <= t, which the thread owning u overwrites.
//               A workgroup owns a span of whole hold periods that starts at
//               an update sample, loads all of it into LDS, passes a barrier
//               and only then stores; spans are disjoint, so no workgroup
//               reads what another writes.  The samples before the call's
//               first update take the carried hold value (read from hold_in,
//               never written by this call).
//
// Every global index is guarded by the row's length and the channel count.
#include "shaper_kernels.hpp"

#include <algorithm>

namespace adsp {
namespace {

__device__ __forceinline__ double clamp_unit(double x) {  // clamp(x, -1, 1) :783-797: a NaN passes
  if (x < -1.0) return -1.0;
  if (x > 1.0) return 1.0;
  return x;
}

__device__ __forceinline__ double soft_clip(double x) {  // :659-666
#pragma clang fp contract(off)
  const double ax = fabs(x);
  if (ax < 1.0) return 1.5 * (x - (x * x * x) / 3.0);
  return copysign(1.0, x);
}

__device__ __forceinline__ double fast_tanh(double x) {  // fastTanhApprox :769-781
#pragma clang fp contract(off)
  if (x > 3.0) return 1.0;
  if (x < -3.0) return -1.0;
  const double x2 = x * x;
  return clamp_unit(x * (27.0 + x2) / (27.0 + 9.0 * x2));
}

template <bool W>
__device__ __forceinline__ double chebyshev(double x, const ShapeParams& p) {  // chebyshevShape :684-728
#pragma clang fp contract(off)
  x = clamp_unit(x);
  double t0 = 1.0, t1 = x;
  double sum = 0.0;
  if (W) sum = p.w[0] * t1;
  double tn = t1;
  for (int n = 2; n <= p.order; ++n) {
    tn = 2.0 * x * t1 - t0;
    if (W) sum += p.w[n - 1] * tn;
    t0 = t1;
    t1 = tn;
  }
  double out = (W ? sum : tn) * p.cheb_gain;
  if (p.invert) out = -out;
  return clamp_unit(out);
}

// shapeSample :608-645
template <int M, bool POLY, bool W>
__device__ __forceinline__ double shape_sample(double x, const ShapeParams& p) {
#pragma clang fp contract(off)
  if constexpr (M == SHAPE_SOFTCLIP) {
    return soft_clip(x);
  } else if constexpr (M == SHAPE_HARDCLIP) {  // :647-657
    if (x > p.clip_level) x = p.clip_level;
    if (x < -p.clip_level) x = -p.clip_level;
    return x / p.clip_level;
  } else if constexpr (M == SHAPE_TANH) {  // :668-674
    return POLY ? fast_tanh(x) : tanh(x);
  } else if constexpr (M == SHAPE_WS1) {
    return clamp_unit(x / (1.0 + p.shape * fabs(x)));
  } else if constexpr (M == SHAPE_WS2) {
    return clamp_unit(((1.0 + p.shape) * x) / (1.0 + p.shape * fabs(x)));
  } else if constexpr (M == SHAPE_WS3) {
    return clamp_unit(x - p.shape * x * x * x / 3.0);
  } else if constexpr (M == SHAPE_WS4) {
    return clamp_unit((3.0 * x) / (2.0 + fabs(2.0 * x)));
  } else if constexpr (M == SHAPE_WS5) {
    return clamp_unit(atan(x * p.scale4) / p.atan_scale4);
  } else if constexpr (M == SHAPE_WS6) {
    return clamp_unit((1.0 + p.shape) * x / (1.0 + p.shape * x * x));
  } else if constexpr (M == SHAPE_WS7) {
    const double y = x * p.scale6;
    return POLY ? fast_tanh(y) : tanh(y);
  } else if constexpr (M == SHAPE_WS8) {
    return clamp_unit(copysign(1.0 - exp(-fabs(x) * p.scale6), x));
  } else if constexpr (M == SHAPE_SATURATE) {
    return clamp_unit(x / (1.0 + fabs(x)));
  } else if constexpr (M == SHAPE_SATURATE2) {
    return soft_clip(x * p.scale2);
  } else if constexpr (M == SHAPE_SOFTSAT) {  // :676-682
    if (POLY) return clamp_unit(x * (27.0 + x * x) / (27.0 + 9.0 * x * x));
    return clamp_unit(M_2_PI * atan(M_PI_2 * x));
  } else {
    return chebyshev<W>(x, p);
  }
}

template <int M, bool POLY, bool W>
__device__ __forceinline__ double shape_wet(double x, const ShapeParams& p) {  // :542-543, 549-551
#pragma clang fp contract(off)
  const double wet = shape_sample<M, POLY, W>(x, p) * p.output_level;
  return isfinite(wet) ? wet : 0.0;
}

template <int M, bool POLY, bool W>
struct ShapeOp {
  const ShapeParams& p;
  __device__ __forceinline__ double operator()(double in, int64_t) const {  // ProcessSample :538-554
#pragma clang fp contract(off)
    const double x = (in + p.bias) * p.drive;
    const double wet = shape_wet<M, POLY, W>(x, p);
    return in * p.one_minus_mix + wet * p.mix;
  }
};

struct CrushOp {  // ProcessSample :192-201 at downsample 1: every sample is an update
  double q, mix, one_minus_mix;
  double* hold_out;
  int64_t last;
  __device__ __forceinline__ double operator()(double in, int64_t t) const {
#pragma clang fp contract(off)
    const double hold = round(in * q) / q;  // quantize :228-230
    if (t == last) *hold_out = hold;
    return in * one_minus_mix + hold * mix;
  }
};

// tile `tile` of a row of n samples: pairs at 16-byte alignment, the samples outside them by two threads of tile 0
template <class Op>
__device__ __forceinline__ void pointwise_tile(double* row, int64_t n, int tile, const Op& op) {
  const int64_t lead = (reinterpret_cast<uintptr_t>(row) & 15) ? 1 : 0;  // a row 8 bytes off: its pairs start at sample 1
  const int64_t pairs = (n - lead) / 2;
  if (tile == 0 && threadIdx.x < 2) {  // the first sample of an off row, an odd one at the end
    const int64_t t = threadIdx.x == 0 ? 0 : lead + 2 * pairs;
    if (threadIdx.x == 0 ? lead == 1 : t < n) row[t] = op(row[t], t);
  }
  const int64_t p0 = (int64_t)tile * (kShapeThreads * kShapeSteps) + threadIdx.x;
#pragma unroll
  for (int k = 0; k < kShapeSteps; ++k) {
    const int64_t p = p0 + (int64_t)k * kShapeThreads;
    if (p >= pairs) break;
    const int64_t t = lead + 2 * p;
    double2* q = reinterpret_cast<double2*>(row + t);
    double2 v = *q;
    v.x = op(v.x, t);
    v.y = op(v.y, t + 1);
    *q = v;
  }
}

template <int M, bool POLY, bool W>
__global__ __launch_bounds__(kShapeThreads) void k_shape(ShapeArgs a, int tiles) {
  const int64_t ch = blockIdx.x / tiles;
  const int tile = (int)(blockIdx.x % tiles);
  pointwise_tile(a.buf + ch * a.stride, a.n, tile, ShapeOp<M, POLY, W>{a.p});
}

template <int M, bool POLY, bool W>
__global__ __launch_bounds__(256) void k_shape_curve(ShapeParams p, const double* x, double* wet, int64_t n) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t < n) wet[t] = shape_wet<M, POLY, W>(x[t], p);
}

__global__ __launch_bounds__(kShapeThreads) void k_crush1(CrushArgs a, int tiles) {
  const int64_t ch = blockIdx.x / tiles;
  const int tile = (int)(blockIdx.x % tiles);
  pointwise_tile(a.buf + ch * a.stride, a.n, tile, CrushOp{a.q, a.mix, a.one_minus_mix, a.hold_out + ch, a.n - 1});
}

// downsample >= 2.  blockIdx.x = channel * spans + span; span s owns the
// samples [t0 + s L, t0 + (s + 1) L) below n, L = crush_span(downsample), and
// span 0 the samples below t0 as well.
__global__ __launch_bounds__(kCrushThreads) void k_crush(CrushArgs a, int spans, int64_t L) {
#pragma clang fp contract(off)
  __shared__ double sm[kCrushSpan];
  const int64_t ch = blockIdx.x / spans;
  const int64_t span = blockIdx.x % spans;
  const int tid = threadIdx.x;
  double* row = a.buf + ch * a.stride;
  if (span == 0) {  // before the first update: the carried hold value; each thread touches its own samples only
    const int head = (int)(a.t0 < a.n ? a.t0 : a.n);
    const double hold = a.hold_in[ch];
    for (int e = tid; e < head; e += kCrushThreads) row[e] = row[e] * a.one_minus_mix + hold * a.mix;
  }
  const int64_t s0 = a.t0 + span * L;  // an update sample
  if (s0 >= a.n) return;               // the whole workgroup: nobody waits at the barrier below
  const int m = (int)(a.n - s0 < L ? a.n - s0 : L);
  for (int e = tid; e < m; e += kCrushThreads) sm[e] = row[s0 + e];
  __syncthreads();  // every load of the span is complete before its first store
  const int64_t u_last = a.t0 + (a.n - 1 - a.t0) / a.downsample * a.downsample;  // the call's last update
  for (int e = tid; e < m; e += kCrushThreads) {
    const int u = e / a.downsample * a.downsample;  // the latest update at or before e
    const double hold = round(sm[u] * a.q) / a.q;
    if (e == u && s0 + e == u_last) a.hold_out[ch] = hold;
    row[s0 + e] = sm[e] * a.one_minus_mix + hold * a.mix;
  }
}

// A workgroup barrier that orders the LDS accesses only: global loads and stores in flight stay in flight.
__device__ __forceinline__ void lds_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// ProcessSample :538-554 in Chebyshev mode with dcBypass, in two parts.  The shaped value does not depend on
// the filter, so it is taken where the work is parallel; the walk keeps the recurrence alone.
template <bool W>
__device__ __forceinline__ double dc_shaped(double in, const ShapeParams& p) {  // :540-543
#pragma clang fp contract(off)
  const double x = (in + p.bias) * p.drive;
  return chebyshev<W>(x, p) * p.output_level;
}

// dcBypass :730-736, the finite check and the mix :549-553.  The finite check comes after the filter and does
// not repair the state: a non-finite y stays in prev_out.
__device__ __forceinline__ double dc_sample(double in, double w, double& prev_in, double& prev_out, const ShapeParams& p) {
#pragma clang fp contract(off)
  const double y = w - prev_in + 0.995 * prev_out;
  prev_in = w;
  prev_out = y;
  const double wet = isfinite(y) ? y : 0.0;
  return in * p.one_minus_mix + wet * p.mix;
}

template <bool W>
__global__ __launch_bounds__(64) void k_shape_dc(ShapeDcArgs a) {
  constexpr int T = kDcTile, P = kDcPitch;
  constexpr int kRows = 64 / T;       // rows a staging step of the wave covers
  constexpr int kSteps = 64 / kRows;  // staging steps per chunk
  __shared__ __attribute__((aligned(16))) double tiles[2][64 * P];
  __shared__ __attribute__((aligned(16))) double shaped[64 * P];  // of the chunk being walked
  const int lane = threadIdx.x;
  const int64_t ch0 = (int64_t)blockIdx.x * 64;
  const int count = (int)(a.channels - ch0 < 64 ? a.channels - ch0 : 64);
  const bool active = lane < count;
  const int64_t ch = ch0 + (active ? lane : 0);
  double prev_in = a.dc[2 * ch], prev_out = a.dc[2 * ch + 1];
  // staging: consecutive lanes take consecutive samples of a row; step k covers rows k * kRows + rl
  const int tl = lane % T, rl = lane / T;
  double* io = a.buf + (ch0 + rl) * a.stride + tl;

  // chunk c is walked in its tile while the loads of chunk c + 1 fly into registers and the stores of
  // chunk c - 1 drain from the other tile (in place: the three touch disjoint samples of the rows)
  double v[kSteps];
  {
    const int m = (int)(a.n < T ? a.n : T);
#pragma unroll
    for (int k = 0; k < kSteps; ++k)
      v[k] = (k * kRows + rl < count && tl < m) ? io[(int64_t)k * kRows * a.stride] : 0.0;
  }
  int mprev = 0, cur = 0;
  for (int64_t t0 = 0; t0 < a.n; t0 += T, cur ^= 1) {
    const int m = (int)(a.n - t0 < T ? a.n - t0 : T);
    double* tile = tiles[cur];
    const double* done = tiles[cur ^ 1];
    // the shaped values in the staging layout: every lane has kSteps independent samples in registers,
    // where the walk would have one at a time behind the recurrence
#pragma unroll
    for (int k = 0; k < kSteps; ++k) {
      tile[(k * kRows + rl) * P + tl] = v[k];
      shaped[(k * kRows + rl) * P + tl] = dc_shaped<W>(v[k], a.p);
    }
    lds_barrier();  // the tile is whole; the walk of the chunk before is complete
#pragma unroll
    for (int k = 0; k < kSteps; ++k)
      if (k * kRows + rl < count && tl < mprev) io[(int64_t)k * kRows * a.stride + (t0 - T)] = done[(k * kRows + rl) * P + tl];
    const int64_t t1 = t0 + T;
    const int m1 = (int)(t1 >= a.n ? 0 : (a.n - t1 < T ? a.n - t1 : T));
#pragma unroll
    for (int k = 0; k < kSteps; ++k)
      v[k] = (k * kRows + rl < count && tl < m1) ? io[(int64_t)k * kRows * a.stride + t1] : 0.0;
    if (active) {
      double* mine = tile + lane * P;
      const double* wets = shaped + lane * P;
      if (m == T) {  // a whole chunk: its samples in registers, so no sample waits for LDS
        double sv[T], wv[T];
#pragma unroll
        for (int t = 0; t < T; ++t) {
          sv[t] = mine[t];
          wv[t] = wets[t];
        }
#pragma unroll
        for (int t = 0; t < T; ++t) sv[t] = dc_sample(sv[t], wv[t], prev_in, prev_out, a.p);
#pragma unroll
        for (int t = 0; t < T; ++t) mine[t] = sv[t];
      } else {
        for (int t = 0; t < m; ++t) mine[t] = dc_sample(mine[t], wets[t], prev_in, prev_out, a.p);
      }
    }
    mprev = m;
    lds_barrier();  // this chunk is walked, the one before has left its tile: the next one may take it
  }
  if (a.n > 0) {  // the last chunk
    const int64_t t0 = (a.n - 1) / T * T;
    const double* done = tiles[cur ^ 1];
#pragma unroll
    for (int k = 0; k < kSteps; ++k)
      if (k * kRows + rl < count && tl < mprev) io[(int64_t)k * kRows * a.stride + t0] = done[(k * kRows + rl) * P + tl];
  }
  if (active) {
    a.dc[2 * ch] = prev_in;
    a.dc[2 * ch + 1] = prev_out;
  }
}

template <int M, bool POLY, bool W>
struct ShapeTag {
  static constexpr int mode = M;
  static constexpr bool poly = POLY, weights = W;
};

// The host's dispatch: one instantiation per transfer function.  The polynomial flag matters to Tanh,
// Waveshaper7 and SoftSat only (:668-682), the weights to Chebyshev only.
template <class Fn>
void dispatch_shape(const ShapeParams& p, Fn&& fn) {
  const bool poly = p.poly != 0;
  switch (p.mode) {
    case SHAPE_HARDCLIP: return fn(ShapeTag<SHAPE_HARDCLIP, false, false>{});
    case SHAPE_TANH:
      return poly ? fn(ShapeTag<SHAPE_TANH, true, false>{}) : fn(ShapeTag<SHAPE_TANH, false, false>{});
    case SHAPE_WS1: return fn(ShapeTag<SHAPE_WS1, false, false>{});
    case SHAPE_WS2: return fn(ShapeTag<SHAPE_WS2, false, false>{});
    case SHAPE_WS3: return fn(ShapeTag<SHAPE_WS3, false, false>{});
    case SHAPE_WS4: return fn(ShapeTag<SHAPE_WS4, false, false>{});
    case SHAPE_WS5: return fn(ShapeTag<SHAPE_WS5, false, false>{});
    case SHAPE_WS6: return fn(ShapeTag<SHAPE_WS6, false, false>{});
    case SHAPE_WS7:
      return poly ? fn(ShapeTag<SHAPE_WS7, true, false>{}) : fn(ShapeTag<SHAPE_WS7, false, false>{});
    case SHAPE_WS8: return fn(ShapeTag<SHAPE_WS8, false, false>{});
    case SHAPE_SATURATE: return fn(ShapeTag<SHAPE_SATURATE, false, false>{});
    case SHAPE_SATURATE2: return fn(ShapeTag<SHAPE_SATURATE2, false, false>{});
    case SHAPE_SOFTSAT:
      return poly ? fn(ShapeTag<SHAPE_SOFTSAT, true, false>{}) : fn(ShapeTag<SHAPE_SOFTSAT, false, false>{});
    case SHAPE_CHEBYSHEV:
      return p.has_weights ? fn(ShapeTag<SHAPE_CHEBYSHEV, false, true>{})
                           : fn(ShapeTag<SHAPE_CHEBYSHEV, false, false>{});
    default: return fn(ShapeTag<SHAPE_SOFTCLIP, false, false>{});  // shapeSample's default :642-643
  }
}

int pointwise_tiles(int64_t n) {
  constexpr int64_t per_tile = (int64_t)kShapeThreads * kShapeSteps;
  return (int)std::max<int64_t>(1, (n / 2 + per_tile - 1) / per_tile);
}

}  // namespace

void launch_shape(const ShapeArgs& a, hipStream_t s) {
  if (a.n <= 0 || a.channels <= 0) return;
  const int tiles = pointwise_tiles(a.n);
  const dim3 grid((unsigned)((int64_t)a.channels * tiles));
  dispatch_shape(a.p, [&](auto tag) {
    using T = decltype(tag);
    k_shape<T::mode, T::poly, T::weights><<<grid, dim3(kShapeThreads), 0, s>>>(a, tiles);
  });
}

void launch_shape_curve(const ShapeParams& p, const double* x, double* wet, int64_t n, hipStream_t s) {
  if (n <= 0) return;
  const dim3 grid((unsigned)((n + 255) / 256));
  dispatch_shape(p, [&](auto tag) {
    using T = decltype(tag);
    k_shape_curve<T::mode, T::poly, T::weights><<<grid, dim3(256), 0, s>>>(p, x, wet, n);
  });
}

void launch_shape_dc(const ShapeDcArgs& a, hipStream_t s) {
  if (a.n <= 0 || a.channels <= 0) return;
  const dim3 grid((unsigned)((a.channels + 63) / 64));
  if (a.p.has_weights)
    k_shape_dc<true><<<grid, dim3(64), 0, s>>>(a);
  else
    k_shape_dc<false><<<grid, dim3(64), 0, s>>>(a);
}

void launch_crush(const CrushArgs& a, hipStream_t s) {
  if (a.n <= 0 || a.channels <= 0) return;
  if (a.downsample == 1) {
    const int tiles = pointwise_tiles(a.n);
    k_crush1<<<dim3((unsigned)((int64_t)a.channels * tiles)), dim3(kShapeThreads), 0, s>>>(a, tiles);
    return;
  }
  const int64_t L = crush_span(a.downsample);
  const int spans = a.n > a.t0 ? (int)((a.n - a.t0 + L - 1) / L) : 1;
  k_crush<<<dim3((unsigned)((int64_t)a.channels * spans)), dim3(kCrushThreads), 0, s>>>(a, spans, L);
}

}  // namespace adsp
