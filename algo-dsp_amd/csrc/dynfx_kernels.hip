// dynamics.TransientShaper.ProcessSample (dsp/effects/dynamics/
// transient_shaper.go:139-170) and DeEsser.ProcessSample (deesser.go:413-475)
// for many channels that share one configuration, in the reference's operation
// order (every product and sum rounded on its own, no FMA).
//
// In both, only the envelope is serial in time: a compare, a select and three
// dependent roundings per sample, behind the detection cascade in the de-esser.
// What follows env[t] is pointwise and never feeds back: the shaper's divide,
// clamp and multiply, the de-esser's log2, exp2, blend, clamp and metrics.  So
// a call is two passes:
//   k_dyn_walk       the recurrence alone, one channel per lane, states in
//                    registers.  A workgroup is one wave of 64 channels; it
//                    stages its samples through LDS tiles at an odd row pitch
//                    as the phaser does, so that consecutive lanes read and
//                    write consecutive samples of a row in global memory, and
//                    leaves env[t] (the de-esser in split-band mode also the
//                    band cascade's output) in a scratch row per channel.  The
//                    envelope keeps the reference's two branch forms; both
//                    candidates are computed before the compare resolves.  In
//                    listen mode the cascade's output is the result and goes
//                    back in place.
//   k_*_point        everything else, one sample per thread over
//                    (channel x time), in place on the caller's rows; the
//                    de-esser's least gain of the call goes through a partial
//                    per workgroup into metrics.GainReduction (k_deesser_gr).
//
// The lookahead limiter (lookahead_limiter.go:191-210) takes the same two
// passes: k_dyn_walk<LimiterWalker> is the detector envelope of the sidechain
// rows, k_lookahead_point the gain times the program D samples before, read
// from a copy and a history so that in place no thread reads what another
// writes (capi_lookahead.cpp).
//
// Every global index is guarded by the row's length and the channel count; a
// scratch row has pitch >= n + 1 entries and is written at columns 0..n only.
#include "dynfx_kernels.hpp"

#include <algorithm>

#include "dsp_device.hpp"

namespace adsp {
namespace {

// A workgroup barrier that orders the LDS accesses only: global loads and stores in flight stay in flight.
__device__ __forceinline__ void lds_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

struct TransientWalker {
  static constexpr int kTile = kDynWalkTile, kOut = 1;
  double env, attack, release;
  __device__ void load(const DynWalkArgs& a, int64_t ch, bool active) {
    env = a.env[ch];
    attack = a.attack;
    release = a.release;
    if (active) a.env_s[ch * a.pitch] = env;
  }
  __device__ __forceinline__ void step(double in, double (&o)[kOut]) {  // :141-149
#pragma clang fp contract(off)
    const double x = fabs(in);
    const double d = x - env;
    const double ea = env + attack * d, er = env + release * d;
    env = x > env ? ea : er;
    o[0] = env;
  }
  __device__ void save(const DynWalkArgs& a, int64_t ch) { a.env[ch] = env; }
  static __device__ double* out_base(const DynWalkArgs& a, int) { return a.env_s + 1; }
  static __device__ int64_t out_pitch(const DynWalkArgs& a, int) { return a.pitch; }
};

// The limiter's detector (dynamics core.go:331-359, feed-forward, peak, no prefilter): the envelope of |sidechain|.
struct LimiterWalker {
  static constexpr int kTile = kDynWalkTile, kOut = 1;
  double env, attack, release;
  __device__ void load(const DynWalkArgs& a, int64_t ch, bool active) {
    env = a.env[ch];
    attack = a.attack;
    release = a.release;
    if (active) a.env_s[ch * a.pitch] = env;
  }
  __device__ __forceinline__ void step(double in, double (&o)[kOut]) {  // :352-356
#pragma clang fp contract(off)
    const double level = fabs(in);
    const double ea = env + (level - env) * attack, er = level + (env - level) * release;
    env = level > env ? ea : er;
    o[0] = env;
  }
  __device__ void save(const DynWalkArgs& a, int64_t ch) { a.env[ch] = env; }
  static __device__ double* out_base(const DynWalkArgs& a, int) { return a.env_s + 1; }
  static __device__ int64_t out_pitch(const DynWalkArgs& a, int) { return a.pitch; }
};

template <int ORDER, int MODE>
struct DeesserWalker {
  static constexpr bool kListen = MODE == DEESS_LISTEN, kSplit = MODE == DEESS_SPLIT_ONE || MODE == DEESS_SPLIT_TWO;
  static constexpr int kTile = kSplit ? kDynWalkTileMulti : kDynWalkTile, kOut = kSplit ? 2 : 1;
  double env, peak, attack, release, b0, b1, b2, a1, a2;
  double d0[ORDER], d1[ORDER];  // detectFilters
  double e0[ORDER], e1[ORDER];  // bandFilters (DEESS_SPLIT_TWO)
  __device__ void load(const DynWalkArgs& a, int64_t ch, bool active) {
    env = a.env[ch];
    peak = a.peak[ch];
    attack = a.attack, release = a.release;
    b0 = a.b0, b1 = a.b1, b2 = a.b2, a1 = a.a1, a2 = a.a2;
#pragma unroll
    for (int i = 0; i < ORDER; ++i) {
      d0[i] = a.det_state[(ch * kDynMaxOrder + i) * 2];
      d1[i] = a.det_state[(ch * kDynMaxOrder + i) * 2 + 1];
      e0[i] = a.band_state[(ch * kDynMaxOrder + i) * 2];
      e1[i] = a.band_state[(ch * kDynMaxOrder + i) * 2 + 1];
    }
    if (!kListen && active) a.env_s[ch * a.pitch] = env;
  }
  // biquad.Section.ProcessSample section.go:47-53 through the cascade
  __device__ __forceinline__ double cascade(double x, double (&s0)[ORDER], double (&s1)[ORDER]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int i = 0; i < ORDER; ++i) {
      const double y = b0 * x + s0[i];
      s0[i] = b1 * x - a1 * y + s1[i];
      s1[i] = b2 * x - a2 * y;
      x = y;
    }
    return x;
  }
  __device__ __forceinline__ void step(double in, double (&o)[kOut]) {
#pragma clang fp contract(off)
    const double detected = cascade(in, d0, d1);  // :416-419
    if (kListen) {
      o[0] = detected;  // :422-424
      return;
    }
    const double level = fabs(detected);  // :427-432
    const double ea = env + (level - env) * attack, er = level + (env - level) * release;
    env = level > env ? ea : er;
    o[0] = env;
    peak = level > peak ? level : peak;  // :438-440
    if (MODE == DEESS_SPLIT_ONE) o[kOut - 1] = detected;
    if (MODE == DEESS_SPLIT_TWO) o[kOut - 1] = cascade(in, e0, e1);  // :452-455
  }
  __device__ void save(const DynWalkArgs& a, int64_t ch) {
#pragma unroll
    for (int i = 0; i < ORDER; ++i) {
      a.det_state[(ch * kDynMaxOrder + i) * 2] = d0[i];
      a.det_state[(ch * kDynMaxOrder + i) * 2 + 1] = d1[i];
      if (MODE == DEESS_SPLIT_ONE) {  // the band cascade saw the same input from the same states
        a.band_state[(ch * kDynMaxOrder + i) * 2] = d0[i];
        a.band_state[(ch * kDynMaxOrder + i) * 2 + 1] = d1[i];
      }
      if (MODE == DEESS_SPLIT_TWO) {
        a.band_state[(ch * kDynMaxOrder + i) * 2] = e0[i];
        a.band_state[(ch * kDynMaxOrder + i) * 2 + 1] = e1[i];
      }
    }
    if (!kListen) {
      a.env[ch] = env;
      a.peak[ch] = peak;
    }
  }
  static __device__ double* out_base(const DynWalkArgs& a, int k) {
    return kListen ? a.buf : (k == 0 ? a.env_s + 1 : a.band_s);
  }
  static __device__ int64_t out_pitch(const DynWalkArgs& a, int) { return kListen ? a.stride : a.pitch; }
};

template <class W>
__global__ __launch_bounds__(64) void k_dyn_walk(DynWalkArgs a) {
#pragma clang fp contract(off)
  constexpr int T = W::kTile, P = T + 1, NOUT = W::kOut;  // P odd: the lanes of an LDS access group meet no bank twice
  constexpr int kRows = 64 / T;       // rows a staging step of the wave covers
  constexpr int kSteps = 64 / kRows;  // staging steps per chunk
  __shared__ __attribute__((aligned(16))) double tiles[2][NOUT][64 * P];
  const int lane = threadIdx.x;
  const int64_t ch0 = (int64_t)blockIdx.x * 64;
  const int count = (int)(a.channels - ch0 < 64 ? a.channels - ch0 : 64);
  const bool active = lane < count;
  const int64_t ch = ch0 + (active ? lane : 0);
  W w;
  w.load(a, ch, active);
  // staging: consecutive lanes take consecutive samples of a row; step k covers rows k * kRows + rl
  const int tl = lane % T, rl = lane / T;
  const double* in = a.buf + (ch0 + rl) * a.stride + tl;
  double* out[NOUT];
  int64_t opitch[NOUT];
#pragma unroll
  for (int o = 0; o < NOUT; ++o) {
    opitch[o] = W::out_pitch(a, o);
    out[o] = W::out_base(a, o) + (ch0 + rl) * opitch[o] + tl;
  }

  // chunk c is walked in its tile while the loads of chunk c + 1 fly into registers and the stores of
  // chunk c - 1 drain from the other tile (in place in listen mode: the three touch disjoint samples)
  double v[kSteps];
  {
    const int m = (int)(a.n < T ? a.n : T);
#pragma unroll
    for (int k = 0; k < kSteps; ++k)
      v[k] = (k * kRows + rl < count && tl < m) ? in[(int64_t)k * kRows * a.stride] : 0.0;
  }
  int mprev = 0, cur = 0;
  for (int64_t t0 = 0; t0 < a.n; t0 += T, cur ^= 1) {
    const int m = (int)(a.n - t0 < T ? a.n - t0 : T);
#pragma unroll
    for (int k = 0; k < kSteps; ++k) tiles[cur][0][(k * kRows + rl) * P + tl] = v[k];
    lds_barrier();  // the tile is whole; the walk of the chunk before is complete
#pragma unroll
    for (int o = 0; o < NOUT; ++o)
#pragma unroll
      for (int k = 0; k < kSteps; ++k)
        if (k * kRows + rl < count && tl < mprev)
          out[o][(int64_t)k * kRows * opitch[o] + (t0 - T)] = tiles[cur ^ 1][o][(k * kRows + rl) * P + tl];
    const int64_t t1 = t0 + T;
    const int m1 = (int)(t1 >= a.n ? 0 : (a.n - t1 < T ? a.n - t1 : T));
#pragma unroll
    for (int k = 0; k < kSteps; ++k)
      v[k] = (k * kRows + rl < count && tl < m1) ? in[(int64_t)k * kRows * a.stride + t1] : 0.0;
    if (active) {
      double o[NOUT];
      if (m == T) {  // a whole chunk: its samples in registers, so no sample waits for LDS
        double sv[T];
#pragma unroll
        for (int t = 0; t < T; ++t) sv[t] = tiles[cur][0][lane * P + t];
#pragma unroll
        for (int t = 0; t < T; ++t) {
          w.step(sv[t], o);
#pragma unroll
          for (int q = 0; q < NOUT; ++q) tiles[cur][q][lane * P + t] = o[q];
        }
      } else {
        for (int t = 0; t < m; ++t) {
          w.step(tiles[cur][0][lane * P + t], o);
#pragma unroll
          for (int q = 0; q < NOUT; ++q) tiles[cur][q][lane * P + t] = o[q];
        }
      }
    }
    mprev = m;
    lds_barrier();  // this chunk is walked, the one before has left its tile: the next one may take it
  }
  if (a.n > 0) {  // the last chunk
    const int64_t t0 = (a.n - 1) / T * T;
#pragma unroll
    for (int o = 0; o < NOUT; ++o)
#pragma unroll
      for (int k = 0; k < kSteps; ++k)
        if (k * kRows + rl < count && tl < mprev)
          out[o][(int64_t)k * kRows * opitch[o] + t0] = tiles[cur ^ 1][o][(k * kRows + rl) * P + tl];
  }
  if (active) w.save(a, ch);
}

__global__ __launch_bounds__(kDynPointThreads) void k_transient_point(TransientPointArgs a, int tiles) {
#pragma clang fp contract(off)
  const int64_t ch = blockIdx.x / tiles;
  const int tile = (int)(blockIdx.x % tiles);
  double* row = a.buf + ch * a.stride;
  const double* env = a.env_s + ch * a.pitch;
  const int64_t p0 = (int64_t)tile * kDynPointSpan + threadIdx.x;
#pragma unroll
  for (int k = 0; k < kDynPointSteps; ++k) {
    const int64_t t = p0 + (int64_t)k * kDynPointThreads;
    if (t >= a.n) break;
    const double prev = env[t], delta = env[t + 1] - prev;  // :141, :151
    double norm = fabs(delta) / (prev + 1e-9);              // :153-156
    if (norm > 1.0) norm = 1.0;
    double gain = 1.0;  // :158-167
    if (delta >= 0.0)
      gain = gain + a.attack_amount * norm;
    else
      gain = gain + a.sustain_amount * norm;
    if (gain < 0.0) gain = 0.0;
    row[t] = row[t] * gain;  // :169
  }
}

// calculateGain deesser.go:513-557.  2^y via exp2 (Go: math.Pow(2, y)).
__device__ __forceinline__ double deess_gain(const DeessGainParams& p, double level) {
#pragma clang fp contract(off)
  if (level <= 0.0) return 1.0;
  const double overshoot = go_log2(level) - p.threshold_log2;
  double eff;
  if (!p.knee_on) {
    if (overshoot <= 0.0) return 1.0;
    eff = overshoot;
  } else {
    if (overshoot < -p.half_knee) return 1.0;
    if (overshoot > p.half_knee) {
      eff = overshoot;
    } else {
      const double s = overshoot + p.half_knee;
      eff = s * s * 0.5 * p.inv_knee_width_log2;
    }
  }
  const double g = exp2(-eff * p.cf);
  return g < p.range_lin ? p.range_lin : g;
}

template <bool SPLIT>
__global__ __launch_bounds__(kDynPointThreads) void k_deesser_point(DeessPointArgs a, int tiles) {
#pragma clang fp contract(off)
  __shared__ double least[kDynPointThreads];
  __shared__ int nans[kDynPointThreads];
  const int64_t ch = blockIdx.x / tiles;
  const int tile = (int)(blockIdx.x % tiles);
  double* row = a.buf + ch * a.stride;
  const double* env = a.env_s + ch * a.pitch + 1;
  const double* band_row = SPLIT ? a.band_s + ch * a.pitch : nullptr;
  const int64_t p0 = (int64_t)tile * kDynPointSpan + threadIdx.x;
  double mine = __builtin_inf();
  int nan = 0;
#pragma unroll
  for (int k = 0; k < kDynPointSteps; ++k) {
    const int64_t t = p0 + (int64_t)k * kDynPointThreads;
    if (t >= a.n) break;
    const double gain = deess_gain(a.g, env[t]);  // :435
    if (gain == gain)
      mine = gain < mine ? gain : mine;
    else
      nan = 1;
    const double x = row[t];
    const double wide = x * gain;  // :449, :466
    double y = wide;
    if (SPLIT) {
      const double band = band_row[t] * a.band_norm;  // :458
      y = x + band * (gain - 1.0);                     // :462
      if (fabs(y) > fabs(wide)) y = wide;              // :467-469
    }
    row[t] = y;
  }
  least[threadIdx.x] = mine;
  nans[threadIdx.x] = nan;
  __syncthreads();
  for (int w = kDynPointThreads / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) {
      const double o = least[threadIdx.x + w];
      if (o < least[threadIdx.x]) least[threadIdx.x] = o;
      nans[threadIdx.x] |= nans[threadIdx.x + w];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    a.part[(ch * tiles + tile) * 2] = least[0];
    a.part[(ch * tiles + tile) * 2 + 1] = nans[0] ? 1.0 : 0.0;
  }
}

// lookahead_limiter.go:197-209 from env_s: the gain of sample t times the program sample D before it.  The
// program comes from a copy (prog_s) and, for its first D samples, from the history of the calls before, so
// no thread reads a sample of buf that another one writes.
__global__ __launch_bounds__(kDynPointThreads) void k_lookahead_point(LookaheadPointArgs a, int tiles) {
#pragma clang fp contract(off)
  const int64_t ch = blockIdx.x / tiles;
  const int tile = (int)(blockIdx.x % tiles);
  if (ch >= a.channels) return;
  double* row = a.buf + ch * a.stride;
  const double* env = a.env_s + ch * a.pitch + 1;
  const double* prog = a.prog_s + ch * a.prog_pitch;
  const double* hist = a.hist + ch * a.delay;  // the D samples before the call, oldest first
  const int64_t p0 = (int64_t)tile * kDynPointSpan + threadIdx.x;
#pragma unroll
  for (int k = 0; k < kDynPointSteps; ++k) {
    const int64_t t = p0 + (int64_t)k * kDynPointThreads;
    if (t >= a.n) break;
    const double gain = deess_gain(a.g, env[t]);  // GainForLevel core.go:288-309 with knee 0
    const double delayed = t >= a.delay ? prog[t - a.delay] : hist[t];
    row[t] = delayed * gain;
  }
}

// metrics.GainReduction over the call's gains (:442-444).  A gain is at most 1
// and, within a call, a NaN gain is followed by NaN gains only (a NaN envelope
// stays one), so the sequential rule is: the least of the finite gains and the
// value before, and NaN if NaN gains follow while that is still exactly 1.
__global__ __launch_bounds__(64) void k_deesser_gr(const double* part, int tiles, double* gr, int channels) {
  const int ch = blockIdx.x * 64 + threadIdx.x;
  if (ch >= channels) return;
  double m = __builtin_inf();
  bool nan = false;
  for (int i = 0; i < tiles; ++i) {
    const double v = part[((int64_t)ch * tiles + i) * 2];
    if (v < m) m = v;
    if (part[((int64_t)ch * tiles + i) * 2 + 1] != 0.0) nan = true;
  }
  double g = gr[ch];
  if (g == g) {
    if (m < g) g = m;
    if (nan && g == 1.0) g = __builtin_nan("");
  }
  gr[ch] = g;
}

__global__ __launch_bounds__(256) void k_deesser_gain(DeessGainParams g, const double* levels, double* gains, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) gains[i] = deess_gain(g, levels[i]);
}

template <int ORDER>
void launch_deesser_walk_o(const DynWalkArgs& a, hipStream_t s) {
  const dim3 grid((unsigned)((a.channels + 63) / 64));
  switch (a.mode) {
    case DEESS_LISTEN: k_dyn_walk<DeesserWalker<ORDER, DEESS_LISTEN>><<<grid, dim3(64), 0, s>>>(a); break;
    case DEESS_WIDE: k_dyn_walk<DeesserWalker<ORDER, DEESS_WIDE>><<<grid, dim3(64), 0, s>>>(a); break;
    case DEESS_SPLIT_ONE: k_dyn_walk<DeesserWalker<ORDER, DEESS_SPLIT_ONE>><<<grid, dim3(64), 0, s>>>(a); break;
    case DEESS_SPLIT_TWO: k_dyn_walk<DeesserWalker<ORDER, DEESS_SPLIT_TWO>><<<grid, dim3(64), 0, s>>>(a); break;
  }
}

}  // namespace

void launch_transient_walk(const DynWalkArgs& a, hipStream_t s) {
  if (a.n <= 0 || a.channels <= 0) return;
  k_dyn_walk<TransientWalker><<<dim3((unsigned)((a.channels + 63) / 64)), dim3(64), 0, s>>>(a);
}

void launch_deesser_walk(const DynWalkArgs& a, hipStream_t s) {
  if (a.n <= 0 || a.channels <= 0) return;
  switch (a.order) {
    case 1: return launch_deesser_walk_o<1>(a, s);
    case 2: return launch_deesser_walk_o<2>(a, s);
    case 3: return launch_deesser_walk_o<3>(a, s);
    case 4: return launch_deesser_walk_o<4>(a, s);
  }
}

void launch_limiter_walk(const DynWalkArgs& a, hipStream_t s) {
  if (a.n <= 0 || a.channels <= 0) return;
  k_dyn_walk<LimiterWalker><<<dim3((unsigned)((a.channels + 63) / 64)), dim3(64), 0, s>>>(a);
}

void launch_lookahead_point(const LookaheadPointArgs& a, hipStream_t s) {
  if (a.n <= 0 || a.channels <= 0) return;
  const int tiles = deess_point_tiles(a.n);
  k_lookahead_point<<<dim3((unsigned)((int64_t)a.channels * tiles)), dim3(kDynPointThreads), 0, s>>>(a, tiles);
}

int deess_point_tiles(int64_t n) { return (int)std::max<int64_t>(1, (n + kDynPointSpan - 1) / kDynPointSpan); }

void launch_transient_point(const TransientPointArgs& a, hipStream_t s) {
  if (a.n <= 0 || a.channels <= 0) return;
  const int tiles = deess_point_tiles(a.n);
  k_transient_point<<<dim3((unsigned)((int64_t)a.channels * tiles)), dim3(kDynPointThreads), 0, s>>>(a, tiles);
}

void launch_deesser_point(const DeessPointArgs& a, hipStream_t s) {
  if (a.n <= 0 || a.channels <= 0) return;
  const int tiles = deess_point_tiles(a.n);
  const dim3 grid((unsigned)((int64_t)a.channels * tiles));
  if (a.band_s)
    k_deesser_point<true><<<grid, dim3(kDynPointThreads), 0, s>>>(a, tiles);
  else
    k_deesser_point<false><<<grid, dim3(kDynPointThreads), 0, s>>>(a, tiles);
  k_deesser_gr<<<dim3((unsigned)((a.channels + 63) / 64)), dim3(64), 0, s>>>(a.part, tiles, a.gr, a.channels);
}

void launch_deesser_gain(const DeessGainParams& g, const double* levels, double* gains, int64_t n, hipStream_t s) {
  if (n <= 0) return;
  k_deesser_gain<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s>>>(g, levels, gains, n);
}

}  // namespace adsp
