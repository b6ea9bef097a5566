// modulation.Phaser.Process (dsp/effects/modulation/phaser.go:268-285),
// Tremolo.Process (tremolo.go:201-217) and RingModulator.Process
// (ring_modulator.go:143-153) for many channels that share one configuration,
// in the reference's operation order (every product and sum rounded on its
// own, no FMA).
//
// The LFO phase is the same for every channel and does not depend on the
// input.  The host steps it through the call's samples, one rounded addition
// and one conditional wrap per sample as the reference does, and uploads the
// phases; everything taken from a phase is then taken once per sample, not
// once per sample and channel:
//   k_mod_table      the carrier, the tremolo's target gain or the phaser's
//                    allpass coefficient of every sample, one thread each;
//   k_tremolo_smooth currentMod += (target - currentMod) * coef, a serial
//                    recurrence that is still the same for every channel: one
//                    lane walks the targets chunk by chunk through LDS while a
//                    second wave writes the chunk before back and fetches the
//                    next one;
//   k_mod_apply      s * (1 - mix) + (s * table[t]) * mix over [channels][n],
//                    a 16-byte pair per thread and step.  A row 8 bytes off
//                    16-byte alignment takes its first sample alone and its
//                    pairs from the second one on, so every pair is aligned;
//   k_phaser         the allpass cascade with global feedback: serial along
//                    time, one channel per lane, the stage states in
//                    registers.  A workgroup is one wave of 64 channels; it
//                    stages kPhaserTile samples of each through LDS so that
//                    consecutive lanes read and write consecutive samples of a
//                    row in global memory, and walks them with lane = channel
//                    at an odd row pitch (no LDS bank twice).  A chunk's
//                    loads are issued, all at once, before the chunk in front
//                    of it is walked, and its stores after the walk of the
//                    chunk behind it has begun (two tiles).
//
// Every global index is guarded by the row's length and the channel count; the
// tables have n entries and are read at t < n only.
#include "modfx_kernels.hpp"

#include <algorithm>

namespace adsp {
namespace {

__global__ __launch_bounds__(kModTableThreads) void k_mod_table(ModTableArgs a) {
#pragma clang fp contract(off)
  const int64_t t = (int64_t)blockIdx.x * kModTableThreads + threadIdx.x;
  if (t >= a.n) return;
  const double sn = sin(a.phase[t]);
  double v = sn;
  if (a.kind != MOD_CARRIER) {
    const double lfo = 0.5 * (1.0 + sn);
    if (a.kind == MOD_TARGET) {
      v = a.one_minus_depth + a.depth * lfo;
    } else {
      double f = a.min_hz + a.span_hz * lfo;  // modulatedFrequency :360-363
      if (f < 1.0)                            // phaserAllpassCoefficient :365-379
        f = 1.0;
      else if (f > a.max_allowed)
        f = a.max_allowed;
      const double g = tan(a.pi * f / a.sample_rate);
      v = (isinf(g) || isnan(g)) ? 0.0 : (1.0 - g) / (1.0 + g);
    }
  }
  a.out[t] = v;
}

__global__ __launch_bounds__(128) void k_tremolo_smooth(double* tab, int64_t n, double coef, double* cur_io, int commit) {
#pragma clang fp contract(off)
  constexpr int K = kModSmoothChunk;
  __shared__ __attribute__((aligned(16))) double sm[2][K];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t chunks = (n + K - 1) / K;
  const int m0 = (int)(n < K ? n : K);
  for (int e = tid; e < m0; e += 128) sm[0][e] = tab[e];
  double cur = *cur_io;
  __syncthreads();
  for (int64_t c = 0; c < chunks; ++c) {
    const int k = (int)(c & 1);
    const int64_t t0 = c * K;
    const int m = (int)(n - t0 < K ? n - t0 : K);
    if (wave == 0) {
      if (lane == 0) {
        double* v = sm[k];
        for (int j = 0; j < m; ++j) {
          cur = cur + (v[j] - cur) * coef;  // tremolo.go:206
          v[j] = cur;
        }
      }
    } else {
      // the chunk before goes out and the next one comes in while the stepper walks this one
      double* o = sm[k ^ 1];
      if (c > 0)
        for (int e = lane; e < K; e += 64) tab[t0 - K + e] = o[e];
      const int64_t left = n - t0 - m;
      const int mn = (int)(left < K ? left : K);
      for (int e = lane; e < mn; e += 64) o[e] = tab[t0 + K + e];
    }
    __syncthreads();
  }
  const int64_t t0 = (chunks - 1) * K;
  const int m = (int)(n - t0);
  for (int e = tid; e < m; e += 128) tab[t0 + e] = sm[(chunks - 1) & 1][e];
  if (commit && tid == 0) *cur_io = cur;
}

__device__ __forceinline__ double mod_mix(double s, double g, double mix, double one_minus_mix) {
#pragma clang fp contract(off)
  const double wet = s * g;
  return s * one_minus_mix + wet * mix;
}

__global__ __launch_bounds__(kModApplyThreads) void k_mod_apply(ModApplyArgs a, int tiles) {
#pragma clang fp contract(off)
  const int64_t ch = blockIdx.x / tiles;
  const int tile = (int)(blockIdx.x % tiles);
  double* row = a.buf + ch * a.stride;
  const int64_t lead = (reinterpret_cast<uintptr_t>(row) & 15) ? 1 : 0;  // a row 8 bytes off: its pairs start at sample 1
  const int64_t pairs = (a.n - lead) / 2;
  if (tile == 0 && threadIdx.x < 2) {  // the samples outside the pairs: the first of an off row, an odd one at the end
    const int64_t t = threadIdx.x == 0 ? 0 : lead + 2 * pairs;
    if (threadIdx.x == 0 ? lead == 1 : t < a.n) row[t] = mod_mix(row[t], a.tab[t], a.mix, a.one_minus_mix);
  }
  const int64_t p0 = (int64_t)tile * (kModApplyThreads * kModApplySteps) + threadIdx.x;
#pragma unroll
  for (int k = 0; k < kModApplySteps; ++k) {
    const int64_t p = p0 + (int64_t)k * kModApplyThreads;
    if (p >= pairs) break;
    const int64_t t = lead + 2 * p;
    double2* q = reinterpret_cast<double2*>(row + t);
    double2 v = *q;
    v.x = mod_mix(v.x, a.tab[t], a.mix, a.one_minus_mix);
    v.y = mod_mix(v.y, a.tab[t + 1], a.mix, a.one_minus_mix);
    *q = v;
  }
}

// A workgroup barrier that orders the LDS accesses only: global loads and stores in flight stay in flight.
__device__ __forceinline__ void lds_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// Phaser.Process :268-285 for one sample s with the coefficient c: advances the stage states and the feedback sample
template <int S>
__device__ __forceinline__ double phaser_sample(double s, double c, double (&x1)[S], double (&y1)[S], double& fb,
                                                const PhaserArgs& a) {
#pragma clang fp contract(off)
  double y = s + fb * a.feedback;  // :269
#pragma unroll
  for (int i = 0; i < S; ++i) {  // phaserAllpassStage.process :122-128
    const double x = y;
    y = c * x + x1[i] - c * y1[i];
    x1[i] = x;
    y1[i] = y;
  }
  fb = y;
  return s * a.one_minus_mix + y * a.mix;  // :284
}

template <int S>
__global__ __launch_bounds__(64) void k_phaser(PhaserArgs a) {
#pragma clang fp contract(off)
  constexpr int T = kPhaserTile, P = kPhaserPitch;
  constexpr int kRows = 64 / T;      // rows a staging step of the wave covers
  constexpr int kSteps = 64 / kRows;  // staging steps per chunk
  __shared__ __attribute__((aligned(16))) double tiles[2][64 * P];
  __shared__ __attribute__((aligned(16))) double cf[T];
  const int lane = threadIdx.x;
  const int64_t ch0 = (int64_t)blockIdx.x * 64;
  const int count = (int)(a.channels - ch0 < 64 ? a.channels - ch0 : 64);
  const bool active = lane < count;
  const int64_t ch = ch0 + (active ? lane : 0);
  double x1[S], y1[S];
  double* st = a.stage + ch * (2 * kPhaserMaxStages);
#pragma unroll
  for (int i = 0; i < S; ++i) {
    x1[i] = st[2 * i];
    y1[i] = st[2 * i + 1];
  }
  double fb = a.fb[ch];
  // staging: consecutive lanes take consecutive samples of a row; step k covers rows k * kRows + rl
  const int tl = lane % T, rl = lane / T;
  double* io = a.buf + (ch0 + rl) * a.stride + tl;

  // Three chunks are under way at a time, none waiting for another's memory
  // traffic: chunk c is walked in its tile while the loads of chunk c + 1 fly
  // into registers and the stores of chunk c - 1 drain from the other tile.
  // (In place: the three touch disjoint samples of the rows.)
  double v[kSteps], cnext = 0.0;
  {
    const int m = (int)(a.n < T ? a.n : T);
#pragma unroll
    for (int k = 0; k < kSteps; ++k)
      v[k] = (k * kRows + rl < count && tl < m) ? io[(int64_t)k * kRows * a.stride] : 0.0;
    if (lane < m) cnext = a.coef[lane];
  }
  int mprev = 0, cur = 0;
  for (int64_t t0 = 0; t0 < a.n; t0 += T, cur ^= 1) {
    const int m = (int)(a.n - t0 < T ? a.n - t0 : T);
    double* tile = tiles[cur];
    const double* done = tiles[cur ^ 1];
#pragma unroll
    for (int k = 0; k < kSteps; ++k) tile[(k * kRows + rl) * P + tl] = v[k];
    if (lane < T) cf[lane] = cnext;
    lds_barrier();  // the tile and its coefficients; the walk of the chunk before is complete
#pragma unroll
    for (int k = 0; k < kSteps; ++k)
      if (k * kRows + rl < count && tl < mprev) io[(int64_t)k * kRows * a.stride + (t0 - T)] = done[(k * kRows + rl) * P + tl];
    const int64_t t1 = t0 + T;
    const int m1 = (int)(t1 >= a.n ? 0 : (a.n - t1 < T ? a.n - t1 : T));
#pragma unroll
    for (int k = 0; k < kSteps; ++k)
      v[k] = (k * kRows + rl < count && tl < m1) ? io[(int64_t)k * kRows * a.stride + t1] : 0.0;
    if (lane < m1) cnext = a.coef[t1 + lane];
    if (active) {
      double* mine = tile + lane * P;
      if (m == T) {  // a whole chunk: its samples and coefficients in registers, so no sample waits for LDS
        double sv[T], cv[T];
#pragma unroll
        for (int t = 0; t < T; ++t) {
          sv[t] = mine[t];
          cv[t] = cf[t];
        }
#pragma unroll
        for (int t = 0; t < T; ++t) sv[t] = phaser_sample<S>(sv[t], cv[t], x1, y1, fb, a);
#pragma unroll
        for (int t = 0; t < T; ++t) mine[t] = sv[t];
      } else {
        for (int t = 0; t < m; ++t) mine[t] = phaser_sample<S>(mine[t], cf[t], x1, y1, fb, a);
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
#pragma unroll
    for (int i = 0; i < S; ++i) {
      st[2 * i] = x1[i];
      st[2 * i + 1] = y1[i];
    }
    a.fb[ch] = fb;
  }
}

template <int S>
void launch_phaser_s(const PhaserArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_phaser<S>, dim3((unsigned)((a.channels + 63) / 64)), dim3(64), 0, s, a);
}

}  // namespace

void launch_mod_table(const ModTableArgs& a, hipStream_t s) {
  if (a.n <= 0) return;
  hipLaunchKernelGGL(k_mod_table, dim3((unsigned)((a.n + kModTableThreads - 1) / kModTableThreads)),
                     dim3(kModTableThreads), 0, s, a);
}

void launch_tremolo_smooth(double* tab, int64_t n, double coef, double* cur, int commit, hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_tremolo_smooth, dim3(1), dim3(128), 0, s, tab, n, coef, cur, commit);
}

void launch_mod_apply(const ModApplyArgs& a, hipStream_t s) {
  if (a.n <= 0) return;
  constexpr int64_t per_tile = (int64_t)kModApplyThreads * kModApplySteps;
  const int tiles = (int)std::max<int64_t>(1, (a.n / 2 + per_tile - 1) / per_tile);
  hipLaunchKernelGGL(k_mod_apply, dim3((unsigned)((int64_t)a.channels * tiles)), dim3(kModApplyThreads), 0, s, a, tiles);
}

void launch_phaser(const PhaserArgs& a, hipStream_t s) {
  if (a.n <= 0) return;
  switch (a.stages) {
    case 1: return launch_phaser_s<1>(a, s);
    case 2: return launch_phaser_s<2>(a, s);
    case 3: return launch_phaser_s<3>(a, s);
    case 4: return launch_phaser_s<4>(a, s);
    case 5: return launch_phaser_s<5>(a, s);
    case 6: return launch_phaser_s<6>(a, s);
    case 7: return launch_phaser_s<7>(a, s);
    case 8: return launch_phaser_s<8>(a, s);
    case 9: return launch_phaser_s<9>(a, s);
    case 10: return launch_phaser_s<10>(a, s);
    case 11: return launch_phaser_s<11>(a, s);
    case 12: return launch_phaser_s<12>(a, s);
  }
}

}  // namespace adsp
