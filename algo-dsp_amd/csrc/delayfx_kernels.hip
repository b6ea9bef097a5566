// effects.Delay.ProcessSample (dsp/effects/delay.go:139-166), the graph's
// delay-simple (dsp/effectchain/runtime_modulation.go:346-362) and
// modulation.Flanger.Process (dsp/effects/modulation/flanger.go:258-282) for
// many channels that share one configuration, bit for bit in the reference's
// operation order (every product and sum rounded on its own, no FMA).
//
// Delay.  Sample n writes slot `write` and reads r0 = floor(write - c) and
// r0 + 1.  Slot write - q holds the write of sample n - q for 1 <= q < len, slot
// `write` itself the one of n - len.  With k = floor(c), float64(write) - c
// rounds to at most write - k, so r0 + 1 is at q >= k - 1: max(1, k - 1)
// consecutive samples read none of each other's writes.  The other way round,
// r0 is at q <= ceil(c), and the slot of q is written again len - q samples
// later: len - ceil(c) consecutive samples overwrite nothing that another of
// them still has to read.  The host takes both bounds over the call's ramp
// (c moves monotonically from its value at the call's start to the target).
//   Regime 1 (k_delay_tile): a launch covers up to min of both bounds samples
//     of every channel, one sample per thread, no barrier; the launches of a
//     call follow each other in the stream.
//   Regime 2 (k_delay_walk): a wave is a tile of 64/S channels x S samples,
//     S a power of two <= the first bound; a workgroup walks the call in
//     sub-blocks of S samples: every read, a barrier, every write, a barrier
//     (so only the first bound applies).
// delay-simple is the same with `pure`: the ring has D slots, sample n reads
// x[n - D] from its own slot and puts x[n] there; nothing is computed.
//
// Flanger.  The taps are write - q, q = max(0, p-1), p, p+1, p+2 with
// p = floor(clamp(max(1, (base + depth * mod) * fs))).  mod is in [0, 1] for any
// sine in [-1, 1], so p >= P = floor(max(1, base * fs)) and max(1, P - 1)
// consecutive samples read none of each other's writes (q = 0 is the sample's
// own slot, still holding the write of n - len).  A workgroup keeps its
// channels' rings in LDS, tiles (channels x samples) over its waves as regime
// 2 does, and stages the input through LDS in chunks of eight sub-blocks.  The
// phase is the same for every channel: one lane steps it through the NEXT
// chunk's samples, a sub-block's worth per sub-block, while the others work on
// this chunk, and all lanes take the chunk's sines together at its start, so a
// sub-block pays neither the phase chain nor the sine's latency.
//
// Ring indices stay in range by construction: 0 <= cur < len, sub-blocks are
// no longer than a ring, every index gets one conditional wrap, and r0 and p
// are clamped as integers, so no input addresses outside a ring.
#include "delayfx_kernels.hpp"

#include <algorithm>

namespace adsp {
namespace {

__device__ __forceinline__ int wrap(int e, int len) {
  if (e < 0) e += len;
  if (e >= len) e -= len;
  return e;
}

// delay.go:145-156: the two read slots and the fraction for write slot w
__device__ __forceinline__ void delay_taps(int w, double c, int len, int& r0, int& r1, double& frac) {
#pragma clang fp contract(off)
  double read_exact = (double)w - c;
  const double buf_len = (double)len;
  // `for readExact < 0`: c <= len - 1, so one pass; bounded whatever c is
  for (int k = 0; k < 2 && read_exact < 0.0; ++k) read_exact = read_exact + buf_len;
  r0 = min(max((int)floor(read_exact), 0), len - 1);
  frac = read_exact - (double)r0;
  r1 = r0 + 1 >= len ? 0 : r0 + 1;
}

struct DelayOut {
  double ring, out;
};

// one sample: its reads and arithmetic, not its stores
__device__ __forceinline__ DelayOut delay_sample(const DelayArgs& a, const double* ring, int w, int64_t t, double in) {
#pragma clang fp contract(off)
  if (a.pure) return {in, ring[w]};
  const double c = t < a.ntraj ? a.traj[t] : a.c_rest;
  int r0, r1;
  double frac;
  delay_taps(w, c, a.len, r0, r1, frac);
  const double delayed = ring[r0] * (1.0 - frac) + ring[r1] * frac;
  return {in + delayed * a.feedback, in * a.one_minus_mix + delayed * a.mix};
}

// wp0: the slot of sample t0; m <= len
__global__ __launch_bounds__(kDelayTileThreads) void k_delay_tile(DelayArgs a, int64_t t0, int m, int wp0, int tiles) {
  const int64_t ch = blockIdx.x / tiles;
  const int s = (int)(blockIdx.x % tiles) * kDelayTileThreads + threadIdx.x;
  if (s >= m) return;
  const int64_t t = t0 + s;
  double* row = a.buf + ch * a.stride;
  double* ring = a.ring + ch * (int64_t)a.len;
  const int w = wrap(wp0 + s, a.len);
  const DelayOut o = delay_sample(a, ring, w, t, row[t]);
  ring[w] = o.ring;
  row[t] = o.out;
}

__global__ __launch_bounds__(kDelayWalkWaves * 64) void k_delay_walk(DelayArgs a, int sub) {
  const int S = sub;
  const int per_wave = 64 / S;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int s = lane % S;
  const int64_t ch = ((int64_t)blockIdx.x * kDelayWalkWaves + wave) * per_wave + lane / S;
  const bool active = ch < a.channels;
  double* row = a.buf + (active ? ch : 0) * a.stride;
  double* ring = a.ring + (active ? ch : 0) * (int64_t)a.len;
  int cur = a.wp;
  for (int64_t t0 = 0; t0 < a.n; t0 += S) {
    const int m = (int)(a.n - t0 < S ? a.n - t0 : S);
    const bool on = active && s < m;
    const int w = wrap(cur + s, a.len);
    DelayOut o{};
    if (on) o = delay_sample(a, ring, w, t0 + s, row[t0 + s]);
    __syncthreads();  // every read of the sub-block before any of its writes
    if (on) {
      ring[w] = o.ring;
      row[t0 + s] = o.out;
    }
    __syncthreads();  // and those before the next sub-block's reads
    cur = wrap(cur + m, a.len);
  }
}

__global__ __launch_bounds__(256) void k_ring_resize(const double* old_ring, int old_len, int old_wp, double* new_ring,
                                                     int new_len, int keep, int channels) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)channels * keep) return;
  const int64_t ch = e / keep;
  const int i = (int)(e % keep);
  new_ring[ch * new_len + (new_len - 1 - i)] = old_ring[ch * old_len + wrap(old_wp - 1 - i, old_len)];
}

__device__ __forceinline__ double hermite4(double t, double xm1, double x0, double x1, double x2) {
#pragma clang fp contract(off)
  // chorus.go:273-280
  const double c1 = 0.5 * (x1 - xm1);
  const double c2 = ((xm1 - 2.5 * x0) + 2.0 * x1) - 0.5 * x2;
  const double c3 = 0.5 * (x2 - xm1) + 1.5 * (x0 - x1);
  return ((c3 * t + c2) * t + c1) * t + x0;
}

__global__ __launch_bounds__(kFlangerMaxWaves * 64) void k_flanger(FlangerArgs a, FlangerShape sh) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) double fl_lds[];
  const int S = sh.sub, K = sh.chunk, pitch = sh.pitch, L = a.len;
  const int G = sh.ch_per_wave * sh.waves;
  double* rings = fl_lds;        // [G][pitch]
  double* xs = rings + G * pitch;  // [G][K] a chunk of the input, then of the output
  double* ph = xs + G * K;       // [2][K] lfoPhase of each sample, this chunk's and the next one's
  double* modv = ph + 2 * K;     // [K] 0.5 (1 + sin(lfoPhase)) of this chunk's samples (:260)
  const int tid = threadIdx.x, threads = blockDim.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int s = lane % S, chl = lane / S;
  const int g = wave * sh.ch_per_wave + chl;  // the lane's channel within the workgroup
  const int64_t ch0 = (int64_t)blockIdx.x * G;
  const int count = (int)(a.channels - ch0 < G ? a.channels - ch0 : G);
  const bool active = chl < sh.ch_per_wave && g < count;
  const bool stepper = tid == threads - 1;
  double* r = rings + (active ? g : 0) * pitch;
  double* xg = xs + (active ? g : 0) * K;
  const double maxd = a.max_delay;

  for (int e = tid; e < count * L; e += threads) rings[(e / L) * pitch + e % L] = a.ring[ch0 * L + e];
  double phase = 0.0;
  if (stepper) {
    phase = *a.phase_in;
    const int m0 = (int)(a.n < K ? a.n : K);
    for (int j = 0; j < m0; ++j) {
      ph[j] = phase;
      phase = phase + a.lfo_inc;  // :276-279
      if (phase >= a.two_pi) phase = phase - a.two_pi;
    }
  }

  int cur = a.wp, k = 0;
  for (int64_t c0 = 0; c0 < a.n; c0 += K, k ^= 1) {
    const int kc = (int)(a.n - c0 < K ? a.n - c0 : K);
    const int64_t left = a.n - c0 - kc;
    const int knext = (int)(left < K ? left : K);  // samples of the next chunk
    for (int e = tid; e < count * K; e += threads)
      if (e % K < kc) xs[e] = a.buf[(ch0 + e / K) * a.stride + c0 + e % K];
    __syncthreads();  // the rings, ph[k]; the previous chunk is done with modv
    for (int e = tid; e < kc; e += threads) modv[e] = 0.5 * (1.0 + sin(ph[k * K + e]));
    __syncthreads();  // the chunk and its modulation
    for (int u0 = 0; u0 < kc; u0 += S) {
      const int m = kc - u0 < S ? kc - u0 : S;
      const bool on = active && s < m;
      const int w = wrap(cur + s, L);
      double in = 0.0, delayed = 0.0;
      if (on) {
        in = xg[u0 + s];
        const double mod = modv[u0 + s];
        double delay = (a.base + a.depth * mod) * a.sample_rate;
        if (delay < 1.0) delay = 1.0;
        if (delay < 0.0) delay = 0.0;  // sampleFractionalDelay :392-411
        if (delay > maxd) delay = maxd;
        const double fl = floor(delay);
        const int p = min(max((int)fl, 0), L - 3);
        const double t = delay - fl;
        const int e2 = wrap(w - p - 2, L);  // delay p + 2, the oldest tap
        const int e1 = wrap(e2 + 1, L);
        const int e0 = wrap(e1 + 1, L);
        const int em = p >= 1 ? wrap(e0 + 1, L) : e0;  // maxInt(0, p - 1)
        delayed = hermite4(t, r[em], r[e0], r[e1], r[e2]);
      }
      if (stepper) {  // the next chunk's phases for the samples this sub-block covers there
        double* pn = ph + (k ^ 1) * K;
        const int jend = u0 + S < knext ? u0 + S : knext;
        for (int j = u0; j < jend; ++j) {
          pn[j] = phase;
          phase = phase + a.lfo_inc;
          if (phase >= a.two_pi) phase = phase - a.two_pi;
        }
      }
      __syncthreads();  // every read of the sub-block before any of its writes; the next phases
      if (on) {
        r[w] = in + delayed * a.feedback;  // :269
        xg[u0 + s] = in * a.one_minus_mix + delayed * a.mix;
      }
      __syncthreads();
      cur = wrap(cur + m, L);
    }
    for (int e = tid; e < count * K; e += threads)
      if (e % K < kc) a.buf[(ch0 + e / K) * a.stride + c0 + e % K] = xs[e];
    __syncthreads();  // before the next chunk replaces xs
  }

  for (int e = tid; e < count * L; e += threads) a.ring[ch0 * L + e] = rings[(e / L) * pitch + e % L];
  if (stepper && blockIdx.x == 0) *a.phase_out = phase;
}

}  // namespace

void launch_delay_tile(const DelayArgs& a, int64_t t0, int m, hipStream_t s) {
  const int tiles = (m + kDelayTileThreads - 1) / kDelayTileThreads;
  const int wp0 = (int)((a.wp + t0) % a.len);
  hipLaunchKernelGGL(k_delay_tile, dim3((unsigned)(a.channels * tiles)), dim3(kDelayTileThreads), 0, s, a, t0, m, wp0,
                     tiles);
}

void launch_delay_walk(const DelayArgs& a, int sub, hipStream_t s) {
  const int group = kDelayWalkWaves * (64 / sub);
  hipLaunchKernelGGL(k_delay_walk, dim3((unsigned)((a.channels + group - 1) / group)), dim3(kDelayWalkWaves * 64), 0, s,
                     a, sub);
}

void launch_ring_resize(const double* old_ring, int old_len, int old_wp, double* new_ring, int new_len, int keep,
                        int channels, hipStream_t s) {
  if (keep <= 0) return;
  const int64_t total = (int64_t)channels * keep;
  hipLaunchKernelGGL(k_ring_resize, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, old_ring, old_len, old_wp,
                     new_ring, new_len, keep, channels);
}

FlangerShape flanger_shape(int block, int len, int channels) {
  FlangerShape sh{};
  sh.sub = pow2_sub(block);
  // pitch = sub (mod 32): the channels of a 32-lane group start 8-byte LDS banks apart by `sub`, so a tile's
  // contiguous reads (lanes = samples) meet no bank twice
  sh.pitch = len + (((sh.sub - len) % 32) + 32) % 32;
  const int cap = kFlangerRingLdsBytes / (sh.pitch * (int)sizeof(double));  // channels whose rings fit (>= 1: validated)
  sh.ch_per_wave = 64 / sh.sub;
  while (sh.ch_per_wave > cap) sh.ch_per_wave /= 2;
  const int want = (channels + sh.ch_per_wave - 1) / sh.ch_per_wave;
  sh.waves = std::max(1, std::min({kFlangerMaxWaves, cap / sh.ch_per_wave, want}));
  sh.chunk = kFlangerChunkSubs * sh.sub;
  return sh;
}

void launch_flanger(const FlangerArgs& a, const FlangerShape& sh, hipStream_t s) {
  const int group = sh.group();
  hipLaunchKernelGGL(k_flanger, dim3((unsigned)((a.channels + group - 1) / group)), dim3(sh.waves * 64),
                     (size_t)sh.lds_bytes(), s, a, sh);
}

}  // namespace adsp
