// Short-frame STFT overlap-add for gfx950 (CDNA4), FP64: the kernels behind
// ad_specfreeze_* and ad_pitchspec_* (dsp/effects/spectral_freeze.go,
// dsp/effects/pitch/pitch_shift_spectral.go).
//
// Four passes, each one launch over a group of channels:
//   frames   one N-point complex transform per (channel, frame) in LDS
//            (fft_device.hpp; Plan::F frames per workgroup at N <= 1024):
//            ANALYSIS windows the frame, transforms, pins bins 0 and N/2 and
//            writes hypot / atan2; SYNTH reads magnitude and phase, forms
//            mag cos, mag sin with the full-range sincos, mirrors, transforms
//            back and writes the windowed frame; FUSED does both with nothing
//            written in between (the unfrozen freeze);
//   walk     the only serial part: one workgroup per channel, lanes over bins,
//            a loop over frames, in the reference's operations and order;
//   ola      a gather: each output sample sums the frames that cover it in
//            ascending frame order, norm the same way; no atomics.
// The walk and the overlap-add are compiled without floating-point
// contraction (the second half of this file): delta = phase - prevPhase -
// omega*hop and phaseAcc += omega*hop decide a wrap at +-pi, and norm += w*w
// is compared bit for bit.
#include <hip/hip_runtime.h>

#include "ad_common.hpp"
#include "fft_device.hpp"
#include "stft_kernels.hpp"

namespace adsp {

namespace {

template <int N>
struct StftPlan {
  static constexpr int V = N <= 1024 ? 8 : 16;
  using Plan = FftPlan<N, V>;
};

// lds[k], k <= N/2, holds the half spectrum: the thread's pass-0 values of the
// inverse transform are its conjugate mirror with real bins 0 and N/2
// (spectral_freeze.go:288-294).
template <int N, int V>
__device__ __forceinline__ void gather_mirrored(double2* v, int tid, const double2* lds) {
#pragma unroll
  for (int s = 0; s < V; ++s) {
    const int i = pass0_index<N, V>(tid, s);
    const int k = i <= N / 2 ? i : N - i;
    double2 z = lds[k];
    if (i == 0 || i == N / 2)
      z.y = 0.0;
    else if (i > N / 2)
      z.y = -z.y;
    v[s] = z;
  }
}

template <int N, int MODE>
__global__ __launch_bounds__((StftPlan<N>::Plan::BLOCK)) void k_stft_frames(StftFrameArgs a) {
  constexpr int V = StftPlan<N>::V;
  using Plan = typename StftPlan<N>::Plan;
  constexpr int T = Plan::T, F = Plan::F, HALF = N / 2;
  __shared__ __attribute__((aligned(16))) double2 lds_all[F * Plan::MP];
  __shared__ __attribute__((aligned(16))) double2 twtab[TwSplit<N>::N];
  const int f = threadIdx.x / T;
  const int tid = threadIdx.x % T;
  const int64_t e = (int64_t)blockIdx.x * F + f;
  const bool active = e < (int64_t)a.channels * a.frames;
  const int64_t c = active ? e / a.frames : 0;
  const int64_t j = active ? e % a.frames : 0;
  double2* lds = lds_all + f * Plan::MP;
  const TwLds<N> tw = tw_lds_compute<N>(twtab, threadIdx.x, Plan::BLOCK);
  __syncthreads();

  double2 v[V];
  if constexpr (MODE != STFT_SYNTH) {
    const double* xc = a.x + c * a.x_stride;
    const int64_t pos = j * a.hop;
#pragma unroll
    for (int s = 0; s < V; ++s) {
      const int i = pass0_index<N, V>(tid, s);
      const int64_t idx = pos + i;
      const double x = (active && idx < a.n) ? xc[idx] : 0.0;  // zero-padded past the end
      v[s] = make_double2(x * a.win[i], 0.0);
    }
    fft_run<N, V, true>(v, tid, lds, tw);
    // polar form of bins 0 ... N/2; the imaginary parts of bins 0 and N/2 are +0.0 by decision
    double* mg = a.mag + c * a.mag_ch + j * a.mag_fr;
    double* ph = a.phase + c * a.ph_ch + j * a.ph_fr;
    if constexpr (MODE == STFT_FUSED) __syncthreads();  // every lane has loaded its last pass
#pragma unroll
    for (int s = 0; s < V; ++s) {
      const int k = last_pass_index<N, V>(tid, s);
      if (k > HALF) continue;
      const double re = v[s].x;
      const double im = (k == 0 || k == HALF) ? 0.0 : v[s].y;
      const double m = hypot(re, im);
      const double p = atan2(im, re);
      if constexpr (MODE == STFT_ANALYSIS) {
        if (active) {
          mg[k] = m;
          ph[k] = p;
        }
      } else {
        double sn, cs;
        sincos(p, &sn, &cs);
        lds[k] = make_double2(m * cs, m * sn);
      }
    }
    if constexpr (MODE == STFT_ANALYSIS) return;
  } else {
    const double* mg = a.mag + c * a.mag_ch + j * a.mag_fr;
    const double* ph = a.phase + c * a.ph_ch + j * a.ph_fr;
    for (int k = tid; k <= HALF; k += T) {
      double2 z = make_double2(0.0, 0.0);
      if (active) {
        const double m = mg[k];
        double sn, cs;
        sincos(ph[k], &sn, &cs);
        z = make_double2(m * cs, m * sn);
      }
      lds[k] = z;
    }
  }
  __syncthreads();
  gather_mirrored<N, V>(v, tid, lds);
  __syncthreads();
  fft_run<N, V, false>(v, tid, lds, tw);
  if (!active) return;
  double* row = a.rows + c * a.row_ch + j * a.row_fr;
  constexpr double inv_n = 1.0 / (double)N;  // the inverse transform's factor: a power of two
#pragma unroll
  for (int s = 0; s < V; ++s) {
    const int i = last_pass_index<N, V>(tid, s);
    row[i] = (v[s].x * inv_n) * a.win[i];
  }
}

template <int N>
void launch_frames_n(int mode, const StftFrameArgs& a, hipStream_t s) {
  using Plan = typename StftPlan<N>::Plan;
  const int64_t items = (int64_t)a.channels * a.frames;
  if (items <= 0) return;
  const int64_t grid = (items + Plan::F - 1) / Plan::F;
  if (grid > 0x7fffffffLL) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "stft: too many frames in one pass");
  const dim3 g((unsigned)grid), b(Plan::BLOCK);
  switch (mode) {
    case STFT_ANALYSIS: hipLaunchKernelGGL((k_stft_frames<N, STFT_ANALYSIS>), g, b, 0, s, a); break;
    case STFT_SYNTH: hipLaunchKernelGGL((k_stft_frames<N, STFT_SYNTH>), g, b, 0, s, a); break;
    case STFT_FUSED: hipLaunchKernelGGL((k_stft_frames<N, STFT_FUSED>), g, b, 0, s, a); break;
    default: AD_FAIL(AD_ERR_INTERNAL, "stft: unknown frame pass");
  }
}

}  // namespace

void launch_stft_frames(int frame, int mode, const StftFrameArgs& a, hipStream_t s) {
  switch (frame) {
    case 64: launch_frames_n<64>(mode, a, s); break;
    case 128: launch_frames_n<128>(mode, a, s); break;
    case 256: launch_frames_n<256>(mode, a, s); break;
    case 512: launch_frames_n<512>(mode, a, s); break;
    case 1024: launch_frames_n<1024>(mode, a, s); break;
    case 2048: launch_frames_n<2048>(mode, a, s); break;
    case 4096: launch_frames_n<4096>(mode, a, s); break;
    default: AD_FAIL(AD_ERR_INVALID_ARGUMENT, "stft: frame size must be a power of two in [64, 4096]");
  }
}

// ---------------------------------------------------------------------------
// From here on: no floating-point contraction.
// ---------------------------------------------------------------------------
#pragma clang fp contract(off)

namespace {

constexpr int kWalkBlock = 512;
constexpr int walk_bins_per_thread(int frame) { return (frame / 2 + 1 + kWalkBlock - 1) / kWalkBlock; }

__device__ __forceinline__ double wrap_phase(double x) {  // wrapPhase pitch_shift_spectral.go:627-634
  constexpr double kPi = 3.14159265358979323846;
  x = fmod(x + kPi, 2 * kPi);
  if (x < 0) x += 2 * kPi;
  return x - kPi;
}

// Nearest set bit of `words` to k (k itself is not set), a tie to the lower:
// what the forward walk of :460-471 settles on.  At least one bit is set.
__device__ __forceinline__ int nearest_peak(const unsigned long long* words, int nwords, int k) {
  int lower = -1, upper = -1;
  {
    int w = k >> 6;
    unsigned long long m = words[w] & (~0ull >> (63 - (k & 63)));
    while (m == 0 && w > 0) m = words[--w];
    if (m != 0) lower = (w << 6) + 63 - __clzll((long long)m);
  }
  {
    int w = k >> 6;
    unsigned long long m = words[w] & (~0ull << (k & 63));
    while (m == 0 && w + 1 < nwords) m = words[++w];
    if (m != 0) upper = (w << 6) + __ffsll((long long)m) - 1;
  }
  if (lower < 0) return upper;
  if (upper < 0) return lower;
  return (upper - k) < (k - lower) ? upper : lower;
}

// processBinShift :300-359 and processTimeStretch :405-483 between the
// transforms.  One workgroup per channel; thread t owns bins t, t + 512, ...: KPT of them, by the frame size
// (1 up to N = 512, 2 at 1024, 3 at 2048, 5 at 4096), so that registers and LDS are what the frame needs.
template <int MODE, int KPT>
__global__ __launch_bounds__(kWalkBlock) void k_stft_walk(StftWalkArgs a, int half) {
  constexpr int kWalkBinsPerThread = KPT;
  constexpr int kSlots = KPT * kWalkBlock;  // >= bins
  __shared__ double s_mag[kSlots];
  __shared__ double s_aux[kSlots];  // bin shift: instFreqs; stretch: prevPhase
  __shared__ double s_sum[MODE == STFT_WALK_STRETCH ? kSlots : 1];
  __shared__ unsigned long long s_words[kSlots / 64];
  const int c = blockIdx.x;
  const int tid = threadIdx.x;
  const int bins = half + 1;
  const int nwords = (bins + 63) >> 6;
  double* rows = a.rows + (int64_t)c * a.row_ch;
  double prev[kWalkBinsPerThread], sum[kWalkBinsPerThread], om[kWalkBinsPerThread];
#pragma unroll
  for (int q = 0; q < kWalkBinsPerThread; ++q) {
    const int k = tid + q * kWalkBlock;
    prev[q] = 0.0;  // Reset() :222-227 at the start of every call
    sum[q] = 0.0;
    om[q] = k < bins ? a.omega[k] : 0.0;
    if (MODE == STFT_WALK_STRETCH && k < bins) s_sum[k] = 0.0;
  }
  const double hop_f = a.hop_f, syn_f = a.syn_hop_f, ratio = a.ratio;
  // the bin shift's source position of every bin (:335-345) does not change from frame to frame
  int lo_of[kWalkBinsPerThread];  // -1: srcK >= half, a dead bin
  double frac_of[kWalkBinsPerThread];
  // the next frame's rows are loaded a frame ahead, so the walk waits for LDS and barriers, not for memory
  double next_mag[kWalkBinsPerThread], next_phase[kWalkBinsPerThread];
#pragma unroll
  for (int q = 0; q < kWalkBinsPerThread; ++q) {
    const int k = tid + q * kWalkBlock;
    const double src_k = (double)k / ratio;
    const bool dead = src_k >= (double)half;
    lo_of[q] = dead ? -1 : (int)src_k;
    frac_of[q] = dead ? 0.0 : src_k - (double)(int)src_k;
    next_mag[q] = (k < bins && a.frames > 0) ? rows[k] : 0.0;
    next_phase[q] = (k < bins && a.frames > 0) ? rows[bins + k] : 0.0;
  }
  for (int64_t j = 0; j < a.frames; ++j) {
    double* mg = rows + j * a.row_fr;
    double* ph = mg + bins;
    double inst[kWalkBinsPerThread], cur_mag[kWalkBinsPerThread], cur_phase[kWalkBinsPerThread];
#pragma unroll
    for (int q = 0; q < kWalkBinsPerThread; ++q) {
      const int k = tid + q * kWalkBlock;
      cur_mag[q] = next_mag[q];
      cur_phase[q] = next_phase[q];
      if (k < bins && j + 1 < a.frames) {
        next_mag[q] = mg[a.row_fr + k];
        next_phase[q] = ph[a.row_fr + k];
      }
    }
#pragma unroll
    for (int q = 0; q < kWalkBinsPerThread; ++q) {
      const int k = tid + q * kWalkBlock;
      inst[q] = 0.0;
      if (k < bins) {
        const double phase = cur_phase[q];
        double delta = phase - prev[q] - om[q] * hop_f;  // :326, :432
        delta = wrap_phase(delta);
        inst[q] = om[q] + delta / hop_f;
        prev[q] = phase;
        s_mag[k] = cur_mag[q];
        s_aux[k] = MODE == STFT_WALK_BINSHIFT ? inst[q] : phase;
      }
    }
    if constexpr (MODE == STFT_WALK_BINSHIFT) {
      __syncthreads();
#pragma unroll
      for (int q = 0; q < kWalkBinsPerThread; ++q) {
        const int k = tid + q * kWalkBlock;
        if (k < bins) {
          double sm, sf;
          if (lo_of[q] < 0) {  // :336-341
            sm = 0.0;
            sf = om[q];
          } else {
            const int lo = lo_of[q];
            const double frac = frac_of[q];
            const int hi = lo + 1 < half ? lo + 1 : half;
            sm = s_mag[lo] * (1 - frac) + s_mag[hi] * frac;
            const double interp = s_aux[lo] * (1 - frac) + s_aux[hi] * frac;
            sf = interp * ratio;
          }
          sum[q] += sf * hop_f;  // :354
          mg[k] = sm;
          ph[k] = sum[q];
        }
      }
      __syncthreads();
    } else {
      __syncthreads();
      int mine = 0;
#pragma unroll
      for (int q = 0; q < kWalkBinsPerThread; ++q) {
        const int k = tid + q * kWalkBlock;  // a wave's 64 lanes: 64 consecutive bins from a multiple of 64
        const bool peak = k >= 1 && k < half && s_mag[k] >= s_mag[k - 1] && s_mag[k] > s_mag[k + 1];  // :441-445
        const unsigned long long word = __ballot(peak);
        if ((tid & 63) == 0 && (k >> 6) < nwords) s_words[k >> 6] = word;
        if (peak) {
          s_sum[k] += inst[q] * syn_f;  // :456-458
          mine |= 1 << q;
        }
      }
      const int any = __syncthreads_or(mine);
#pragma unroll
      for (int q = 0; q < kWalkBinsPerThread; ++q) {
        const int k = tid + q * kWalkBlock;
        if (k < bins) {
          if (!any) {
            s_sum[k] += inst[q] * syn_f;  // :447-454
          } else if (!(mine & (1 << q))) {
            const int pk = nearest_peak(s_words, nwords, k);
            s_sum[k] = s_sum[pk] + (s_aux[k] - s_aux[pk]);  // :473-476: peaks are not written here
          }
          ph[k] = s_sum[k];
        }
      }
      __syncthreads();
    }
  }
}

template <int MODE, int KPT>
void launch_walk(const StftWalkArgs& a, int frame, hipStream_t s) {
  hipLaunchKernelGGL((k_stft_walk<MODE, KPT>), dim3((unsigned)a.channels), dim3(kWalkBlock), 0, s, a, frame / 2);
}

__global__ __launch_bounds__(256) void k_stft_freeze_walk(StftFreezeWalkArgs a) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)a.channels * a.bins) return;
  const int64_t c = e / a.bins;
  const int k = (int)(e % a.bins);
  double acc = a.phase_acc[e];
  const double step = a.omega[k] * a.hop_f;
  double* ph = a.rows + c * a.row_ch + a.bins + k;
  for (int64_t j = 0; j < a.frames; ++j) {
    if (a.advance && !(a.just_captured && j == 0)) acc += step;  // spectral_freeze.go:264-266
    ph[j * a.row_fr] = acc;
  }
  a.phase_acc[e] = acc;
}

__global__ __launch_bounds__(256) void k_stft_ola(StftOlaArgs a) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int c = blockIdx.y;
  if (i >= a.out_n) return;
  const int64_t last = a.frames - 1;
  int64_t hi = i / a.hop;
  if (hi > last) hi = last;
  const int64_t lo = i >= a.frame ? (i - a.frame) / a.hop + 1 : 0;
  const double* rows = a.rows + (int64_t)c * a.row_ch;
  double wet = 0.0, norm = 0.0;
  for (int64_t j = lo; j <= hi; ++j) {
    const int64_t t = i - j * a.hop;  // in [0, frame)
    const double w = a.win[t];
    if (!a.norm_only) wet += rows[j * a.row_fr + t];
    norm += w * w;
  }
  double* o = a.out + (int64_t)c * a.out_stride + i;
  if (a.norm_only) {
    *o = norm;
    return;
  }
  if (norm > kStftNormFloor) wet /= norm;
  *o = a.mix_dry ? *o * (1 - a.mix) + wet * a.mix : wet;  // spectral_freeze.go:316
}

}  // namespace

void launch_stft_walk(int frame, int mode, const StftWalkArgs& a, hipStream_t s) {
  if (frame < kStftMinFrame || frame > kStftMaxFrame || !is_pow2(frame))
    AD_FAIL(AD_ERR_INVALID_ARGUMENT, "stft: frame size must be a power of two in [64, 4096]");
  if (a.channels <= 0 || a.frames <= 0) return;
  const bool shift = mode == STFT_WALK_BINSHIFT;
  switch (walk_bins_per_thread(frame)) {
    case 1: shift ? launch_walk<STFT_WALK_BINSHIFT, 1>(a, frame, s) : launch_walk<STFT_WALK_STRETCH, 1>(a, frame, s); break;
    case 2: shift ? launch_walk<STFT_WALK_BINSHIFT, 2>(a, frame, s) : launch_walk<STFT_WALK_STRETCH, 2>(a, frame, s); break;
    case 3: shift ? launch_walk<STFT_WALK_BINSHIFT, 3>(a, frame, s) : launch_walk<STFT_WALK_STRETCH, 3>(a, frame, s); break;
    default: shift ? launch_walk<STFT_WALK_BINSHIFT, 5>(a, frame, s) : launch_walk<STFT_WALK_STRETCH, 5>(a, frame, s); break;
  }
}

void launch_stft_freeze_walk(const StftFreezeWalkArgs& a, hipStream_t s) {
  const int64_t items = (int64_t)a.channels * a.bins;
  if (items <= 0 || a.frames <= 0) return;
  hipLaunchKernelGGL(k_stft_freeze_walk, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, s, a);
}

void launch_stft_ola(const StftOlaArgs& a, hipStream_t s) {
  if (a.channels <= 0 || a.out_n <= 0) return;
  if (a.channels > 65535) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "stft: more than 65535 channels in one pass");
  hipLaunchKernelGGL(k_stft_ola, dim3((unsigned)((a.out_n + 255) / 256), (unsigned)a.channels), dim3(256), 0, s, a);
}

}  // namespace adsp
