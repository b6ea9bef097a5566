// FDNReverb.ProcessSample (dsp/effects/reverb/fdn_reverb.go:199-241) for many
// channels that share one configuration, bit for bit in the reference's
// operation order (every product and sum rounded on its own, no FMA).
//
// Dependencies.  Sample n of a line reads that line's writes at times
// n-1-q, q = max(0, p-1), p, p+1, p+2 with p = floor(delay) (:369-390: the read
// comes before the sample's own write, so delay 0 is the write of n-1).  The
// modulation lies in [0, 1] and the depth is >= 0, so delay >= base[0] * scale
// and p >= P = floor(1537 * scale): the newest write a read can touch is
// n - max(P, 1).  max(1, P) consecutive samples therefore read nothing that any
// of them writes.  A workgroup owns one channel and walks its call in
// sub-blocks of `sub` <= max(1, P) samples (also <= kFdnMaxSub, the LDS budget):
//   1. pre-delay (:201-205), a feed-forward 4-point Hermite read of the input
//      (the sub-block's own samples from LDS, older ones from the ring);
//   2. the eight lines' modulated reads (:207-213), wave i = line i, lanes =
//      samples: coalesced ring reads, all of a lane's taps requested before
//      the first is used, d -> LDS [line][sample];
//   3. the Hadamard feedback rows times (1 - damp) -> LDS (wave i = row i), and
//      the output (:233-240) into the caller's row;
//   4. the two serial recurrences: lanes 0..7 of wave 0 run the damping filter
//      (:227-228; one line each, a rounded multiply and add per sample, the
//      inputs read from LDS eight samples ahead of the chain), and
//      one lane of wave 1 meanwhile steps the LFO phase (:215-218) through the
//      NEXT sub-block's samples, so the phase chain never adds to the serial time;
//   5. the line writes (:229-230) from the filtered values, coalesced.
// The rings live in global memory ([channels][len] per line, about 165 KB per
// channel at 48 kHz); a workgroup is the only reader and writer of its
// channel's rings, ordered by its own barriers.  Every workgroup computes the
// phase sequence itself: no workgroup waits for another.
//
// Ring indices stay in range by construction: 0 <= cur < len, sub <= len, and
// p is clamped to [0, len - 3] as an integer as well, so even a NaN delay
// addresses inside the ring.
#include "fdn_kernels.hpp"

namespace adsp {
namespace {

__device__ __forceinline__ double hermite4(double t, double xm1, double x0, double x1, double x2) {
#pragma clang fp contract(off)
  // interp_helpers.go:3-10
  const double c1 = 0.5 * (x1 - xm1);
  const double c2 = ((xm1 - 2.5 * x0) + 2.0 * x1) - 0.5 * x2;
  const double c3 = 0.5 * (x2 - xm1) + 1.5 * (x0 - x1);
  return ((c3 * t + c2) * t + c1) * t + x0;
}

__device__ __forceinline__ int wrap(int e, int len) {
  if (e < 0) e += len;
  if (e >= len) e -= len;
  return e;
}

__global__ __launch_bounds__(kFdnThreads) void k_fdn(FdnArgs a) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) double fdn_lds[];
  const int S = a.sub;
  const int pitch = fdn_pitch(S);
  double* xs = fdn_lds;                // [S] the raw input
  double* ins = xs + S;                // [S] in * inputGain
  double* ph = ins + S;                // [2][S] lfoPhase of each sample, this sub-block's and the next one's
  double* dl = ph + 2 * S;             // [8][pitch] the reads d, then the filtered values
  double* ul = dl + kFdnLines * pitch;  // [8][pitch] feedback * (1 - damp)
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int i = __builtin_amdgcn_readfirstlane(tid >> 6);  // this wave's line
  const int64_t c = blockIdx.x;
  const int64_t n = a.n;
  double* row = a.buf + c * a.stride;
  const int L = a.len[i];
  double* ring = a.line[i] + c * L;
  const int Lp = a.pre_len;
  double* pring = a.pre + c * Lp;
  const double base = a.base[i], off = a.offset[i], fbg = a.fb_gain[i];
  const double maxd = (double)(L - 3);
  int cur = a.wp[i];      // ring slot of this sub-block's first write
  int curp = a.pre_wp;

  // the pre-delay's constant read position (:355-370)
  const bool has_pre = a.pre_delay > 0.0;
  int pp = 0, pq0 = 0;
  double pt = 0.0;
  if (has_pre) {
    double d = a.pre_delay;
    const double md = (double)(Lp - 3);
    if (d > md) d = md;
    const double fl = floor(d);
    pp = min(max((int)fl, 0), Lp - 3);
    pt = d - fl;
    pq0 = max(0, pp - 1);
  }

  double fs = 0.0, phase = 0.0;
  if (tid < kFdnLines) fs = a.fstate[c * kFdnLines + tid];
  if (tid == 64) {
    phase = *a.phase_in;
    const int m0 = (int)(n < S ? n : S);
    for (int s = 0; s < m0; ++s) {
      ph[s] = phase;
      phase = phase + a.lfo_inc;
      if (phase >= a.two_pi) phase = phase - a.two_pi;
    }
  }

  int k = 0;
  for (int64_t t0 = 0; t0 < n; t0 += S, k ^= 1) {
    const int m = (int)(n - t0 < S ? n - t0 : S);
    const int64_t left = n - t0 - m;
    const int mnext = (int)(left < S ? left : S);
    for (int s = tid; s < m; s += kFdnThreads) xs[s] = row[t0 + s];
    __syncthreads();  // xs, ph[k]; and the previous sub-block's ring writes

    // 1. pre-delay: the write of sample s is delay 0 (:202-205)
    for (int s = tid; s < m; s += kFdnThreads) {
      double in = xs[s];
      if (has_pre) {
        auto tap = [&](int q) { return q <= s ? xs[s - q] : pring[wrap(curp + s - q, Lp)]; };
        in = hermite4(pt, tap(pq0), tap(pp), tap(pp + 1), tap(pp + 2));
      }
      ins[s] = in * a.gain;
    }
    // 2. the lines' reads (:207-213).  First every sample's delay (each lane
    // parks its own in `ul`, free until step 3, and reads them back itself).
    // Then a lane's samples lane, lane + 64, ...: all their taps are requested
    // before the first is used, so one ring latency covers the sub-block (a
    // lane past m re-reads an entry its own wave parked -- a wave's LDS
    // operations execute in order -- and stores nothing).
    const double* phk = ph + k * S;
    for (int s = lane; s < m; s += 64) {
      const double mod = 0.5 * (1.0 + sin(phk[s] + off));
      double delay = base + a.mod_depth * mod;
      if (delay < 0.0) delay = 0.0;
      if (delay > maxd) delay = maxd;
      ul[i * pitch + s] = delay;
    }
    constexpr int kRounds = (kFdnMaxSub + 63) / 64;
    double tt[kRounds], xm[kRounds], x0[kRounds], x1[kRounds], x2[kRounds];
#pragma unroll
    for (int r = 0; r < kRounds; ++r) {
      const int s = lane + 64 * r < m ? lane + 64 * r : lane < m ? lane : 0;
      const double delay = ul[i * pitch + s];
      const double fl = floor(delay);
      tt[r] = delay - fl;
      const int p = min(max((int)fl, 0), L - 3);
      const int e2 = wrap(cur + s - 3 - p, L);  // delay p + 2, the oldest tap
      const int e1 = wrap(e2 + 1, L);
      const int e0 = wrap(e1 + 1, L);
      const int em = p >= 1 ? wrap(e0 + 1, L) : e0;  // maxInt(0, p - 1)
      xm[r] = ring[em];
      x0[r] = ring[e0];
      x1[r] = ring[e1];
      x2[r] = ring[e2];
    }
#pragma unroll
    for (int r = 0; r < kRounds; ++r) {
      const int s = lane + 64 * r;
      if (s < m) dl[i * pitch + s] = hermite4(tt[r], xm[r], x0[r], x1[r], x2[r]);
    }
    __syncthreads();

    // 3. feedback row i (:220-227, up to the damping state), output (:233-240)
    for (int s = lane; s < m; s += 64) {
      double fb = 0.0;
#pragma unroll
      for (int j = 0; j < kFdnLines; ++j) {
        const double d = dl[j * pitch + s];
        fb = fb + ((__builtin_popcount(i & j) & 1) ? -d : d);  // fdnHadamard[i][j] * d
      }
      fb = fb * a.gain;
      ul[i * pitch + s] = fb * a.one_minus_damp;
    }
    for (int s = tid; s < m; s += kFdnThreads) {
      double out = 0.0;
#pragma unroll
      for (int j = 0; j < kFdnLines; ++j) out = out + dl[j * pitch + s];
      out = out * a.gain;
      const double x = xs[s];
      row[t0 + s] = x * a.dry + out * a.wet;
      // the pre-delay ring keeps the newest pre_len inputs (all its reads are done)
      if (has_pre && s >= m - Lp) pring[(curp + s) % Lp] = x;
    }
    __syncthreads();

    // 4. the serial recurrences
    if (tid < kFdnLines) {
      // eight samples' inputs are read one chunk ahead, so the chain never
      // waits for LDS: per sample one rounded multiply and one rounded add
      const double* __restrict__ u = ul + tid * pitch;
      double* __restrict__ f = dl + tid * pitch;
      const int full = m & ~7;
      double nx[8];
      if (full) {
#pragma unroll
        for (int j = 0; j < 8; ++j) nx[j] = u[j];
      }
      for (int s = 0; s < full; s += 8) {
        double v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = nx[j];
        if (s + 8 < full) {
#pragma unroll
          for (int j = 0; j < 8; ++j) nx[j] = u[s + 8 + j];
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          fs = v[j] + fs * a.damp;
          v[j] = fs;
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) f[s + j] = v[j];
      }
      for (int s = full; s < m; ++s) {
        fs = u[s] + fs * a.damp;
        f[s] = fs;
      }
    } else if (tid == 64) {
      double* pn = ph + (k ^ 1) * S;
      for (int s = 0; s < mnext; ++s) {
        pn[s] = phase;
        phase = phase + a.lfo_inc;
        if (phase >= a.two_pi) phase = phase - a.two_pi;
      }
    }
    __syncthreads();

    // 5. the lines' writes (:229-230)
    for (int s = lane; s < m; s += 64) ring[wrap(cur + s, L)] = ins[s] + dl[i * pitch + s] * fbg;
    cur = wrap(cur + m, L);
    curp = (curp + m) % Lp;
  }

  if (tid < kFdnLines) a.fstate[c * kFdnLines + tid] = fs;
  if (tid == 64 && c == 0) *a.phase_out = phase;
}

}  // namespace

void launch_fdn(const FdnArgs& a, int channels, hipStream_t s) {
  hipLaunchKernelGGL(k_fdn, dim3((unsigned)channels), dim3(kFdnThreads), (size_t)fdn_lds_bytes(a.sub), s, a);
}

}  // namespace adsp
