// effects.Vocoder.ProcessSample (dsp/effects/vocoder.go:578-630) for many
// channels that share one configuration, in the reference's operation order
// (every product and sum rounded on its own, no FMA).
//
// One channel is up to 32 band recurrences whose products are summed per
// sample, so the parallel axis is the band, not the channel.  A workgroup is
// one wave and carries one channel:
//   walk   lanes 0..31 take the modulator side of band b, lanes 32..63 the
//          carrier side.  Both halves run one instruction stream: a
//          biquad.Section.ProcessSample per sample with coefficients, state
//          and input chosen by role (analysis on the modulator, synthesis on
//          the carrier), then the envelope step, whose result only the
//          modulator half keeps.  With downsampling the modulator half's
//          first section is its group's anti-alias section (every band of a
//          group walks the same section from the same state, so the copies
//          agree bit for bit and the group's first band saves it), and a
//          second section, the decimated analysis, with the envelope is
//          kept only on the group's ticks, (cnt & mask) == 0.  The chunk's
//          samples come from LDS as same-address reads of a half wave; env[b][t]
//          and syn[b][t] go to LDS tiles at an odd row pitch.
//   sum    lane t takes sample t: vocoded = 0.0, then + env[b][t] * syn[b][t]
//          for b = 0 .. numBands-1 in that order, then the mix :629, stored
//          with consecutive lanes on consecutive samples.
// The next chunk's samples are loaded into registers before the walk of this
// one, so they fly during it.  The tiles are not doubled: a workgroup is one
// wave, whose LDS operations complete in order, so a second set of product
// tiles would overlap nothing and would halve the workgroups a CU holds.
// `out` may be the modulator's or the carrier's rows: a chunk's samples are
// in registers before any of them is stored, and no other workgroup touches
// the channel's rows.
//
// Every global index is guarded by n and the channel count; lanes of bands
// past numBands walk zero coefficients and save nothing.
#include "vocoder_kernels.hpp"

namespace adsp {
namespace {

// A workgroup barrier that orders the LDS accesses only: global loads and stores in flight stay in flight.
__device__ __forceinline__ void lds_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

template <bool DS>
struct VocLane {
  double c0, c1, c2, c3, c4, p0, p1;  // the section every sample runs, and its state
  double d0, d1, d2, d3, d4, q0, q1;  // DS, modulator half: the decimated analysis section
  double env, attack, release;
  int role, mask;

  // section.go:47-53, then the envelope :591-600 / :615-624; returns what the lane leaves in its product row
  __device__ __forceinline__ double step(double x, int cnt) {
#pragma clang fp contract(off)
    const double y = c0 * x + p0;
    p0 = c1 * x - c3 * y + p1;
    p1 = c2 * x - c4 * y;
    if (DS) {
      const double y2 = d0 * y + q0;
      const double n0 = d1 * y - d3 * y2 + q1;
      const double n1 = d2 * y - d4 * y2;
      const double level = fabs(y2);
      const double ea = env + (level - env) * attack, er = level + (env - level) * release;
      const double ne = level > env ? ea : er;
      const bool keep = role == 0 && (cnt & mask) == 0;  // :585
      q0 = keep ? n0 : q0;
      q1 = keep ? n1 : q1;
      env = keep ? ne : env;
    } else {
      const double level = fabs(y);
      const double ea = env + (level - env) * attack, er = level + (env - level) * release;
      env = level > env ? ea : er;  // the carrier half's value is never read
    }
    return role ? y : env;
  }
};

template <bool DS>
__global__ __launch_bounds__(64) void k_vocoder(VocArgs a) {
#pragma clang fp contract(off)
  constexpr int T = kVocTile, P = kVocPitch, B = kVocBands;
  __shared__ __attribute__((aligned(16))) double xin[2 * T];   // [role][t]
  __shared__ __attribute__((aligned(16))) double prod[2 * B * P];  // [role][band][P]: env rows, then syn rows
  const int64_t ch = blockIdx.x;
  if (ch >= a.channels) return;  // the whole workgroup
  const int lane = threadIdx.x, role = lane >> 5, b = lane & (B - 1);
  const bool live = b < a.num_bands;
  double* st = a.state + ch * (VOC_STATE_ROWS * B);

  VocLane<DS> w;
  w.role = role;
  const int grp = DS ? a.itab[VOC_GROUP * B + b] : 0;
  const bool first = DS && a.itab[VOC_FIRST * B + b] != 0;
  w.mask = DS ? a.itab[VOC_MASK * B + b] : 0;
  const int row1 = role ? VOC_SYNTHESIS : (DS ? VOC_ANTIALIAS : VOC_ANALYSIS);
  const int srow1 = role ? VOC_S_SYNTHESIS : (DS ? VOC_S_ANTIALIAS : VOC_S_ANALYSIS);
  const int scol1 = (DS && !role) ? grp : b;
  w.c0 = live ? a.tab[(row1 + 0) * B + b] : 0.0;
  w.c1 = live ? a.tab[(row1 + 1) * B + b] : 0.0;
  w.c2 = live ? a.tab[(row1 + 2) * B + b] : 0.0;
  w.c3 = live ? a.tab[(row1 + 3) * B + b] : 0.0;
  w.c4 = live ? a.tab[(row1 + 4) * B + b] : 0.0;
  w.p0 = live ? st[srow1 * B + scol1] : 0.0;
  w.p1 = live ? st[(srow1 + 1) * B + scol1] : 0.0;
  const bool dec = DS && live && role == 0;
  w.d0 = dec ? a.tab[(VOC_DECIMATED + 0) * B + b] : 0.0;
  w.d1 = dec ? a.tab[(VOC_DECIMATED + 1) * B + b] : 0.0;
  w.d2 = dec ? a.tab[(VOC_DECIMATED + 2) * B + b] : 0.0;
  w.d3 = dec ? a.tab[(VOC_DECIMATED + 3) * B + b] : 0.0;
  w.d4 = dec ? a.tab[(VOC_DECIMATED + 4) * B + b] : 0.0;
  w.q0 = dec ? st[VOC_S_DECIMATED * B + b] : 0.0;
  w.q1 = dec ? st[(VOC_S_DECIMATED + 1) * B + b] : 0.0;
  w.env = (live && role == 0) ? st[VOC_S_ENV * B + b] : 0.0;
  w.attack = dec ? a.tab[VOC_DS_ATTACK * B + b] : a.attack;
  w.release = dec ? a.tab[VOC_DS_RELEASE * B + b] : a.release;

  const double* mod = a.mod + ch * a.mod_stride;
  const double* car = a.car + ch * a.car_stride;
  double* out = a.out + ch * a.out_stride;
  const double* x = xin + role * T;
  double* mine = prod + lane * P;  // lane = role * B + b

  // lane t holds sample t of the next chunk of both rows
  double vm = lane < a.n ? mod[lane] : 0.0;
  double vc = lane < a.n ? car[lane] : 0.0;
  for (int64_t t0 = 0; t0 < a.n; t0 += T) {
    const int m = (int)(a.n - t0 < T ? a.n - t0 : T);
    const double xm = vm, xc = vc;
    xin[lane] = xm;
    xin[T + lane] = xc;
    const int64_t t1 = t0 + T + lane;
    vm = t1 < a.n ? mod[t1] : 0.0;
    vc = t1 < a.n ? car[t1] : 0.0;
    lds_barrier();  // the chunk is whole; the sums of the chunk before have left the product tiles
    const int cnt = (int)((a.cnt0 + t0) & a.cnt_mask);  // masks are 2^k - 1 <= cnt_mask: wrapping cnt is not needed
    if (m == T) {
#pragma unroll
      for (int t = 0; t < T; ++t) mine[t] = w.step(x[t], cnt + t);
    } else {
      for (int t = 0; t < m; ++t) mine[t] = w.step(x[t], cnt + t);
    }
    lds_barrier();  // the product tiles are whole
    if (lane < m) {
      double vocoded = 0.0;  // :579
      for (int k = 0; k < a.num_bands; ++k) vocoded = vocoded + prod[k * P + lane] * prod[(B + k) * P + lane];
      out[t0 + lane] = (a.vocoder_level * vocoded + a.synth_level * xc) + a.input_level * xm;  // :629
    }
    lds_barrier();  // the sums are read: the next chunk may take the tiles
  }

  if (!live) return;
  if (!(DS && role == 0) || first) {  // a group's anti-alias state: its first band alone
    st[srow1 * B + scol1] = w.p0;
    st[(srow1 + 1) * B + scol1] = w.p1;
  }
  if (dec) {
    st[VOC_S_DECIMATED * B + b] = w.q0;
    st[(VOC_S_DECIMATED + 1) * B + b] = w.q1;
  }
  if (role == 0) st[VOC_S_ENV * B + b] = w.env;
}

}  // namespace

void launch_vocoder(const VocArgs& a, bool downsample, hipStream_t s) {
  if (a.n <= 0 || a.channels <= 0) return;
  const dim3 grid((unsigned)a.channels), block(64);
  if (downsample)
    k_vocoder<true><<<grid, block, 0, s>>>(a);
  else
    k_vocoder<false><<<grid, block, 0, s>>>(a);
}

}  // namespace adsp
