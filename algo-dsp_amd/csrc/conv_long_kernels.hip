// Kernels of the long-block overlap-save plan; the index map is in
// conv_long_kernels.hpp.  A and C transform a tile of kLongW adjacent columns:
// two real columns ride in one complex N1-point FFT (z = a + i b), so a tile
// is kLongW / 2 transforms of FftPlan<N1>, and the tile is moved between its
// global layout (rows of kLongW values) and the per-transform LDS images, so
// global rows are read and written in runs of kLongW elements while each
// 32-lane group owns whole columns.  B keeps one row in the registers of one
// workgroup from its load to its store.
#include "conv_long_kernels.hpp"

#include "conv_kernels.hpp"
#include "fft_device.hpp"

namespace adsp {

constexpr int N1 = kLongN1, N2 = kLongN2, W = kLongW;
constexpr int kColThreads = 256;
constexpr int kRowsPerInstr = kColThreads / W;  // tile rows one load / store instruction covers
constexpr int FS = N1 + 1;                      // LDS elements per column transform (odd: spreads the images over the banks)
using ColPlan = FftPlan<N1, 16>;
constexpr int RV = 8;  // values per thread of the row transform
using RowPlan = FftPlan<N2, RV>;
static_assert(ColPlan::T * (W / 2) == kColThreads, "a tile's transforms fill the workgroup");
static_assert(N1 % kRowsPerInstr == 0, "whole load rounds");
// A column transform is ColPlan::T lanes of one wave and its image is its own,
// so the exchanges inside it order nothing across waves.  C syncs them at wave
// scope (fft_run_wave) and keeps the two workgroup barriers that order
// cross-wave traffic: after Z has gone into the images, and before the stores
// read across them.  The same change was measured on A and gains nothing
// there, so A keeps fft_run.
static_assert(ColPlan::T <= 64 && 64 % ColPlan::T == 0, "a column transform sits inside one wave");

// Tile I/O of A and C.  Thread (r0, col) = (tid / W, tid % W) holds rows r0 +
// kRowsPerInstr i of column col, so access instruction i covers tile rows
// kRowsPerInstr i .. + kRowsPerInstr - 1: its place against the signal or the
// output is the same for all lanes and is classified from scalars
// (long_tile_bounds): an instruction inside the range is a plain access, one
// outside is not issued, only a straddling one tests per lane.  Rows are
// stepped through a scalar base with one 32-bit offset per thread.  On the LDS
// side row r0 + kRowsPerInstr i has slot lds_slot(r0) ^ lds_slot(kRowsPerInstr i)
// (disjoint bits): one swizzle per thread.
static_assert(kRowsPerInstr == 16 && kRowsPerInstr == kLongTileRows, "lds_slot_split16: r0 is the low nibble of the row");
static_assert(N1 / 2 % kRowsPerInstr == 0, "row N1/2 is instruction N1/2 / kRowsPerInstr of r0 = 0");
constexpr int kHalfInstr = N1 / 2 / kRowsPerInstr;  // instructions over rows 0 .. N1/2 - 1; row N1/2 is r0 = 0 of one more

// Slot of the mirror row (N1 - k1) mod N1 of k1 = r0 + kRowsPerInstr i, i <
// kHalfInstr.  Its low nibble (16 - r0) mod 16 is the thread's own (sm its
// swizzle) and above it stands 16 h, h = 31 - i; r0 = 0 borrows nothing and
// has 16 (h + 1) with nibble 0 (row 0 mirrors itself).  The swizzle of 16 h
// depends on h mod 8 only, so a thread has eight such bases, each a select
// between two forms, and every access adds its 16 h as a constant.
__device__ __forceinline__ int mirror_slot(int sm, int r0, int i) {
  constexpr int kTop = N1 / kRowsPerInstr - 1;
  const int h = kTop - i, k = h & 7;
  const int base = r0 ? (sm ^ (lds_slot(kRowsPerInstr * k) & 15))
                      : kRowsPerInstr + (lds_slot(kRowsPerInstr * ((k + 1) & 7)) & 15);
  if (i == 0) return r0 ? kRowsPerInstr * h + base : 0;
  return kRowsPerInstr * h + base;
}

__global__ __launch_bounds__(kColThreads) void k_long_cols_fwd(LongColArgs a) {
  __shared__ double2 lds[(W / 2) * FS];
  __shared__ double2 ltab[TwSplit<N1>::N];
  const int tid = threadIdx.x;
  const int item = xcd_remap(blockIdx.x, gridDim.x);
  constexpr int kTiles = N2 / W;
  const int tile = item % kTiles, cb = item / kTiles;
  const int c = cb / a.blocks, j = cb % a.blocks;
  const int col = tid % W, r0 = tid / W;
  const int64_t origin = a.start + (int64_t)j * a.hop;  // signal index of the block's point 0
  const LongBlockRange rng = long_block_range(origin, 0, a.n);
  const LongTileBounds tb = long_tile_bounds(tile, rng);
  const double* x = a.x + (int64_t)c * a.x_stride + origin;  // the block's point 0
  const unsigned xoff = r0 * N2 + col;
  double in[N1 / kRowsPerInstr];
#pragma unroll
  for (int i = 0; i < N1 / kRowsPerInstr; ++i) {
    const int first = long_tile_first(tile, i);
    if (long_tile_inside(i, tb)) {
      in[i] = (x + first)[xoff];
    } else if (long_tile_touched(i, tb)) {
      // no branch per lane: a lane outside reads the range's first point and drops it
      const int e = first + (int)xoff;
      const bool ok = long_point_valid(e, rng);
      const double xe = x[ok ? e : rng.lo];
      in[i] = ok ? xe : 0.0;
    } else {
      in[i] = 0.0;
    }
  }
  const TwLds<N1> tw = tw_lds_compute<N1>(ltab, tid, kColThreads);
  double* img = reinterpret_cast<double*>(lds + (col >> 1) * FS) + (col & 1);
  const int sk = lds_slot(r0);
#pragma unroll
  for (int i = 0; i < N1 / kRowsPerInstr; ++i) img[2 * lds_slot_split16(sk, kRowsPerInstr * i)] = in[i];
  __syncthreads();
  const int f = tid / ColPlan::T, t = tid % ColPlan::T;
  double2* my = lds + f * FS;
  double2 v[16];
#pragma unroll
  for (int s = 0; s < 16; ++s) v[s] = my[pass0_slot<N1, 16>(t, s)];
  __syncthreads();
  fft_run<N1, 16, true>(v, t, my, tw);
  __syncthreads();
#pragma unroll
  for (int s = 0; s < 16; ++s) my[last_pass_slot<N1, 16>(t, s)] = v[s];
  __syncthreads();
  // separation of the two real columns: even col a = (Z[k] + conj Z[-k]) / 2,
  // odd col b = (Z[k] - conj Z[-k]) / 2i.  The image reads of a batch of rows
  // are issued together, ahead of the batch's stores.
  const double2* zc = lds + (col >> 1) * FS;
  const int sm = lds_slot((kRowsPerInstr - r0) & (kRowsPerInstr - 1));
  double2* T = a.T + (int64_t)cb * kLongRows * kLongPitch + tile * W;
  const unsigned toff = r0 * kLongPitch + col;
  const auto separate = [col](double2 zk, double2 zm) {
    return (col & 1) ? make_double2(0.5 * (zk.y + zm.y), 0.5 * (zm.x - zk.x))
                     : make_double2(0.5 * (zk.x + zm.x), 0.5 * (zk.y - zm.y));
  };
  constexpr int kBatch = 8;
  static_assert(kHalfInstr % kBatch == 0, "whole batches");
#pragma unroll
  for (int b = 0; b < kHalfInstr; b += kBatch) {
    double2 zk[kBatch], zm[kBatch];
#pragma unroll
    for (int u = 0; u < kBatch; ++u) {
      zk[u] = zc[lds_slot_split16(sk, kRowsPerInstr * (b + u))];
      zm[u] = zc[mirror_slot(sm, r0, b + u)];
    }
#pragma unroll
    for (int u = 0; u < kBatch; ++u)
      st2<true>(T + (int64_t)(b + u) * kRowsPerInstr * kLongPitch + toff, separate(zk[u], zm[u]));
  }
  if (r0 == 0) {  // row N1/2, its own mirror
    const double2 zh = zc[lds_slot(N1 / 2)];
    st2<true>(T + (int64_t)(N1 / 2) * kLongPitch + toff, separate(zh, zh));
  }
}

__global__ __launch_bounds__(kColThreads) void k_long_cols_inv(LongColArgs a) {
  __shared__ double2 lds[(W / 2) * FS];
  __shared__ double2 ltab[TwSplit<N1>::N];
  const int tid = threadIdx.x;
  const int item = xcd_remap(blockIdx.x, gridDim.x);
  constexpr int kTiles = N2 / W;
  const int tile = item % kTiles, cb = item / kTiles;
  const int c = cb / a.blocks, j = cb % a.blocks;
  const int col = tid % W, r0 = tid / W;
  const double2* T = a.T + (int64_t)cb * kLongRows * kLongPitch + tile * W;
  const unsigned toff = r0 * kLongPitch + col;
  double2 in[kHalfInstr + 1];
#pragma unroll
  for (int i = 0; i < kHalfInstr; ++i) in[i] = ld2<true>(T + (int64_t)i * kRowsPerInstr * kLongPitch + toff);
  in[kHalfInstr] = r0 == 0 ? ld2<true>(T + (int64_t)(N1 / 2) * kLongPitch + toff) : make_double2(0, 0);  // row N1/2
  const TwLds<N1> tw = tw_lds_compute<N1>(ltab, tid, kColThreads);
  // Z = Va + i Vb over all N1 rows, rows above N1/2 from the mirror
  // (V[N1 - k] = conj V[k]: the columns are real).  The even lane of a column
  // pair writes row k, the odd lane row N1 - k; rows 0 and N1/2 (r0 = 0 of the
  // first and the last instruction) are real and have no mirror to write.
  double2* zc = lds + (col >> 1) * FS;
  const int sk = lds_slot(r0);
  const int sm = lds_slot((kRowsPerInstr - r0) & (kRowsPerInstr - 1));
  const bool even = !(col & 1);
#pragma unroll
  for (int i = 0; i <= kHalfInstr; ++i) {
    const double px = lane_xor1(in[i].x);
    const double py = lane_xor1(in[i].y);
    if (i == kHalfInstr) {
      if (even && r0 == 0) zc[lds_slot(N1 / 2)] = make_double2(in[i].x, px);
    } else if (even) {  // Va = in, Vb = partner
      const bool edge = i == 0 && r0 == 0;
      zc[lds_slot_split16(sk, kRowsPerInstr * i)] =
          edge ? make_double2(in[i].x, px) : make_double2(in[i].x - py, in[i].y + px);
    } else if (i != 0 || r0 != 0) {  // Va = partner, Vb = in
      zc[mirror_slot(sm, r0, i)] = make_double2(px + in[i].y, in[i].x - py);
    }
  }
  __syncthreads();
  const int f = tid / ColPlan::T, t = tid % ColPlan::T;
  double2* my = lds + f * FS;
  double2 v[16];
#pragma unroll
  for (int s = 0; s < 16; ++s) v[s] = my[pass0_slot<N1, 16>(t, s)];
  wave_lds_sync();
  fft_run_wave<N1, 16, false>(v, t, my, tw);
  wave_lds_sync();
#pragma unroll
  for (int s = 0; s < 16; ++s) my[last_pass_slot<N1, 16>(t, s)] = v[s];
  __syncthreads();  // the stores below read across the images
  // 8-byte stores, runs of W per row.  The per-row 16-byte pair scheme K3 uses
  // for rows off alignment was measured here and is slower (DESIGN.md §2:
  // C 154 us against 124 us, the step 0.418 against 0.385 ms).  The image
  // reads of the instructions inside the block's outputs are issued together,
  // ahead of their stores.
  const double* img = reinterpret_cast<const double*>(zc) + (col & 1);
  double* y = a.y + (int64_t)c * a.y_stride;
  const int64_t lo = (int64_t)j * a.hop;
  const int64_t hi = a.out_len < lo + a.hop ? a.out_len : lo + a.hop;
  const int64_t origin = lo - a.skip;  // output index of the block's point 0
  const LongBlockRange rng = long_block_range(origin, lo, hi);
  const LongTileBounds tb = long_tile_bounds(tile, rng);
  y += origin;
  const unsigned yoff = r0 * N2 + col;
  double out[N1 / kRowsPerInstr];
#pragma unroll
  for (int i = 0; i < N1 / kRowsPerInstr; ++i)
    if (long_tile_inside(i, tb)) out[i] = img[2 * lds_slot_split16(sk, kRowsPerInstr * i)];
#pragma unroll
  for (int i = 0; i < N1 / kRowsPerInstr; ++i)
    if (long_tile_inside(i, tb)) (y + long_tile_first(tile, i))[yoff] = out[i];
  // The one or two instructions an end of the range cuts through, per lane.  A
  // loop that is not unrolled (unrolled into the loop above, the compiler folds
  // the two cases into one masked store per instruction).
#pragma unroll 1
  for (int i = long_tile_next_straddling(tb.any_first - 1, tb); i < tb.any_first + tb.any_count;
       i = long_tile_next_straddling(i, tb)) {
    const int first = long_tile_first(tile, i);
    if (long_point_valid(first + (int)yoff, rng)) (y + first)[yoff] = img[2 * lds_slot(r0 + kRowsPerInstr * i)];
  }
}

// One row per workgroup of N2 / RV threads, RV values per thread: the four
// radix-8 Stockham passes of RowPlan, with the butterflies dealt to threads so
// that one exchange per transform crosses waves.  Input digits n2 = 512 a3 +
// 64 a2 + 8 a1 + a0, output digits k2 = k0 + 8 k1 + 64 k2' + 512 k3; a thread
// is (wave; lane), its RV values the slot:
//
//   pass  forward thread        slot   inverse thread        slot
//   0     (a2; 8 a1 + a0)       a3     (k0; 8 k1 + k2')      k3
//   1     (k0; 8 a1 + a0)       a2     (k0; 8 k1 + m0)       k2'
//   2     (k0; 8 k1 + a0)       a1     (k0; 8 m1 + m0)       k1
//   3     (k0; 8 k1 + k2')      a0     (m2; 8 m1 + m0)       k0
//
// (m: the inverse's output digits, n2 = m0 + 8 m1 + 64 m2 + 512 m3.)  From the
// forward pass 1 to the inverse pass 2 wave k0 works inside its own slice
// lds[512 k0 ..]: those four exchanges sync at wave scope.  The forward pass 0
// writes into the other waves' slices (nothing has read the image yet) and the
// inverse pass 2 writes its own slice for pass 3 to read across: one workgroup
// barrier each.  The forward result sits where the inverse's pass 0 wants it,
// and the inverse's last pass is back at tid + T s, the order of the row's
// loads and stores.  The butterflies, twiddle exponents and powering order are
// RowPlan's (jb below is the plan's butterfly index); H rows are stored and
// read positionally by this kernel alone, in the forward result's order.
//
// Slice addresses (tools/lds_conflicts.py: no conflicts): a read of slot r by
// lane l is 64 r + l, or 64 r + (l ^ r) where the writers' eight-lane groups
// run over the slot digit (forward pass 2 -> 3, inverse pass 0 -> 1).
// BUILD: forward half only, the scaled spectrum stored to Hout (the IR's H rows).
constexpr int kRowThreads = RowPlan::T;
static_assert(RowPlan::NPASS == 4 && RowPlan::R0 == RV && RV == 8 && kRowThreads == 8 * 64,
              "k_long_rows: four radix-8 passes over eight waves of 64 lanes, wave = k0");

// lane l's x in every lane (l known at compile time), through scalar registers
__device__ __forceinline__ double wave_bcast(double x, int l) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(x), l);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(x), l);
  return __hiloint2double(hi, lo);
}

// two workgroups per CU: 2 N2 / RV / 64 waves over the CU's 4 SIMDs
constexpr int kRowWavesPerSimd = 2 * kRowThreads / 256;
template <bool BUILD>
__global__ __launch_bounds__(kRowThreads, kRowWavesPerSimd) void k_long_rows(LongRowArgs a) {
  __shared__ double2 lds[N2];
  __shared__ double2 ltab[TwSplit<N2>::N];
  __shared__ double2 wtab[kRowThreads];  // each thread's own W_N^(k1 tid), parked between its two uses
  constexpr int T = kRowThreads;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l0 = lane & 7, l1 = lane & 56;
  const int item = xcd_remap(blockIdx.x, gridDim.x);
  const int ncb = a.blocks * a.channels;
  const int cb = item % ncb, k1 = item / ncb;  // block and channel fastest: co-resident items share H rows
  double2* row = a.T + ((int64_t)cb * kLongRows + k1) * kLongPitch;
  double2 v[RV];
#pragma unroll
  for (int s = 0; s < RV; ++s) v[s] = ld2<true>(row + tid + T * s);
  const TwLds<N2> tw = tw_lds_compute<N2>(ltab, tid, T);
  // W_N^(k1 n2), n2 = tid + T s: W_N^(k1 tid) * W_N^(T k1 s).  The second
  // factor is the row's own; every wave computes it in its lanes 0 .. RV-1 and
  // hands it round in scalar registers, so no barrier stands before pass 0.
  double2 rt[RV];
  {
    double2 r;
    sincospi(-2.0 * (double)(T * k1 * l0) / (double)kLongN, &r.y, &r.x);
#pragma unroll
    for (int s = 0; s < RV; ++s) rt[s] = make_double2(wave_bcast(r.x, s), wave_bcast(r.y, s));
  }
  {
    double2 w0;
    sincospi(-2.0 * (double)(k1 * tid) / (double)kLongN, &w0.y, &w0.x);
    wtab[tid] = w0;
#pragma unroll
    for (int s = 0; s < RV; ++s) v[s] = c_mul(v[s], c_mul(w0, rt[s]));
  }
  // forward pass 0, value k0 into wave k0's slice; the H row's loads are
  // issued behind it (v is free there) and land while the later passes run
  Dft<RV, true>::run(v);
#pragma unroll
  for (int r = 0; r < RV; ++r) lds[T * r + tid] = v[r];
  double2 h[BUILD ? 1 : RV];
  if constexpr (!BUILD) {
    const double2* hrow = a.H + ((int64_t)a.ir_index[cb / a.blocks] * kLongRows + k1) * kLongPitch;
#pragma unroll
    for (int s = 0; s < RV; ++s) h[s] = hrow[tid + T * s];
  }
  __syncthreads();  // the slices are whole; ltab is filled
  double2* sl = lds + 64 * RV * wv;
  double2 w = twiddle_root<N2, RV, 8, true>(wv, tw);  // jb = 64 a1 + 8 a0 + k0
#pragma unroll
  for (int r = 0; r < RV; ++r) v[r] = sl[64 * r + lane];
  twiddle_powers<RV>(v, w);
  Dft<RV, true>::run(v);
  wave_lds_sync();
#pragma unroll
  for (int r = 0; r < RV; ++r) sl[8 * l1 + 8 * r + l0] = v[r];  // 64 a1 + 8 k1 + a0
  w = twiddle_root<N2, RV, 64, true>(l1 + wv, tw);  // jb = 64 a0 + 8 k1 + k0
  wave_lds_sync();
#pragma unroll
  for (int r = 0; r < RV; ++r) v[r] = sl[64 * r + lane];
  twiddle_powers<RV>(v, w);
  Dft<RV, true>::run(v);
  wave_lds_sync();
#pragma unroll
  for (int r = 0; r < RV; ++r) sl[64 * l0 + ((l1 + r) ^ l0)] = v[r];  // 64 a0 + ((8 k1 + k2') ^ a0)
  w = twiddle_root<N2, RV, 512, true>(64 * l0 + l1 + wv, tw);  // jb = 64 k2' + 8 k1 + k0
  wave_lds_sync();
#pragma unroll
  for (int r = 0; r < RV; ++r) v[r] = sl[64 * r + (lane ^ r)];
  twiddle_powers<RV>(v, w);
  Dft<RV, true>::run(v);  // v[s] = X[k1 + N1 (wv + 8 (lane / 8) + 64 (lane % 8) + T s)]
  if constexpr (BUILD) {
    double2* out = a.Hout + ((int64_t)cb * kLongRows + k1) * kLongPitch;
#pragma unroll
    for (int s = 0; s < RV; ++s) out[tid + T * s] = c_scale(v[s], a.scale);
  } else {
#pragma unroll
    for (int s = 0; s < RV; ++s) v[s] = c_mul(v[s], h[s]);
    Dft<RV, false>::run(v);  // inverse pass 0
    wave_lds_sync();
#pragma unroll
    for (int r = 0; r < RV; ++r) sl[64 * l0 + ((l1 + r) ^ l0)] = v[r];  // 64 k2' + ((8 k1 + m0) ^ k2')
    w = twiddle_root<N2, RV, 8, false>(l0, tw);  // jb = 64 k1 + 8 k0 + m0
    wave_lds_sync();
#pragma unroll
    for (int r = 0; r < RV; ++r) v[r] = sl[64 * r + (lane ^ r)];
    twiddle_powers<RV>(v, w);
    Dft<RV, false>::run(v);
    wave_lds_sync();
#pragma unroll
    for (int r = 0; r < RV; ++r) sl[8 * l1 + 8 * r + l0] = v[r];  // 64 k1 + 8 m1 + m0
    w = twiddle_root<N2, RV, 64, false>(lane, tw);  // jb = 64 k0 + 8 m1 + m0
    wave_lds_sync();
#pragma unroll
    for (int r = 0; r < RV; ++r) v[r] = sl[64 * r + lane];
    twiddle_powers<RV>(v, w);
    Dft<RV, false>::run(v);
    wave_lds_sync();
#pragma unroll
    for (int r = 0; r < RV; ++r) sl[64 * r + lane] = v[r];  // own slice: 512 k0 + 64 m2 + 8 m1 + m0
    w = twiddle_root<N2, RV, 512, false>(tid, tw);  // jb = 64 m2 + 8 m1 + m0
    const double2 w0 = wtab[tid];
    __syncthreads();  // pass 3 reads across the slices
#pragma unroll
    for (int r = 0; r < RV; ++r) v[r] = lds[T * r + tid];
    twiddle_powers<RV>(v, w);
    Dft<RV, false>::run(v);  // v[s] = y[tid + T s]
#pragma unroll
    for (int s = 0; s < RV; ++s) st2<true>(row + tid + T * s, c_mul(v[s], c_conj(c_mul(w0, rt[s]))));
  }
}

void launch_long_cols_fwd(const LongColArgs& a, hipStream_t s) {
  const unsigned items = (unsigned)a.channels * a.blocks * (N2 / W);
  timed_launch(k_long_cols_fwd, dim3(items), dim3(kColThreads), s, a);
}

void launch_long_rows(const LongRowArgs& a, bool build_h, hipStream_t s) {
  const unsigned items = (unsigned)a.channels * a.blocks * kLongRows;
  if (build_h)
    timed_launch(k_long_rows<true>, dim3(items), dim3(kRowThreads), s, a);
  else
    timed_launch(k_long_rows<false>, dim3(items), dim3(kRowThreads), s, a);
}

void launch_long_cols_inv(const LongColArgs& a, hipStream_t s) {
  const unsigned items = (unsigned)a.channels * a.blocks * (N2 / W);
  timed_launch(k_long_cols_inv, dim3(items), dim3(kColThreads), s, a);
}

}  // namespace adsp
