// Memory-pattern probe for the long-block overlap-save plan:
// replays the global-memory access shapes of its three kernels for the bench
// instance (2 channels x 9 blocks of N = N1 x N2 = 2^21 points, K = 131072),
// with no arithmetic.  A dummy LDS allocation pins the occupancy the real
// kernels would have (a tile of W columns of the two-column-packed N1-point
// complex FFT: W/2 * N1 * 16 B).
//   A: per (block, tile of W columns): N1 rows of W doubles, row stride N2
//      doubles, from x at an 8-byte-aligned block start (hop is odd); writes
//      N1/2+1 rows of W double2 at pitch N2+8 into the intermediate.
//   B: per (row k1, block): one row of N2 double2 in, the same row out in
//      place, plus the H row of the channel (block and channel fastest, so
//      co-resident items share it).
//   C: the mirror of A; only the hop's rows are stored.
// Both factorizations and several tile widths; the sum A + B + C is the figure
// to set against the three-kernel UPOLS step timed on the same box.
//   hipcc --offload-arch=gfx950 -O3 tools/long_probe.hip -o tools/long_probe
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>

#define CK(x)                                                     \
  do {                                                            \
    hipError_t e = (x);                                           \
    if (e != hipSuccess) {                                        \
      std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e)); \
      std::exit(1);                                               \
    }                                                             \
  } while (0)

typedef double d2v __attribute__((ext_vector_type(2)));

constexpr int kCh = 2, kBlocks = 9, kCB = kCh * kBlocks;
constexpr long kN = 1L << 21, kK = 131072, kHop = kN - kK + 1;

struct Args {
  const double* x;   // [kCh][xs]
  double* y;         // [kCh][ys]
  double2* t;        // [kCB][N1/2+1][pitch]
  const double2* h;  // [kCh][N1/2+1][pitch]
  long xs, ys;
  int n1, n2, pitch, tiles;
};

extern __shared__ double2 pin[];

__device__ __forceinline__ int xcd_remap(int b, int G) {
  const int xcd = b & 7, r = b >> 3;
  const int q = G >> 3, rem = G & 7;
  return (xcd < rem) ? xcd * (q + 1) + r : rem * (q + 1) + (xcd - rem) * q + r;
}

// W doubles per row in (8-byte loads: the block start is odd), W double2 per row out
template <int W, bool NT>
__global__ __launch_bounds__(256) void k_a(Args a) {
  const int item = xcd_remap(blockIdx.x, gridDim.x);
  const int cb = item / a.tiles, tile = item % a.tiles;
  const int c = cb / kBlocks, j = cb % kBlocks;
  const int tid = threadIdx.x;
  const double* x = a.x + c * a.xs + j * kHop + tile * W;
  double acc0 = 0, acc1 = 0;
  constexpr int RPI = 256 / W;  // rows per instruction
  const int col = tid % W, r0 = tid / W;
#pragma unroll 16
  for (int r = r0; r < a.n1; r += RPI) {
    const double v = x[(long)r * a.n2 + col];
    if ((r / RPI) & 1) acc1 += v; else acc0 += v;
  }
  if (acc0 == 1.2345e300) pin[tid] = make_double2(acc0, acc1);  // never: keeps the allocation
  double2* t = a.t + (long)cb * (a.n1 / 2 + 1) * a.pitch + tile * W;
#pragma unroll 8
  for (int r = r0; r <= a.n1 / 2; r += RPI) {
    double2* p = t + (long)r * a.pitch + col;
    if (NT)
      __builtin_nontemporal_store(d2v{acc0, acc1}, reinterpret_cast<d2v*>(p));
    else
      *p = make_double2(acc0, acc1);
  }
}

template <int W, bool NT>
__global__ __launch_bounds__(256) void k_c(Args a) {
  const int item = xcd_remap(blockIdx.x, gridDim.x);
  const int cb = item / a.tiles, tile = item % a.tiles;
  const int c = cb / kBlocks, j = cb % kBlocks;
  const int tid = threadIdx.x;
  constexpr int RPI = 256 / W;
  const int col = tid % W, r0 = tid / W;
  const double2* t = a.t + (long)cb * (a.n1 / 2 + 1) * a.pitch + tile * W;
  double acc0 = 0, acc1 = 0;
#pragma unroll 8
  for (int r = r0; r <= a.n1 / 2; r += RPI) {
    const double2* p = t + (long)r * a.pitch + col;
    double2 v;
    if (NT) {
      const d2v q = __builtin_nontemporal_load(reinterpret_cast<const d2v*>(p));
      v = make_double2(q.x, q.y);
    } else {
      v = *p;
    }
    acc0 += v.x;
    acc1 += v.y;
  }
  if (acc0 == 1.2345e300) pin[tid] = make_double2(acc0, acc1);
  // block j's outputs are samples [K-1, N) of the block: y[j hop ...)
  double* y = a.y + c * a.ys + j * kHop - (kK - 1) + tile * W;
  const int rfirst = (int)((kK - 1) / a.n2);
#pragma unroll 16
  for (int r = rfirst + r0; r < a.n1; r += RPI) {
    const long i = (long)r * a.n2 + col + tile * W;
    if (i >= kK - 1) y[(long)r * a.n2 + col] = acc0 + acc1;
  }
}

// one row per workgroup: 256 threads, n2 / 256 double2 each
template <int PER, bool NT>
__global__ __launch_bounds__(256) void k_b(Args a) {
  const int item = xcd_remap(blockIdx.x, gridDim.x);
  const int cb = item % kCB, row = item / kCB;  // block and channel fastest
  const int c = cb / kBlocks;
  const int tid = threadIdx.x;
  double2* t = a.t + ((long)cb * (a.n1 / 2 + 1) + row) * a.pitch;
  const double2* h = a.h + ((long)c * (a.n1 / 2 + 1) + row) * a.pitch;
  double2 v[PER], w[PER];
#pragma unroll
  for (int s = 0; s < PER; ++s) {
    const double2* p = t + tid + 256 * s;
    if (NT) {
      const d2v q = __builtin_nontemporal_load(reinterpret_cast<const d2v*>(p));
      v[s] = make_double2(q.x, q.y);
    } else {
      v[s] = *p;
    }
  }
#pragma unroll
  for (int s = 0; s < PER; ++s) w[s] = h[tid + 256 * s];
  if (v[0].x == 1.2345e300) pin[tid] = v[0];
#pragma unroll
  for (int s = 0; s < PER; ++s) {
    const d2v o{v[s].x + w[s].x, v[s].y + w[s].y};
    double2* p = t + tid + 256 * s;
    if (NT)
      __builtin_nontemporal_store(o, reinterpret_cast<d2v*>(p));
    else
      *p = make_double2(o.x, o.y);
  }
}

template <class F>
double timeit(const char* name, F launch, double bytes) {
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  for (int w = 0; w < 3; ++w) launch();
  CK(hipGetLastError());
  const int reps = 10;
  float tot = 0;
  for (int w = 0; w < reps; ++w) {
    CK(hipEventRecord(e0));
    launch();
    CK(hipEventRecord(e1));
    CK(hipEventSynchronize(e1));
    float ms = 0;
    CK(hipEventElapsedTime(&ms, e0, e1));
    tot += ms;
  }
  const double us = tot * 1e3 / reps;
  std::printf("  %-34s %8.1f us  %7.1f GB/s\n", name, us, bytes / (us * 1e-6) / 1e9);
  return us;
}

template <int W, bool NT>
void config(Args a, int n1) {
  a.n1 = n1;
  a.n2 = (int)(kN / n1);
  a.pitch = a.n2 + 8;
  a.tiles = a.n2 / W;
  const int lds = W / 2 * n1 * 16;
  if (lds > 160 * 1024) return;
  CK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_a<W, NT>), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
  CK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_c<W, NT>), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
  const int rows = n1 / 2 + 1;
  const double tb = 16.0 * rows * a.n2 * kCB;
  std::printf("N1 %d x N2 %d, W %d, LDS %d KiB, nt %d: A/C items %d, B items %d\n", n1, a.n2, W, lds / 1024, (int)NT,
              kCB * a.tiles, kCB * rows);
  double us = 0;
  us += timeit("A (x -> T columns)", [&] { hipLaunchKernelGGL((k_a<W, NT>), dim3(kCB * a.tiles), dim3(256), lds, 0, a); },
               8.0 * kN * kCB + tb);
  const double hb = 16.0 * rows * a.n2 * kCh;
  if (a.n2 == 2048)
    us += timeit("B (T rows in place, + H)", [&] { hipLaunchKernelGGL((k_b<8, NT>), dim3(kCB * rows), dim3(256), 40960, 0, a); },
                 2 * tb + hb);
  else if (a.n2 == 4096)
    us += timeit("B (T rows in place, + H)", [&] { hipLaunchKernelGGL((k_b<16, NT>), dim3(kCB * rows), dim3(256), 65536, 0, a); },
                 2 * tb + hb);
  else
    us += timeit("B (T rows in place, + H)", [&] { hipLaunchKernelGGL((k_b<4, NT>), dim3(kCB * rows), dim3(256), 20480, 0, a); },
                 2 * tb + hb);
  us += timeit("C (T columns -> y)", [&] { hipLaunchKernelGGL((k_c<W, NT>), dim3(kCB * a.tiles), dim3(256), lds, 0, a); },
               tb + 8.0 * kHop * kCB);
  std::printf("  A + B + C %8.1f us\n", us);
}

int main() {
  Args a{};
  a.xs = (1L << 24);
  a.ys = a.xs + kK - 1;
  // the last block reads past n in the real kernel only as implied zeros; the
  // probe's buffers cover 9 whole blocks instead
  const long xlen = kBlocks * kHop + kN, ylen = kBlocks * kHop + kN;
  if (xlen > a.xs) a.xs = xlen;
  if (ylen > a.ys) a.ys = ylen;
  const long trows = 1025, tp = 2048 + 8;  // covers both factorizations
  double *x, *y;
  double2 *t, *h;
  CK(hipMalloc(&x, kCh * a.xs * 8));
  CK(hipMalloc(&y, kCh * a.ys * 8));
  CK(hipMalloc(&t, kCB * trows * tp * 16));
  CK(hipMalloc(&h, kCh * trows * tp * 16));
  CK(hipMemset(x, 0, kCh * a.xs * 8));
  CK(hipMemset(y, 0, kCh * a.ys * 8));
  CK(hipMemset(t, 0, kCB * trows * tp * 16));
  CK(hipMemset(h, 0, kCh * trows * tp * 16));
  // the real plan reads block j from x + j hop - (K-1); the probe's allocation
  // starts K-1 samples early, so block j reads [j hop, j hop + N) of it
  a.x = x;
  a.y = y;
  a.t = t;
  a.h = h;
  config<8, false>(a, 1024);
  config<8, true>(a, 1024);
  config<16, true>(a, 1024);
  config<4, true>(a, 1024);
  config<4, true>(a, 2048);
  config<8, true>(a, 2048);
  config<16, true>(a, 512);
  return 0;
}
