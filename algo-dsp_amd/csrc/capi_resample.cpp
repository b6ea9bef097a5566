// C ABI of the rational polyphase resampler (dsp/resample/resample.go).
// The prototype comes from the host designer; the handle keeps the reference's
// scalar state on the host and the T-1 delay line of every channel on the device.
#include <hip/hip_runtime.h>

#include <cmath>
#include <memory>
#include <vector>

#include "ad_common.hpp"
#include "stream_order.hpp"
#include "resample_kernels.hpp"

using namespace adsp;

namespace {

// Bounds that keep every product of the index arithmetic inside int64: with
// up, down <= 2^30 and n_in < 2^31, L*up and n_out*down stay below 2^62.
constexpr int64_t kMaxRatio = (int64_t)1 << 30;
constexpr int64_t kMaxIn = ((int64_t)1 << 31) - 1;

int64_t gcd64(int64_t a, int64_t b) {  // resample_design.go:116-134
  while (b != 0) {
    const int64_t r = a % b;
    a = b;
    b = r;
  }
  return a == 0 ? 1 : a;
}

}  // namespace

struct ad_resampler {
  int device = 0, channels = 0;
  int64_t up = 0, down = 0, T = 0;
  // resample.go:146-148 keeps phase, inputIndex and totalIn.  Only
  // inputIndex - totalIn (`ahead`, never negative between calls) matters, and
  // unlike the two counters it does not grow with the stream.
  int64_t phase = 0, ahead = 0;
  ResamplePlan plan;
  hipStream_t stream = nullptr;  // host-buffer calls
  StreamOrder order;             // calls may come on any stream
  DevBuf<double> tab;            // [up][pitch], phase-major
  DevBuf<double> hist[2];        // [C][T-1] delay line, ping-pong (cur = hist[cur])
  int cur = 0;
  DevBuf<double> io_in, io_out;  // host-buffer calls
  ~ad_resampler() {
    order.release();
    if (stream) {
      (void)hipStreamSynchronize(stream);
      (void)lib_stream_destroy(stream);
    }
  }
};

namespace {

// PredictOutputLen (resample.go:295-313) in closed form: outputs are emitted
// while ahead + (phase + j*down) / up <= n_in - 1, i.e. j*down < L*up - phase.
int64_t predict(const ad_resampler* r, int64_t n_in) {
  if (n_in <= 0) return 0;
  const int64_t L = n_in - r->ahead;
  if (L <= 0) return 0;
  return (L * r->up - r->phase + r->down - 1) / r->down;
}

void check_n_in(int64_t n_in) {
  if (n_in < 0 || n_in > kMaxIn) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "n_in must be in [0, 2^31)");
}

// one launch covers a call: its tiles must fit the grid's x dimension
void check_n_out(int64_t n_out) {
  if (n_out > ((int64_t)1 << 38)) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "more than 2^38 outputs in one call");
}

// n_out outputs from n_in new samples per channel, device in/out; then the
// state and the delay line advance.  Ordering as fir_run: the next delay line
// is built in the other history buffer, so nothing the kernel reads is written.
void resample_run(ad_resampler* r, const double* d_in, int64_t in_stride, int64_t n_in, double* d_out,
                  int64_t out_stride, int64_t n_out, hipStream_t s) {
  r->order.enter(s);
  const int64_t hn = r->T - 1;
  const size_t C = (size_t)r->channels;
  const double* hold = r->hist[r->cur].p;
  delay_line_next(r->hist[r->cur ^ 1].p, hold, hn, d_in, in_stride, n_in, C, s);
  if (n_out > 0) {
    ResampleArgs a{};
    a.tab = r->tab.p;
    a.up = r->up;
    a.down = r->down;
    a.T = (int)r->T;
    a.pitch = (int)rs_pitch(r->T);
    a.hist = hold;
    a.src = d_in;
    a.sstride = in_stride;
    a.y = d_out;
    a.ystride = out_stride;
    a.n_out = n_out;
    a.phase0 = r->phase;
    a.ii0 = r->ahead + hn;
    a.channels = r->channels;
    launch_resample(r->plan, a, s);
    AD_HIP(hipGetLastError());
  }
  if (hn > 0) r->cur ^= 1;
  // resample.go:280-285 after n_out steps
  const int64_t num = r->phase + n_out * r->down;
  r->ahead += num / r->up - n_in;
  r->phase = num % r->up;
  r->order.leave(s);
}

}  // namespace

extern "C" {

int ad_resampler_create(int64_t up, int64_t down, const double* taps, int64_t n_taps, int channels, int device,
                        ad_resampler** out) {
  if (out) *out = nullptr;
  ad_resampler* raw = nullptr;
  const int rc = guard([&] {
    if (!out) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "null output handle");
    if (up <= 0 || down <= 0) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "resample: invalid ratio");  // resample.go:154-156
    if (channels <= 0) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "channels must be positive");
    const int64_t g = gcd64(up, down);  // resample.go:158-160
    up /= g;
    down /= g;
    if (up > kMaxRatio || down > kMaxRatio) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "reduced up and down must be <= 2^30");
    if (!taps || n_taps <= 0 || n_taps % up != 0)
      AD_FAIL(AD_ERR_INVALID_ARGUMENT, "n_taps must be a positive multiple of the reduced up");
    for (int64_t i = 0; i < n_taps; ++i)
      if (!std::isfinite(taps[i])) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "non-finite tap");
    const int64_t T = n_taps / up;
    if (T > kMaxIn) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "too many taps per phase");
    // phase p is taps[p], taps[p + up], ... (resample_design.go:55-66)
    const int64_t pitch = rs_pitch(T);
    std::vector<double> tab((size_t)(up * pitch), 0.0);
    for (int64_t p = 0; p < up; ++p)
      for (int64_t k = 0; k < T; ++k) tab[(size_t)(p * pitch + k)] = taps[p + k * up];

    const int dev = pick_device(device);
    DeviceScope ds(dev);
    std::unique_ptr<ad_resampler> r(new ad_resampler());
    r->device = dev;
    r->channels = channels;
    r->up = up;
    r->down = down;
    r->T = T;
    r->plan = resample_plan(up, down, T);
    AD_HIP(lib_stream_create(&r->stream));
    r->tab.alloc(tab.size());
    AD_HIP(hipMemcpy(r->tab.p, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice));
    if (T > 1) {
      for (auto& hb : r->hist) {
        hb.alloc((size_t)channels * (T - 1));
        AD_HIP(hipMemset(hb.p, 0, hb.n * sizeof(double)));
      }
    }
    raw = r.release();
  });
  if (rc == AD_OK && out) *out = raw;
  return rc;
}

int ad_resampler_predict_output_len(const ad_resampler* r, int64_t n_in, int64_t* n_out) {
  return guard([&] {
    if (!r || !n_out) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "null resampler handle or output");
    if (n_in > kMaxIn) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "n_in must be below 2^31");
    *n_out = predict(r, n_in);
  });
}

int ad_resampler_process(ad_resampler* r, const double* in, int64_t n_in, double* out, int64_t out_cap,
                         int64_t* n_out) {
  return guard([&] {
    if (!r || !n_out) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "null resampler handle or output count");
    check_n_in(n_in);
    const int64_t no = predict(r, n_in);
    if (out_cap < no) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "output capacity below the predicted length");
    check_n_out(no);
    *n_out = no;
    if (n_in == 0) return;
    if (!in || (no > 0 && !out)) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "null buffer");
    DeviceScope ds(r->device);
    const size_t C = (size_t)r->channels;
    r->io_in.reserve(C * n_in);
    if (no > 0) r->io_out.reserve(C * no);
    AD_HIP(hipMemcpyAsync(r->io_in.p, in, C * n_in * sizeof(double), hipMemcpyHostToDevice, r->stream));
    resample_run(r, r->io_in.p, n_in, n_in, r->io_out.p, no, no, r->stream);
    if (no > 0) AD_HIP(hipMemcpyAsync(out, r->io_out.p, C * no * sizeof(double), hipMemcpyDeviceToHost, r->stream));
    AD_HIP(hipStreamSynchronize(r->stream));
  });
}

int ad_resampler_process_device(ad_resampler* r, const double* d_in, int64_t in_stride, int64_t n_in, double* d_out,
                                int64_t out_stride, int64_t out_cap, int64_t* n_out, void* stream) {
  return guard([&] {
    if (!r || !n_out) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "null resampler handle or output count");
    check_n_in(n_in);
    const int64_t no = predict(r, n_in);
    if (out_cap < no) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "output capacity below the predicted length");
    check_n_out(no);
    if (n_in > 0) {
      if (!d_in || (no > 0 && !d_out)) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "null buffer");
      if (in_stride < n_in || (no > 0 && out_stride < no)) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "bad strides");
      if (no > 0) {
        const int64_t C1 = r->channels - 1;
        const char* s0 = reinterpret_cast<const char*>(d_in);
        const char* s1 = reinterpret_cast<const char*>(d_in + C1 * in_stride + n_in);
        const char* o0 = reinterpret_cast<const char*>(d_out);
        const char* o1 = reinterpret_cast<const char*>(d_out + C1 * out_stride + no);
        if (s0 < o1 && o0 < s1) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "input and output overlap");
      }
    }
    *n_out = no;
    if (n_in == 0) return;
    DeviceScope ds(r->device);
    resample_run(r, d_in, in_stride, n_in, d_out, out_stride, no, reinterpret_cast<hipStream_t>(stream));
  });
}

int ad_resampler_reset(ad_resampler* r) {
  // resample.go:241-246; ordered after the last call, whatever stream it used
  return guard([&] {
    if (!r) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "null resampler handle");
    DeviceScope ds(r->device);
    r->order.join(r->stream);
    for (auto& hb : r->hist)
      if (hb.p) AD_HIP(hipMemsetAsync(hb.p, 0, hb.n * sizeof(double), r->stream));
    r->order.leave(r->stream);
    AD_HIP(hipStreamSynchronize(r->stream));
    r->phase = 0;
    r->ahead = 0;
  });
}

int ad_resampler_ratio(const ad_resampler* r, int64_t* up, int64_t* down) {
  return guard([&] {
    if (!r) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "null resampler handle");
    if (up) *up = r->up;
    if (down) *down = r->down;
  });
}

int ad_resampler_taps_per_phase(const ad_resampler* r) { return r ? (int)r->T : 0; }

int ad_resampler_kernel_info(const ad_resampler* r, int* tile, int* tiles_per_workgroup, int* table_in_lds,
                             int* window_in_lds, int* window_prefetch, int64_t* lds_bytes) {
  return guard([&] {
    if (!r) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "null resampler handle");
    if (tile) *tile = (int)r->plan.tile();
    if (tiles_per_workgroup) *tiles_per_workgroup = r->plan.tiles_per_wg;
    if (table_in_lds) *table_in_lds = r->plan.tab_lds;
    if (window_in_lds) *window_in_lds = r->plan.win_lds;
    if (window_prefetch) *window_prefetch = r->plan.prefetch;
    if (lds_bytes) *lds_bytes = r->plan.lds_bytes;
  });
}

void ad_resampler_destroy(ad_resampler* r) {
  if (!r) return;
  (void)guard([&] {
    DeviceScope ds(r->device);
    delete r;
  });
}

}  // extern "C"
