// The host-side scaffold of an effect handle's C ABI, written once: the core
// every handle derives from, create / process / destroy around the handle's
// own work, and the small validators and device helpers the handles share.
//
// A handle is a struct deriving from HandleCore (or from a family's core that
// does) with a member `cfg`; its file keeps validate(const Cfg&), a run
// function per call shape, and the entry points, which are one line each where
// the signature is the common one:
//   create          create_handle(cfg, channels, device, out, validate, init)
//   process         process_host(h, buf, n, run)
//   process_device  process_device(h, d_buf, stride, n, stream, run)
//   destroy         destroy_handle(h)
// and with_handle(h, fn) for every entry point of another shape.  A run
// function orders itself against the handle's other calls with a CallScope
// (stream_order.hpp).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <memory>
#include <vector>

#include "ad_common.hpp"
#include "stream_order.hpp"

namespace adsp {

// ---- validators ---------------------------------------------------------------
inline bool is_finite(double v) { return std::isfinite(v); }
inline bool positive(double v) { return v > 0 && is_finite(v); }
inline bool in_range(double v, double lo, double hi) { return v >= lo && v <= hi; }  // false for NaN
inline bool flag(int v) { return v == 0 || v == 1; }

// a whole number in [lo, hi], as the reference's int and bool setters take
inline int whole(double value, int lo, int hi, const char* msg) {
  if (!in_range(value, lo, hi) || value != std::floor(value)) AD_FAIL(AD_ERR_INVALID_ARGUMENT, msg);
  return (int)value;
}

template <class H>
void check_channel(const H* h, int channel) {
  if (!h) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "null handle");
  if (channel < 0 || channel >= h->channels) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "channel out of range");
}

// ---- device helpers -------------------------------------------------------------
inline void zero(DevBuf<double>& b, hipStream_t s) {
  if (b.p) AD_HIP(hipMemsetAsync(b.p, 0, b.n * sizeof(double), s));
}

inline void fill(DevBuf<double>& b, double v, hipStream_t s) {
  if (v == 0.0) return zero(b, s);
  const std::vector<double> h(b.n, v);
  AD_HIP(hipMemcpyAsync(b.p, h.data(), b.n * sizeof(double), hipMemcpyHostToDevice, s));
  AD_HIP(hipStreamSynchronize(s));  // h leaves scope
}

// Samples of a call one pass takes, so that `rows` scratch rows per channel stay within kSegmentScratchBytes:
// a call longer than this is cut.
constexpr size_t kSegmentScratchBytes = (size_t)256 << 20;
constexpr int64_t kMinSegment = 1024;
inline int64_t scratch_segment(int64_t n, int channels, int rows) {
  const int64_t fit = (int64_t)(kSegmentScratchBytes / ((size_t)channels * rows * sizeof(double))) - 1;
  return std::min(n, std::max(fit, kMinSegment));
}

// A table a call computes on the host and its kernels read: a pinned host buffer and its device twin.
//   double* h = stage(n);  ...fill h[0..n)...  send(n, s);
// stage() waits until the previous upload has left the host buffer, and grows both buffers together.
struct PinnedUpload {
  DevBuf<double> dev;
  double* host = nullptr;  // pinned; reused once `sent` has passed
  size_t cap = 0;
  hipEvent_t sent = nullptr;
  bool pending = false;
  PinnedUpload() = default;
  PinnedUpload(const PinnedUpload&) = delete;
  PinnedUpload& operator=(const PinnedUpload&) = delete;
  ~PinnedUpload() {
    if (sent) {
      (void)hipEventSynchronize(sent);
      (void)hipEventDestroy(sent);
    }
    if (host) (void)hipHostFree(host);
  }
  double* stage(size_t n) {
    if (pending) AD_HIP(hipEventSynchronize(sent));
    pending = false;
    if (n > cap) {
      if (host) AD_HIP(hipHostFree(host));
      host = nullptr;
      cap = 0;
      const size_t grown = std::max<size_t>(n, 4096);
      AD_HIP(hipHostMalloc(reinterpret_cast<void**>(&host), grown * sizeof(double), hipHostMallocDefault));
      cap = grown;
      dev.reserve(cap);  // hipFree waits for the device, so no earlier call still reads the old one
    }
    return host;
  }
  void send(size_t n, hipStream_t s) {
    AD_HIP(hipMemcpyAsync(dev.p, host, n * sizeof(double), hipMemcpyHostToDevice, s));
    if (!sent) AD_HIP(hipEventCreateWithFlags(&sent, hipEventDisableTiming));
    AD_HIP(hipEventRecord(sent, s));
    pending = true;
  }
};

// ---- the handle ---------------------------------------------------------------
struct HandleCore {
  int device = 0, channels = 0;
  hipStream_t stream = nullptr;  // host-buffer calls, resets, state access
  StreamOrder order;             // calls may come on any stream
  DevBuf<double> io;             // host-buffer calls
  ~HandleCore() {
    order.release();
    if (stream) {
      (void)hipStreamSynchronize(stream);
      (void)lib_stream_destroy(stream);
    }
  }
};

// ad_X_validate
template <class Cfg>
int validate_config(const Cfg* cfg, void (*validate)(const Cfg&)) {
  return guard([&] {
    if (!cfg) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "null config");
    validate(*cfg);
  });
}

// ad_X_create.  The arguments and the config are checked before any device call (a bad config is
// AD_ERR_INVALID_ARGUMENT on a machine without a device too).  init(H*, const Cfg&) allocates and fills the
// handle's own state, on h->stream where it can; it sees the caller's config, the handle holds a copy in h->cfg.
template <class H, class Cfg, class Init>
int create_handle(const Cfg* cfg, int channels, int device, H** out, void (*validate)(const Cfg&), Init init) {
  if (out) *out = nullptr;
  H* raw = nullptr;
  const int rc = guard([&] {
    if (!out) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "null output handle");
    if (!cfg) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "null config");
    if (channels <= 0) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "channels must be positive");
    validate(*cfg);
    const int dev = pick_device(device);
    DeviceScope ds(dev);
    std::unique_ptr<H> h(new H());
    h->device = dev;
    h->channels = channels;
    h->cfg = *cfg;
    AD_HIP(lib_stream_create(&h->stream));
    init(h.get(), *cfg);
    AD_HIP(hipStreamSynchronize(h->stream));
    raw = h.release();
  });
  if (rc == AD_OK && out) *out = raw;
  return rc;
}

// An entry point of any shape: the null check, the status translation and the handle's device.
template <class H, class Fn>
int with_handle(H* h, Fn&& fn) {
  return guard([&] {
    if (!h) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "null handle");
    DeviceScope ds(h->device);
    fn();
  });
}

// ad_X_process: buf [channels][n] on the host, in place, through the handle's staging buffer and stream.
// run(h, d_buf, stride, n, stream) is the call's device work; `limit` bounds n where the kernels index by int.
template <class H, class Run>
int process_host(H* h, double* buf, int64_t n, Run run, int64_t limit = std::numeric_limits<int64_t>::max()) {
  return guard([&] {
    if (!h) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "null handle");
    if (n < 0 || n >= limit || (n > 0 && !buf)) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "bad buffer");
    if (n == 0) return;
    DeviceScope ds(h->device);
    const size_t count = (size_t)h->channels * n;
    h->io.reserve(count);
    AD_HIP(hipMemcpyAsync(h->io.p, buf, count * sizeof(double), hipMemcpyHostToDevice, h->stream));
    run(h, h->io.p, n, n, h->stream);
    AD_HIP(hipMemcpyAsync(buf, h->io.p, count * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    AD_HIP(hipStreamSynchronize(h->stream));
  });
}

// ad_X_process_device: d_buf [channels][stride] on the device, in place, on the caller's stream.
template <class H, class Run>
int process_device(H* h, double* d_buf, int64_t stride, int64_t n, void* stream, Run run,
                   int64_t limit = std::numeric_limits<int64_t>::max()) {
  return guard([&] {
    if (!h) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "null handle");
    if (n < 0 || n >= limit || (n > 0 && (!d_buf || stride < n))) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "bad buffer geometry");
    if (n == 0) return;
    DeviceScope ds(h->device);
    run(h, d_buf, stride, n, reinterpret_cast<hipStream_t>(stream));
  });
}

// ad_X_destroy.  The handle's last call has finished before anything of the handle is freed: a derived
// handle's buffers go before HandleCore's destructor runs, and hipFree waiting for the device is not a contract.
template <class H>
void destroy_handle(H* h) {
  if (!h) return;
  (void)guard([&] {
    DeviceScope ds(h->device);
    h->order.release();
    delete h;
  });
}

}  // namespace adsp
