// Call ordering and the ping-pong delay line shared by the handles that may be
// called on any stream (ad_conv, ad_fir, ad_resampler and every effect handle of fx_handle.hpp).
#pragma once

#include <hip/hip_runtime.h>

#include "ad_common.hpp"

namespace adsp {

// Orders the calls of a handle that may be called on any stream: its device
// state is shared by every stream a caller uses, so a call on another stream
// than the previous one first waits for that call's last operation.
//   enter(s) ... the call's work on s ... leave(s)
// `last` may be the NULL stream, which is a stream like any other and compares
// equal to nullptr: has_last, not last, says whether a call has been enqueued.
// (capi_spectral.cpp's CallOrder is another thing: per device, not per handle.)
struct StreamOrder {
  hipEvent_t done = nullptr;   // recorded on `last` after each call's last operation
  hipStream_t last = nullptr;  // stream of the last call (valid when has_last)
  bool has_last = false;
  StreamOrder() = default;
  StreamOrder(const StreamOrder&) = delete;
  StreamOrder& operator=(const StreamOrder&) = delete;
  ~StreamOrder() { release(); }
  void enter(hipStream_t s) {
    ensure();
    if (has_last && last != s) AD_HIP(hipStreamWaitEvent(s, done, 0));
  }
  void leave(hipStream_t s) {
    ensure();
    AD_HIP(hipEventRecord(done, s));
    last = s;
    has_last = true;
  }
  // a library stream's work (a reset) after the last call, whatever stream it used
  void join(hipStream_t s) {
    if (has_last) AD_HIP(hipStreamWaitEvent(s, done, 0));
  }
  void wait_host() const {
    if (has_last) AD_HIP(hipEventSynchronize(done));
  }
  void clear() { has_last = false; }  // the handle is idle: the next call waits for nothing
  // waits for the last call and frees the event (a destructor that must free it before other members)
  void release() {
    if (done) {
      (void)hipEventSynchronize(done);
      (void)hipEventDestroy(done);
      done = nullptr;
    }
    has_last = false;
  }

 private:
  void ensure() {
    if (!done) AD_HIP(hipEventCreateWithFlags(&done, hipEventDisableTiming));
  }
};

// One call of a handle on stream s: enter(s) now, leave(s) when the scope ends, by an exception too, so
// that what was enqueued before a failure is still covered by the event the next call waits for.  Every
// run function of an effect handle opens one after its early returns (a call that enqueues nothing does
// not count as a call); a hand-written enter / leave pair would skip leave on a throw in between.
struct CallScope {
  StreamOrder& calls;
  hipStream_t s;
  CallScope(StreamOrder& c, hipStream_t stream) : calls(c), s(stream) { calls.enter(s); }
  CallScope(const CallScope&) = delete;
  CallScope& operator=(const CallScope&) = delete;
  ~CallScope() {
    try {
      calls.leave(s);
    } catch (...) {  // the call's own error, if any, is the one to report
    }
  }
};

// The next delay line of a ping-pong pair: the last hn samples per channel of
// [hold | src] into hnew (hold, hnew: [C][hn]; src: n new samples per channel
// at row stride src_stride).  Nothing a kernel of the same call reads (hold,
// src) is written.
inline void delay_line_next(double* hnew, const double* hold, int64_t hn, const double* src, int64_t src_stride,
                            int64_t n, size_t C, hipStream_t s) {
  if (hn <= 0) return;
  if (n >= hn) {
    AD_HIP(hipMemcpy2DAsync(hnew, hn * sizeof(double), src + (n - hn), src_stride * sizeof(double),
                            hn * sizeof(double), C, hipMemcpyDeviceToDevice, s));
  } else {
    AD_HIP(hipMemcpy2DAsync(hnew, hn * sizeof(double), hold + n, hn * sizeof(double), (hn - n) * sizeof(double), C,
                            hipMemcpyDeviceToDevice, s));
    AD_HIP(hipMemcpy2DAsync(hnew + (hn - n), hn * sizeof(double), src, src_stride * sizeof(double),
                            n * sizeof(double), C, hipMemcpyDeviceToDevice, s));
  }
}

}  // namespace adsp
