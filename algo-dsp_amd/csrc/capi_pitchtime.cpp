// The time-domain pitch shifter's handle (dsp/effects/pitch/pitch_shifter.go):
// the node AD_FXN_PITCHTIME of an fx graph.  The processor is stateless per
// call (Reset :222 is a no-op): a call stretches its whole block into scratch
// rows and resamples them back into the caller's rows, so in place needs no
// copy of the input.  What the handle keeps is the configuration, the fade-in
// table on the device, the scratch, and the resample's position row while the
// length of the call repeats.
//
// Scratch is [channels][nFrames * stepOut + sequenceLen + 1] doubles (:306-308),
// at ratio 4 more than four times the call, and the algorithm spans the block:
// a call cannot be cut in time.  So the channels run in groups whose rows stay
// within kScratchBytes, each group stretched and resampled before the next.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <memory>

#include "fx_handle.hpp"
#include "pitchtime_kernels.hpp"

namespace adsp {

namespace {

constexpr double kIdentityEps = 1e-9;                // pitchShifterIdentityEps :29
constexpr size_t kScratchBytes = (size_t)2 << 30;    // the stretched rows of one channel group (the STFT handles' bound)
constexpr int64_t kMaxLength = (int64_t)1 << 24;     // sequenceLen and searchLen: the kernels index a frame by int
constexpr int64_t kMaxCall = (int64_t)1 << 29;       // n: 4 n + the frame slack stays below 2^31
constexpr int64_t kMaxGrid = (int64_t)1 << 30;       // workgroups of one launch

struct Derived {  // rebuild :252-296
  int64_t sequence = 0, overlap = 0, search = 0, step = 0;
};

Derived derive(const ad_pitchtime_config& c) {
  if (!positive(c.sample_rate)) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "pitch shifter sample rate must be positive and finite");
  if (!positive(c.pitch_ratio) || !in_range(c.pitch_ratio, 0.25, 4.0))
    AD_FAIL(AD_ERR_INVALID_ARGUMENT, "pitch shifter ratio must be in [0.25, 4]");
  if (!in_range(c.sequence_ms, 20.0, 120.0)) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "pitch shifter sequence must be in [20, 120] ms");
  if (!in_range(c.overlap_ms, 4.0, 60.0)) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "pitch shifter overlap must be in [4, 60] ms");
  if (!in_range(c.search_ms, 2.0, 40.0)) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "pitch shifter search must be in [2, 40] ms");
  if (c.overlap_ms >= c.sequence_ms) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "pitch shifter overlap must be smaller than sequence");
  const double seq = std::round(c.sequence_ms * 0.001 * c.sample_rate);  // math.Round: halves away from zero
  const double ov = std::round(c.overlap_ms * 0.001 * c.sample_rate);
  const double se = std::round(c.search_ms * 0.001 * c.sample_rate);
  if (seq > (double)kMaxLength || se > (double)kMaxLength)
    AD_FAIL(AD_ERR_INVALID_ARGUMENT, "pitch shifter: the sample rate makes a frame longer than the kernels index");
  Derived d;
  d.sequence = std::max<int64_t>((int64_t)seq, 32);
  d.overlap = std::max<int64_t>((int64_t)ov, 8);
  if (d.overlap >= d.sequence) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "pitch shifter overlap too large for sequence");
  d.step = d.sequence - d.overlap;
  if (d.step < 4) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "pitch shifter output hop too small");
  d.search = std::max<int64_t>((int64_t)se, 1);
  if (c.fade_in && c.fade_len != d.overlap)
    AD_FAIL(AD_ERR_INVALID_ARGUMENT, "pitch shifter: the fade-in table must hold overlapLen values");
  return d;
}

void validate(const ad_pitchtime_config& c) { (void)derive(c); }

}  // namespace

struct PitchTime : HandleCore {
  ad_pitchtime_config cfg{};  // fade_in is null here: the table lies in `fade`
  Derived d{};
  DevBuf<double> fade;     // [overlap]
  DevBuf<double> scratch;  // [group][out_pitch]
  DevBuf<double> ref, ref_energy, tile_score;
  DevBuf<int64_t> prev_start;
  DevBuf<int> done, tile_cand;
  PinnedUpload pos;  // the resample's positions of the last call's (n, targetLen)
  int64_t pos_n = -1, pos_len = -1;
};

namespace {

void run(PitchTime* f, double* d_buf, int64_t stride, int64_t n, hipStream_t s) {
  const double ratio = f->cfg.pitch_ratio;
  if (std::fabs(ratio - 1) <= kIdentityEps) return;  // :230-235: the caller's rows are the copy
  CallScope call(f->order, s);
  const Derived& d = f->d;
  const int64_t target = std::max<int64_t>((int64_t)std::round((double)n * ratio), 1);  // :299
  double nominal = (double)d.step / ratio;                                                // :301-304
  if (nominal < 1) nominal = 1;
  const int64_t n_frames = target / d.step + 4;                 // :306
  const int64_t out_pitch = n_frames * d.step + d.sequence + 1;  // :307
  const int mode = (target == 1 || n == 1) ? 1 : 0;              // :397-408
  if (!mode && (f->pos_n != n || f->pos_len != target)) {
    f->pos_n = -1;
    double* h = f->pos.stage((size_t)n);
    const double step = (double)(target - 1) / (double)(n - 1);  // :410
    double p = 0.0;
    for (int64_t i = 0; i < n; ++i) {  // :412-416
      h[i] = p;
      p += step;
    }
    f->pos.send((size_t)n, s);
    f->pos_n = n;
    f->pos_len = target;
  }
  const int tiles = (int)((2 * d.search + 1 + kPtTile - 1) / kPtTile);
  const int64_t ref_pitch = (d.overlap + kPtR - 1) / kPtR * kPtR;
  const int64_t widest = std::max<int64_t>(tiles, (n + 255) / 256);  // workgroups per channel of the widest launch
  int64_t group = std::max<int64_t>((int64_t)(kScratchBytes / ((size_t)out_pitch * sizeof(double))), 1);
  group = std::min<int64_t>(std::min<int64_t>(group, f->channels), std::max<int64_t>(kMaxGrid / widest, 1));
  // hipFree waits for the device, so no earlier call still reads a buffer that grows here
  f->scratch.reserve((size_t)group * out_pitch);
  f->ref.reserve((size_t)group * ref_pitch);
  f->ref_energy.reserve((size_t)group);
  f->prev_start.reserve((size_t)group);
  f->done.reserve((size_t)group);
  f->tile_score.reserve((size_t)group * tiles);
  f->tile_cand.reserve((size_t)group * tiles);
  for (int64_t c0 = 0; c0 < f->channels; c0 += group) {
    PtArgs a{};
    a.channels = (int)std::min<int64_t>(group, f->channels - c0);
    a.in = d_buf + c0 * stride;
    a.stride = stride;
    a.n = n;
    a.out = f->scratch.p;
    a.out_pitch = out_pitch;
    a.ref = f->ref.p;
    a.ref_pitch = ref_pitch;
    a.ref_energy = f->ref_energy.p;
    a.prev_start = f->prev_start.p;
    a.done = f->done.p;
    a.tile_score = f->tile_score.p;
    a.tile_cand = f->tile_cand.p;
    a.fade_in = f->fade.p;
    a.sequence = (int)d.sequence;
    a.overlap = (int)d.overlap;
    a.search = (int)d.search;
    a.tiles = tiles;
    // The rows are not zeroed as `out = make(...)` :308 is: frame 0 writes [0, sequenceLen), every later frame
    // cross-fades only over what the frame before wrote and extends the row to outLen, a channel leaves the loop
    // early (:344) only with outLen >= targetLen, and the resample clamps its reads to [0, targetLen).
    launch_pt_first(a, s);  // :310-317
    int64_t out_len = d.sequence;
    double next_nominal = nominal;
    while (out_len < target + d.sequence) {  // :319
      const int64_t predicted = (int64_t)std::round(next_nominal);  // :325
      const int64_t out_start = out_len - d.overlap;                // :328
      out_len = out_start + d.sequence;                             // :340
      launch_pt_search(a, predicted, s);
      launch_pt_assemble(a, predicted, out_start, out_len >= target ? 1 : 0, s);
      next_nominal += nominal;  // :342
    }
    // out[:targetLen] :349-351 (targetLen <= outCap always: nFrames * stepOut > targetLen)
    launch_pt_resample(f->scratch.p, out_pitch, target, f->pos.dev.p, d_buf + c0 * stride, stride, n, a.channels, mode, s);
  }
  AD_HIP(hipGetLastError());
}

}  // namespace

int pitchtime_validate(const ad_pitchtime_config* cfg) { return validate_config(cfg, validate); }

int pitchtime_create(const ad_pitchtime_config* cfg, int channels, int device, PitchTime** out) {
  return create_handle(cfg, channels, device, out, validate, [](PitchTime* f, const ad_pitchtime_config& c) {
    f->d = derive(c);
    const size_t len = (size_t)f->d.overlap;
    std::vector<double> table(len);
    if (c.fade_in) {
      std::copy(c.fade_in, c.fade_in + len, table.begin());
    } else {
      for (size_t i = 0; i < len; ++i)  // :288-293 (overlapLen is at least 8)
        table[i] = 0.5 - 0.5 * std::cos(M_PI * ((double)i / (double)(len - 1)));
    }
    f->fade.alloc(len);
    AD_HIP(hipMemcpyAsync(f->fade.p, table.data(), len * sizeof(double), hipMemcpyHostToDevice, f->stream));
    AD_HIP(hipStreamSynchronize(f->stream));  // table leaves scope
    f->cfg.fade_in = nullptr;
    f->cfg.fade_len = 0;
  });
}

int pitchtime_process_device(PitchTime* p, double* d_buf, int64_t stride, int64_t n, void* stream) {
  return process_device(p, d_buf, stride, n, stream, run, kMaxCall);
}

int pitchtime_reset(PitchTime* p) {
  return with_handle(p, [] {});  // Reset :222: the processor keeps nothing between calls
}

void pitchtime_destroy(PitchTime* p) { destroy_handle(p); }

}  // namespace adsp
