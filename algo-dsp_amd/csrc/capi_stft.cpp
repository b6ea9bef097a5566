// C ABI of the spectral freeze (dsp/effects/spectral_freeze.go) and the
// spectral pitch shifter (dsp/effects/pitch/pitch_shift_spectral.go).  A handle
// keeps the reference's configuration on the host, the window and omega tables
// and (the freeze) heldMagnitude and phaseAcc on the device, one set per
// channel.  A call is the reference's Process of the whole buffer: the frame
// passes, the walk and the overlap-add of stft_kernels.hip over groups of
// channels, so that the scratch rows of a group stay within kScratchBytes.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <memory>
#include <numeric>
#include <vector>

#include "fx_handle.hpp"
#include "stft_kernels.hpp"

using namespace adsp;

namespace {

constexpr size_t kScratchBytes = (size_t)2 << 30;  // the scratch rows of one group of channels
constexpr double kBinShiftThreshold = 0.15;        // pitch_shift_spectral.go:24
constexpr double kIdentityEps = 1e-9;              // pitch_shifter.go:29
constexpr double kMinRatio = 0.25, kMaxRatio = 4.0;  // pitch_shifter.go:19-20
constexpr int64_t kMaxSamples = (int64_t)1 << 31;

void check_frame(int size, const char* who) {
  if (size < kStftMinFrame || !is_pow2(size))
    AD_FAIL(AD_ERR_INVALID_ARGUMENT, std::string(who) + " frame size must be power-of-two and >= 64");
  if (size > kStftMaxFrame)
    AD_FAIL(AD_ERR_INVALID_ARGUMENT, std::string(who) + " frame size above 4096 is not supported on the device");
}

void check_window(const double* w, int n, const char* who) {
  if (!w) AD_FAIL(AD_ERR_INVALID_ARGUMENT, std::string(who) + " needs a window table of frame_size coefficients");
  for (int i = 0; i < n; ++i)
    if (!std::isfinite(w[i])) AD_FAIL(AD_ERR_INVALID_ARGUMENT, std::string(who) + " window coefficient is not finite");
}

void validate(const ad_specfreeze_config& c) {  // validate spectral_freeze.go:340-369
  if (!positive(c.sample_rate)) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "spectral freeze sample rate must be > 0");
  check_frame(c.frame_size, "spectral freeze");
  if (c.hop_size <= 0 || c.hop_size >= c.frame_size)
    AD_FAIL(AD_ERR_INVALID_ARGUMENT, "spectral freeze hop size must be in [1, frame size)");
  if (!(c.mix >= 0 && c.mix <= 1)) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "spectral freeze mix must be in [0, 1]");
  if (c.phase_mode != AD_SPECFREEZE_PHASE_HOLD && c.phase_mode != AD_SPECFREEZE_PHASE_ADVANCE)
    AD_FAIL(AD_ERR_INVALID_ARGUMENT, "spectral freeze phase mode invalid");
  if (c.frozen != 0 && c.frozen != 1) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "spectral freeze frozen must be 0 or 1");
  check_window(c.window, c.frame_size, "spectral freeze");
}

void validate(const ad_pitchspec_config& c) {  // validate pitch_shift_spectral.go:547-570
  if (!positive(c.sample_rate))
    AD_FAIL(AD_ERR_INVALID_ARGUMENT, "spectral pitch shifter sample rate must be positive and finite");
  if (!positive(c.pitch_ratio) || c.pitch_ratio < kMinRatio || c.pitch_ratio > kMaxRatio)
    AD_FAIL(AD_ERR_INVALID_ARGUMENT, "spectral pitch ratio must be in [0.25, 4]");
  check_frame(c.frame_size, "spectral");
  if (c.analysis_hop <= 0 || c.analysis_hop >= c.frame_size)
    AD_FAIL(AD_ERR_INVALID_ARGUMENT, "spectral analysis hop must be in [1, frame size)");
  check_window(c.window, c.frame_size, "spectral pitch shifter");
  if (c.resample_taps && c.n_resample_taps <= 0) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "resampling prototype without taps");
}


// What the two handles share: the tables and the scratch rows.
struct StftCore : HandleCore {
  int frame = 0;
  std::vector<double> h_win;
  DevBuf<double> win, omega;     // [N], [N/2 + 1]
  DevBuf<double> rows;           // [group][frames][N + 2]
  // ad_*_profile: events between the passes of the calls made while it is on
  bool profiling = false;
  std::vector<std::pair<int, hipEvent_t>> marks;  // (the pass that ends here, or -1: a group starts)
  void mark(int pass, hipStream_t s) {
    if (!profiling) return;
    hipEvent_t e = nullptr;
    AD_HIP(hipEventCreate(&e));
    marks.emplace_back(pass, e);
    AD_HIP(hipEventRecord(e, s));
  }
  void read_marks(double* ms) {
    for (int i = 0; i < AD_STFT_PASSES; ++i) ms[i] = 0;
    for (size_t i = 0; i < marks.size(); ++i) {
      AD_HIP(hipEventSynchronize(marks[i].second));
      if (i > 0 && marks[i].first >= 0) {
        float t = 0;
        AD_HIP(hipEventElapsedTime(&t, marks[i - 1].second, marks[i].second));
        ms[marks[i].first] += t;
      }
    }
    drop_marks();
  }
  void drop_marks() {
    for (auto& m : marks) (void)hipEventDestroy(m.second);
    marks.clear();
  }
  ~StftCore() { drop_marks(); }
  int bins() const { return frame / 2 + 1; }
  // rebuildState's tables (spectral_freeze.go:388-400): the caller's window, omega[k] = 2*pi*k/N
  void set_tables(int n, const double* window) {
    order.wait_host();
    frame = n;
    h_win.assign(window, window + n);
    std::vector<double> om((size_t)n / 2 + 1);
    for (size_t k = 0; k < om.size(); ++k) om[k] = 2 * M_PI * (double)k / (double)n;
    win.alloc((size_t)n);
    omega.alloc(om.size());
    AD_HIP(hipMemcpy(win.p, h_win.data(), (size_t)n * sizeof(double), hipMemcpyHostToDevice));
    AD_HIP(hipMemcpy(omega.p, om.data(), om.size() * sizeof(double), hipMemcpyHostToDevice));
  }
  // channels of one pass, so that their scratch rows stay within kScratchBytes (one channel at least)
  int group(int64_t frames) const {
    const size_t per = (size_t)frames * (size_t)stft_pitch(frame) * sizeof(double);
    const size_t fit = std::max<size_t>(1, kScratchBytes / std::max<size_t>(per, 1));
    return (int)std::min<size_t>((size_t)channels, fit);
  }
  StftFrameArgs frame_args(const double* x, int64_t stride, int64_t n, int hop, int ch, int64_t frames) const {
    StftFrameArgs a{};
    a.x = x;
    a.x_stride = stride;
    a.n = n;
    a.win = win.p;
    a.hop = hop;
    a.channels = ch;
    a.frames = frames;
    const int64_t pitch = stft_pitch(frame);
    a.mag = rows.p;
    a.mag_ch = frames * pitch, a.mag_fr = pitch;
    a.phase = rows.p + bins();
    a.ph_ch = frames * pitch, a.ph_fr = pitch;
    a.rows = rows.p;
    a.row_ch = frames * pitch, a.row_fr = pitch;
    return a;
  }
  StftOlaArgs ola_args(int hop, int64_t frames, double* out, int64_t out_stride, int64_t out_n, int ch) const {
    StftOlaArgs o{};
    const int64_t pitch = stft_pitch(frame);
    o.rows = rows.p;
    o.row_ch = frames * pitch, o.row_fr = pitch;
    o.win = win.p;
    o.frame = frame;
    o.hop = hop;
    o.frames = frames;
    o.out = out;
    o.out_stride = out_stride;
    o.out_n = out_n;
    o.channels = ch;
    return o;
  }
};

}  // namespace

struct ad_specfreeze : StftCore {
  ad_specfreeze_config cfg{};  // window: NULL (h_win holds it)
  DevBuf<double> held, acc;    // heldMagnitude, phaseAcc [channels][bins]
  bool has_frozen = false;     // hasFrozenFrame
};

struct ResamplerDel {
  void operator()(ad_resampler* r) const { ad_resampler_destroy(r); }
};

struct ad_pitchspec : StftCore {
  ad_pitchspec_config cfg{};  // pointers NULL (h_win, taps hold them)
  int synthesis_hop = 0;      // updateSynthesisHop :614-618
  std::vector<double> taps;   // the resampling prototype for the reduced hops
  std::unique_ptr<ad_resampler, ResamplerDel> rs;
  int rs_channels = 0;
  DevBuf<double> stretched, rs_out;
};

namespace {

// rebuildState :371-410: new tables, cleared capture
void freeze_rebuild(ad_specfreeze* f, int n, const double* window) {
  DeviceScope ds(f->device);
  f->set_tables(n, window);
  const size_t count = (size_t)f->channels * f->bins();
  f->held.alloc(count);
  f->acc.alloc(count);
  zero(f->held, f->stream);
  zero(f->acc, f->stream);
  AD_HIP(hipStreamSynchronize(f->stream));
  f->has_frozen = false;
}

void freeze_run(ad_specfreeze* f, double* d_buf, int64_t stride, int64_t n, hipStream_t s) {
  CallScope call(f->order, s);
  const int hop = f->cfg.hop_size, N = f->frame, B = f->bins();
  const int64_t frames = 1 + (n - 1) / hop;  // ProcessWithError :220-221
  const int64_t pitch = stft_pitch(N);
  const bool frozen = f->cfg.frozen != 0;
  const bool capture = frozen && !f->has_frozen;
  if (capture) {  // :250-260: the first frame of the call, every channel
    StftFrameArgs a = f->frame_args(d_buf, stride, n, hop, f->channels, 1);
    a.mag = f->held.p, a.mag_ch = B, a.mag_fr = 0;
    a.phase = f->acc.p, a.ph_ch = B, a.ph_fr = 0;
    launch_stft_frames(N, STFT_ANALYSIS, a, s);
  }
  const int G = f->group(frames);
  f->rows.reserve((size_t)G * frames * pitch);  // hipFree waits for the device, so no earlier call still reads the old one
  for (int c0 = 0; c0 < f->channels; c0 += G) {
    const int cg = std::min(G, f->channels - c0);
    double* buf = d_buf + (int64_t)c0 * stride;
    StftFrameArgs a = f->frame_args(buf, stride, n, hop, cg, frames);
    f->mark(-1, s);
    if (!frozen) {
      launch_stft_frames(N, STFT_FUSED, a, s);  // :276-286
      f->mark(AD_STFT_PASS_FUSED, s);
    } else {
      StftFreezeWalkArgs w{};
      w.rows = f->rows.p;
      w.row_ch = frames * pitch, w.row_fr = pitch;
      w.phase_acc = f->acc.p + (size_t)c0 * B;
      w.omega = f->omega.p;
      w.bins = B;
      w.channels = cg;
      w.frames = frames;
      w.hop_f = (double)hop;
      w.advance = f->cfg.phase_mode == AD_SPECFREEZE_PHASE_ADVANCE;
      w.just_captured = capture;
      launch_stft_freeze_walk(w, s);
      f->mark(AD_STFT_PASS_WALK, s);
      a.mag = f->held.p + (size_t)c0 * B, a.mag_ch = B, a.mag_fr = 0;
      launch_stft_frames(N, STFT_SYNTH, a, s);  // :262-274: no forward transform for a captured frame
      f->mark(AD_STFT_PASS_SYNTHESIS, s);
    }
    StftOlaArgs o = f->ola_args(hop, frames, buf, stride, n, cg);
    o.mix_dry = 1;
    o.mix = f->cfg.mix;
    launch_stft_ola(o, s);
    f->mark(AD_STFT_PASS_OLA, s);
  }
  AD_HIP(hipGetLastError());
  if (capture) f->has_frozen = true;
}

int pitch_path(const ad_pitchspec* p) {
  if (std::fabs(p->cfg.pitch_ratio - 1) <= kIdentityEps) return 0;  // Process :243
  return std::fabs(p->cfg.pitch_ratio - 1) <= kBinShiftThreshold ? 1 : 2;  // useBinShifting :230-232
}

void pitch_update_hop(ad_pitchspec* p) {  // updateSynthesisHop :614-618
  const int h = (int)std::round((double)p->cfg.analysis_hop * p->cfg.pitch_ratio);
  const int now = std::max(h, 1);
  if (now != p->synthesis_hop) {
    p->taps.clear();
    p->rs.reset();
  }
  p->synthesis_hop = now;
}

void pitch_install_taps(ad_pitchspec* p, const double* taps, int64_t n) {
  if (!taps || n <= 0) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "spectral pitch shifter: empty resampling prototype");
  const int64_t g = std::gcd((int64_t)p->cfg.analysis_hop, (int64_t)p->synthesis_hop);
  const int64_t up = p->cfg.analysis_hop / g;
  if (n % up != 0) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "spectral pitch shifter: prototype length must be a multiple of the reduced analysis hop");
  for (int64_t i = 0; i < n; ++i)
    if (!std::isfinite(taps[i])) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "spectral pitch shifter: non-finite tap");
  p->order.wait_host();
  p->taps.assign(taps, taps + n);
  p->rs.reset();
}

void pitch_rebuild(ad_pitchspec* p, int n, const double* window) {
  DeviceScope ds(p->device);
  p->set_tables(n, window);
}

void pitch_run(ad_pitchspec* p, double* d_buf, int64_t stride, int64_t n, hipStream_t s) {
  const int path = pitch_path(p);
  if (path == 0) return;  // the input's own bits
  const int hop = p->cfg.analysis_hop, N = p->frame, shop = path == 1 ? hop : p->synthesis_hop;
  const bool resample = shop != hop;
  if (resample && p->taps.empty())
    AD_FAIL(AD_ERR_INVALID_ARGUMENT, "spectral pitch shifter: the time stretch needs a resampling prototype for its hops");
  CallScope call(p->order, s);
  const int64_t frames = 1 + (n - 1) / hop;  // :291, :396
  const int64_t pitch = stft_pitch(N);
  const int G = p->group(frames);
  p->rows.reserve((size_t)G * frames * pitch);
  const int64_t slen = (frames - 1) * shop + N;  // :397
  int64_t no = 0, opitch = 0;
  if (resample) {
    if (slen >= kMaxSamples) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "spectral pitch shifter: stretched signal of 2^31 samples or more");
    if (!p->rs || p->rs_channels != G) {
      ad_resampler* r = nullptr;
      if (ad_resampler_create(hop, shop, p->taps.data(), (int64_t)p->taps.size(), G, p->device, &r) != AD_OK)
        AD_FAIL(AD_ERR_INVALID_ARGUMENT, std::string("spectral pitch shifter: resampler: ") + ad_last_error());
      p->rs.reset(r);
      p->rs_channels = G;
    }
    if (p->stretched.n < (size_t)G * slen) {
      p->stretched.alloc((size_t)G * slen);
      zero(p->stretched, s);
    }
  }
  for (int c0 = 0; c0 < p->channels; c0 += G) {
    const int cg = std::min(G, p->channels - c0);
    double* buf = d_buf + (int64_t)c0 * stride;
    const StftFrameArgs a = p->frame_args(buf, stride, n, hop, cg, frames);
    p->mark(-1, s);
    launch_stft_frames(N, STFT_ANALYSIS, a, s);
    p->mark(AD_STFT_PASS_ANALYSIS, s);
    StftWalkArgs w{};
    w.rows = p->rows.p;
    w.row_ch = frames * pitch, w.row_fr = pitch;
    w.omega = p->omega.p;
    w.channels = cg;
    w.frames = frames;
    w.hop_f = (double)hop;
    w.syn_hop_f = (double)shop;
    w.ratio = p->cfg.pitch_ratio;
    launch_stft_walk(N, path == 1 ? STFT_WALK_BINSHIFT : STFT_WALK_STRETCH, w, s);
    p->mark(AD_STFT_PASS_WALK, s);
    launch_stft_frames(N, STFT_SYNTH, a, s);
    p->mark(AD_STFT_PASS_SYNTHESIS, s);
    if (!resample) {  // fitLength of a signal at least n long (:389, :512-514)
      launch_stft_ola(p->ola_args(shop, frames, buf, stride, n, cg), s);
      p->mark(AD_STFT_PASS_OLA, s);
      continue;
    }
    launch_stft_ola(p->ola_args(shop, frames, p->stretched.p, slen, slen, cg), s);
    p->mark(AD_STFT_PASS_OLA, s);
    // resample.Resample(stretched, analysisHop, synthesisHop, quality) :516-521 from a fresh state, then fitLength
    if (ad_resampler_reset(p->rs.get()) != AD_OK || ad_resampler_predict_output_len(p->rs.get(), slen, &no) != AD_OK)
      AD_FAIL(AD_ERR_INTERNAL, std::string("spectral pitch shifter: resampler: ") + ad_last_error());
    opitch = std::max(no, n);
    p->rs_out.reserve((size_t)G * opitch);
    AD_HIP(hipMemsetAsync(p->rs_out.p, 0, (size_t)G * opitch * sizeof(double), s));
    if (ad_resampler_process_device(p->rs.get(), p->stretched.p, slen, slen, p->rs_out.p, opitch, opitch, &no, s) != AD_OK)
      AD_FAIL(AD_ERR_INTERNAL, std::string("spectral pitch shifter: resampler: ") + ad_last_error());
    AD_HIP(hipMemcpy2DAsync(buf, stride * sizeof(double), p->rs_out.p, opitch * sizeof(double), n * sizeof(double), cg,
                            hipMemcpyDeviceToDevice, s));
    p->mark(AD_STFT_PASS_RESAMPLE, s);
  }
  AD_HIP(hipGetLastError());
}

template <class H>
int profile(H* f, int enable, double* ms) {
  return with_handle(f, [&] {
    f->order.wait_host();
    if (ms)
      f->read_marks(ms);
    else
      f->drop_marks();
    f->profiling = enable != 0;
  });
}

}  // namespace

extern "C" {

// ---- ad_specfreeze ----------------------------------------------------------
void ad_specfreeze_default_config(ad_specfreeze_config* cfg, double sample_rate) {
  if (!cfg) return;
  *cfg = ad_specfreeze_config{};
  cfg->sample_rate = sample_rate;  // NewSpectralFreeze spectral_freeze.go:65-72
  cfg->frame_size = 1024;
  cfg->hop_size = 256;
  cfg->mix = 1;
  cfg->window_type = 1;  // window.TypeHann
  cfg->phase_mode = AD_SPECFREEZE_PHASE_ADVANCE;
  cfg->frozen = 0;
}

int ad_specfreeze_validate(const ad_specfreeze_config* cfg) { return validate_config(cfg, validate); }

int ad_specfreeze_create(const ad_specfreeze_config* cfg, int channels, int device, ad_specfreeze** out) {
  return create_handle(cfg, channels, device, out, validate, [](ad_specfreeze* f, const ad_specfreeze_config& c) {
    freeze_rebuild(f, c.frame_size, c.window);
    f->cfg.window = nullptr;
  });
}

int ad_specfreeze_set_param(ad_specfreeze* f, int which, double value) {
  return with_handle(f, [&] {
    ad_specfreeze_config c = f->cfg;
    c.window = f->h_win.data();
    switch (which) {
      case AD_SPECFREEZE_SAMPLE_RATE: c.sample_rate = value; break;
      case AD_SPECFREEZE_HOP:
        c.hop_size = whole(value, INT_MIN, INT_MAX, "spectral freeze hop size must be a whole number");
        break;
      case AD_SPECFREEZE_MIX: c.mix = value; break;
      case AD_SPECFREEZE_PHASE_MODE:
        c.phase_mode = whole(value, INT_MIN, INT_MAX, "spectral freeze phase mode invalid");
        break;
      case AD_SPECFREEZE_FROZEN:
        c.frozen = whole(value, INT_MIN, INT_MAX, "spectral freeze frozen must be 0 or 1");
        break;
      default: AD_FAIL(AD_ERR_INVALID_ARGUMENT, "unknown spectral freeze parameter");
    }
    validate(c);  // every other field is valid already: the setter's own check
    if (c.frozen != f->cfg.frozen) f->has_frozen = false;  // SetFrozen :169-175
    c.window = nullptr;
    f->cfg = c;
  });
}

int ad_specfreeze_set_frame(ad_specfreeze* f, int frame_size, const double* window) {
  return with_handle(f, [&] {
    check_frame(frame_size, "spectral freeze");
    check_window(window, frame_size, "spectral freeze");
    f->cfg.frame_size = frame_size;  // SetFrameSize :115-127
    if (f->cfg.hop_size >= frame_size) f->cfg.hop_size = std::max(frame_size / 4, 1);
    freeze_rebuild(f, frame_size, window);
  });
}

int ad_specfreeze_set_window(ad_specfreeze* f, int window_type, const double* window) {
  return with_handle(f, [&] {
    check_window(window, f->frame, "spectral freeze");
    f->cfg.window_type = window_type;  // SetWindowType :152-155
    const std::vector<double> w(window, window + f->frame);  // window may be h_win itself
    freeze_rebuild(f, f->frame, w.data());
  });
}

int ad_specfreeze_get_config(const ad_specfreeze* f, ad_specfreeze_config* cfg) {
  return guard([&] {
    if (!f || !cfg) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "null spectral freeze handle or config");
    *cfg = f->cfg;
  });
}

int ad_specfreeze_state(ad_specfreeze* f, double* held_magnitude, double* phase_acc, int* has_frozen) {
  return with_handle(f, [&] {
    f->order.wait_host();
    const size_t bytes = (size_t)f->channels * f->bins() * sizeof(double);
    if (held_magnitude) AD_HIP(hipMemcpy(held_magnitude, f->held.p, bytes, hipMemcpyDeviceToHost));
    if (phase_acc) AD_HIP(hipMemcpy(phase_acc, f->acc.p, bytes, hipMemcpyDeviceToHost));
    if (has_frozen) *has_frozen = f->has_frozen ? 1 : 0;
  });
}

int ad_specfreeze_norm(ad_specfreeze* f, double* norm, int64_t n) {
  return with_handle(f, [&] {
    if (n < 0 || n >= kMaxSamples || (n > 0 && !norm)) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "bad buffer");
    if (n == 0) return;
    f->order.wait_host();
    f->io.reserve((size_t)n);
    StftOlaArgs o = f->ola_args(f->cfg.hop_size, 1 + (n - 1) / f->cfg.hop_size, f->io.p, n, n, 1);
    o.norm_only = 1;
    launch_stft_ola(o, f->stream);
    AD_HIP(hipGetLastError());
    AD_HIP(hipMemcpyAsync(norm, f->io.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, f->stream));
    AD_HIP(hipStreamSynchronize(f->stream));
  });
}

int ad_specfreeze_process(ad_specfreeze* f, double* buf, int64_t n) { return process_host(f, buf, n, freeze_run, kMaxSamples); }

int ad_specfreeze_process_device(ad_specfreeze* f, double* d_buf, int64_t stride, int64_t n, void* stream) {
  return process_device(f, d_buf, stride, n, stream, freeze_run, kMaxSamples);
}

int ad_specfreeze_reset(ad_specfreeze* f) {
  // Reset :184-189: the captured frame and the phase accumulators; ordered after the last call
  return with_handle(f, [&] {
    f->order.wait_host();
    zero(f->acc, f->stream);
    AD_HIP(hipStreamSynchronize(f->stream));
    f->has_frozen = false;
  });
}

int ad_specfreeze_profile(ad_specfreeze* f, int enable, double* ms) { return profile(f, enable, ms); }

void ad_specfreeze_destroy(ad_specfreeze* f) { destroy_handle(f); }

// ---- ad_pitchspec -----------------------------------------------------------
void ad_pitchspec_default_config(ad_pitchspec_config* cfg, double sample_rate) {
  if (!cfg) return;
  *cfg = ad_pitchspec_config{};
  cfg->sample_rate = sample_rate;  // NewSpectralPitchShifter pitch_shift_spectral.go:71-78
  cfg->pitch_ratio = 1.0;
  cfg->frame_size = 1024;
  cfg->analysis_hop = 256;
  cfg->window_type = 1;       // window.TypeHann
  cfg->resample_quality = 1;  // resample.QualityBalanced
}

int ad_pitchspec_validate(const ad_pitchspec_config* cfg) { return validate_config(cfg, validate); }

int ad_pitchspec_create(const ad_pitchspec_config* cfg, int channels, int device, ad_pitchspec** out) {
  return create_handle(cfg, channels, device, out, validate, [](ad_pitchspec* p, const ad_pitchspec_config& c) {
    pitch_rebuild(p, c.frame_size, c.window);
    pitch_update_hop(p);
    if (c.resample_taps) pitch_install_taps(p, c.resample_taps, c.n_resample_taps);
    p->cfg.window = p->cfg.resample_taps = nullptr;
    p->cfg.n_resample_taps = 0;
  });
}

int ad_pitchspec_set_param(ad_pitchspec* p, int which, double value) {
  return with_handle(p, [&] {
    ad_pitchspec_config c = p->cfg;
    c.window = p->h_win.data();
    switch (which) {
      case AD_PITCHSPEC_SAMPLE_RATE: c.sample_rate = value; break;
      case AD_PITCHSPEC_RATIO: c.pitch_ratio = value; break;
      case AD_PITCHSPEC_HOP:
        c.analysis_hop = whole(value, INT_MIN, INT_MAX, "spectral analysis hop must be a whole number");
        break;
      case AD_PITCHSPEC_RESAMPLE_QUALITY:
        c.resample_quality = whole(value, INT_MIN, INT_MAX, "resample quality must be a whole number");
        break;
      default: AD_FAIL(AD_ERR_INVALID_ARGUMENT, "unknown spectral pitch shifter parameter");
    }
    validate(c);
    c.window = nullptr;
    const bool drop = c.resample_quality != p->cfg.resample_quality || c.analysis_hop != p->cfg.analysis_hop;
    p->order.wait_host();
    p->cfg = c;
    if (drop) {  // the prototype belongs to the reduced hops and the quality's profile
      p->taps.clear();
      p->rs.reset();
    }
    pitch_update_hop(p);
  });
}

int ad_pitchspec_set_frame(ad_pitchspec* p, int frame_size, const double* window) {
  return with_handle(p, [&] {
    check_frame(frame_size, "spectral");
    check_window(window, frame_size, "spectral pitch shifter");
    p->order.wait_host();
    p->cfg.frame_size = frame_size;  // SetFrameSize :180-196
    if (p->cfg.analysis_hop >= frame_size) {
      p->cfg.analysis_hop = std::max(frame_size / 4, 1);
      p->taps.clear();
      p->rs.reset();
    }
    pitch_update_hop(p);
    pitch_rebuild(p, frame_size, window);
  });
}

int ad_pitchspec_set_window(ad_pitchspec* p, int window_type, const double* window) {
  return with_handle(p, [&] {
    check_window(window, p->frame, "spectral pitch shifter");
    p->cfg.window_type = window_type;  // SetWindowType :211-214
    const std::vector<double> w(window, window + p->frame);
    pitch_rebuild(p, p->frame, w.data());
  });
}

int ad_pitchspec_set_resample_taps(ad_pitchspec* p, const double* taps, int64_t n_taps) {
  return with_handle(p, [&] {
    pitch_install_taps(p, taps, n_taps);
  });
}

int ad_pitchspec_get_config(const ad_pitchspec* p, ad_pitchspec_config* cfg) {
  return guard([&] {
    if (!p || !cfg) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "null spectral pitch shifter handle or config");
    *cfg = p->cfg;
    cfg->n_resample_taps = (int64_t)p->taps.size();
  });
}

int ad_pitchspec_effective_ratio(const ad_pitchspec* p, double* ratio) {
  return guard([&] {
    if (!p || !ratio) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "null spectral pitch shifter handle or output");
    const bool bin = std::fabs(p->cfg.pitch_ratio - 1) <= kBinShiftThreshold;
    *ratio = bin ? p->cfg.pitch_ratio : (double)p->synthesis_hop / (double)p->cfg.analysis_hop;
  });
}

int ad_pitchspec_synthesis_hop(const ad_pitchspec* p, int* hop) {
  return guard([&] {
    if (!p || !hop) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "null spectral pitch shifter handle or output");
    const bool bin = std::fabs(p->cfg.pitch_ratio - 1) <= kBinShiftThreshold;
    *hop = bin ? p->cfg.analysis_hop : p->synthesis_hop;
  });
}

int ad_pitchspec_path(const ad_pitchspec* p, int* path) {
  return guard([&] {
    if (!p || !path) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "null spectral pitch shifter handle or output");
    *path = pitch_path(p);
  });
}

int ad_pitchspec_process(ad_pitchspec* p, double* buf, int64_t n) { return process_host(p, buf, n, pitch_run, kMaxSamples); }

int ad_pitchspec_process_device(ad_pitchspec* p, double* d_buf, int64_t stride, int64_t n, void* stream) {
  return process_device(p, d_buf, stride, n, stream, pitch_run, kMaxSamples);
}

int ad_pitchspec_reset(ad_pitchspec* p) {
  // Reset :222-227 clears prevPhase and sumPhase, which every call clears itself: nothing is kept between calls
  return with_handle(p, [&] {
  });
}

int ad_pitchspec_profile(ad_pitchspec* p, int enable, double* ms) { return profile(p, enable, ms); }

void ad_pitchspec_destroy(ad_pitchspec* p) { destroy_handle(p); }

}  // extern "C"
