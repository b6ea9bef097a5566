// C ABI of the N-way crossover (crossover.MultiBand, dsp/filter/crossover/
// crossover.go:113-222) and the multiband compressor (dynamics.
// MultibandCompressor, dsp/effects/dynamics/multiband.go).
//
// ad_xover designs its Linkwitz-Riley sections on the host with the operations
// of pass.LinkwitzRileyLP / HP / HPInverted (pass/linkwitz_riley.go,
// pass/butterworth.go, pass/common.go) in their order, keeps them on the device
// and runs k_xover_walk over them; the sections' states live on the device,
// [channels][stages][2][S][2].
//
// ad_multiband owns an ad_xover and one ad_fx_chain with the compressor stage
// alone per band, as the graph runtime owns chains.  A call splits into the
// planes of a scratch buffer [bands][channels][pitch], runs band b's chain on
// plane b and sums the planes in band order.  Everything of a call is enqueued
// on the caller's stream, band after band: a chain's call ends with its stream
// waiting for all of its work, so the sum follows every band without a join.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <vector>

#include "fx_handle.hpp"
#include "xover_kernels.hpp"

using namespace adsp;

namespace {

constexpr int kMaxOrder = 2 * kXoverMaxSections;              // maxMultibandOrder multiband.go:15
constexpr double kMinCrossoverFrequency = 20.0;               // multiband.go:17
constexpr size_t kScratchBytes = (size_t)2 << 30;             // the band planes of one pass (DESIGN §4i's figure)
constexpr int64_t kMinChunk = 64;

// ---- design ---------------------------------------------------------------
struct Sec {
  double c[5];  // b0, b1, b2, a1, a2
};
const Sec kZero{{0, 0, 0, 0, 0}};

Sec norm(double b0, double b1, double b2, double a0, double a1, double a2) {  // normalizeBiquad design.go:214-223
  if (a0 == 0 || !is_finite(a0)) return kZero;
  return Sec{{b0 / a0, b1 / a0, b2 / a0, a1 / a0, a2 / a0}};
}

Sec rbj(double freq, double q, double fs, bool high) {  // pass.LowpassRBJ / HighpassRBJ butterworth.go:56-123
  if (fs <= 0 || freq <= 0 || freq >= fs / 2) return kZero;
  if (q <= 0) q = 1 / std::sqrt(2.0);
  const double w0 = 2 * M_PI * freq / fs;
  const double cw = std::cos(w0), sw = std::sin(w0);
  const double alpha = sw / (2 * q);
  if (high) return norm((1 + cw) / 2, -(1 + cw), (1 + cw) / 2, 1 + alpha, -2 * cw, 1 - alpha);
  return norm((1 - cw) / 2, 1 - cw, (1 - cw) / 2, 1 + alpha, -2 * cw, 1 - alpha);
}

double butterworth_q(int order, int index) {  // butterworthQ pass/common.go:20-30
  const double theta = M_PI * (double)(2 * index + 1) / (2 * (double)order);
  const double s = std::sin(theta);
  if (s == 0) return 1 / std::sqrt(2.0);
  return 1 / (2 * s);
}

Sec first_order(double freq, double fs, bool high) {  // butterworthFirstOrderLP/HP pass/common.go:34-70
  if (fs <= 0 || freq <= 0 || freq >= fs / 2) return kZero;
  const double k = std::tan(M_PI * freq / fs);
  const double n = 1 / (1 + k);
  if (high) return Sec{{n, -n, 0.0, (k - 1) * n, 0.0}};
  return Sec{{k * n, k * n, 0.0, (k - 1) * n, 0.0}};
}

void butterworth(double freq, int order, double fs, bool high, std::vector<Sec>& out) {  // butterworth.go:12-53
  for (int i = order / 2 - 1; i >= 0; --i) out.push_back(rbj(freq, butterworth_q(order, i), fs, high));
  if (order % 2) out.push_back(first_order(freq, fs, high));
}

// crossover.New :45-52: the halved-order Butterworth prototype twice (linkwitz_riley.go:23-122); for orders
// = 2 mod 4 the first HP section's B coefficients are negated (LinkwitzRileyHPInverted)
void linkwitz_riley(double freq, int order, double fs, std::vector<Sec>& lp, std::vector<Sec>& hp) {
  const int o0 = order / 2, o1 = (order + 1) / 2;
  butterworth(freq, o0, fs, false, lp);
  butterworth(freq, o1, fs, false, lp);
  butterworth(freq, o0, fs, true, hp);
  butterworth(freq, o1, fs, true, hp);
  if (order % 4 == 2)
    for (int k = 0; k < 3; ++k) hp[0].c[k] = -hp[0].c[k];
}

int sections_per_side(int order) { return order / 2 / 2 + (order / 2) % 2 + (order + 1) / 2 / 2 + ((order + 1) / 2) % 2; }

// crossover.go:32-43, 135-144, and the kernel's limits
void validate_xover(const double* freqs, int nfreq, int order, double fs) {
  if (nfreq < 1 || !freqs) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "crossover: at least one frequency is required");
  if (nfreq > kXoverMaxStages) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "crossover: at most 7 frequencies");
  if (order <= 0 || order % 2 != 0) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "crossover: order must be a positive even integer");
  if (order > kMaxOrder) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "crossover: order must be at most 24");
  if (!(fs > 0) || !is_finite(fs)) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "crossover: sample rate must be positive and finite");
  for (int i = 0; i < nfreq; ++i) {
    if (!(freqs[i] > 0 && freqs[i] < fs / 2)) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "crossover: frequency must be in (0, fs/2)");
    if (i > 0 && !(freqs[i] > freqs[i - 1])) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "crossover: frequencies must be strictly ascending");
  }
}

// validateMultibandParams multiband.go:661-709
void validate_multiband(const double* freqs, int nfreq, int order, double fs) {
  if (!(fs > 0) || !is_finite(fs)) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "multiband compressor: sample rate must be positive and finite");
  if (nfreq < 1 || !freqs) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "multiband compressor: at least one crossover frequency is required");
  if (nfreq + 1 > kXoverMaxStages + 1) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "multiband compressor: maximum 8 bands");
  if (order < 2 || order > kMaxOrder) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "multiband compressor: order must be in [2, 24]");
  if (order % 2 != 0) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "multiband compressor: order must be even (Linkwitz-Riley)");
  const double nyquist = fs / 2;
  for (int i = 0; i < nfreq; ++i) {
    const double f = freqs[i];
    if (!is_finite(f)) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "multiband compressor: crossover frequency must be finite");
    if (f < kMinCrossoverFrequency) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "multiband compressor: crossover frequency must be >= 20 Hz");
    if (f >= nyquist) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "multiband compressor: crossover frequency must be < Nyquist");
    if (i > 0 && f <= freqs[i - 1])
      AD_FAIL(AD_ERR_INVALID_ARGUMENT, "multiband compressor: crossover frequencies must be strictly ascending");
  }
}

// [nfreq][2][S][5]
std::vector<double> design_table(const double* freqs, int nfreq, int order, double fs, int* S) {
  const int s = sections_per_side(order);
  std::vector<double> tab;
  tab.reserve((size_t)nfreq * 2 * s * 5);
  for (int i = 0; i < nfreq; ++i) {
    std::vector<Sec> lp, hp;
    linkwitz_riley(freqs[i], order, fs, lp, hp);
    if ((int)lp.size() != s || (int)hp.size() != s) AD_FAIL(AD_ERR_INTERNAL, "crossover: section count");
    for (const auto* side : {&lp, &hp})
      for (const Sec& sec : *side) tab.insert(tab.end(), sec.c, sec.c + 5);
  }
  *S = s;
  return tab;
}

void check_rc(int rc) {
  if (rc != AD_OK) AD_FAIL(rc, ad_last_error());
}

}  // namespace

struct ad_xover {
  int device = 0, channels = 0, stages = 0, sections = 0, order = 0;
  double sample_rate = 0;
  bool pipelined = true;
  std::vector<double> table;     // [stages][2][S][5]
  DevBuf<double> coef, state;    // the table; [channels][stages][2][S][2]
  DevBuf<double> io_in, io_out;  // host-buffer calls
  hipStream_t stream = nullptr;  // host-buffer calls, resets, state access
  StreamOrder calls;             // calls may come on any stream
  size_t per_channel() const { return (size_t)stages * 2 * sections * 2; }
  ~ad_xover() {
    calls.release();
    if (stream) {
      (void)hipStreamSynchronize(stream);
      (void)lib_stream_destroy(stream);
    }
  }
};

struct ad_multiband {
  int device = 0, channels = 0, bands = 0;
  double sample_rate = 0;
  ad_xover* xover = nullptr;
  std::vector<ad_fx_chain*> chains;
  std::vector<ad_compressor_config> cfg;
  DevBuf<double> scratch;  // [bands][channels][pitch] of one pass
  DevBuf<double> io, io_bands;
  int64_t chunk = 0;  // ad_multiband_set_chunk; 0: what the scratch cap allows
  hipStream_t stream = nullptr;
  StreamOrder calls;  // calls may come on any stream
  ~ad_multiband() {
    calls.release();
    if (stream) {
      (void)hipStreamSynchronize(stream);
      (void)lib_stream_destroy(stream);
    }
    for (ad_fx_chain* c : chains) ad_fx_chain_destroy(c);
    ad_xover_destroy(xover);
  }
};

namespace {

// the walk over n samples, without the handle's call ordering (the multiband handle orders its own calls)
void xover_launch(ad_xover* h, const double* d_in, int64_t in_stride, double* d_bands, int64_t row_stride,
                  int64_t band_stride, int64_t n, hipStream_t s) {
  XoverWalkArgs a{};
  a.in = d_in;
  a.in_stride = in_stride;
  a.bands = d_bands;
  a.row_stride = row_stride;
  a.band_stride = band_stride;
  a.n = n;
  a.coef = h->coef.p;
  a.state = h->state.p;
  a.stages = h->stages;
  a.sections = h->sections;
  a.channels = h->channels;
  if (h->pipelined) {
    a.stage_begin = 0;
    a.stage_end = h->stages;
    launch_xover_walk(a, s);
  } else {
    for (int i = 0; i < h->stages; ++i) {
      a.stage_begin = i;
      a.stage_end = i + 1;
      launch_xover_walk(a, s);
    }
  }
  AD_HIP(hipGetLastError());
}

void check_bands(const ad_xover* h, const void* d_in, int64_t in_stride, const void* d_bands, int64_t row_stride,
                 int64_t band_stride, int64_t n) {
  if (n < 0) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "bad buffer geometry");
  if (n == 0) return;
  if (!d_in || !d_bands || in_stride < n || row_stride < n || band_stride < (int64_t)(h->channels - 1) * row_stride + n)
    AD_FAIL(AD_ERR_INVALID_ARGUMENT, "bad buffer geometry");
}

void xover_run(ad_xover* h, const double* d_in, int64_t in_stride, double* d_bands, int64_t row_stride,
               int64_t band_stride, int64_t n, hipStream_t s) {
  CallScope call(h->calls, s);
  xover_launch(h, d_in, in_stride, d_bands, row_stride, band_stride, n, s);
}

void xover_reset(ad_xover* h) {
  h->calls.wait_host();
  AD_HIP(hipMemsetAsync(h->state.p, 0, h->state.n * sizeof(double), h->stream));
  AD_HIP(hipStreamSynchronize(h->stream));
}

void xover_get_state(ad_xover* h, int channel, double* state, int64_t cap) {
  check_channel(h, channel);
  const size_t per = h->per_channel();
  if (cap < (int64_t)per) AD_FAIL(AD_ERR_LENGTH_MISMATCH, "state buffer too small");
  if (!state) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "null state buffer");
  h->calls.wait_host();
  AD_HIP(hipMemcpy(state, h->state.p + channel * per, per * sizeof(double), hipMemcpyDeviceToHost));
}

ad_xover* xover_new(const double* freqs, int nfreq, int order, double fs, int channels, int device) {
  if (channels <= 0) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "channels must be positive");
  validate_xover(freqs, nfreq, order, fs);
  const int dev = pick_device(device);
  DeviceScope ds(dev);
  std::unique_ptr<ad_xover> h(new ad_xover());
  h->device = dev;
  h->channels = channels;
  h->stages = nfreq;
  h->order = order;
  h->sample_rate = fs;
  h->table = design_table(freqs, nfreq, order, fs, &h->sections);
  AD_HIP(lib_stream_create(&h->stream));
  h->coef.alloc(h->table.size());
  AD_HIP(hipMemcpy(h->coef.p, h->table.data(), h->table.size() * sizeof(double), hipMemcpyHostToDevice));
  h->state.alloc((size_t)channels * h->per_channel());
  AD_HIP(hipMemset(h->state.p, 0, h->state.n * sizeof(double)));
  return h.release();
}

// samples of a call one pass takes
int64_t multiband_chunk(const ad_multiband* f, int64_t n) {
  if (f->chunk > 0) return std::min(n, f->chunk);
  const int64_t fit = (int64_t)(kScratchBytes / ((size_t)f->bands * f->channels * sizeof(double)));
  return std::min(n, std::max(fit, kMinChunk));
}

void run_bands(ad_multiband* f, double* planes, int64_t row_stride, int64_t band_stride, int64_t m, hipStream_t s) {
  for (int b = 0; b < f->bands; ++b)
    check_rc(ad_fx_chain_process_device(f->chains[b], planes + (int64_t)b * band_stride, row_stride, m, s));
}

// ProcessInPlace multiband.go:468-489
void multiband_run(ad_multiband* f, double* d_buf, int64_t stride, int64_t n, hipStream_t s) {
  CallScope call(f->calls, s);
  const int64_t seg = multiband_chunk(f, n);
  const int64_t pitch = (seg + 1) & ~(int64_t)1;  // even: every plane row keeps the 16-byte phase
  f->scratch.reserve((size_t)f->bands * f->channels * pitch);  // hipFree waits for the device: no earlier call still uses the old one
  const int64_t band_stride = (int64_t)f->channels * pitch;
  for (int64_t off = 0; off < n; off += seg) {
    const int64_t m = std::min(seg, n - off);
    xover_launch(f->xover, d_buf + off, stride, f->scratch.p, pitch, band_stride, m, s);
    run_bands(f, f->scratch.p, pitch, band_stride, m, s);
    BandSumArgs a{};
    a.dst = d_buf + off;
    a.dst_stride = stride;
    a.bands = f->scratch.p;
    a.row_stride = pitch;
    a.band_stride = band_stride;
    a.n = m;
    a.nbands = f->bands;
    a.channels = f->channels;
    launch_band_sum(a, s);
    AD_HIP(hipGetLastError());
  }
}

// ProcessInPlaceMulti multiband.go:507-523: the bands go straight to the caller's planes
void multiband_run_multi(ad_multiband* f, const double* d_in, int64_t in_stride, double* d_bands, int64_t row_stride,
                         int64_t band_stride, int64_t n, hipStream_t s) {
  CallScope call(f->calls, s);
  const int64_t seg = multiband_chunk(f, n);
  for (int64_t off = 0; off < n; off += seg) {
    const int64_t m = std::min(seg, n - off);
    xover_launch(f->xover, d_in + off, in_stride, d_bands + off, row_stride, band_stride, m, s);
    run_bands(f, d_bands + off, row_stride, band_stride, m, s);
  }
}

template <class H>
void check_handle(const H* h) {
  if (!h) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "null handle");
}

void check_band(const ad_multiband* f, int band) {  // checkBand multiband.go:555-561
  check_handle(f);
  if (band < 0 || band >= f->bands) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "multiband compressor: band index out of range");
}

}  // namespace

extern "C" {

// ---- ad_xover ---------------------------------------------------------------
int ad_xover_validate(const double* freqs, int nfreq, int order, double sample_rate) {
  return guard([&] { validate_xover(freqs, nfreq, order, sample_rate); });
}

int ad_xover_sections(const double* freqs, int nfreq, int order, double sample_rate, double* sections, int64_t cap,
                      int* sections_per_side_out) {
  return guard([&] {
    validate_xover(freqs, nfreq, order, sample_rate);
    int s = 0;
    const std::vector<double> tab = design_table(freqs, nfreq, order, sample_rate, &s);
    if (sections_per_side_out) *sections_per_side_out = s;
    if (sections) {
      if (cap < (int64_t)tab.size()) AD_FAIL(AD_ERR_LENGTH_MISMATCH, "section buffer too small");
      std::memcpy(sections, tab.data(), tab.size() * sizeof(double));
    }
  });
}

int ad_xover_create(const double* freqs, int nfreq, int order, double sample_rate, int channels, int device,
                    ad_xover** out) {
  if (out) *out = nullptr;
  ad_xover* raw = nullptr;
  const int rc = guard([&] {
    if (!out) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "null output handle");
    raw = xover_new(freqs, nfreq, order, sample_rate, channels, device);
  });
  if (rc == AD_OK && out) *out = raw;
  return rc;
}

int ad_xover_process(ad_xover* h, const double* in, double* bands, int64_t n) {
  return guard([&] {
    check_handle(h);
    if (n < 0 || (n > 0 && (!in || !bands))) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "bad buffer");
    if (n == 0) return;
    DeviceScope ds(h->device);
    const size_t count = (size_t)h->channels * n;
    h->io_in.reserve(count);
    h->io_out.reserve(count * (h->stages + 1));
    AD_HIP(hipMemcpyAsync(h->io_in.p, in, count * sizeof(double), hipMemcpyHostToDevice, h->stream));
    xover_run(h, h->io_in.p, n, h->io_out.p, n, (int64_t)count, n, h->stream);
    AD_HIP(hipMemcpyAsync(bands, h->io_out.p, count * (h->stages + 1) * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    AD_HIP(hipStreamSynchronize(h->stream));
  });
}

int ad_xover_process_device(ad_xover* h, const double* d_in, int64_t in_stride, double* d_bands, int64_t row_stride,
                            int64_t band_stride, int64_t n, void* stream) {
  return guard([&] {
    check_handle(h);
    check_bands(h, d_in, in_stride, d_bands, row_stride, band_stride, n);
    if (n == 0) return;
    DeviceScope ds(h->device);
    xover_run(h, d_in, in_stride, d_bands, row_stride, band_stride, n, reinterpret_cast<hipStream_t>(stream));
  });
}

int ad_xover_get_state(ad_xover* h, int channel, double* state, int64_t cap) {
  return guard([&] {
    check_handle(h);
    DeviceScope ds(h->device);
    xover_get_state(h, channel, state, cap);
  });
}

int ad_xover_set_state(ad_xover* h, int channel, const double* state, int64_t n) {
  return guard([&] {
    check_channel(h, channel);
    const size_t per = h->per_channel();
    if (n < (int64_t)per) AD_FAIL(AD_ERR_LENGTH_MISMATCH, "state too short");
    if (!state) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "null state");
    DeviceScope ds(h->device);
    h->calls.wait_host();
    AD_HIP(hipMemcpy(h->state.p + channel * per, state, per * sizeof(double), hipMemcpyHostToDevice));
  });
}

int ad_xover_reset(ad_xover* h) {
  // MultiBand.Reset :218-222; ordered after the last call
  return guard([&] {
    check_handle(h);
    DeviceScope ds(h->device);
    xover_reset(h);
  });
}

int ad_xover_kernel_info(const ad_xover* h, int* waves_per_workgroup, int* tile, int* lds_bytes) {
  return guard([&] {
    check_handle(h);
    if (waves_per_workgroup) *waves_per_workgroup = h->pipelined ? h->stages : 1;
    if (tile) *tile = kXoverTile;
    if (lds_bytes) *lds_bytes = xover_lds_bytes(h->pipelined ? h->stages : 1);
  });
}

int ad_xover_set_pipelined(ad_xover* h, int on) {
  return guard([&] {
    check_handle(h);
    if (on != 0 && on != 1) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "pipelined must be 0 or 1");
    h->pipelined = on != 0;
  });
}

void ad_xover_destroy(ad_xover* h) {
  if (!h) return;
  (void)guard([&] {
    DeviceScope ds(h->device);
    delete h;
  });
}

// ---- ad_multiband -----------------------------------------------------------
int ad_multiband_validate(const double* freqs, int nfreq, int order, double sample_rate) {
  return guard([&] { validate_multiband(freqs, nfreq, order, sample_rate); });
}

int ad_multiband_create(const double* freqs, int nfreq, int order, double sample_rate, int channels, int device,
                        ad_multiband** out) {
  if (out) *out = nullptr;
  ad_multiband* raw = nullptr;
  const int rc = guard([&] {
    if (!out) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "null output handle");
    if (channels <= 0) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "channels must be positive");
    validate_multiband(freqs, nfreq, order, sample_rate);
    const int dev = pick_device(device);
    DeviceScope ds(dev);
    std::unique_ptr<ad_multiband> f(new ad_multiband());
    f->device = dev;
    f->channels = channels;
    f->bands = nfreq + 1;
    f->sample_rate = sample_rate;
    f->xover = xover_new(freqs, nfreq, order, sample_rate, channels, dev);
    AD_HIP(lib_stream_create(&f->stream));
    for (int b = 0; b < f->bands; ++b) {  // NewCompressor(sampleRate) per band :105-113
      ad_fx_chain* c = nullptr;
      check_rc(ad_fx_chain_create(channels, dev, &c));
      f->chains.push_back(c);
      ad_compressor_config cfg;
      ad_compressor_default_config(&cfg, sample_rate);
      check_rc(ad_fx_chain_set_compressor(c, &cfg));
      f->cfg.push_back(cfg);
    }
    raw = f.release();
  });
  if (rc == AD_OK && out) *out = raw;
  return rc;
}

int ad_multiband_set_band(ad_multiband* f, int band, const ad_compressor_config* cfg) {
  return guard([&] {
    check_band(f, band);
    if (!cfg) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "null compressor config");
    check_rc(ad_compressor_validate(cfg));
    if (cfg->sample_rate != f->sample_rate)
      AD_FAIL(AD_ERR_INVALID_ARGUMENT, "multiband compressor: a band runs at the handle's sample rate");
    DeviceScope ds(f->device);
    f->calls.wait_host();
    check_rc(ad_fx_chain_set_compressor(f->chains[band], cfg));
    f->cfg[band] = *cfg;
  });
}

int ad_multiband_get_band(const ad_multiband* f, int band, ad_compressor_config* cfg) {
  return guard([&] {
    check_band(f, band);
    if (!cfg) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "null compressor config");
    *cfg = f->cfg[band];
  });
}

int ad_multiband_process(ad_multiband* f, double* buf, int64_t n) {
  return guard([&] {
    check_handle(f);
    if (n < 0 || (n > 0 && !buf)) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "bad buffer");
    if (n == 0) return;  // :469-471
    DeviceScope ds(f->device);
    const size_t count = (size_t)f->channels * n;
    f->io.reserve(count);
    AD_HIP(hipMemcpyAsync(f->io.p, buf, count * sizeof(double), hipMemcpyHostToDevice, f->stream));
    multiband_run(f, f->io.p, n, n, f->stream);
    AD_HIP(hipMemcpyAsync(buf, f->io.p, count * sizeof(double), hipMemcpyDeviceToHost, f->stream));
    AD_HIP(hipStreamSynchronize(f->stream));
  });
}

int ad_multiband_process_device(ad_multiband* f, double* d_buf, int64_t stride, int64_t n, void* stream) {
  return guard([&] {
    check_handle(f);
    if (n < 0 || (n > 0 && (!d_buf || stride < n))) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "bad buffer geometry");
    if (n == 0) return;
    DeviceScope ds(f->device);
    multiband_run(f, d_buf, stride, n, reinterpret_cast<hipStream_t>(stream));
  });
}

int ad_multiband_process_multi(ad_multiband* f, const double* in, double* bands, int64_t n) {
  return guard([&] {
    check_handle(f);
    if (n < 0 || (n > 0 && (!in || !bands))) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "bad buffer");
    if (n == 0) return;  // :508-515
    DeviceScope ds(f->device);
    const size_t count = (size_t)f->channels * n;
    f->io.reserve(count);
    f->io_bands.reserve(count * f->bands);
    AD_HIP(hipMemcpyAsync(f->io.p, in, count * sizeof(double), hipMemcpyHostToDevice, f->stream));
    multiband_run_multi(f, f->io.p, n, f->io_bands.p, n, (int64_t)count, n, f->stream);
    AD_HIP(hipMemcpyAsync(bands, f->io_bands.p, count * f->bands * sizeof(double), hipMemcpyDeviceToHost, f->stream));
    AD_HIP(hipStreamSynchronize(f->stream));
  });
}

int ad_multiband_process_multi_device(ad_multiband* f, const double* d_in, int64_t in_stride, double* d_bands,
                                      int64_t row_stride, int64_t band_stride, int64_t n, void* stream) {
  return guard([&] {
    check_handle(f);
    check_bands(f->xover, d_in, in_stride, d_bands, row_stride, band_stride, n);
    if (n == 0) return;
    DeviceScope ds(f->device);
    multiband_run_multi(f, d_in, in_stride, d_bands, row_stride, band_stride, n, reinterpret_cast<hipStream_t>(stream));
  });
}

int ad_multiband_metrics(ad_multiband* f, int band, int channel, double* input_peak, double* output_peak,
                         double* gain_reduction) {
  return guard([&] {
    check_band(f, band);
    DeviceScope ds(f->device);
    f->calls.wait_host();
    check_rc(ad_fx_chain_compressor_metrics(f->chains[band], channel, input_peak, output_peak, gain_reduction));
  });
}

int ad_multiband_reset_metrics(ad_multiband* f) {
  // ResetMetrics :547-551
  return guard([&] {
    check_handle(f);
    DeviceScope ds(f->device);
    f->calls.wait_host();
    for (ad_fx_chain* c : f->chains) check_rc(ad_fx_chain_reset_compressor_metrics(c));
  });
}

int ad_multiband_reset(ad_multiband* f) {
  // Reset :528-534: the crossover and every compressor; ordered after the last call
  return guard([&] {
    check_handle(f);
    DeviceScope ds(f->device);
    f->calls.wait_host();
    xover_reset(f->xover);
    for (ad_fx_chain* c : f->chains) check_rc(ad_fx_chain_reset(c));
  });
}

int ad_multiband_xover_state(ad_multiband* f, int channel, double* state, int64_t cap) {
  return guard([&] {
    check_handle(f);
    DeviceScope ds(f->device);
    f->calls.wait_host();
    xover_get_state(f->xover, channel, state, cap);
  });
}

int ad_multiband_set_chunk(ad_multiband* f, int64_t samples) {
  return guard([&] {
    check_handle(f);
    if (samples < 0) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "chunk must be 0 (automatic) or positive");
    f->chunk = samples;
  });
}

void ad_multiband_destroy(ad_multiband* f) {
  if (!f) return;
  (void)guard([&] {
    DeviceScope ds(f->device);
    delete f;
  });
}

}  // extern "C"
