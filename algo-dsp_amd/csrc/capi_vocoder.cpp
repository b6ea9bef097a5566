// C ABI of the vocoder (dsp/effects/vocoder.go).  A handle keeps the
// reference's configuration on the host and derives what the reference caches
// (band tables, Q values, every section, the downsample factors and groups,
// the envelope coefficients) there with the C library's cos, sin and exp, in
// the reference's operation order; they go to the device as tables, and the
// device computes no transcendental.  The sections' states and the envelopes
// live on the device, one set per channel.  downsampleCount is one integer on
// the host: every channel advances by the same n, and calls are ordered.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <vector>

#include "fx_handle.hpp"
#include "vocoder_kernels.hpp"

using namespace adsp;

static_assert(AD_VOCODER_MAX_BANDS == kVocBands, "a band per lane of a half wave");

namespace {

constexpr double kThirdOctaveFreqs[32] = {16,  20,  25,  31,   40,   50,   63,   80,   100,  125,  160,
                                          200, 250, 315, 400,  500,  630,  800,  1000, 1250, 1600, 2000,
                                          2500, 3150, 4000, 5000, 6300, 8000, 10000, 12500, 16000, 20000};  // :27-31
constexpr double kBarkFreqs[24] = {100,  200,  300,  400,  510,  630,  770,  920,  1080, 1270, 1480,  1720,
                                   2000, 2320, 2700, 3150, 3700, 4400, 5300, 6400, 7700, 9500, 12000, 15500};  // :33-36
constexpr double kThirdOctaveQ = 4.3184727050832485;  // :39

struct Layout {
  const double* freqs;
  int count;
};
Layout layout_of(int layout) { return layout == 1 ? Layout{kBarkFreqs, 24} : Layout{kThirdOctaveFreqs, 32}; }

int usable_bands(const ad_vocoder_config& c) {  // :309-318, :351-359
  const Layout l = layout_of(c.layout);
  const double nyquist = c.sample_rate / 2;
  int n = 0;
  for (int i = 0; i < l.count; ++i)
    if (l.freqs[i] < nyquist * 0.9) ++n;
  return n;
}

void validate(const ad_vocoder_config& c) {
  if (!(c.sample_rate > 0) || !is_finite(c.sample_rate)) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "vocoder: sample rate must be > 0");
  if (!flag(c.layout)) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "vocoder: invalid band layout");
  if (!in_range(c.synth_q, 0.1, 20)) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "vocoder: synthesis Q must be in [0.1, 20]");
  if (!in_range(c.attack_ms, 0.01, 100)) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "vocoder: attack must be in [0.01, 100] ms");
  if (!in_range(c.release_ms, 0.01, 1000)) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "vocoder: release must be in [0.01, 1000] ms");
  if (!in_range(c.input_level, 0, 10)) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "vocoder: input level must be in [0, 10]");
  if (!in_range(c.synth_level, 0, 10)) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "vocoder: synth level must be in [0, 10]");
  if (!in_range(c.vocoder_level, 0, 10)) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "vocoder: vocoder level must be in [0, 10]");
  if (!flag(c.synth_q_set)) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "vocoder: synth_q_set must be 0 or 1");
  if (!flag(c.downsample)) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "vocoder: downsample must be 0 or 1");
  if (usable_bands(c) == 0)
    AD_FAIL(AD_ERR_INVALID_ARGUMENT, c.layout == 1 ? "vocoder: no usable Bark bands at this sample rate"
                                                   : "vocoder: no usable bands at this sample rate");
}

// cpgBandpass :527-547 -> {b0, b1, b2, a1, a2}; false where it returns the zero value
bool cpg_bandpass(double freq, double q, double fs, double* sec) {
  for (int i = 0; i < 5; ++i) sec[i] = 0;
  const double w0 = 2 * M_PI * freq / fs;
  if (w0 <= 0 || w0 >= M_PI) return false;
  const double cw = std::cos(w0), sw = std::sin(w0);
  const double alpha = sw / (2 * q);
  const double a0 = 1 + alpha;
  const double inv = 1.0 / a0;
  sec[0] = alpha * inv;
  sec[1] = 0;
  sec[2] = -alpha * inv;
  sec[3] = -2 * cw * inv;
  sec[4] = (1 - alpha) * inv;
  return true;
}

// antiAliasDecimatorLowpass :493-521
void anti_alias(double fs, int factor, double* sec) {
  sec[0] = 1, sec[1] = sec[2] = sec[3] = sec[4] = 0;
  if (factor <= 1) return;
  const double cutoff = 0.35 * fs / (double)factor;
  if (cutoff <= 0 || cutoff >= 0.5 * fs) return;
  const double w0 = 2 * M_PI * cutoff / fs;
  const double cw = std::cos(w0), sw = std::sin(w0);
  const double q = 0.7071067811865476;
  const double alpha = sw / (2 * q);
  const double a0 = 1 + alpha;
  const double inv = 1.0 / a0;
  sec[0] = ((1 - cw) * 0.5) * inv;
  sec[1] = (1 - cw) * inv;
  sec[2] = ((1 - cw) * 0.5) * inv;
  sec[3] = (-2 * cw) * inv;
  sec[4] = (1 - alpha) * inv;
}

double bark_band_q(int i) {  // :550-572
  const double lower = i == 0 ? kBarkFreqs[0] * 0.5 : (kBarkFreqs[i - 1] + kBarkFreqs[i]) / 2;
  const double upper = i >= 23 ? kBarkFreqs[i] * 1.25 : (kBarkFreqs[i] + kBarkFreqs[i + 1]) / 2;
  const double bw = upper - lower;
  if (bw <= 0) return kThirdOctaveQ;
  return kBarkFreqs[i] / bw;
}

ad_vocoder_tables derive(const ad_vocoder_config& c) {
  ad_vocoder_tables t{};
  const Layout l = layout_of(c.layout);
  const double fs = c.sample_rate;
  const int n = usable_bands(c);
  t.num_bands = n;
  // computeEnvelopeCoeffs :282-295 (attack and release are positive by validation)
  t.attack_coeff = 1.0 - std::exp(-1.0 / (c.attack_ms * 0.001 * fs));
  t.release_coeff = std::exp(-1.0 / (c.release_ms * 0.001 * fs));
  double analysis_q[kVocBands];
  for (int i = 0; i < n; ++i) {  // buildThirdOctaveBanks :330-341, buildBarkBanks :371-388
    const double q = c.layout == 1 ? bark_band_q(i) : kThirdOctaveQ;
    analysis_q[i] = q;
    const double sq = (c.layout == 1 && !c.synth_q_set) ? q : c.synth_q;
    cpg_bandpass(l.freqs[i], q, fs, t.analysis[i]);
    cpg_bandpass(l.freqs[i], sq, fs, t.synthesis[i]);
  }
  if (!c.downsample) return t;
  // computeDownsampleFactors :401-438
  int max_factor = 1;
  const double threshold = 0.1 * fs;
  for (int i = 0; i < n; ++i) {
    int factor = 1;
    while ((double)(2 * (factor << 1)) * l.freqs[i] < threshold) factor <<= 1;
    t.factors[i] = factor;
    max_factor = std::max(max_factor, factor);
  }
  // buildDownsampleGroups :440-468: the distinct factors ascending
  std::vector<int> factors(t.factors, t.factors + n);
  std::sort(factors.begin(), factors.end());
  factors.erase(std::unique(factors.begin(), factors.end()), factors.end());
  t.num_groups = (int)factors.size();
  for (int g = 0; g < t.num_groups; ++g) {
    t.group_factors[g] = factors[g];
    anti_alias(fs, factors[g], t.antialias[g]);
  }
  for (int i = 0; i < n; ++i)
    t.group_of_band[i] = (int)(std::find(factors.begin(), factors.end(), t.factors[i]) - factors.begin());
  for (int i = 0; i < n; ++i) {
    const double ds_rate = fs / (double)t.factors[i];
    if (!cpg_bandpass(l.freqs[i], analysis_q[i], ds_rate, t.decimated[i]))
      cpg_bandpass(l.freqs[i], analysis_q[i], fs, t.decimated[i]);  // :427-430
    const double scale = (double)t.factors[i];                     // computeDownsampleEnvelopeCoeffs :470-489
    t.ds_attack[i] = 1.0 - std::exp(-scale / (c.attack_ms * 0.001 * fs));
    t.ds_release[i] = std::exp(-scale / (c.release_ms * 0.001 * fs));
  }
  t.downsample_max = max_factor;
  return t;
}

}  // namespace

struct ad_vocoder : HandleCore {
  ad_vocoder_config cfg{};
  ad_vocoder_tables t{};
  int counter = 0;               // downsampleCount
  DevBuf<double> state;          // [channels][VOC_STATE_ROWS][kVocBands]
  DevBuf<double> tab;            // [VOC_TAB_ROWS][kVocBands]
  DevBuf<int> itab;              // [VOC_INT_ROWS][kVocBands]
};

namespace {

// The tables by band, after the last call that may still read the old ones.
void upload(ad_vocoder* f) {
  std::vector<double> tab((size_t)VOC_TAB_ROWS * kVocBands, 0.0);
  std::vector<int> itab((size_t)VOC_INT_ROWS * kVocBands, 0);
  const ad_vocoder_tables& t = f->t;
  std::vector<bool> seen(kVocBands, false);
  for (int b = 0; b < t.num_bands; ++b) {
    const int g = t.group_of_band[b];
    for (int k = 0; k < 5; ++k) {
      tab[(VOC_ANALYSIS + k) * kVocBands + b] = t.analysis[b][k];
      tab[(VOC_SYNTHESIS + k) * kVocBands + b] = t.synthesis[b][k];
      tab[(VOC_DECIMATED + k) * kVocBands + b] = t.decimated[b][k];
      tab[(VOC_ANTIALIAS + k) * kVocBands + b] = t.num_groups ? t.antialias[g][k] : 0.0;
    }
    tab[VOC_DS_ATTACK * kVocBands + b] = t.ds_attack[b];
    tab[VOC_DS_RELEASE * kVocBands + b] = t.ds_release[b];
    itab[VOC_MASK * kVocBands + b] = t.num_groups ? t.group_factors[g] - 1 : 0;
    itab[VOC_GROUP * kVocBands + b] = g;
    itab[VOC_FIRST * kVocBands + b] = seen[g] ? 0 : 1;
    seen[g] = true;
  }
  f->order.wait_host();
  AD_HIP(hipMemcpy(f->tab.p, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice));
  AD_HIP(hipMemcpy(f->itab.p, itab.data(), itab.size() * sizeof(int), hipMemcpyHostToDevice));
}

// Zeroes `rows` state rows from `row` on in every channel, after the last call.
void clear_rows(ad_vocoder* f, int row, int rows) {
  f->order.wait_host();
  AD_HIP(hipMemset2DAsync(f->state.p + (size_t)row * kVocBands, (size_t)VOC_STATE_ROWS * kVocBands * sizeof(double), 0,
                          (size_t)rows * kVocBands * sizeof(double), (size_t)f->channels, f->stream));
  AD_HIP(hipStreamSynchronize(f->stream));
}

bool overlap(const double* a, int64_t a_stride, const double* b, int64_t b_stride, int channels, int64_t n) {
  const double* a_end = a + (int64_t)(channels - 1) * a_stride + n;
  const double* b_end = b + (int64_t)(channels - 1) * b_stride + n;
  return a < b_end && b < a_end;
}

void run(ad_vocoder* f, const double* mod, int64_t ms, const double* car, int64_t cs, double* out, int64_t os, int64_t n,
         hipStream_t s) {
  CallScope call(f->order, s);
  VocArgs a{};
  a.mod = mod, a.car = car, a.out = out;
  a.mod_stride = ms, a.car_stride = cs, a.out_stride = os, a.n = n;
  a.state = f->state.p;
  a.tab = f->tab.p;
  a.itab = f->itab.p;
  a.attack = f->t.attack_coeff, a.release = f->t.release_coeff;
  a.vocoder_level = f->cfg.vocoder_level, a.synth_level = f->cfg.synth_level, a.input_level = f->cfg.input_level;
  a.num_bands = f->t.num_bands;
  a.channels = f->channels;
  const bool ds = f->cfg.downsample && f->t.num_groups > 0;  // :581
  a.cnt0 = ds ? f->counter : 0;
  a.cnt_mask = ds ? f->t.downsample_max - 1 : 0;
  launch_vocoder(a, ds, s);
  AD_HIP(hipGetLastError());
  if (ds) f->counter = (int)((f->counter + n) & (int64_t)(f->t.downsample_max - 1));  // :608-611, downsampleMax = 2^k
}

}  // namespace

extern "C" {

void ad_vocoder_default_config(ad_vocoder_config* cfg, double sample_rate) {
  if (!cfg) return;
  *cfg = ad_vocoder_config{};
  cfg->sample_rate = sample_rate;  // defaultVocoderConfig :74-84
  cfg->synth_q = kThirdOctaveQ;
  cfg->attack_ms = 0.5;
  cfg->release_ms = 2.0;
  cfg->input_level = 0.0;
  cfg->synth_level = 0.0;
  cfg->vocoder_level = 1.0;
}

int ad_vocoder_validate(const ad_vocoder_config* cfg) { return validate_config(cfg, validate); }

int ad_vocoder_derived(const ad_vocoder_config* cfg, ad_vocoder_tables* out) {
  return guard([&] {
    if (!cfg || !out) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "null vocoder config or tables");
    validate(*cfg);
    *out = derive(*cfg);
  });
}

int ad_vocoder_create(const ad_vocoder_config* cfg, int channels, int device, ad_vocoder** out) {
  return create_handle(cfg, channels, device, out, validate, [](ad_vocoder* f, const ad_vocoder_config& c) {
    f->t = derive(c);
    f->state.alloc((size_t)f->channels * VOC_STATE_ROWS * kVocBands);
    f->tab.alloc((size_t)VOC_TAB_ROWS * kVocBands);
    f->itab.alloc((size_t)VOC_INT_ROWS * kVocBands);
    zero(f->state, f->stream);
    AD_HIP(hipStreamSynchronize(f->stream));
    upload(f);
  });
}

int ad_vocoder_set_param(ad_vocoder* f, int which, double value) {
  return with_handle(f, [&] {
    ad_vocoder_config c = f->cfg;
    switch (which) {
      case AD_VOCODER_SAMPLE_RATE: c.sample_rate = value; break;      // SetSampleRate :673-683
      case AD_VOCODER_ATTACK: c.attack_ms = value; break;             // SetAttack :772-783
      case AD_VOCODER_RELEASE: c.release_ms = value; break;           // SetRelease :786-797
      case AD_VOCODER_INPUT_LEVEL: c.input_level = value; break;      // SetInputLevel :800-809
      case AD_VOCODER_SYNTH_LEVEL: c.synth_level = value; break;      // SetSynthLevel :812-821
      case AD_VOCODER_VOCODER_LEVEL: c.vocoder_level = value; break;  // SetVocoderLevel :824-833
      case AD_VOCODER_DOWNSAMPLING:                                   // SetDownsampling :737-769
        if (value != 0 && value != 1) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "vocoder: downsampling must be 0 or 1");
        c.downsample = (int)value;
        break;
      default: AD_FAIL(AD_ERR_INVALID_ARGUMENT, "unknown vocoder parameter");
    }
    validate(c);  // every other field is valid already: the setter's own check
    if (which >= AD_VOCODER_INPUT_LEVEL && which <= AD_VOCODER_VOCODER_LEVEL) {
      f->cfg = c;  // the next call's arguments
      return;
    }
    const ad_vocoder_tables t = derive(c);
    if (which == AD_VOCODER_SAMPLE_RATE) {
      // v.envelopes = nil and buildFilterBanks: new sections everywhere.  The decimation sections and the
      // counter are rebuilt here only with downsampling on, but with it off they hold nothing a call reads
      // before SetDownsampling(true) rebuilds them, and the counter is 0 already.
      clear_rows(f, 0, VOC_STATE_ROWS);
      f->counter = 0;
    } else if (which == AD_VOCODER_DOWNSAMPLING) {
      if (c.downsample) {  // computeDownsampleFactors: new decimated analysis and anti-alias sections
        clear_rows(f, VOC_S_DECIMATED, 2);
        clear_rows(f, VOC_S_ANTIALIAS, 2);
      }
      f->counter = 0;
    }
    f->cfg = c;
    f->t = t;
    upload(f);
  });
}

int ad_vocoder_get_config(const ad_vocoder* f, ad_vocoder_config* cfg) {
  return guard([&] {
    if (!f || !cfg) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "null vocoder handle or config");
    *cfg = f->cfg;
  });
}

int ad_vocoder_num_bands(const ad_vocoder* f, int* num_bands) {
  return guard([&] {
    if (!f || !num_bands) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "null vocoder handle or output");
    *num_bands = f->t.num_bands;
  });
}

int ad_vocoder_downsample_factors(const ad_vocoder* f, int* factors, int cap, int* count) {
  return guard([&] {
    if (!f || !count) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "null vocoder handle or count");
    *count = f->cfg.downsample ? f->t.num_bands : 0;
    if (*count == 0) return;
    if (!factors || cap < *count) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "vocoder: factors buffer too small");
    std::memcpy(factors, f->t.factors, (size_t)*count * sizeof(int));
  });
}

int ad_vocoder_kernel_info(const ad_vocoder* f, int* lanes_per_channel, int* tile, int* lds_bytes) {
  return with_handle(f, [&] {
    if (lanes_per_channel) *lanes_per_channel = 64;
    if (tile) *tile = kVocTile;
    if (lds_bytes) *lds_bytes = kVocLdsBytes;
  });
}

int ad_vocoder_get_state(ad_vocoder* f, int channel, double* state, int* counter) {
  return guard([&] {
    check_channel(f, channel);
    DeviceScope ds(f->device);
    f->order.wait_host();
    const size_t per = (size_t)VOC_STATE_ROWS * kVocBands;
    if (state) AD_HIP(hipMemcpy(state, f->state.p + channel * per, per * sizeof(double), hipMemcpyDeviceToHost));
    if (counter) *counter = f->counter;
  });
}

int ad_vocoder_process(ad_vocoder* f, const double* modulator, const double* carrier, double* out, int64_t n) {
  return with_handle(f, [&] {
    if (n < 0 || (n > 0 && (!modulator || !carrier || !out))) AD_FAIL(AD_ERR_INVALID_ARGUMENT, "bad buffer");
    if (n == 0) return;
    const size_t count = (size_t)f->channels * n;
    f->order.wait_host();
    f->io.reserve(2 * count);
    double* d_mod = f->io.p;
    double* d_car = f->io.p + count;
    AD_HIP(hipMemcpyAsync(d_mod, modulator, count * sizeof(double), hipMemcpyHostToDevice, f->stream));
    AD_HIP(hipMemcpyAsync(d_car, carrier, count * sizeof(double), hipMemcpyHostToDevice, f->stream));
    run(f, d_mod, n, d_car, n, d_mod, n, n, f->stream);
    AD_HIP(hipMemcpyAsync(out, d_mod, count * sizeof(double), hipMemcpyDeviceToHost, f->stream));
    AD_HIP(hipStreamSynchronize(f->stream));
  });
}

int ad_vocoder_process_device(ad_vocoder* f, const double* d_mod, int64_t ms, const double* d_car, int64_t cs,
                              double* d_out, int64_t os, int64_t n, void* stream) {
  return with_handle(f, [&] {
    if (n < 0 || (n > 0 && (!d_mod || !d_car || !d_out || ms < n || cs < n || os < n)))
      AD_FAIL(AD_ERR_INVALID_ARGUMENT, "bad buffer geometry");
    if (n == 0) return;
    // a workgroup reads its channel's samples before it stores them, so exact aliasing is safe; rows that
    // overlap another channel's are not
    if (!(d_out == d_mod && os == ms) && overlap(d_out, os, d_mod, ms, f->channels, n))
      AD_FAIL(AD_ERR_INVALID_ARGUMENT, "vocoder: out overlaps the modulator without being it");
    if (!(d_out == d_car && os == cs) && overlap(d_out, os, d_car, cs, f->channels, n))
      AD_FAIL(AD_ERR_INVALID_ARGUMENT, "vocoder: out overlaps the carrier without being it");
    run(f, d_mod, ms, d_car, cs, d_out, os, n, reinterpret_cast<hipStream_t>(stream));
  });
}

int ad_vocoder_reset(ad_vocoder* f) {
  // Reset :648-670: the envelopes, every section, the counter; ordered after the last call
  return with_handle(f, [&] {
    clear_rows(f, 0, VOC_STATE_ROWS);
    f->counter = 0;
  });
}

void ad_vocoder_destroy(ad_vocoder* f) { destroy_handle(f); }

}  // extern "C"
