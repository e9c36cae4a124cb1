// Host side of the BS.1770 loudness meter (layout and arithmetic: afx_loudness.h): the K-weighting design, the block count,
// the cost record, the final host arithmetic on a clip's gated means (log10, the gain), and afx_loudness_host -- one clip
// through the block decomposition the kernels of afx_loudness.hip run, with the same tables and the same operations in the
// same order, on the CPU.  No device code: part of the sanitizer build.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "afx.h"
#define AFX_FILT_HOST_ONLY
#include "afx_hpss.h"
#include "afx_loudness.h"
#include "afx_internal.h"

namespace afx {

static_assert(kLoudModeMeasure == AFX_LOUD_MEASURE && kLoudModeLoudness == AFX_LOUD_NORM_LOUDNESS && kLoudModePeak == AFX_LOUD_NORM_PEAK,
              "the modes of afx_loudness.h are the ABI's");

const char* loud_refusal(int rate, double block_size, int* code) {
  *code = AFX_ERR_INVALID;
  if (rate < 1) return "the rate must be positive";
  if (!(block_size > 0.0) || !std::isfinite(block_size)) return "block_size must be positive and finite";
  *code = AFX_ERR_UNSUPPORTED;
  if (rate < kLoudMinRate || rate > kLoudMaxRate) return "rates outside 4000 .. 192000 Hz are not supported";
  if (block_size > 3600.0) return "block sizes above 3600 s are not supported";
  // segments are block_size * rate / 4 samples long to within one sample
  if (block_size * 0.25 * (double)rate < (double)(kFiltL + 1)) return "a quarter of block_size must span more than 64 samples";
  return nullptr;
}

int64_t loud_n_blocks(int64_t n, int rate, double block_size) {
  if ((double)n < block_size * (double)rate) return 0;
  const double T = (double)n / (double)rate;
  return (int64_t)(std::nearbyint((T - block_size) / (block_size * 0.25)) + 1.0);     // np.round: half to even
}

// pyloudnorm's IIRfilter ('high_shelf', 'high_pass'): the RBJ forms, divided through by a0
static void kweight(int rate, double* sos) {
  {
    const double G = 4.0, Q = 1.0 / std::sqrt(2.0), fc = 1500.0;
    const double A = std::pow(10.0, G / 40.0), w0 = 2.0 * M_PI * (fc / (double)rate), al = std::sin(w0) / (2.0 * Q);
    const double cw = std::cos(w0), sa = 2.0 * std::sqrt(A) * al;
    const double b0 = A * ((A + 1.0) + (A - 1.0) * cw + sa), b1 = -2.0 * A * ((A - 1.0) + (A + 1.0) * cw),
                 b2 = A * ((A + 1.0) + (A - 1.0) * cw - sa);
    const double a0 = (A + 1.0) - (A - 1.0) * cw + sa, a1 = 2.0 * ((A - 1.0) - (A + 1.0) * cw), a2 = (A + 1.0) - (A - 1.0) * cw - sa;
    sos[0] = b0 / a0; sos[1] = b1 / a0; sos[2] = b2 / a0; sos[3] = 1.0; sos[4] = a1 / a0; sos[5] = a2 / a0;
  }
  {
    const double Q = 0.5, fc = 38.0;
    const double w0 = 2.0 * M_PI * (fc / (double)rate), al = std::sin(w0) / (2.0 * Q), cw = std::cos(w0);
    const double b0 = (1.0 + cw) / 2.0, b1 = -(1.0 + cw), b2 = (1.0 + cw) / 2.0, a0 = 1.0 + al, a1 = -2.0 * cw, a2 = 1.0 - al;
    sos[6] = b0 / a0; sos[7] = b1 / a0; sos[8] = b2 / a0; sos[9] = 1.0; sos[10] = a1 / a0; sos[11] = a2 / a0;
  }
}

void loud_build_tab(int rate, FiltTab& t) {
  double sos[12];
  kweight(rate, sos);
  const char* why = "";
  (void)filt_build_tab(sos, kLoudS, t, &why);        // finite, a0 == 1, no pole at z = 1 at every accepted rate
}

double loud_abs_gate() { return std::pow(10.0, (-70.0 + 0.691) / 10.0); }

float loud_finish(const double* dev, int mode, double target, double* rec) {
  const double nan = std::numeric_limits<double>::quiet_NaN();
  const bool measured = dev[kLdBlocks] > 0.0;
  rec[AFX_LOUD_LUFS] = measured ? -0.691 + 10.0 * std::log10(dev[kLdMean2]) : nan;
  rec[AFX_LOUD_BLOCKS] = dev[kLdBlocks]; rec[AFX_LOUD_N1] = dev[kLdN1]; rec[AFX_LOUD_N2] = dev[kLdN2];
  rec[AFX_LOUD_GAMMA_R] = measured ? -0.691 + 10.0 * std::log10(dev[kLdMean1]) - 10.0 : nan;
  rec[AFX_LOUD_GATED_MS] = measured ? dev[kLdMean2] : nan;
  rec[AFX_LOUD_FIRST_MS] = measured ? dev[kLdMean1] : nan;
  rec[AFX_LOUD_UNGATED_MS] = measured ? dev[kLdMeanAll] : nan;
  rec[AFX_LOUD_PEAK] = dev[kLdPeak];
  rec[AFX_LOUD_GAIN] = rec[AFX_LOUD_PEAK_OUT] = nan;
  if (mode == kLoudModeMeasure) return 1.0f;
  float g = 1.0f;                                    // a clip without a level (silence) comes back unchanged
  if (mode == kLoudModeLoudness) {
    const double L = rec[AFX_LOUD_LUFS];
    if (std::isfinite(L)) g = (float)std::pow(10.0, (target - L) / 20.0);
  } else if (dev[kLdPeak] > 0.0) {
    g = (float)(std::pow(10.0, target / 20.0) / dev[kLdPeak]);
  }
  rec[AFX_LOUD_GAIN] = (double)g;
  rec[AFX_LOUD_PEAK_OUT] = (double)(g * (float)dev[kLdPeak]);      // rounding is monotonic: max |g x| = |g max|x||
  return g;
}

void loud_cost(int sample_fmt, int mem_kind, int out_mem_kind, int mode, StftCost& cost) {
  const int64_t esz = sample_fmt == AFX_FMT_S16 ? 2 : 4;
  cost = StftCost{};
  // a frame of the chunk rule is 512 samples = 8 blocks: each block's state (32 bytes) and two sums (16), and, as
  // segments and gating blocks are no shorter than a block, a segment sum and a z_j
  cost.per_frame = 8 * (kLoudZ * 8 + 16 + 8 + 8);
  cost.per_tile = 8;                                                         // the tile's peak and flag
  cost.per_sample = (mem_kind == AFX_MEM_HOST ? esz : 0) + (mode != kLoudModeMeasure && out_mem_kind == AFX_MEM_HOST ? 4 : 0);
  cost.per_clip = kFiltB * (kLoudZ * 8 + 16) + 4 * 16 + 512;                 // the last tile's unused blocks, three more segments, records
  cost.tile = kFiltTile / 512;
  cost.tile_cap = 1 << 24;
}

}  // namespace afx

using namespace afx;

extern "C" int afx_kweight_sos(int rate, double* sos) {
  if (!sos) { set_error("afx_kweight_sos: null argument"); return AFX_ERR_INVALID; }
  if (rate < kLoudMinRate || rate > kLoudMaxRate) { set_error("afx_kweight_sos: the rate must lie in 4000 .. 192000 Hz"); return AFX_ERR_INVALID; }
  kweight(rate, sos);
  return AFX_OK;
}

extern "C" int afx_loudness_geometry(int32_t* info) {
  if (!info) { set_error("afx_loudness_geometry: null argument"); return AFX_ERR_INVALID; }
  info[0] = kFiltL; info[1] = kFiltB; info[2] = kLoudMinRate; info[3] = kLoudMaxRate; info[4] = kLoudMaxRates;
  return AFX_OK;
}

extern "C" int afx_loudness_blocks(int64_t n, int rate, double block_size, int64_t* n_blocks) {
  const std::string who = "afx_loudness_blocks: ";
  if (!n_blocks || n < 0) { set_error(who + "null/invalid argument"); return AFX_ERR_INVALID; }
  int code;
  if (const char* why = loud_refusal(rate, block_size, &code)) { set_error(who + why); return code; }
  if (n > ((int64_t)1 << 31)) { set_error(who + "more than 2^31 samples is not supported"); return AFX_ERR_UNSUPPORTED; }
  *n_blocks = loud_n_blocks(n, rate, block_size);
  return AFX_OK;
}

extern "C" int afx_loudness_cost(int sample_fmt, int mem_kind, int out_mem_kind, int mode, int64_t* cost) {
  const std::string who = "afx_loudness_cost: ";
  if (!cost) { set_error(who + "null argument"); return AFX_ERR_INVALID; }
  if ((sample_fmt != AFX_FMT_F32 && sample_fmt != AFX_FMT_S16) || (mem_kind != AFX_MEM_HOST && mem_kind != AFX_MEM_DEVICE) ||
      (out_mem_kind != AFX_MEM_HOST && out_mem_kind != AFX_MEM_DEVICE)) {
    set_error(who + "unknown sample format or memory kind");
    return AFX_ERR_INVALID;
  }
  if (mode != AFX_LOUD_MEASURE && mode != AFX_LOUD_NORM_LOUDNESS && mode != AFX_LOUD_NORM_PEAK) { set_error(who + "unknown mode"); return AFX_ERR_INVALID; }
  StftCost c;
  loud_cost(sample_fmt, mem_kind, out_mem_kind, mode, c);
  const int64_t v[6] = {c.per_frame, c.per_tile, c.per_sample, c.per_clip, c.tile, c.tile_cap};
  std::memcpy(cost, v, sizeof(v));
  return AFX_OK;
}

extern "C" int afx_loudness_host(const void* samples, int sample_fmt, int64_t n, int rate, double block_size, double target,
                                 int mode, double* out_rec, double* out_blocks, float* out, int32_t* out_status) {
  const std::string who = "afx_loudness_host: ";
  if (!out_rec || !out_status || n < 0 || (n > 0 && !samples)) { set_error(who + "null/invalid argument"); return AFX_ERR_INVALID; }
  if (sample_fmt != AFX_FMT_F32 && sample_fmt != AFX_FMT_S16) { set_error(who + "unknown sample format"); return AFX_ERR_INVALID; }
  if (mode != AFX_LOUD_MEASURE && mode != AFX_LOUD_NORM_LOUDNESS && mode != AFX_LOUD_NORM_PEAK) { set_error(who + "unknown mode"); return AFX_ERR_INVALID; }
  if (mode != AFX_LOUD_MEASURE && !std::isfinite(target)) { set_error(who + "the target must be finite"); return AFX_ERR_INVALID; }
  int code;
  if (const char* why = loud_refusal(rate, block_size, &code)) { set_error(who + why); return code; }
  if (n > ((int64_t)1 << 31)) { set_error(who + "more than 2^31 samples is not supported"); return AFX_ERR_UNSUPPORTED; }
  std::fill(out_rec, out_rec + AFX_LOUD_N, std::numeric_limits<double>::quiet_NaN());
  const int64_t nbk = loud_n_blocks(n, rate, block_size);
  if (mode == AFX_LOUD_NORM_PEAK ? n == 0 : nbk == 0) { *out_status = AFX_CLIP_TOO_SHORT; return AFX_OK; }
  if (mode != AFX_LOUD_MEASURE && !out) { set_error(who + "null out"); return AFX_ERR_INVALID; }
  // 1. peak and the non-finite flag
  float peak = 0.0f;
  bool bad = false;
  for (int64_t i = 0; i < n; ++i) {
    const float a = std::fabs(loud_raw(samples, sample_fmt, i));
    if (!(a <= FLT_MAX)) bad = true;
    peak = std::max(peak, a);
  }
  if (bad) { *out_status = AFX_CLIP_NONFINITE; return AFX_OK; }
  FiltTab t;
  loud_build_tab(rate, t);
  const double tg = block_size, fr = (double)rate;
  const int64_t nb = (n + kFiltL - 1) / kFiltL, lim = loud_limit(tg, fr, n, (int32_t)nbk);
  auto sample = [&](int64_t j) { return j < n ? loud_raw(samples, sample_fmt, j) : 0.0f; };
  // 2. every block from zero state: its end state
  std::vector<double> carry((size_t)nb * kLoudZ), part((size_t)nb * 2);
  for (int64_t k = 0; k < nb; ++k) {
    double z[kLoudZ] = {0};
    for (int m = 0; m < kFiltL; ++m) (void)filt_cascade<kLoudS>(t.sec, (double)sample(k * kFiltL + m), z);
    for (int j = 0; j < kLoudZ; ++j) carry[k * kLoudZ + j] = z[j];
  }
  // 3. the entry states
  {
    double z[kLoudZ] = {0};
    for (int64_t k = 0; k < nb; ++k) {
      double fin[kLoudZ];
      for (int j = 0; j < kLoudZ; ++j) { fin[j] = carry[k * kLoudZ + j]; carry[k * kLoudZ + j] = z[j]; }
      filt_carry<kLoudS>(t.T, z, fin);
    }
  }
  // 4. every block from its entry state: two sums of squares
  for (int64_t k = 0; k < nb; ++k) {
    int split, stop;
    loud_block_cut(tg, fr, k * kFiltL, lim, &split, &stop);
    double p[2] = {0.0, 0.0};
    if (stop > 0) {
      double z[kLoudZ];
      for (int j = 0; j < kLoudZ; ++j) z[j] = carry[k * kLoudZ + j];
      loud_block_sums(t.sec, z, split, stop, [&](int m) { return sample(k * kFiltL + m); }, p);
    }
    part[2 * k] = p[0]; part[2 * k + 1] = p[1];
  }
  // 5. segments, z_j, the gates
  std::vector<double> seg((size_t)(nbk > 0 ? nbk + 3 : 0)), z((size_t)nbk);
  for (int64_t k = 0; k < (int64_t)seg.size(); ++k) seg[k] = loud_seg_sum(tg, fr, lim, k, part.data());
  for (int64_t j = 0; j < nbk; ++j) z[j] = loud_z(seg.data(), j, tg * fr);
  const double gate = loud_abs_gate();
  double dev[kLoudRec];
  int64_t c1 = 0, c2 = 0;
  for (int64_t j = 0; j < nbk; ++j) c1 += z[j] >= gate;
  const double s_all = loud_sum64_host(nbk, [&](int64_t j) { return z[j]; });
  const double s1 = loud_sum64_host(nbk, [&](int64_t j) { return z[j] >= gate ? z[j] : 0.0; });
  const double mean1 = c1 > 0 ? s1 / (double)c1 : 0.0, rel = mean1 / 10.0;
  for (int64_t j = 0; j < nbk; ++j) c2 += z[j] > rel && z[j] > gate;
  const double s2 = loud_sum64_host(nbk, [&](int64_t j) { return z[j] > rel && z[j] > gate ? z[j] : 0.0; });
  dev[kLdBlocks] = (double)nbk; dev[kLdN1] = (double)c1; dev[kLdN2] = (double)c2;
  dev[kLdMean1] = mean1; dev[kLdMean2] = c2 > 0 ? s2 / (double)c2 : 0.0; dev[kLdMeanAll] = nbk > 0 ? s_all / (double)nbk : 0.0;
  dev[kLdPeak] = (double)peak; dev[kLdBad] = 0.0;
  const float g = loud_finish(dev, mode, target, out_rec);
  if (out_blocks) std::copy(z.begin(), z.end(), out_blocks);
  if (mode != AFX_LOUD_MEASURE)
    for (int64_t i = 0; i < n; ++i) out[i] = g * loud_raw(samples, sample_fmt, i);
  *out_status = AFX_CLIP_OK;
  return AFX_OK;
}
