// Host-only part of the recording screen and the compare sums: the cost record afx_assess_batch / afx_compare_batch cut a
// batch with, the argument refusals they share with the host executors, and the executors themselves -- one clip or one
// pair through the definitions of include/afx.h in plain C++, float64 sums in sample order.  They are the specification of
// the kernels (which sum the same exact squares in another order), what the Python layer runs when no GPU is visible, and
// part of the host-only sanitizer build.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "afx_assess.h"
#include "afx_internal.h"

namespace afx {

void assess_cost(int what, int sample_fmt, int mem_kind, StftCost& cost) {
  const int64_t esz = sample_fmt == AFX_FMT_S16 ? 2 : 4, up = mem_kind == AFX_MEM_HOST ? esz : 0;
  cost = StftCost{};
  if (what == AFX_COST_ASSESS) {
    cost.per_sample = 17 + up;                            // the pieces and span records of both framings at frame length 1
    cost.per_clip = 256;                                  // their rounding, the clip record, the result, the status
  } else {
    cost.per_sample = 1 + 2 * up;                         // 80 bytes per span of 4096 samples; both sides uploaded
    cost.per_clip = 256;
  }
  cost.tile = kHpssTile;                                  // no kernel here works in tiles; the count only has to fit an int
  cost.tile_cap = INT32_MAX / 2;
}

const char* assess_refusal(int64_t len, int32_t frame_short, int32_t frame_long, double threshold_db, int64_t noise_cap) {
  if (len < 0) return "negative length";
  if (frame_short < 1 || frame_long < 1) return "frame lengths must be >= 1";
  if (!std::isfinite(threshold_db)) return "threshold_db must be finite";
  if (noise_cap < 0) return "noise_cap must be >= 0";
  return nullptr;
}

static inline float host_sample(const void* p, int fmt, int64_t j) {
  return fmt == AFX_FMT_S16 ? (float)((const int16_t*)p)[j] * 0x1p-15f : ((const float*)p)[j];
}

// sum of squares of the centred frame t of hop = length fl, cut to the clip
static double frame_ss(const void* p, int fmt, int64_t len, int32_t fl, int64_t t) {
  const int64_t a = std::max<int64_t>(t * fl - fl / 2, 0), e = std::min<int64_t>(t * fl - fl / 2 + fl, len);
  double s = 0.0;
  for (int64_t j = a; j < e; ++j) { const double x = host_sample(p, fmt, j); s += x * x; }
  return s;
}

}  // namespace afx

using namespace afx;

extern "C" int afx_assess_cost(int what, int sample_fmt, int mem_kind, int64_t* cost) {
  if (!cost) { set_error("afx_assess_cost: null argument"); return AFX_ERR_INVALID; }
  if (what != AFX_COST_ASSESS && what != AFX_COST_COMPARE) { set_error("afx_assess_cost: unknown entry point"); return AFX_ERR_INVALID; }
  if ((sample_fmt != AFX_FMT_F32 && sample_fmt != AFX_FMT_S16) || (mem_kind != AFX_MEM_HOST && mem_kind != AFX_MEM_DEVICE)) {
    set_error("afx_assess_cost: unknown sample format or memory kind");
    return AFX_ERR_INVALID;
  }
  StftCost c;
  assess_cost(what, sample_fmt, mem_kind, c);
  const int64_t v[6] = {c.per_frame, c.per_tile, c.per_sample, c.per_clip, c.tile, c.tile_cap};
  std::memcpy(cost, v, sizeof(v));
  return AFX_OK;
}

extern "C" int afx_assess_host(const void* samples, int sample_fmt, int64_t n, int32_t frame_short, int32_t frame_long,
                               double threshold_db, int64_t noise_cap, double* out_rec, int32_t* out_status) {
  const std::string who = "afx_assess_host: ";
  if (!out_rec || !out_status || (n > 0 && !samples)) { set_error(who + "null/invalid argument"); return AFX_ERR_INVALID; }
  if (sample_fmt != AFX_FMT_F32 && sample_fmt != AFX_FMT_S16) { set_error(who + "unknown sample format"); return AFX_ERR_INVALID; }
  if (const char* why = assess_refusal(n, frame_short, frame_long, threshold_db, noise_cap)) { set_error(who + why); return AFX_ERR_INVALID; }
  const double nan = std::nan("");
  std::fill(out_rec, out_rec + AFX_ASSESS_N, nan);
  if (n == 0) { *out_status = AFX_CLIP_TOO_SHORT; return AFX_OK; }
  double total = 0.0, peak = 0.0;
  for (int64_t j = 0; j < n; ++j) {
    const float x = host_sample(samples, sample_fmt, j);
    if (!std::isfinite(x)) { *out_status = AFX_CLIP_NONFINITE; return AFX_OK; }
    total += (double)x * (double)x;
    peak = std::max(peak, (double)std::fabs(x));
  }
  const int64_t T = as_frames(n, frame_short), TL = as_frames(n, frame_long);
  std::vector<double> p((size_t)T);
  double pmax = 0.0;
  for (int64_t t = 0; t < T; ++t) {
    p[t] = frame_ss(samples, sample_fmt, n, frame_short, t) / (double)frame_short;
    pmax = std::max(pmax, p[t]);
  }
  // silent: 10 log10(max(amin^2, p)) - 10 log10(max(amin^2, pmax)), clamped at -80 from below, < threshold_db
  const double a2 = 1e-10, lim = std::max(a2, pmax) * std::pow(10.0, threshold_db / 10.0);
  int64_t silent = 0, run = 0, longest = 0;
  for (int64_t t = 0; t < T; ++t) {
    if (threshold_db > -80.0 && std::max(a2, p[t]) < lim) { ++silent; ++run; longest = std::max(longest, run); }
    else run = 0;
  }
  const int64_t nw = std::min<int64_t>((int64_t)(0.1 * (double)n), noise_cap);
  double noise = 0.0;
  for (int64_t j = 0; j < nw; ++j) { const double x = host_sample(samples, sample_fmt, j); noise += x * x; }
  std::vector<double> r((size_t)TL);
  double sum = 0.0, dev = 0.0;
  for (int64_t t = 0; t < TL; ++t) { r[t] = std::sqrt(frame_ss(samples, sample_fmt, n, frame_long, t) / (double)frame_long); sum += r[t]; }
  const double mean = sum / (double)TL;
  for (int64_t t = 0; t < TL; ++t) dev += (r[t] - mean) * (r[t] - mean);
  out_rec[0] = (double)T; out_rec[1] = (double)silent; out_rec[2] = (double)longest; out_rec[3] = std::sqrt(pmax);
  out_rec[4] = total / (double)n; out_rec[5] = peak; out_rec[6] = nw > 0 ? noise / (double)nw : nan;
  out_rec[7] = (double)TL; out_rec[8] = mean; out_rec[9] = std::sqrt(dev / (double)TL);
  *out_status = AFX_CLIP_OK;
  return AFX_OK;
}

extern "C" int afx_compare_host(const void* ref, const void* deg, int sample_fmt, int64_t n_ref, int64_t n_deg,
                                double* out_rec, int32_t* out_status) {
  const std::string who = "afx_compare_host: ";
  if (!out_rec || !out_status || n_ref < 0 || n_deg < 0 || (std::min(n_ref, n_deg) > 0 && (!ref || !deg))) {
    set_error(who + "null/invalid argument");
    return AFX_ERR_INVALID;
  }
  if (sample_fmt != AFX_FMT_F32 && sample_fmt != AFX_FMT_S16) { set_error(who + "unknown sample format"); return AFX_ERR_INVALID; }
  const int64_t n = std::min(n_ref, n_deg);
  std::fill(out_rec, out_rec + AFX_COMPARE_N, std::nan(""));
  if (n == 0) { *out_status = AFX_CLIP_TOO_SHORT; return AFX_OK; }
  double a[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int64_t j = 0; j < n; ++j) {
    const float r = host_sample(ref, sample_fmt, j), d = host_sample(deg, sample_fmt, j);
    if (!std::isfinite(r) || !std::isfinite(d)) { *out_status = AFX_CLIP_NONFINITE; return AFX_OK; }
    const double x = r, y = d, z = (double)(d - r);                    // the difference in float32, as numpy's
    a[0] += x; a[1] += y; a[2] += x * x; a[3] += y * y; a[4] += x * y; a[5] += z * z;
  }
  const double mr = a[0] / (double)n, md = a[1] / (double)n;
  double m[3] = {0.0, 0.0, 0.0};
  for (int64_t j = 0; j < n; ++j) {
    const double x = (double)host_sample(ref, sample_fmt, j) - mr, y = (double)host_sample(deg, sample_fmt, j) - md;
    m[0] += x * x; m[1] += y * y; m[2] += x * y;
  }
  out_rec[0] = (double)n;
  for (int q = 0; q < 6; ++q) out_rec[1 + q] = a[q];
  for (int q = 0; q < 3; ++q) out_rec[7 + q] = m[q];
  *out_status = AFX_CLIP_OK;
  return AFX_OK;
}
