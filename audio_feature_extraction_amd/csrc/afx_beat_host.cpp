// Host side of beat tracking: afx_beat_track_host -- one envelope through the definition the kernels of afx_beat.hip run
// (tests/beat_ref.py), in float64 with the same order of every sum, on the CPU.  The second opinion the device result is
// compared with.  No device code: part of the sanitizer build.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "afx.h"
#include "afx_beat.h"
#include "afx_internal.h"

namespace afx {

// what k_beat_score's block reduction computes: kBeatThreads strided partial results in element order, then a halving tree
template <typename F, typename Op>
static double strided_tree(int64_t T, double init, F term, Op op) {
  double part[kBeatThreads];
  for (int t = 0; t < kBeatThreads; ++t) {
    double v = init;
    for (int64_t i = t; i < T; i += kBeatThreads) v = op(v, term(i));
    part[t] = v;
  }
  for (int s = kBeatThreads / 2; s > 0; s >>= 1)
    for (int t = 0; t < s; ++t) part[t] = op(part[t], part[t + s]);
  return part[0];
}

// frames per beat of a tempo; false when it is outside [1, 768]
bool beat_fpb(double fps, double bpm, int32_t* fpb) {
  const double q = fps * 60.0;
  const double r = std::nearbyint(q / bpm);              // half to even in the default rounding mode
  if (!(r >= 1.0 && r <= (double)kBeatMaxFpb)) return false;
  *fpb = (int32_t)r;
  return true;
}

}  // namespace afx

using namespace afx;

extern "C" int afx_beat_track_host(const float* env, int64_t T, double fps, double bpm, double tightness, int trim,
                                   uint8_t* out_mask, int64_t* out_n_beats, double* out_localscore, double* out_cumscore,
                                   int32_t* out_backlink) {
  const std::string who = "afx_beat_track_host: ";
  if (T < 0 || !out_n_beats || (T > 0 && (!env || !out_mask))) { set_error(who + "null/invalid argument"); return AFX_ERR_INVALID; }
  if (T > ((int64_t)1 << 22)) { set_error(who + "more than 2^22 frames is not supported"); return AFX_ERR_UNSUPPORTED; }
  if (!std::isfinite(bpm) || !std::isfinite(fps) || !std::isfinite(tightness) || bpm < 0.0 || fps <= 0.0 || tightness <= 0.0) {
    set_error(who + "bpm must be finite and >= 0, fps and tightness finite and > 0");
    return AFX_ERR_INVALID;
  }
  int32_t fpb = 0;
  if (bpm > 0.0 && !beat_fpb(fps, bpm, &fpb)) { set_error(who + "the tempo must give 1 .. 768 frames per beat"); return AFX_ERR_INVALID; }
  bool nz = false;
  for (int64_t i = 0; i < T; ++i) {
    if (!std::isfinite(env[i])) { set_error(who + "the envelope holds a NaN / inf"); return AFX_ERR_INVALID; }
    nz |= env[i] != 0.f;
  }
  *out_n_beats = 0;
  if (T > 0) std::memset(out_mask, 0, (size_t)T);
  if (out_localscore) std::fill(out_localscore, out_localscore + T, 0.0);
  if (out_cumscore) std::fill(out_cumscore, out_cumscore + T, 0.0);
  if (out_backlink) std::fill(out_backlink, out_backlink + T, -1);
  if (T < 2 || !nz || bpm == 0.0) return AFX_OK;

  auto add = [](double a, double b) { return a + b; };
  const double mean = strided_tree(T, 0.0, [&](int64_t i) { return (double)env[i]; }, add) / (double)T;
  const double var = strided_tree(T, 0.0, [&](int64_t i) { const double d = (double)env[i] - mean; return d * d; }, add) / (double)(T - 1);
  const double denom = std::sqrt(var) + DBL_MIN;
  std::vector<double> x((size_t)T), ls((size_t)T), cum((size_t)T);
  std::vector<int32_t> bl((size_t)T);
  for (int64_t i = 0; i < T; ++i) x[i] = (double)env[i] / denom;
  std::vector<double> w((size_t)2 * fpb + 1);
  for (int k = 0; k <= 2 * fpb; ++k) {
    const double a = (double)(k - fpb) * 32.0 / (double)fpb;
    const double a2 = a * a;
    w[k] = std::exp(-0.5 * a2);
  }
  for (int64_t i = 0; i < T; ++i) {
    const int64_t k0 = std::max<int64_t>(0, i + fpb - (T - 1)), k1 = std::min<int64_t>(2 * fpb, i + fpb);
    double acc = 0.0;
    for (int64_t k = k0; k <= k1; ++k) {
      const double p = w[k] * x[i + fpb - k];
      acc += p;
    }
    ls[i] = acc;
  }
  const double maxls = strided_tree(T, -INFINITY, [&](int64_t i) { return ls[i]; }, [](double a, double b) { return b > a ? b : a; });
  const double thresh = 0.01 * maxls;
  const int lo = (int)std::nearbyint((double)fpb / 2.0);
  const int dmin = std::max(lo, 1);                       // distance 0 (fpb 1) scores -inf and never wins
  std::vector<double> pen((size_t)2 * fpb + 1, 0.0);
  const double logf = std::log((double)fpb);
  for (int d = dmin; d <= 2 * fpb; ++d) {
    const double g = std::log((double)d) - logf;
    const double g2 = g * g;
    pen[d] = -(tightness * g2);
  }
  bool first = true;
  for (int64_t i = 0; i < T; ++i) {
    double best = -INFINITY;
    int bd = 0;
    const int64_t dmax = std::min<int64_t>(2 * fpb, i);
    for (int64_t d = dmin; d <= dmax; ++d) {
      const double sc = cum[i - d] + pen[d];
      if (sc > best) { best = sc; bd = (int)d; }
    }
    cum[i] = bd ? ls[i] + best : ls[i];
    if (first && ls[i] < thresh) bl[i] = -1;
    else { bl[i] = bd ? (int32_t)(i - bd) : -1; first = false; }
  }
  if (out_localscore) std::copy(ls.begin(), ls.end(), out_localscore);
  if (out_cumscore) std::copy(cum.begin(), cum.end(), out_cumscore);
  if (out_backlink) std::copy(bl.begin(), bl.end(), out_backlink);

  // the last beat: the last local maximum that reaches half the median of the local maxima
  auto is_max = [&](int64_t i) { return cum[i] > cum[std::max<int64_t>(i - 1, 0)] && cum[i] >= cum[std::min<int64_t>(i + 1, T - 1)]; };
  std::vector<double> peaks;
  for (int64_t i = 0; i < T; ++i)
    if (is_max(i)) peaks.push_back(cum[i]);
  if (peaks.empty()) return AFX_OK;
  const size_t k = (peaks.size() - 1) / 2;
  std::nth_element(peaks.begin(), peaks.begin() + k, peaks.end());
  double med = peaks[k];
  if (peaks.size() % 2 == 0) med = (med + *std::min_element(peaks.begin() + k + 1, peaks.end())) * 0.5;
  const double half = 0.5 * med;
  int64_t tail = -1;
  for (int64_t i = T - 1; i >= 0 && tail < 0; --i)
    if (is_max(i) && cum[i] >= half) tail = i;
  if (tail < 0) return AFX_OK;

  // the chain from the last beat back; the trim walks it the same way (0.5 s[j - 1] + s[j] + 0.5 s[j + 1], summed from the
  // last beat down)
  int64_t nb = 0, keep_lo = -1, keep_hi = -1;
  if (trim) {
    double sum = 0.0, later = 0.0;
    for (int64_t n = tail; n >= 0; n = bl[n]) {
      const double earlier = bl[n] >= 0 ? ls[bl[n]] : 0.0;
      const double sm = (0.5 * earlier + ls[n]) + 0.5 * later;
      sum += sm * sm;
      later = ls[n];
      ++nb;
    }
    const double th = 0.5 * std::sqrt(sum / (double)nb);
    later = 0.0;
    for (int64_t n = tail; n >= 0; n = bl[n]) {
      const double earlier = bl[n] >= 0 ? ls[bl[n]] : 0.0;
      const double sm = (0.5 * earlier + ls[n]) + 0.5 * later;
      if (sm > th) { if (keep_hi < 0) keep_hi = n; keep_lo = n; }
      later = ls[n];
    }
    if (keep_hi < 0) return AFX_OK;
  } else {
    keep_lo = 0; keep_hi = tail;
  }
  nb = 0;
  for (int64_t n = tail; n >= 0; n = bl[n])
    if (n >= keep_lo && n <= keep_hi) { out_mask[n] = 1; ++nb; }
  *out_n_beats = nb;
  return AFX_OK;
}
