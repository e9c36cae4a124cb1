// Host side of the zero-phase IIR filter (layout and arithmetic: afx_filt.h): the Butterworth design, the tables of a
// section cascade, and afx_sosfiltfilt_host -- one clip through the block decomposition the kernels of afx_filt.hip run, with
// the same tables and the same fused operations in the same order, on the CPU.  No device code: part of the sanitizer build.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <complex>
#include <cstring>
#include <string>
#include <vector>

#include "afx.h"
#define AFX_FILT_HOST_ONLY
#include "afx_filt.h"
#include "afx_internal.h"

namespace afx {

bool filt_build_tab(const double* sos, int n_sections, FiltTab& t, const char** why) {
  std::memset(&t, 0, sizeof(t));
  double scale = 1.0;
  for (int s = 0; s < n_sections; ++s) {
    const double* r = sos + 6 * s;
    for (int k = 0; k < 6; ++k)
      if (!std::isfinite(r[k])) { *why = "a section coefficient is not finite"; return false; }
    if (r[3] != 1.0) { *why = "sections must be normalised to a0 = 1"; return false; }
    FiltSec& c = t.sec[s];
    c.b0 = r[0]; c.b1 = r[1]; c.b2 = r[2]; c.a1 = r[4]; c.a2 = r[5];
    const double den = 1.0 + c.a1 + c.a2;
    if (den == 0.0) { *why = "a section has a pole at z = 1: no steady state"; return false; }
    // the section's state under a constant input `scale`: y = g x, z0 = y - b0 x, z1 = b2 x - a2 y
    const double g = (c.b0 + c.b1 + c.b2) / den;
    t.zi[2 * s] = scale * (g - c.b0);
    t.zi[2 * s + 1] = scale * (c.b2 - c.a2 * g);
    scale *= g;
  }
  // zero-input responses by running the recurrences: column j is the cascade started from unit state j
  for (int j = 0; j < 2 * n_sections; ++j) {
    double z[kFiltZ] = {0};
    z[j] = 1.0;
    for (int m = 0; m < kFiltL; ++m) {
      double x = 0.0;
      for (int s = 0; s < n_sections; ++s) x = filt_step(t.sec[s], x, z[2 * s], z[2 * s + 1]);
      t.R[m][j] = x;
    }
    for (int i = 0; i < 2 * n_sections; ++i) t.T[i][j] = z[i];
  }
  return true;
}

namespace {

template <int S>
void host_clip(const FiltTab& t, FiltIn f, float* out, double* peaks, int32_t* status) {
  // 1. peak and the non-finite flag
  float peak = 0.0f;
  bool bad = false;
  for (int64_t i = 0; i < f.n; ++i) {
    const float a = std::fabs(filt_raw(f, i));
    if (!(a <= FLT_MAX)) bad = true;
    peak = std::max(peak, a);
  }
  if (bad) { *status = AFX_CLIP_NONFINITE; return; }
  f.peak = peak;
  f.norm = f.mode == kFiltModeExperiment && peak >= FLT_MIN;
  const int64_t p = f.padlen, N = f.n + 2 * p, nb = (N + kFiltL - 1) / kFiltL;
  std::vector<double> W((size_t)N), carry((size_t)nb * kFiltZ, 0.0);
  // 2. forward blocks
  for (int64_t k = 0; k < nb; ++k) {
    double z[2 * S] = {0};
    if (k == 0) {
      const double e0 = filt_e(f, 0);
      for (int j = 0; j < 2 * S; ++j) z[j] = t.zi[j] * e0;
    }
    const int len = (int)std::min<int64_t>(kFiltL, N - k * kFiltL);
    for (int m = 0; m < len; ++m) W[k * kFiltL + m] = filt_cascade<S>(t.sec, filt_e(f, k * kFiltL + m), z);
    for (int j = 0; j < 2 * S; ++j) carry[k * kFiltZ + j] = z[j];
  }
  // 3. forward carries
  auto scan = [&](bool backward) {
    double z[2 * S] = {0};
    for (int64_t q = 0; q < nb; ++q) {
      double* c = &carry[(backward ? nb - 1 - q : q) * kFiltZ];
      double fin[2 * S];
      for (int j = 0; j < 2 * S; ++j) { fin[j] = c[j]; c[j] = z[j]; }
      filt_carry<S>(t.T, z, fin);
    }
  };
  scan(false);
  // 4. forward correction + backward blocks
  for (int64_t k = 0; k < nb; ++k) {
    double zin[2 * S], z[2 * S] = {0};
    for (int j = 0; j < 2 * S; ++j) zin[j] = carry[k * kFiltZ + j];
    const int len = (int)std::min<int64_t>(kFiltL, N - k * kFiltL);
    for (int m = len - 1; m >= 0; --m) {
      const double v = filt_correct<S>(W[k * kFiltL + m], t.R[m], zin);
      if (k == nb - 1 && m == len - 1)
        for (int j = 0; j < 2 * S; ++j) z[j] = t.zi[j] * v;
      W[k * kFiltL + m] = filt_cascade<S>(t.sec, v, z);
    }
    for (int j = 0; j < 2 * S; ++j) carry[k * kFiltZ + j] = z[j];
  }
  // 5. backward carries
  scan(true);
  // 6. backward correction, the extension stripped, the peak
  double ymax = 0.0;
  for (int64_t j = p; j < p + f.n; ++j) {
    const int64_t k = j / kFiltL;
    const int m = (int)(j - k * kFiltL);
    const double y = filt_correct<S>(W[j], t.R[kFiltL - 1 - m], &carry[k * kFiltZ]);
    W[j] = y;
    ymax = std::max(ymax, std::fabs(y));
  }
  const bool scale = f.mode == kFiltModeExperiment && ymax >= DBL_MIN;
  for (int64_t i = 0; i < f.n; ++i) out[i] = (float)(scale ? W[p + i] / ymax : W[p + i]);
  if (peaks) { peaks[0] = (double)peak; peaks[1] = ymax; }
  *status = AFX_CLIP_OK;
}

}  // namespace
}  // namespace afx

using namespace afx;

extern "C" int afx_butter_sos(int order, double wn, int highpass, double* sos) {
  if (!sos) { set_error("afx_butter_sos: null argument"); return AFX_ERR_INVALID; }
  if (order < 1) { set_error("afx_butter_sos: the order must be at least 1"); return AFX_ERR_INVALID; }
  if (order > 2 * kFiltMaxS) { set_error("afx_butter_sos: orders above 8 are not supported"); return AFX_ERR_UNSUPPORTED; }
  if (!(wn > 0.0 && wn < 1.0)) { set_error("afx_butter_sos: Digital filter critical frequencies must be 0 < Wn < 1"); return AFX_ERR_INVALID; }
  // analogue prototype poles -exp(i pi m / 2N), m = -N + 1, -N + 3 .. N - 1; low-pass s = w p, high-pass s = w / p with
  // w = tan(pi wn / 2) (the pre-warped edge at fs = 2, over 2 fs); bilinear z = (1 + s) / (1 - s).  Zeros at z = -1
  // (low-pass) or z = +1 (high-pass); every section has unit gain at the far end of its pass band.
  const double w = std::tan(M_PI * wn / 2.0), zs = highpass ? -1.0 : 1.0;
  int row = 0;
  for (int m = order - 1; m >= 0; m -= 2, ++row) {
    const double th = M_PI * m / (2.0 * order);
    const std::complex<double> pa(-std::cos(th), -std::sin(th));
    const std::complex<double> s = highpass ? w / pa : w * pa;
    const std::complex<double> z = (1.0 + s) / (1.0 - s);
    double* r = sos + 6 * row;
    r[3] = 1.0;
    if (m == 0) {                                    // the real pole of an odd order
      const double a1 = -z.real(), g = (1.0 + zs * a1) / 2.0;
      r[0] = g; r[1] = zs * g; r[2] = 0.0; r[4] = a1; r[5] = 0.0;
    } else {
      const double a1 = -2.0 * z.real(), a2 = std::norm(z), g = (1.0 + zs * a1 + a2) / 4.0;
      r[0] = g; r[1] = 2.0 * zs * g; r[2] = g; r[4] = a1; r[5] = a2;
    }
  }
  return AFX_OK;
}

extern "C" int afx_filtfilt_geometry(int32_t* info) {
  if (!info) { set_error("afx_filtfilt_geometry: null argument"); return AFX_ERR_INVALID; }
  info[0] = kFiltL; info[1] = kFiltB; info[2] = kFiltMaxS; info[3] = kFiltMaxPad;
  return AFX_OK;
}

extern "C" int afx_sosfiltfilt_host(const void* samples, int sample_fmt, int64_t n, const double* sos, int n_sections,
                                    int padlen, int mode, float preemph, float* out, double* out_peak, int32_t* out_status) {
  const char* who = "afx_sosfiltfilt_host: ";
  if (!sos || !out_status || n < 0 || (n > 0 && (!samples || !out))) { set_error(std::string(who) + "null/invalid argument"); return AFX_ERR_INVALID; }
  if (sample_fmt != AFX_FMT_F32 && sample_fmt != AFX_FMT_S16) { set_error(std::string(who) + "unknown sample format"); return AFX_ERR_INVALID; }
  if (mode != AFX_FILT_PLAIN && mode != AFX_FILT_EXPERIMENT) { set_error(std::string(who) + "unknown mode"); return AFX_ERR_INVALID; }
  if (n_sections < 1 || padlen < 0) { set_error(std::string(who) + "n_sections must be >= 1 and padlen >= 0"); return AFX_ERR_INVALID; }
  if (n_sections > kFiltMaxS || padlen > kFiltMaxPad) { set_error(std::string(who) + "more than 4 sections or padlen > 4096 is not supported"); return AFX_ERR_UNSUPPORTED; }
  if (n > ((int64_t)1 << 31)) { set_error(std::string(who) + "more than 2^31 samples is not supported"); return AFX_ERR_UNSUPPORTED; }
  FiltTab t;
  const char* why = "";
  if (!filt_build_tab(sos, n_sections, t, &why)) { set_error(std::string(who) + why); return AFX_ERR_INVALID; }
  if (out_peak) out_peak[0] = out_peak[1] = 0.0;
  if (n <= padlen) { *out_status = AFX_CLIP_TOO_SHORT; return AFX_OK; }
  FiltIn f{};
  f.in = samples; f.off = 0; f.n = n; f.fmt = sample_fmt; f.mode = mode; f.coef = -preemph; f.padlen = padlen;
  switch (n_sections) {
    case 1: host_clip<1>(t, f, out, out_peak, out_status); break;
    case 2: host_clip<2>(t, f, out, out_peak, out_status); break;
    case 3: host_clip<3>(t, f, out, out_peak, out_status); break;
    default: host_clip<4>(t, f, out, out_peak, out_status); break;
  }
  return AFX_OK;
}
