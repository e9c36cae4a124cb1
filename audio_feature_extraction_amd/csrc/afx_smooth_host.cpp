// Host side of the sample-domain smoothers and of the energy and ZCR groups (layout and arithmetic: afx_smooth.h): the
// Savitzky-Golay tables, the argument refusals, and the host executors afx_medfilt_host, afx_savgol_host and
// afx_energy_zcr_host -- one clip through the operations the kernels of afx_smooth.hip run, in the same order, on the CPU.
// No device code: part of the sanitizer build.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "afx.h"
#define AFX_FILT_HOST_ONLY
#include "afx_smooth.h"
#include "afx_internal.h"

namespace afx {

const char* medfilt_refusal(int K, int* code) {
  *code = AFX_ERR_INVALID;
  if (K < 1) return "kernel_size must be positive";
  if (K % 2 == 0) return "Each element of kernel_size should be odd.";
  *code = AFX_ERR_UNSUPPORTED;
  if (K > kSmMaxK) return "kernel sizes above 31 are not supported";
  return nullptr;
}

const char* savgol_refusal(int W, int P, int deriv, double delta, int* code) {
  *code = AFX_ERR_INVALID;
  if (W < 1) return "window_length must be positive";
  if (P < 0) return "polyorder must be >= 0";
  if (P >= W) return "polyorder must be less than window_length.";
  if (deriv < 0) return "deriv must be >= 0";
  if (!std::isfinite(delta) || delta == 0.0) return "delta must be finite and not 0";
  *code = AFX_ERR_UNSUPPORTED;
  if (W % 2 == 0) return "an even window_length is not supported";
  if (W < 3 || W > kSmMaxK) return "window lengths outside 3 .. 31 are not supported";
  if (P > kSgMaxP) return "polynomial orders above 5 are not supported";
  if (deriv > kSgMaxDeriv) return "derivatives above the second are not supported";
  return nullptr;
}

const char* ez_refusal(int sr, int frame_length, int hop_length, int flags, int* code) {
  *code = AFX_ERR_INVALID;
  if (sr < 1) return "the sample rate must be positive";
  if ((flags & AFX_EZ_PREPROCESS) && sr <= 400) return "the preprocess needs a sample rate above 400 Hz";
  if (flags & ~(AFX_EZ_PREPROCESS | AFX_EZ_ENERGY | AFX_EZ_ZCR)) return "unknown flags";
  if (frame_length < 64 || frame_length > 2048 || (frame_length & (frame_length - 1))) return "frame_length must be a power of two in [64, 2048]";
  if (hop_length < 1) return "hop_length must be positive";
  return nullptr;
}

// The least-squares polynomial of degree P through W samples at u_k = (k - h) / h in [-1, 1]: pinv[j][k] is the weight of
// sample k in the coefficient of u^j.  The columns 1, u, u^2, .. are orthogonalised by modified Gram-Schmidt, twice (on the
// scaled abscissa the Vandermonde matrix of degree 5 has a condition number of a few tens), then R b = Q^T e_k is solved
// by back substitution.
static void sg_pinv(int W, int P, double pinv[kSgMaxP + 1][kSgRow]) {
  const int h = W / 2, m = P + 1;
  double Q[kSgMaxP + 1][kSgRow], R[kSgMaxP + 1][kSgMaxP + 1] = {};
  for (int j = 0; j < m; ++j)
    for (int k = 0; k < W; ++k) Q[j][k] = std::pow((double)(k - h) / (double)h, j);
  for (int j = 0; j < m; ++j) {
    for (int pass = 0; pass < 2; ++pass)
      for (int i = 0; i < j; ++i) {
        double d = 0.0;
        for (int k = 0; k < W; ++k) d += Q[i][k] * Q[j][k];
        for (int k = 0; k < W; ++k) Q[j][k] -= d * Q[i][k];
        R[i][j] += d;
      }
    double nn = 0.0;
    for (int k = 0; k < W; ++k) nn += Q[j][k] * Q[j][k];
    nn = std::sqrt(nn);
    for (int k = 0; k < W; ++k) Q[j][k] /= nn;
    R[j][j] = nn;
  }
  for (int k = 0; k < W; ++k)
    for (int j = m - 1; j >= 0; --j) {
      double b = Q[j][k];
      for (int i = j + 1; i < m; ++i) b -= R[j][i] * pinv[i][k];
      pinv[j][k] = b / R[j][j];
    }
}

// weights of the deriv-th derivative (per delta^deriv) of the fitted polynomial at sample position pos (0 .. W - 1)
static void sg_row(int W, int P, int deriv, double delta, const double pinv[kSgMaxP + 1][kSgRow], int pos, double* row) {
  const int h = W / 2;
  const double u = (double)(pos - h) / (double)h, scale = std::pow((double)h * delta, deriv);
  for (int k = 0; k < W; ++k) {
    double a = 0.0;
    for (int j = P; j >= deriv; --j) {         // Horner over the differentiated polynomial
      double f = 1.0;
      for (int q = 0; q < deriv; ++q) f *= (double)(j - q);
      a = a * u + f * pinv[j][k];
    }
    row[k] = a / scale;
  }
}

void savgol_build_tab(int W, int P, int deriv, double delta, SgTab& t) {
  std::memset(&t, 0, sizeof(t));
  const int h = W / 2;
  t.W = W; t.h = h;
  double pinv[kSgMaxP + 1][kSgRow] = {};
  sg_pinv(W, P, pinv);
  sg_row(W, P, deriv, delta, pinv, h, t.t);
  for (int r = 0; r < h; ++r) {
    sg_row(W, P, deriv, delta, pinv, r, t.left[r]);
    sg_row(W, P, deriv, delta, pinv, h + 1 + r, t.right[r]);
  }
}

namespace {

bool clip_is_finite(const SmSrc& s, int64_t n) {
  for (int64_t i = 0; i < n; ++i)
    if (!(std::fabs(sm_raw(s, i)) <= FLT_MAX)) return false;
  return true;
}

void medfilt_clip(const SmSrc& s, int64_t n, int K, float* out) {
  const int h = K / 2;
  float w[kSmMaxK];
  for (int64_t i = 0; i < n; ++i) {
    for (int k = 0; k < K; ++k) {
      const int64_t j = i - h + k;
      w[k] = j >= 0 && j < n ? sm_raw(s, j) : 0.0f;
    }
    out[i] = sm_median(w, K);
  }
}

void savgol_clip(const SgTab& t, const SmSrc& s, int64_t n, float* out) {
  for (int64_t i = 0; i < n; ++i) {
    if (i < t.h || i >= n - t.h) out[i] = sg_edge(&t, s, n, i);
    else out[i] = (float)sg_dot(t.t, SmSrcAt{s, i - t.h}, t.W);
  }
}

// sum over t of term(a, t) in the order of the statistics kernel
template <typename F>
double stat_sum(int64_t T, F term) {
  double p[kEzStatLanes];
  for (int j = 0; j < kEzStatLanes; ++j) {
    double a = 0.0;
    for (int64_t t = j; t < T; t += kEzStatLanes) a = term(a, t);
    p[j] = a;
  }
  return sm_tree_sum(p, kEzStatLanes);
}

void mean_std(const std::vector<double>& v, double* mean, double* sd) {
  const int64_t T = (int64_t)v.size();
  const double m = stat_sum(T, [&](double a, int64_t t) { return a + v[t]; }) / (double)T;
  const double q = stat_sum(T, [&](double a, int64_t t) { const double d = v[t] - m; return std::fma(d, d, a); });
  *mean = m; *sd = std::sqrt(q / (double)T);
}

}  // namespace
}  // namespace afx

using namespace afx;

extern "C" int afx_smooth_geometry(int32_t* info) {
  if (!info) { set_error("afx_smooth_geometry: null argument"); return AFX_ERR_INVALID; }
  info[0] = kSmTile; info[1] = kSmMaxK; info[2] = kSgMaxP; info[3] = kSgMaxDeriv;
  return AFX_OK;
}

extern "C" int afx_savgol_tables(int window_length, int polyorder, int deriv, double delta, double* coeffs, double* left,
                                 double* right) {
  const std::string who = "afx_savgol_tables: ";
  int code;
  if (const char* why = savgol_refusal(window_length, polyorder, deriv, delta, &code)) { set_error(who + why); return code; }
  if (!coeffs || !left || !right) { set_error(who + "null argument"); return AFX_ERR_INVALID; }
  SgTab t;
  savgol_build_tab(window_length, polyorder, deriv, delta, t);
  const int W = window_length, h = W / 2;
  for (int k = 0; k < W; ++k) coeffs[k] = t.t[W - 1 - k];
  for (int r = 0; r < h; ++r)
    for (int k = 0; k < W; ++k) { left[r * W + k] = t.left[r][k]; right[r * W + k] = t.right[r][k]; }
  return AFX_OK;
}

static int check_host_clip(const std::string& who, const void* samples, int sample_fmt, int64_t n, const float* out,
                           const int32_t* out_status) {
  if (!out_status || n < 0 || (n > 0 && (!samples || !out))) { set_error(who + "null/invalid argument"); return AFX_ERR_INVALID; }
  if (sample_fmt != AFX_FMT_F32 && sample_fmt != AFX_FMT_S16) { set_error(who + "unknown sample format"); return AFX_ERR_INVALID; }
  if (n > ((int64_t)1 << 31)) { set_error(who + "more than 2^31 samples is not supported"); return AFX_ERR_UNSUPPORTED; }
  return AFX_OK;
}

extern "C" int afx_medfilt_host(const void* samples, int sample_fmt, int64_t n, int kernel_size, float* out, int32_t* out_status) {
  const std::string who = "afx_medfilt_host: ";
  int code;
  if (const char* why = medfilt_refusal(kernel_size, &code)) { set_error(who + why); return code; }
  if (int rc = check_host_clip(who, samples, sample_fmt, n, out, out_status)) return rc;
  if (n == 0) { *out_status = AFX_CLIP_TOO_SHORT; return AFX_OK; }
  const SmSrc s{samples, 0, sample_fmt};
  if (!clip_is_finite(s, n)) { *out_status = AFX_CLIP_NONFINITE; return AFX_OK; }
  medfilt_clip(s, n, kernel_size, out);
  *out_status = AFX_CLIP_OK;
  return AFX_OK;
}

extern "C" int afx_savgol_host(const void* samples, int sample_fmt, int64_t n, int window_length, int polyorder, int deriv,
                               double delta, float* out, int32_t* out_status) {
  const std::string who = "afx_savgol_host: ";
  int code;
  if (const char* why = savgol_refusal(window_length, polyorder, deriv, delta, &code)) { set_error(who + why); return code; }
  if (int rc = check_host_clip(who, samples, sample_fmt, n, out, out_status)) return rc;
  if (n < window_length) { *out_status = AFX_CLIP_TOO_SHORT; return AFX_OK; }
  const SmSrc s{samples, 0, sample_fmt};
  if (!clip_is_finite(s, n)) { *out_status = AFX_CLIP_NONFINITE; return AFX_OK; }
  SgTab t;
  savgol_build_tab(window_length, polyorder, deriv, delta, t);
  savgol_clip(t, s, n, out);
  *out_status = AFX_CLIP_OK;
  return AFX_OK;
}

extern "C" int afx_energy_zcr_host(const float* samples, int64_t n, int frame_length, int hop_length, int flags,
                                   double* out_rec, int32_t* out_status) {
  const std::string who = "afx_energy_zcr_host: ";
  int code;
  if (const char* why = ez_refusal(1, frame_length, hop_length, flags & ~AFX_EZ_PREPROCESS, &code)) { set_error(who + why); return code; }
  if (!out_rec || !out_status || n < 0 || (n > 0 && !samples)) { set_error(who + "null/invalid argument"); return AFX_ERR_INVALID; }
  if (n > ((int64_t)1 << 31)) { set_error(who + "more than 2^31 samples is not supported"); return AFX_ERR_UNSUPPORTED; }
  std::fill(out_rec, out_rec + AFX_EZ_N, std::nan(""));
  if (n == 0) { *out_status = AFX_CLIP_TOO_SHORT; return AFX_OK; }
  const SmSrc y{samples, 0, AFX_FMT_F32};
  if (!clip_is_finite(y, n)) { *out_status = AFX_CLIP_NONFINITE; return AFX_OK; }
  const EzFrame fr = ez_framing(n, frame_length, hop_length);
  const int64_t T = fr.T;
  out_rec[AFX_EZ_T] = (double)T; out_rec[AFX_EZ_FL] = fr.fl; out_rec[AFX_EZ_HOP] = fr.hop;
  std::vector<double> v((size_t)T);
  if (flags & AFX_EZ_ENERGY) {
    for (int64_t t = 0; t < T; ++t) {
      const int64_t g0 = t * fr.hop - fr.fl / 2;
      double p[kEzFrameLanes];
      for (int l = 0; l < kEzFrameLanes; ++l) {
        double a = 0.0;
        for (int k = l; k < fr.fl; k += kEzFrameLanes) {
          const int64_t j = g0 + k;
          const double x = j >= 0 && j < n ? (double)samples[j] : 0.0;
          a = std::fma(x, x, a);
        }
        p[l] = a;
      }
      v[t] = std::sqrt(sm_tree_sum(p, kEzFrameLanes) / (double)fr.fl);
    }
    mean_std(v, &out_rec[AFX_EZ_ENERGY_MEAN], &out_rec[AFX_EZ_ENERGY_STD]);
    int64_t k0, k1;
    double g;
    ez_p10_index(T, &k0, &k1, &g);
    std::vector<double> s(v);
    std::sort(s.begin(), s.end());
    out_rec[AFX_EZ_ENERGY_P10] = ez_lerp(s[k0], s[k1], g);
  }
  if (flags & AFX_EZ_ZCR) {
    std::vector<float> m((size_t)n), sm;
    medfilt_clip(y, n, 3, m.data());
    if (n > 11) {
      SgTab tab;
      savgol_build_tab(11, 3, 0, 1.0, tab);
      sm.resize((size_t)n);
      savgol_clip(tab, SmSrc{m.data(), 0, AFX_FMT_F32}, n, sm.data());
    } else {
      sm = m;
    }
    float peak = 0.0f;
    for (int64_t i = 0; i < n; ++i) peak = std::max(peak, std::fabs(sm[i]));
    out_rec[AFX_EZ_PEAK_SMOOTH] = (double)peak;
    std::vector<uint8_t> neg((size_t)n);
    for (int64_t i = 0; i < n; ++i) neg[i] = ez_neg(sm[i], peak) ? 1 : 0;
    for (int64_t t = 0; t < T; ++t) {
      const int64_t g0 = t * fr.hop - fr.fl / 2;
      auto at = [&](int64_t j) -> int { return neg[j < 0 ? 0 : (j >= n ? n - 1 : j)]; };
      int cnt = 0;
      for (int k = 1; k < fr.fl; ++k) cnt += at(g0 + k) != at(g0 + k - 1) ? 1 : 0;
      v[t] = (double)cnt / (double)fr.fl;
    }
    double sd;
    mean_std(v, &out_rec[AFX_EZ_ZCR_MEAN], &sd);
    out_rec[AFX_EZ_ZCR_STD] = sd;
    const int w = T < kEzWin ? (int)T : kEzWin;
    double local = sd;
    if (w > 1) {
      const int64_t nw = T - w + 1;
      local = stat_sum(nw, [&](double a, int64_t i) { return a + ez_window_std(v.data() + i, w); }) / (double)nw;
    }
    out_rec[AFX_EZ_ZCR_LOCAL] = local;
  }
  *out_status = AFX_CLIP_OK;
  return AFX_OK;
}
