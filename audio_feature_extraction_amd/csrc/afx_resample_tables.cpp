// Host side of the resampler: the filter wavio._resample_filter designs (scipy.signal.kaiserord / firwin with a Kaiser
// window, unity DC gain) and the grouped tap table of the kernel (afx_resample.h).  No device code: part of the host
// sanitizer build.
#include <algorithm>
#include <cmath>
#include <numeric>
#include <string>

#include "afx.h"
#include "afx_internal.h"
#include "afx_resample.h"

namespace afx {

static int64_t floor_div(int64_t a, int64_t b) { int64_t q = a / b; return (a % b != 0 && ((a < 0) != (b < 0))) ? q - 1 : q; }
static int64_t ceil_div(int64_t a, int64_t b) { return -floor_div(-a, b); }

int64_t resample_out_len(int64_t n, int up, int down) { return n <= 0 ? 0 : (n * up + down - 1) / down; }

// modified Bessel function I0 by its power series (x <= 13 here: 40 terms leave nothing above 1e-17 of the sum)
static double bessel_i0(double x) {
  const double q = 0.25 * x * x;
  double term = 1.0, sum = 1.0;
  for (int k = 1; k < 200; ++k) {
    term *= q / ((double)k * (double)k);
    sum += term;
    if (term < 1e-18 * sum) break;
  }
  return sum;
}

int resample_design(int sr_in, int sr_out, RsDesign& d, bool want_taps, std::string& why) {
  if (sr_in <= 0 || sr_out <= 0) { why = "sample rates must be positive"; return AFX_ERR_INVALID; }
  const int g = std::gcd(sr_in, sr_out);
  d.up = sr_out / g; d.down = sr_in / g;
  d.h.clear();
  if (d.up == d.down) { d.n_taps = 1; d.half = 0; if (want_taps) d.h.assign(1, 1.0); return AFX_OK; }
  // wavio._resample_filter, expression for expression (the tap count is a ceil of these doubles)
  const double fs = (double)d.up;
  const double nyq_low = 0.5 * std::min(1.0, (double)d.up / (double)d.down);
  const double width = (1.0 - 0.913) * nyq_low;
  const double A = 125.0;
  const double beta = 0.1102 * (A - 8.7);                                   // kaiser_beta, A > 50
  const double wn = width / (0.5 * fs);
  const double nt = (A - 7.95) / 2.285 / (M_PI * wn) + 1.0;                 // kaiserord
  if (!(nt < 4.0 * kRsMaxTaps)) { why = "the filter of this rate pair has more than 2^21 taps"; return AFX_ERR_UNSUPPORTED; }
  int64_t n = (int64_t)std::ceil(nt);
  n |= 1;
  d.n_taps = (int)n; d.half = (int)((n - 1) / 2);
  if (d.up > kRsMaxUp || n > kRsMaxTaps) {
    why = "rate pair " + std::to_string(sr_in) + " -> " + std::to_string(sr_out) + " (up " + std::to_string(d.up) + ", " +
          std::to_string(n) + " taps) is beyond the resampler's table bounds (up <= 2048, taps <= 2^21)";
    return AFX_ERR_UNSUPPORTED;
  }
  if (!want_taps) return AFX_OK;
  const double cutoff = (0.5 * (0.913 + 1.0) * nyq_low) / (0.5 * fs);       // firwin: in units of the Nyquist rate
  const double alpha = 0.5 * (double)(n - 1);
  const double i0b = bessel_i0(beta);
  d.h.resize((size_t)n);
  long double sum = 0.0L;
  for (int64_t k = 0; k < n; ++k) {
    const double m = (double)k - alpha;
    const double x = cutoff * m;
    const double sinc = x == 0.0 ? 1.0 : std::sin(M_PI * x) / (M_PI * x);
    const double r = m / alpha;
    const double win = bessel_i0(beta * std::sqrt(std::max(0.0, 1.0 - r * r))) / i0b;
    d.h[(size_t)k] = cutoff * sinc * win;
    sum += d.h[(size_t)k];
  }
  const double s = (double)sum;
  for (double& v : d.h) v /= s;
  return AFX_OK;
}

int resample_tables(int up, int down, const double* h, int n_taps, RsTables& t, std::string& why) {
  if (up < 1 || down < 1 || !h || n_taps < 1 || !(n_taps & 1)) { why = "the tap count must be odd and positive"; return AFX_ERR_INVALID; }
  if (up > kRsMaxUp || n_taps > kRsMaxTaps) { why = "up > 2048 or more than 2^21 taps"; return AFX_ERR_UNSUPPORTED; }
  RsParams& p = t.p;
  const int64_t L = n_taps, half = (L - 1) / 2;
  const int pl = up >= kRsGroup ? 1 : (kRsGroup + up - 1) / up;
  p.up = up; p.down = down; p.opp = pl * up;
  if ((int64_t)pl * down > kRsMaxRow) { why = "down too large for the resampler's LDS tile (ceil(8 / up) * down <= 2048)"; return AFX_ERR_UNSUPPORTED; }
  p.rw = pl * down; p.stride = p.rw | 1;
  p.n_groups = (p.opp + kRsGroup - 1) / kRsGroup;
  std::vector<int64_t> lo((size_t)p.n_groups);
  int64_t n_steps = 1;
  for (int g = 0; g < p.n_groups; ++g) {
    const int64_t o0 = (int64_t)g * kRsGroup, o1 = std::min<int64_t>(o0 + kRsGroup, p.opp) - 1;
    lo[g] = ceil_div(o0 * down + half - (L - 1), up);                       // first t with a tap of output o0
    const int64_t hi = floor_div(o1 * down + half, up);                     // last t with a tap of output o1
    n_steps = std::max(n_steps, hi - lo[g] + 1);
  }
  int64_t tmin = 0, tmax = 0;
  for (int g = 0; g < p.n_groups; ++g) { tmin = std::min(tmin, lo[g]); tmax = std::max(tmax, lo[g] + n_steps - 1); }
  p.n_steps = (int)n_steps;
  p.r_back = (int)ceil_div(-tmin, p.rw);
  const int r_fwd = (int)floor_div(tmax, p.rw);
  const int halo = p.r_back + r_fwd;
  const int64_t row_bytes = (int64_t)p.stride * 4;
  const int64_t fit = kRsLdsBytes / row_bytes - halo;                       // super-periods one workgroup can hold
  if (fit < 8) { why = "no LDS tile holds this rate pair's filter span"; return AFX_ERR_UNSUPPORTED; }
  p.lanes = (int)std::min<int64_t>(64, fit);
  // small rows: several wave passes per tile (the halo is loaded once), within 48 KB so that a few workgroups share a CU
  p.tc = 1;
  if (p.lanes == 64) p.tc = (int)std::max<int64_t>(1, std::min<int64_t>(16, (48 * 1024 / row_bytes - halo) / 64));
  p.tile_sp = p.lanes * p.tc;
  p.rows = p.tile_sp + halo;
  const int units = p.n_groups * p.tc, rounds = (units + 15) / 16;
  p.n_waves = (units + rounds - 1) / rounds;
  t.tstart.resize((size_t)p.n_groups);
  t.G.assign((size_t)p.n_groups * n_steps * kRsGroup, 0.0);
  for (int g = 0; g < p.n_groups; ++g) {
    t.tstart[g] = (int32_t)lo[g];
    for (int64_t s = 0; s < n_steps; ++s)
      for (int j = 0; j < kRsGroup; ++j) {
        const int64_t o = (int64_t)g * kRsGroup + j, idx = o * down + half - (lo[g] + s) * up;
        if (o < p.opp && idx >= 0 && idx < L) t.G[((size_t)g * n_steps + s) * kRsGroup + j] = (double)up * h[idx];
      }
  }
  return AFX_OK;
}

}  // namespace afx

using namespace afx;

extern "C" int afx_resample_design(int sr_in, int sr_out, int32_t* info, double* taps) {
  RsDesign d;
  std::string why;
  const int rc = resample_design(sr_in, sr_out, d, taps != nullptr, why);
  if (rc != AFX_OK) { set_error("afx_resample_design: " + why); return rc; }
  if (info) { info[0] = d.up; info[1] = d.down; info[2] = d.n_taps; info[3] = d.half; }
  if (taps) std::copy(d.h.begin(), d.h.end(), taps);
  return AFX_OK;
}
