// The host side of phase_vocoder / time_stretch (afx_pvoc.h): the shapes taken, the frame and length rules, the cost records
// afx_pvoc_batch / afx_time_stretch_batch cut a batch with, and afx_pvoc_host, one clip through the definition in plain
// C++ in the kernels' own summation order -- their specification.  No device.
#include <algorithm>
#include <climits>
#include <cmath>
#include <complex>
#include <cstring>
#include <string>
#include <vector>

#include "afx.h"
#include "afx_internal.h"
#include "afx_pvoc.h"

namespace afx {

int pvoc_check(int n_fft, int hop, const char** why) {
  if (n_fft < 2 || n_fft > 4096 || (n_fft & 1)) { *why = "n_fft must be even and in [2, 4096]"; return AFX_ERR_UNSUPPORTED; }
  if (hop < 1 || hop > n_fft) { *why = "hop must be in [1, n_fft]"; return AFX_ERR_UNSUPPORTED; }
  return AFX_OK;
}

bool pvoc_rate_ok(double rate) { return std::isfinite(rate) && rate > 0.0; }

bool pvoc_frames(int n_fft, int64_t T, double rate, int64_t* T_out) {
  const double t = std::ceil((double)T / rate);
  if (!(t * (double)stft_bins(n_fft) < 2147483648.0)) return false;
  *T_out = (int64_t)t;
  return true;
}

bool stretch_length(int64_t length, double rate, int64_t* n_out) {
  const double v = std::rint((double)length / rate);             // the default rounding mode: halves to even
  if (!(v <= 2147483648.0)) return false;
  *n_out = (int64_t)v;
  return true;
}

void pvoc_cost(int n_fft, int mem_kind, int out_mem_kind, StftCost& cost) {
  const int64_t bins = stft_bins(n_fft);
  cost = StftCost{};
  // per row, in or out: the angle and magnitude planes (in), the staged rows (host, either side), a tile's share of the sums
  cost.per_sample = bins * (8 + 4) + (mem_kind == AFX_MEM_HOST ? bins * 8 : 0) + (out_mem_kind == AFX_MEM_HOST ? bins * 8 : 0) +
                    (bins * 8 + kPvocTile - 1) / kPvocTile;
  cost.per_clip = 256 + (int64_t)sizeof(PvocClip) + bins * 8;    // the last tile is charged whole
  cost.tile = 16;
  cost.tile_cap = INT32_MAX / 2;
}

void stretch_cost(const afx_stft_opts& o, int sample_fmt, int mem_kind, int out_mem_kind, StftCost& cost) {
  const int64_t bins = stft_bins(o.n_fft), hop = o.hop;
  cost = StftCost{};
  // per unit of stretch_weight, whichever of its four terms it is: a row of D with its angle and magnitude, a row of the
  // result with its time row and a tile's share of the sums, a hop of samples in (upload, y) or out (the result, staged)
  const int64_t up = mem_kind != AFX_MEM_HOST ? 0 : sample_fmt == AFX_FMT_S16 ? 2 : 4;
  const int64_t row_in = bins * (8 + 8 + 4), row_out = bins * 8 + (int64_t)o.n_fft * 4 + (bins * 8 + kPvocTile - 1) / kPvocTile;
  const int64_t hop_in = hop * (4 + up), hop_out = hop * (4 + (out_mem_kind == AFX_MEM_HOST ? 4 : 0));
  cost.per_sample = std::max(std::max(row_in, row_out), std::max(hop_in, hop_out));
  cost.per_clip = 256 + (int64_t)(sizeof(PvocClip) + sizeof(StftClip) + sizeof(IstftClip) + sizeof(HpssClip)) + bins * 8;
  cost.tile = 16;
  cost.tile_cap = INT32_MAX / 2;
}

}  // namespace afx

using namespace afx;

static int fail(const char* who, int code, const char* why) {
  set_error(std::string(who) + ": " + why);
  return code;
}

static int pvoc_shape_arg(const char* who, int n_fft, int hop, double rate) {
  if (!pvoc_rate_ok(rate)) return fail(who, AFX_ERR_INVALID, "rate must be finite and > 0");
  const char* why = "";
  const int rc = pvoc_check(n_fft, hop, &why);
  return rc == AFX_OK ? rc : fail(who, rc, why);
}

extern "C" int afx_pvoc_frames(int n_fft, int hop, int64_t T, double rate, int64_t* T_out, int32_t* clip_status) {
  const char* who = "afx_pvoc_frames";
  if (!T_out || !clip_status) return fail(who, AFX_ERR_INVALID, "null argument");
  if (int rc = pvoc_shape_arg(who, n_fft, hop, rate)) return rc;
  if (T < 0 || T > (int64_t)1 << 31) return fail(who, AFX_ERR_INVALID, "T must be in [0, 2^31]");
  *T_out = 0;
  *clip_status = T == 0 ? AFX_CLIP_TOO_SHORT : AFX_CLIP_OK;
  if (T > 0 && !pvoc_frames(n_fft, T, rate, T_out)) return fail(who, AFX_ERR_UNSUPPORTED, "T_out x bins must be below 2^31");
  return AFX_OK;
}

extern "C" int afx_time_stretch_samples(const afx_stft_opts* opts, int64_t length, double rate, int64_t* T, int64_t* T_out,
                                        int64_t* n_out, int32_t* clip_status) {
  const char* who = "afx_time_stretch_samples";
  if (!opts || !T || !T_out || !n_out || !clip_status) return fail(who, AFX_ERR_INVALID, "null argument");
  if (!pvoc_rate_ok(rate)) return fail(who, AFX_ERR_INVALID, "rate must be finite and > 0");
  const char* why = "";
  if (int rc = stft_check_opts(*opts, &why)) return fail(who, rc, why);
  if (length < 0 || length > (int64_t)1 << 31) return fail(who, AFX_ERR_INVALID, "length must be in [0, 2^31]");
  *T = *T_out = *n_out = 0;
  stft_frames(*opts, length, T, clip_status);
  if (*clip_status != AFX_CLIP_OK) return AFX_OK;
  if (!stretch_length(length, rate, n_out)) return fail(who, AFX_ERR_INVALID, "length / rate must be at most 2^31");
  if (!pvoc_frames(opts->n_fft, *T, rate, T_out)) return fail(who, AFX_ERR_UNSUPPORTED, "T_out x bins must be below 2^31");
  return AFX_OK;
}

static void cost_out(const StftCost& c, int64_t* cost) {
  const int64_t v[6] = {c.per_frame, c.per_tile, c.per_sample, c.per_clip, c.tile, c.tile_cap};
  std::memcpy(cost, v, sizeof(v));
}

static bool mem_ok(int m) { return m == AFX_MEM_HOST || m == AFX_MEM_DEVICE; }

extern "C" int afx_pvoc_cost(int n_fft, int mem_kind, int out_mem_kind, int64_t* cost) {
  const char* who = "afx_pvoc_cost";
  if (!cost) return fail(who, AFX_ERR_INVALID, "null argument");
  if (!mem_ok(mem_kind) || !mem_ok(out_mem_kind)) return fail(who, AFX_ERR_INVALID, "unknown memory kind");
  if (int rc = pvoc_shape_arg(who, n_fft, 1, 1.0)) return rc;
  StftCost c;
  pvoc_cost(n_fft, mem_kind, out_mem_kind, c);
  cost_out(c, cost);
  return AFX_OK;
}

extern "C" int afx_time_stretch_cost(const afx_stft_opts* opts, int sample_fmt, int mem_kind, int out_mem_kind, int64_t* cost) {
  const char* who = "afx_time_stretch_cost";
  if (!opts || !cost) return fail(who, AFX_ERR_INVALID, "null argument");
  if ((sample_fmt != AFX_FMT_F32 && sample_fmt != AFX_FMT_S16) || !mem_ok(mem_kind) || !mem_ok(out_mem_kind))
    return fail(who, AFX_ERR_INVALID, "unknown sample format or memory kind");
  const char* why = "";
  if (int rc = stft_check_opts(*opts, &why)) return fail(who, rc, why);
  StftCost c;
  stretch_cost(*opts, sample_fmt, mem_kind, out_mem_kind, c);
  cost_out(c, cost);
  return AFX_OK;
}

// The definition, one clip: the same step rule, increments, tile-ordered sums and reduction as the kernels; libm's atan2,
// cos and sin where the device has its own.
extern "C" int afx_pvoc_host(const void* spec, int64_t T, double rate, int n_fft, int hop, void* out, int32_t* clip_status) {
  const char* who = "afx_pvoc_host";
  if (!clip_status) return fail(who, AFX_ERR_INVALID, "null argument");
  if (int rc = pvoc_shape_arg(who, n_fft, hop, rate)) return rc;
  if (T < 0 || T > (int64_t)1 << 31) return fail(who, AFX_ERR_INVALID, "T must be in [0, 2^31]");
  *clip_status = AFX_CLIP_TOO_SHORT;
  if (T == 0) return AFX_OK;
  int64_t T_out = 0;
  if (!pvoc_frames(n_fft, T, rate, &T_out)) return fail(who, AFX_ERR_UNSUPPORTED, "T_out x bins must be below 2^31");
  if (!spec || !out) return fail(who, AFX_ERR_INVALID, "null spec / out");
  const int bins = stft_bins(n_fft);
  const float* D = (const float*)spec;
  float* P = (float*)out;
  std::vector<double> ang((size_t)T * bins);
  std::vector<float> mag((size_t)T * bins);
  bool bad = false;
  for (int64_t e = 0; e < T * bins; ++e) {
    const float re = D[2 * e], im = D[2 * e + 1];
    bad = bad || !(std::isfinite(re) && std::isfinite(im));
    ang[(size_t)e] = std::atan2((double)im, (double)re);
    const float a = re * re, b = im * im;
    mag[(size_t)e] = std::sqrt(a + b);
  }
  if (bad) {
    std::memset(P, 0, (size_t)T_out * bins * 2 * sizeof(float));
    *clip_status = AFX_CLIP_NONFINITE;
    return AFX_OK;
  }
  auto A = [&](int64_t j, int b) { return j < T ? ang[(size_t)(j * bins + b)] : 0.0; };
  auto M = [&](int64_t j, int b) { return j < T ? mag[(size_t)(j * bins + b)] : 0.f; };
  for (int b = 0; b < bins; ++b) {
    const double phi = pvoc_phi(hop, n_fft, b), phi_r = pvoc_wrap(phi);
    double acc = A(0, b);
    for (int64_t t0 = 0; t0 < T_out; t0 += kPvocTile) {
      const int64_t t1 = std::min<int64_t>(t0 + kPvocTile, T_out);
      double sum = 0.0;
      for (int64_t t = t0; t < t1; ++t) {
        int64_t j;
        double a;
        pvoc_step(t, rate, &j, &a);
        const float m = pvoc_mag(M(j, b), M(j + 1, b), a);
        const double ph = acc + sum;
        P[2 * (t * bins + b)] = (float)((double)m * std::cos(ph));
        P[2 * (t * bins + b) + 1] = (float)((double)m * std::sin(ph));
        sum += pvoc_inc(A(j, b), A(j + 1, b), phi, phi_r);
      }
      acc = pvoc_wrap(acc + sum);
    }
  }
  *clip_status = AFX_CLIP_OK;
  return AFX_OK;
}
