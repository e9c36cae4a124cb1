// Host-only part of the whole-clip DFT and the spectral term of the PESQ-like score: the cost record
// afx_specdist_batch / afx_clip_fft_batch cut a batch with, the stage twiddle table the kernels read, and the host
// executors -- one pair or one clip through the definitions of include/afx.h in plain C++: the same Bluestein, the same
// integer reduction of the chirp's phase, a radix-2 transform of the whole M points, sums in bin order.  They are the
// specification of the kernels, what the Python layer runs when no GPU is visible or a clip is over the device's limit,
// and part of the host-only sanitizer build.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "afx_cfft.h"
#include "afx_internal.h"

namespace afx {

void specdist_cost(int sample_fmt, int mem_kind, StftCost& cost) {
  const int64_t esz = sample_fmt == AFX_FMT_S16 ? 2 : 4, up = mem_kind == AFX_MEM_HOST ? esz : 0;
  cost = StftCost{};
  cost.per_sample = 128 + 2 * up;                         // 16 M of work + 16 M of filter spectrum, M < 4 n; both sides uploaded
  cost.per_clip = 256;                                    // the job record, the result, the flag, the staging's rounding
  cost.tile = kHpssTile;                                  // no kernel here works in frame tiles; the count only has to fit an int
  cost.tile_cap = INT32_MAX / 2;
}

namespace {

struct cplx { double re, im; };
inline cplx cmul(cplx a, cplx b) { return {a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }

// exp(-i pi num / den), num reduced to [0, 2 den) by the caller; evaluated in long double
inline cplx cispi_neg(uint64_t num, uint64_t den) {
  const long double th = 3.14159265358979323846264338327950288L * (long double)num / (long double)den;
  return {(double)cosl(th), (double)-sinl(th)};
}
inline cplx chirp(int64_t k, int64_t n) { return cispi_neg(((uint64_t)k * (uint64_t)k) % (uint64_t)(2 * n), (uint64_t)n); }

inline float host_sample(const void* p, int fmt, int64_t j) {
  return fmt == AFX_FMT_S16 ? (float)((const int16_t*)p)[j] * 0x1p-15f : ((const float*)p)[j];
}

// in place, M = 2^logM points: forwards natural -> bit-reversed, backwards bit-reversed -> natural (not scaled);
// tw[j] = exp(-2 pi i j / M), j < M / 2
void fft_dif(std::vector<cplx>& x, int logM, const std::vector<cplx>& tw) {
  const size_t M = (size_t)1 << logM;
  for (int h = logM - 1; h >= 0; --h) {
    const size_t half = (size_t)1 << h, step = (M >> 1) >> h;
    for (size_t g = 0; g < M; g += 2 * half)
      for (size_t j = 0; j < half; ++j) {
        const cplx a = x[g + j], b = x[g + j + half];
        x[g + j] = {a.re + b.re, a.im + b.im};
        x[g + j + half] = cmul({a.re - b.re, a.im - b.im}, tw[j * step]);
      }
  }
}
void fft_dit(std::vector<cplx>& x, int logM, const std::vector<cplx>& tw) {
  const size_t M = (size_t)1 << logM;
  for (int h = 0; h < logM; ++h) {
    const size_t half = (size_t)1 << h, step = (M >> 1) >> h;
    for (size_t g = 0; g < M; g += 2 * half)
      for (size_t j = 0; j < half; ++j) {
        const cplx w = tw[j * step], a = x[g + j], b = cmul(x[g + j + half], {w.re, -w.im});
        x[g + j] = {a.re + b.re, a.im + b.im};
        x[g + j + half] = {a.re - b.re, a.im - b.im};
      }
  }
}

constexpr int64_t kHostMaxN = (int64_t)1 << 27;           // 2^28 points of work, filter and twiddles at 16 bytes each

// Z = DFT_n(r + i d) (d == nullptr: no imaginary part); false when a sample is NaN / inf
bool bluestein(const void* r, const void* d, int fmt, int64_t n, std::vector<cplx>& Z) {
  const int logM = cf_log_m(n);
  const size_t M = (size_t)1 << logM;
  std::vector<cplx> tw(std::max<size_t>(M / 2, 1)), a(M, cplx{0.0, 0.0}), b(M, cplx{0.0, 0.0}), w((size_t)n);
  for (size_t j = 0; j < M / 2; ++j) tw[j] = cispi_neg(2 * j, M);
  for (int64_t k = 0; k < n; ++k) {
    const float x = host_sample(r, fmt, k), y = d ? host_sample(d, fmt, k) : 0.f;
    if (!std::isfinite(x) || !std::isfinite(y)) return false;
    w[k] = chirp(k, n);
    a[k] = cmul({(double)x, (double)y}, w[k]);
    b[k] = {w[k].re, -w[k].im};
    if (k) b[M - k] = b[k];
  }
  fft_dif(a, logM, tw);
  fft_dif(b, logM, tw);
  for (size_t i = 0; i < M; ++i) a[i] = cmul(a[i], b[i]);
  fft_dit(a, logM, tw);
  const double scale = 1.0 / (double)M;
  Z.resize((size_t)n);
  for (int64_t k = 0; k < n; ++k) {
    const cplx v = cmul(a[k], w[k]);
    Z[k] = {v.re * scale, v.im * scale};
  }
  return true;
}

}  // namespace

void cf_twiddle_table(double* out) {
  for (int j = 0; j < kCfTile / 2; ++j) {
    const cplx w = cispi_neg(2 * (uint64_t)j, kCfTile);
    out[2 * j] = w.re; out[2 * j + 1] = w.im;
  }
}

}  // namespace afx

using namespace afx;

extern "C" int afx_specdist_cost(int sample_fmt, int mem_kind, int64_t* cost) {
  if (!cost) { set_error("afx_specdist_cost: null argument"); return AFX_ERR_INVALID; }
  if ((sample_fmt != AFX_FMT_F32 && sample_fmt != AFX_FMT_S16) || (mem_kind != AFX_MEM_HOST && mem_kind != AFX_MEM_DEVICE)) {
    set_error("afx_specdist_cost: unknown sample format or memory kind");
    return AFX_ERR_INVALID;
  }
  StftCost c;
  specdist_cost(sample_fmt, mem_kind, c);
  const int64_t v[6] = {c.per_frame, c.per_tile, c.per_sample, c.per_clip, c.tile, c.tile_cap};
  std::memcpy(cost, v, sizeof(v));
  return AFX_OK;
}

extern "C" int afx_specdist_host(const void* ref, const void* deg, int sample_fmt, int64_t n_ref, int64_t n_deg,
                                 double* out_rec, int32_t* out_status) {
  const std::string who = "afx_specdist_host: ";
  if (!out_rec || !out_status || n_ref < 0 || n_deg < 0 || (std::min(n_ref, n_deg) > 0 && (!ref || !deg))) {
    set_error(who + "null/invalid argument");
    return AFX_ERR_INVALID;
  }
  if (sample_fmt != AFX_FMT_F32 && sample_fmt != AFX_FMT_S16) { set_error(who + "unknown sample format"); return AFX_ERR_INVALID; }
  const int64_t n = std::min(n_ref, n_deg);
  if (n > kHostMaxN) { set_error(who + "more than 2^27 samples are not supported"); return AFX_ERR_UNSUPPORTED; }
  std::fill(out_rec, out_rec + AFX_SPECDIST_N, std::nan(""));
  if (n == 0) { *out_status = AFX_CLIP_TOO_SHORT; return AFX_OK; }
  std::vector<cplx> Z;
  if (!bluestein(ref, deg, sample_fmt, n, Z)) { *out_status = AFX_CLIP_NONFINITE; return AFX_OK; }
  bool differs = false;                                                // equal sample for sample: D = R by definition
  for (int64_t k = 0; k < n && !differs; ++k) differs = host_sample(ref, sample_fmt, k) != host_sample(deg, sample_fmt, k);
  double a[3] = {0.0, 0.0, 0.0};
  for (int64_t k = 0; k < n; ++k) {
    const cplx p = Z[k], m = Z[k == 0 ? 0 : n - k];
    const double rr = 0.5 * (p.re + m.re), ri = 0.5 * (p.im - m.im), dr = 0.5 * (p.im + m.im), di = 0.5 * (m.re - p.re);
    const double R2 = rr * rr + ri * ri, D2 = differs ? dr * dr + di * di : R2, R = std::sqrt(R2), D = std::sqrt(D2);
    a[0] += std::fabs(R - D) / (R + 1e-10); a[1] += R2; a[2] += D2;
  }
  out_rec[0] = (double)n; out_rec[1] = a[0]; out_rec[2] = a[1]; out_rec[3] = a[2];
  *out_status = AFX_CLIP_OK;
  return AFX_OK;
}

extern "C" int afx_clip_fft_host(const void* samples, int sample_fmt, int64_t n, double* out, int32_t* out_status) {
  const std::string who = "afx_clip_fft_host: ";
  if (!out_status || n < 0 || (n > 0 && (!samples || !out))) { set_error(who + "null/invalid argument"); return AFX_ERR_INVALID; }
  if (sample_fmt != AFX_FMT_F32 && sample_fmt != AFX_FMT_S16) { set_error(who + "unknown sample format"); return AFX_ERR_INVALID; }
  if (n > kHostMaxN) { set_error(who + "more than 2^27 samples are not supported"); return AFX_ERR_UNSUPPORTED; }
  if (n == 0) { *out_status = AFX_CLIP_TOO_SHORT; return AFX_OK; }
  std::vector<cplx> Z;
  if (!bluestein(samples, nullptr, sample_fmt, n, Z)) {
    std::fill(out, out + 2 * (n / 2 + 1), std::nan(""));
    *out_status = AFX_CLIP_NONFINITE;
    return AFX_OK;
  }
  for (int64_t k = 0; k <= n / 2; ++k) { out[2 * k] = Z[k].re; out[2 * k + 1] = Z[k].im; }
  *out_status = AFX_CLIP_OK;
  return AFX_OK;
}
