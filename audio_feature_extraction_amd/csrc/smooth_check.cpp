// Stand-alone check of the host side of the smoothers and of the energy and ZCR groups (afx_smooth_host.cpp: afx_savgol_tables,
// afx_medfilt_host, afx_savgol_host, afx_energy_zcr_host), built with AddressSanitizer + UBSan by `make smooth-check` and run
// on the CPU: the tables of every window, order and derivative into exactly sized buffers, and the executors over the lengths
// around the windows, the tile and the framing switches with exactly sized heap buffers for the samples and the result (an
// index past either is an ASan report).  The results are checked for what needs no reference: statuses, refusals, the taps'
// moments, a constant and a ramp through both filters, the records' framing.
// Exit status 0: every check held.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "afx.h"

namespace {

int g_fail = 0;
#define CHECK(cond)                                                              \
  do {                                                                           \
    if (!(cond)) { std::fprintf(stderr, "smooth_check: line %d: %s\n", __LINE__, #cond); ++g_fail; } \
  } while (0)

uint32_t g_seed = 2463534242u;
float noise() {
  g_seed = g_seed * 1664525u + 1013904223u;
  return (float)((int)(g_seed >> 17) - 16384) / 16384.0f;
}

}  // namespace

int main() {
  int32_t geo[4] = {0, 0, 0, 0};
  CHECK(afx_smooth_geometry(geo) == AFX_OK);
  const int tile = geo[0], maxw = geo[1];
  CHECK(tile >= 64 && maxw == 31 && geo[2] == 5 && geo[3] == 2);
  CHECK(afx_smooth_geometry(nullptr) == AFX_ERR_INVALID);

  // tables: sum c = 1 (deriv 0) or 0, and the first moment of the first derivative's taps is -1 in convolution order
  for (int W = 3; W <= maxw; W += 2)
    for (int P = 0; P <= 5 && P < W; ++P)
      for (int d = 0; d <= 2; ++d) {
        std::vector<double> c((size_t)W, -7.0), l((size_t)(W / 2) * W, -7.0), r((size_t)(W / 2) * W, -7.0);
        CHECK(afx_savgol_tables(W, P, d, 1.0, c.data(), l.data(), r.data()) == AFX_OK);
        double s0 = 0.0, s1 = 0.0;
        for (int k = 0; k < W; ++k) { CHECK(std::isfinite(c[k]) && c[k] != -7.0); s0 += c[k]; s1 += c[k] * (k - W / 2); }
        for (double v : l) CHECK(std::isfinite(v) && v != -7.0);
        for (double v : r) CHECK(std::isfinite(v) && v != -7.0);
        CHECK(std::fabs(s0 - (d == 0 ? 1.0 : 0.0)) < 1e-12);
        if (d == 1 && P >= 1) CHECK(std::fabs(s1 + 1.0) < 1e-12);
        for (int q = 0; q < W / 2; ++q) {          // every edge row has the same zeroth moment
          double e0 = 0.0, f0 = 0.0;
          for (int k = 0; k < W; ++k) { e0 += l[(size_t)q * W + k]; f0 += r[(size_t)q * W + k]; }
          CHECK(std::fabs(e0 - (d == 0 ? 1.0 : 0.0)) < 1e-11 && std::fabs(f0 - (d == 0 ? 1.0 : 0.0)) < 1e-11);
        }
      }
  {
    std::vector<double> c(33), l(16 * 33), r(16 * 33);
    CHECK(afx_savgol_tables(33, 3, 0, 1.0, c.data(), l.data(), r.data()) == AFX_ERR_UNSUPPORTED);
    CHECK(afx_savgol_tables(10, 3, 0, 1.0, c.data(), l.data(), r.data()) == AFX_ERR_UNSUPPORTED);
    CHECK(afx_savgol_tables(1, 0, 0, 1.0, c.data(), l.data(), r.data()) == AFX_ERR_UNSUPPORTED);
    CHECK(afx_savgol_tables(11, 6, 0, 1.0, c.data(), l.data(), r.data()) == AFX_ERR_UNSUPPORTED);
    CHECK(afx_savgol_tables(11, 3, 3, 1.0, c.data(), l.data(), r.data()) == AFX_ERR_UNSUPPORTED);
    CHECK(afx_savgol_tables(5, 5, 0, 1.0, c.data(), l.data(), r.data()) == AFX_ERR_INVALID);
    CHECK(afx_savgol_tables(0, 0, 0, 1.0, c.data(), l.data(), r.data()) == AFX_ERR_INVALID);
    CHECK(afx_savgol_tables(11, -1, 0, 1.0, c.data(), l.data(), r.data()) == AFX_ERR_INVALID);
    CHECK(afx_savgol_tables(11, 3, -1, 1.0, c.data(), l.data(), r.data()) == AFX_ERR_INVALID);
    CHECK(afx_savgol_tables(11, 3, 0, 0.0, c.data(), l.data(), r.data()) == AFX_ERR_INVALID);
    CHECK(afx_savgol_tables(11, 3, 0, NAN, c.data(), l.data(), r.data()) == AFX_ERR_INVALID);
    CHECK(afx_savgol_tables(11, 3, 0, 1.0, nullptr, l.data(), r.data()) == AFX_ERR_INVALID);
  }

  // the median over the lengths around every window and the tile, both formats
  const int kernels[] = {1, 3, 5, 7, 25, 31};
  for (int K : kernels) {
    const int h = K / 2;
    const int64_t lens[] = {0, 1, 2, h, h + 1, K, tile - 1, tile, tile + 1, tile + h, 2 * (int64_t)tile + 1};
    for (int64_t n : lens)
      for (int fmt = 0; fmt < 2; ++fmt) {
        std::vector<float> xf((size_t)(fmt == AFX_FMT_F32 ? n : 0));
        std::vector<int16_t> xs((size_t)(fmt == AFX_FMT_S16 ? n : 0));
        float lo = 0.0f, hi = 0.0f;                // the padding's zero is a candidate
        for (int64_t i = 0; i < n; ++i) {
          const float v = noise();
          float got;
          if (fmt == AFX_FMT_F32) got = xf[i] = v; else { xs[i] = (int16_t)(v * 8192.0f); got = (float)xs[i] / 32768.0f; }
          lo = std::fmin(lo, got); hi = std::fmax(hi, got);
        }
        std::vector<float> out((size_t)n, -3.0f);
        int32_t st = -1;
        const void* x = fmt == AFX_FMT_F32 ? (const void*)xf.data() : (const void*)xs.data();
        CHECK(afx_medfilt_host(x, fmt, n, K, out.data(), &st) == AFX_OK);
        CHECK(st == (n == 0 ? AFX_CLIP_TOO_SHORT : AFX_CLIP_OK));
        for (float v : out) CHECK(v >= lo && v <= hi && !std::signbit(v == 0.0f ? v : 1.0f));
      }
  }
  {
    std::vector<float> x(40, 0.25f), out(40, -3.0f);
    int32_t st = -1;
    CHECK(afx_medfilt_host(x.data(), AFX_FMT_F32, 40, 5, out.data(), &st) == AFX_OK && st == AFX_CLIP_OK);
    for (float v : out) CHECK(v == 0.25f);         // at most two of five are padding
    CHECK(afx_medfilt_host(x.data(), AFX_FMT_F32, 2, 5, out.data(), &st) == AFX_OK && st == AFX_CLIP_OK);
    CHECK(out[0] == 0.0f && out[1] == 0.0f && out[2] == 0.25f);   // three of five are: a kernel longer than the clip is legal
    x[39] = INFINITY;
    out.assign(40, -3.0f);
    CHECK(afx_medfilt_host(x.data(), AFX_FMT_F32, 40, 5, out.data(), &st) == AFX_OK && st == AFX_CLIP_NONFINITE && out[0] == -3.0f);
    CHECK(afx_medfilt_host(x.data(), AFX_FMT_F32, 40, 4, out.data(), &st) == AFX_ERR_INVALID);
    CHECK(afx_medfilt_host(x.data(), AFX_FMT_F32, 40, 0, out.data(), &st) == AFX_ERR_INVALID);
    CHECK(afx_medfilt_host(x.data(), AFX_FMT_F32, 40, 33, out.data(), &st) == AFX_ERR_UNSUPPORTED);
    CHECK(afx_medfilt_host(x.data(), 7, 40, 3, out.data(), &st) == AFX_ERR_INVALID);
    CHECK(afx_medfilt_host(x.data(), AFX_FMT_F32, -1, 3, out.data(), &st) == AFX_ERR_INVALID);
    CHECK(afx_medfilt_host(nullptr, AFX_FMT_F32, 40, 3, out.data(), &st) == AFX_ERR_INVALID);
  }

  // Savitzky-Golay: a ramp comes back (order >= 1) and its derivative is its slope, edges included
  const int cases[][3] = {{11, 3, 0}, {5, 0, 0}, {3, 2, 0}, {9, 1, 1}, {9, 2, 2}, {31, 5, 0}, {31, 5, 2}, {31, 5, 1}};
  for (const auto& cs : cases) {
    const int W = cs[0], P = cs[1], d = cs[2], h = W / 2;
    const int64_t lens[] = {0, W - 1, W, W + 1, 2 * W - 1, tile - 1, tile, tile + 1, tile + h, 2 * (int64_t)tile + 1};
    for (int64_t n : lens) {
      std::vector<float> x((size_t)n), out((size_t)n, -3.0f);
      for (int64_t i = 0; i < n; ++i) x[i] = 0.5f + 0.25f * (float)i;       // exact in float32
      int32_t st = -1;
      CHECK(afx_savgol_host(x.data(), AFX_FMT_F32, n, W, P, d, 0.5, out.data(), &st) == AFX_OK);
      if (n < W) { CHECK(st == AFX_CLIP_TOO_SHORT); for (float v : out) CHECK(v == -3.0f); continue; }
      CHECK(st == AFX_CLIP_OK);
      if (P < 1) continue;
      for (int64_t i = 0; i < n; ++i) {
        const float want = d == 0 ? x[i] : (d == 1 ? 0.5f : 0.0f);
        CHECK(std::fabs(out[i] - want) <= 1e-6f * (1.0f + std::fabs(want)) * (d == 2 ? 100.0f : 1.0f));
      }
    }
    std::vector<int16_t> q((size_t)(3 * W));
    for (auto& v : q) v = (int16_t)(noise() * 20000.0f);
    std::vector<float> out((size_t)(3 * W), -3.0f);
    int32_t st = -1;
    CHECK(afx_savgol_host(q.data(), AFX_FMT_S16, 3 * W, W, P, d, 1.0, out.data(), &st) == AFX_OK && st == AFX_CLIP_OK);
    for (float v : out) CHECK(std::isfinite(v));
  }
  {
    std::vector<float> x(50, 1.0f), out(50, -3.0f);
    int32_t st = -1;
    x[0] = NAN;
    CHECK(afx_savgol_host(x.data(), AFX_FMT_F32, 50, 11, 3, 0, 1.0, out.data(), &st) == AFX_OK && st == AFX_CLIP_NONFINITE && out[0] == -3.0f);
    CHECK(afx_savgol_host(x.data(), AFX_FMT_F32, 50, 12, 3, 0, 1.0, out.data(), &st) == AFX_ERR_UNSUPPORTED);
    CHECK(afx_savgol_host(x.data(), AFX_FMT_F32, 50, 11, 11, 0, 1.0, out.data(), &st) == AFX_ERR_INVALID);
    CHECK(afx_savgol_host(x.data(), AFX_FMT_F32, 50, 11, 3, 0, 1.0, nullptr, &st) == AFX_ERR_INVALID);
  }

  // the groups over the lengths at which the framing and the window of the local stability switch
  {
    const int64_t lens[] = {0, 1, 5, 11, 12, 19, 63, 64, 65, 127, 128, 2047, 2048, 2049, 9 * 512 - 1, 9 * 512, 10 * 512, 16 * 512 + 3};
    for (int64_t n : lens)
      for (int flags = 0; flags < 8; flags += 2) {
        std::vector<float> y((size_t)n);
        for (auto& v : y) v = noise();
        double rec[AFX_EZ_N];
        for (double& v : rec) v = -7.0;
        int32_t st = -1;
        CHECK(afx_energy_zcr_host(y.data(), n, 2048, 512, flags, rec, &st) == AFX_OK);
        if (n == 0) { CHECK(st == AFX_CLIP_TOO_SHORT && std::isnan(rec[AFX_EZ_T])); continue; }
        CHECK(st == AFX_CLIP_OK);
        const int fl = (int)rec[AFX_EZ_FL], hop = (int)rec[AFX_EZ_HOP];
        CHECK(fl >= 64 && fl <= 2048 && (fl & (fl - 1)) == 0 && (n >= 2048 ? fl == 2048 : (fl == 64 || (fl <= n && 2 * fl > n))));
        CHECK(hop == (fl / 4 < 512 ? fl / 4 : 512) && rec[AFX_EZ_T] == (double)(1 + n / hop));
        CHECK(std::isnan(rec[AFX_EZ_PEAK_IN]) && std::isnan(rec[AFX_EZ_PEAK_FILT]));
        if (flags & AFX_EZ_ENERGY) {
          CHECK(rec[AFX_EZ_ENERGY_MEAN] > 0.0 && rec[AFX_EZ_ENERGY_STD] >= 0.0 && rec[AFX_EZ_ENERGY_P10] >= 0.0);
          CHECK(rec[AFX_EZ_ENERGY_P10] <= rec[AFX_EZ_ENERGY_MEAN] + 3.0 * rec[AFX_EZ_ENERGY_STD] + 1e-12);
        } else {
          CHECK(std::isnan(rec[AFX_EZ_ENERGY_MEAN]) && std::isnan(rec[AFX_EZ_ENERGY_STD]) && std::isnan(rec[AFX_EZ_ENERGY_P10]));
        }
        if (flags & AFX_EZ_ZCR) {
          CHECK(rec[AFX_EZ_ZCR_MEAN] >= 0.0 && rec[AFX_EZ_ZCR_MEAN] < 1.0 && rec[AFX_EZ_ZCR_STD] >= 0.0 && rec[AFX_EZ_ZCR_LOCAL] >= 0.0);
          CHECK(rec[AFX_EZ_PEAK_SMOOTH] >= 0.0 && rec[AFX_EZ_PEAK_SMOOTH] <= 2.0 && (n < 12 || rec[AFX_EZ_PEAK_SMOOTH] > 0.0));
        } else {
          CHECK(std::isnan(rec[AFX_EZ_ZCR_MEAN]) && std::isnan(rec[AFX_EZ_ZCR_LOCAL]) && std::isnan(rec[AFX_EZ_PEAK_SMOOTH]));
        }
      }
    std::vector<float> z(5000, 0.0f);
    double rec[AFX_EZ_N];
    int32_t st = -1;
    CHECK(afx_energy_zcr_host(z.data(), 5000, 2048, 512, AFX_EZ_ENERGY | AFX_EZ_ZCR, rec, &st) == AFX_OK && st == AFX_CLIP_OK);
    CHECK(rec[AFX_EZ_ENERGY_MEAN] == 0.0 && rec[AFX_EZ_ZCR_MEAN] == 0.0 && rec[AFX_EZ_PEAK_SMOOTH] == 0.0 && rec[AFX_EZ_ZCR_LOCAL] == 0.0);
    z[4999] = NAN;
    CHECK(afx_energy_zcr_host(z.data(), 5000, 2048, 512, AFX_EZ_ENERGY, rec, &st) == AFX_OK && st == AFX_CLIP_NONFINITE && std::isnan(rec[AFX_EZ_T]));
    CHECK(afx_energy_zcr_host(z.data(), 5000, 1000, 512, AFX_EZ_ENERGY, rec, &st) == AFX_ERR_INVALID);
    CHECK(afx_energy_zcr_host(z.data(), 5000, 4096, 512, AFX_EZ_ENERGY, rec, &st) == AFX_ERR_INVALID);
    CHECK(afx_energy_zcr_host(z.data(), 5000, 2048, 0, AFX_EZ_ENERGY, rec, &st) == AFX_ERR_INVALID);
    CHECK(afx_energy_zcr_host(z.data(), 5000, 2048, 512, 64, rec, &st) == AFX_ERR_INVALID);
    CHECK(afx_energy_zcr_host(z.data(), 5000, 2048, 512, AFX_EZ_ENERGY, nullptr, &st) == AFX_ERR_INVALID);
  }
  if (g_fail) { std::fprintf(stderr, "smooth_check: %d check(s) failed\n", g_fail); return 1; }
  std::printf("smooth_check: ok\n");
  return 0;
}
