// Stand-alone check of the host executors of the recording screen and the compare sums (afx_assess_host.cpp:
// afx_assess_host, afx_compare_host), built with AddressSanitizer + UBSan by `make assess-check` and run on the CPU: the
// lengths either side of the framing's and the noise window's boundaries (0, 1, 9, 10, frame - 1, frame, frame + 1, a frame
// longer than the clip), both sample formats, with exactly sized heap buffers (an index past one is an ASan report).  The
// results are checked for what needs no reference: the frame counts, the identities between the fields, the status values,
// the refusals.  Exit status 0: every check held.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "afx.h"

namespace {

int g_fail = 0;
#define CHECK(cond)                                                              \
  do {                                                                           \
    if (!(cond)) { std::fprintf(stderr, "assess_check: line %d: %s\n", __LINE__, #cond); ++g_fail; } \
  } while (0)

bool close_to(double a, double b) { return std::fabs(a - b) <= 1e-12 * std::fmax(std::fabs(a), std::fabs(b)); }

}  // namespace

int main() {
  uint32_t seed = 77u;
  const int32_t frames[] = {1, 2, 3, 80, 441};
  for (int32_t fs : frames)
    for (int32_t fl : {fs, 10 * fs, 100000}) {
      const int64_t lens[] = {0, 1, 9, 10, 11, fs - 1, fs, fs + 1, 2 * (int64_t)fs - 1, fl - 1, fl, fl + 1, 3 * (int64_t)fl + fs / 2, 25000};
      for (int64_t n : lens) {
        if (n < 0) continue;
        for (int fmt : {AFX_FMT_F32, AFX_FMT_S16}) {
          std::vector<float> xf((size_t)(fmt == AFX_FMT_F32 ? n : 0));
          std::vector<int16_t> xs((size_t)(fmt == AFX_FMT_S16 ? n : 0));
          double ss = 0.0, pk = 0.0;
          for (int64_t i = 0; i < n; ++i) {
            seed = seed * 1664525u + 1013904223u;
            const int16_t q = (int16_t)(seed >> 16);
            const float v = (float)q / 32768.0f * (i < n / 2 ? 1.0f : 1e-4f);      // a loud half, then a quiet one
            if (fmt == AFX_FMT_F32) xf[i] = v; else xs[i] = q;
            const double x = fmt == AFX_FMT_F32 ? (double)v : (double)q / 32768.0;
            ss += x * x; pk = std::fmax(pk, std::fabs(x));
          }
          const void* p = fmt == AFX_FMT_F32 ? (const void*)xf.data() : (const void*)xs.data();
          std::vector<double> rec(AFX_ASSESS_N, -7.0);
          int32_t st = -7;
          CHECK(afx_assess_host(p, fmt, n, fs, fl, -40.0, 2000, rec.data(), &st) == AFX_OK);
          if (n == 0) {
            CHECK(st == AFX_CLIP_TOO_SHORT);
            for (double v : rec) CHECK(std::isnan(v));
            continue;
          }
          CHECK(st == AFX_CLIP_OK);
          CHECK(rec[0] == (double)(1 + (n - fs % 2) / fs) && rec[7] == (double)(1 + (n - fl % 2) / fl));
          CHECK(rec[1] >= 0 && rec[1] <= rec[0] && rec[2] >= 0 && rec[2] <= rec[1]);
          CHECK((rec[1] == 0) == (rec[2] == 0));
          CHECK(close_to(rec[4], ss / (double)n) && rec[5] == pk);
          CHECK(rec[3] >= 0 && rec[3] <= pk + 1e-15);
          CHECK((n < 10) == std::isnan(rec[6]));
          CHECK(rec[8] >= 0 && rec[9] >= 0 && rec[9] <= rec[8] * std::sqrt(rec[7]) + 1e-300);
          if (fl > 2 * n) CHECK(rec[7] == 1 && rec[9] == 0 && close_to(rec[8], std::sqrt(ss / (double)fl)));
          // a threshold at or below the clamp silences nothing; one above 0 dB everything
          std::vector<double> r2(AFX_ASSESS_N);
          CHECK(afx_assess_host(p, fmt, n, fs, fl, -80.0, 0, r2.data(), &st) == AFX_OK && r2[1] == 0 && r2[2] == 0 && std::isnan(r2[6]));
          CHECK(afx_assess_host(p, fmt, n, fs, fl, 1.0, 5, r2.data(), &st) == AFX_OK && r2[1] == r2[0] && r2[2] == r2[0]);
          // the pair (x, x) and the pair cut to the shorter side
          std::vector<double> cr(AFX_COMPARE_N, -7.0);
          CHECK(afx_compare_host(p, p, fmt, n, n, cr.data(), &st) == AFX_OK && st == AFX_CLIP_OK);
          CHECK(cr[0] == (double)n && cr[1] == cr[2] && cr[3] == cr[4] && cr[4] == cr[5] && cr[6] == 0 && close_to(cr[3], ss));
          CHECK(cr[7] == cr[8] && cr[8] == cr[9] && cr[7] >= 0 && cr[7] <= cr[3] * (1 + 1e-12));
          CHECK(afx_compare_host(p, p, fmt, n, n / 2, cr.data(), &st) == AFX_OK && (n / 2 ? cr[0] == (double)(n / 2) : st == AFX_CLIP_TOO_SHORT));
        }
      }
    }
  // non-finite samples and the refusals
  {
    std::vector<float> x(100, 0.25f);
    std::vector<double> rec(AFX_ASSESS_N), cr(AFX_COMPARE_N);
    int32_t st = -7;
    int64_t cost[6];
    CHECK(afx_assess_host(x.data(), AFX_FMT_F32, 100, 0, 10, -40.0, 2000, rec.data(), &st) == AFX_ERR_INVALID);
    CHECK(afx_assess_host(x.data(), AFX_FMT_F32, 100, 10, -1, -40.0, 2000, rec.data(), &st) == AFX_ERR_INVALID);
    CHECK(afx_assess_host(x.data(), AFX_FMT_F32, 100, 10, 100, NAN, 2000, rec.data(), &st) == AFX_ERR_INVALID);
    CHECK(afx_assess_host(x.data(), AFX_FMT_F32, 100, 10, 100, INFINITY, 2000, rec.data(), &st) == AFX_ERR_INVALID);
    CHECK(afx_assess_host(x.data(), AFX_FMT_F32, 100, 10, 100, -40.0, -1, rec.data(), &st) == AFX_ERR_INVALID);
    CHECK(afx_assess_host(x.data(), AFX_FMT_F32, -1, 10, 100, -40.0, 2000, rec.data(), &st) == AFX_ERR_INVALID);
    CHECK(afx_assess_host(x.data(), 5, 100, 10, 100, -40.0, 2000, rec.data(), &st) == AFX_ERR_INVALID);
    CHECK(afx_assess_host(nullptr, AFX_FMT_F32, 100, 10, 100, -40.0, 2000, rec.data(), &st) == AFX_ERR_INVALID);
    CHECK(afx_compare_host(x.data(), x.data(), AFX_FMT_F32, -1, 100, cr.data(), &st) == AFX_ERR_INVALID);
    CHECK(afx_compare_host(x.data(), nullptr, AFX_FMT_F32, 100, 100, cr.data(), &st) == AFX_ERR_INVALID);
    x[99] = INFINITY;
    CHECK(afx_assess_host(x.data(), AFX_FMT_F32, 100, 10, 100, -40.0, 2000, rec.data(), &st) == AFX_OK && st == AFX_CLIP_NONFINITE && std::isnan(rec[0]));
    CHECK(afx_assess_host(x.data(), AFX_FMT_F32, 99, 10, 100, -40.0, 2000, rec.data(), &st) == AFX_OK && st == AFX_CLIP_OK);
    CHECK(afx_compare_host(x.data(), x.data(), AFX_FMT_F32, 100, 100, cr.data(), &st) == AFX_OK && st == AFX_CLIP_NONFINITE && std::isnan(cr[0]));
    CHECK(afx_compare_host(x.data(), x.data(), AFX_FMT_F32, 100, 99, cr.data(), &st) == AFX_OK && st == AFX_CLIP_OK);
    CHECK(afx_assess_cost(AFX_COST_ASSESS, AFX_FMT_S16, AFX_MEM_HOST, cost) == AFX_OK && cost[2] == 19 && cost[3] == 256 && cost[0] == 0);
    CHECK(afx_assess_cost(AFX_COST_COMPARE, AFX_FMT_F32, AFX_MEM_DEVICE, cost) == AFX_OK && cost[2] == 1);
    CHECK(afx_assess_cost(2, AFX_FMT_F32, AFX_MEM_HOST, cost) == AFX_ERR_INVALID && afx_assess_cost(0, 7, AFX_MEM_HOST, cost) == AFX_ERR_INVALID);
    CHECK(afx_assess_cost(0, AFX_FMT_F32, AFX_MEM_HOST, nullptr) == AFX_ERR_INVALID);
  }
  if (g_fail) { std::fprintf(stderr, "assess_check: %d check(s) failed\n", g_fail); return 1; }
  std::printf("assess_check: ok\n");
  return 0;
}
