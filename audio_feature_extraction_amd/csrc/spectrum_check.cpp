// Stand-alone check of the host executors of the whole-clip DFT and the spectral distance (afx_cfft_host.cpp:
// afx_specdist_host, afx_clip_fft_host), built with AddressSanitizer + UBSan by `make spectrum-check` and run on the CPU:
// the trivial lengths, a prime, and the lengths either side of the kernels' tile (N = 0, 1, 2, 3, 97, 2048, 2049, 4097),
// both sample formats, with exactly sized heap buffers (an index past one is an ASan report).  The results are checked
// for what needs no library: the bins against the defining sum at small N, Parseval's identity, the symmetry of a pair
// with itself, the status values, the refusals.  Exit status 0: every check held.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "afx.h"

namespace {

int g_fail = 0;
#define CHECK(cond)                                                              \
  do {                                                                           \
    if (!(cond)) { std::fprintf(stderr, "spectrum_check: line %d: %s\n", __LINE__, #cond); ++g_fail; } \
  } while (0)

bool close_to(double a, double b, double rel) { return std::fabs(a - b) <= rel * std::fmax(std::fabs(a), std::fabs(b)); }

}  // namespace

int main() {
  uint32_t seed = 22u;
  const int64_t lens[] = {0, 1, 2, 3, 97, 2048, 2049, 4097};
  for (int64_t n : lens)
    for (int fmt : {AFX_FMT_F32, AFX_FMT_S16}) {
      std::vector<float> rf((size_t)(fmt == AFX_FMT_F32 ? n : 0)), df(rf.size());
      std::vector<int16_t> rs((size_t)(fmt == AFX_FMT_S16 ? n : 0)), ds(rs.size());
      std::vector<double> r((size_t)n), d((size_t)n);
      double ssr = 0.0, ssd = 0.0;
      for (int64_t i = 0; i < n; ++i) {
        seed = seed * 1664525u + 1013904223u;
        const int16_t q = (int16_t)(seed >> 18);
        seed = seed * 1664525u + 1013904223u;
        const int16_t e = (int16_t)(q + (int16_t)(seed >> 22) - 512);
        if (fmt == AFX_FMT_F32) { rf[i] = (float)q / 32768.0f; df[i] = (float)e / 32768.0f; } else { rs[i] = q; ds[i] = e; }
        r[i] = (double)q / 32768.0; d[i] = (double)e / 32768.0;
        ssr += r[i] * r[i]; ssd += d[i] * d[i];
      }
      const void* pr = fmt == AFX_FMT_F32 ? (const void*)rf.data() : (const void*)rs.data();
      const void* pd = fmt == AFX_FMT_F32 ? (const void*)df.data() : (const void*)ds.data();
      std::vector<double> rec(AFX_SPECDIST_N, -7.0), bins((size_t)(n ? 2 * (n / 2 + 1) : 0), -7.0);
      int32_t st = -1;
      CHECK(afx_specdist_host(pr, pd, fmt, n, n, rec.data(), &st) == AFX_OK);
      if (n == 0) {
        CHECK(st == AFX_CLIP_TOO_SHORT && std::isnan(rec[0]) && std::isnan(rec[3]));
        CHECK(afx_clip_fft_host(pr, fmt, 0, bins.data(), &st) == AFX_OK && st == AFX_CLIP_TOO_SHORT);
        continue;
      }
      CHECK(st == AFX_CLIP_OK && rec[0] == (double)n && rec[1] >= 0.0);
      CHECK(close_to(rec[2], (double)n * ssr, 1e-12) && close_to(rec[3], (double)n * ssd, 1e-12));       // Parseval
      CHECK(afx_specdist_host(pr, pr, fmt, n, n, rec.data(), &st) == AFX_OK && st == AFX_CLIP_OK && rec[1] <= 1e-9 * (double)n);
      CHECK(afx_specdist_host(pr, pd, fmt, n, n / 2, rec.data(), &st) == AFX_OK && (n / 2 ? rec[0] == (double)(n / 2) : st == AFX_CLIP_TOO_SHORT));
      CHECK(afx_clip_fft_host(pr, fmt, n, bins.data(), &st) == AFX_OK && st == AFX_CLIP_OK);
      double sum = 0.0;
      for (int64_t i = 0; i < n; ++i) sum += r[i];
      CHECK(std::fabs(bins[0] - sum) <= 1e-12 * std::sqrt((double)n * ssr + 1e-300) && std::fabs(bins[1]) <= 1e-12 * std::sqrt((double)n * ssr + 1e-300));
      if (n <= 97)
        for (int64_t k = 0; k <= n / 2; ++k) {                           // the defining sum
          double re = 0.0, im = 0.0;
          for (int64_t j = 0; j < n; ++j) {
            const double th = -2.0 * M_PI * (double)((j * k) % n) / (double)n;
            re += r[j] * std::cos(th); im += r[j] * std::sin(th);
          }
          CHECK(std::fabs(bins[2 * k] - re) + std::fabs(bins[2 * k + 1] - im) <= 1e-12 * std::sqrt((double)n * ssr));
        }
    }
  {  // refusals, and a sample that is not finite
    std::vector<float> x(100, 0.25f);
    std::vector<double> rec(AFX_SPECDIST_N), bins(2 * 51);
    int32_t st = -1;
    int64_t cost[6];
    CHECK(afx_specdist_host(x.data(), x.data(), AFX_FMT_F32, -1, 100, rec.data(), &st) == AFX_ERR_INVALID);
    CHECK(afx_specdist_host(x.data(), nullptr, AFX_FMT_F32, 100, 100, rec.data(), &st) == AFX_ERR_INVALID);
    CHECK(afx_specdist_host(x.data(), x.data(), 5, 100, 100, rec.data(), &st) == AFX_ERR_INVALID);
    CHECK(afx_specdist_host(x.data(), x.data(), AFX_FMT_F32, 100, 100, nullptr, &st) == AFX_ERR_INVALID);
    CHECK(afx_specdist_host(x.data(), x.data(), AFX_FMT_F32, (int64_t)1 << 28, (int64_t)1 << 28, rec.data(), &st) == AFX_ERR_UNSUPPORTED);
    CHECK(afx_clip_fft_host(x.data(), AFX_FMT_F32, -1, bins.data(), &st) == AFX_ERR_INVALID);
    CHECK(afx_clip_fft_host(nullptr, AFX_FMT_F32, 100, bins.data(), &st) == AFX_ERR_INVALID);
    CHECK(afx_clip_fft_host(x.data(), AFX_FMT_F32, 100, nullptr, &st) == AFX_ERR_INVALID);
    CHECK(afx_clip_fft_host(x.data(), AFX_FMT_F32, (int64_t)1 << 28, bins.data(), &st) == AFX_ERR_UNSUPPORTED);
    x[99] = NAN;
    CHECK(afx_specdist_host(x.data(), x.data(), AFX_FMT_F32, 100, 100, rec.data(), &st) == AFX_OK && st == AFX_CLIP_NONFINITE && std::isnan(rec[0]));
    CHECK(afx_specdist_host(x.data(), x.data(), AFX_FMT_F32, 100, 99, rec.data(), &st) == AFX_OK && st == AFX_CLIP_OK);
    CHECK(afx_clip_fft_host(x.data(), AFX_FMT_F32, 100, bins.data(), &st) == AFX_OK && st == AFX_CLIP_NONFINITE && std::isnan(bins[101]));
    CHECK(afx_specdist_cost(AFX_FMT_S16, AFX_MEM_HOST, cost) == AFX_OK && cost[2] == 132 && cost[3] == 256 && cost[0] == 0);
    CHECK(afx_specdist_cost(AFX_FMT_F32, AFX_MEM_DEVICE, cost) == AFX_OK && cost[2] == 128);
    CHECK(afx_specdist_cost(7, AFX_MEM_HOST, cost) == AFX_ERR_INVALID && afx_specdist_cost(AFX_FMT_F32, AFX_MEM_HOST, nullptr) == AFX_ERR_INVALID);
  }
  if (g_fail) { std::fprintf(stderr, "spectrum_check: %d check(s) failed\n", g_fail); return 1; }
  std::printf("spectrum_check: ok\n");
  return 0;
}
