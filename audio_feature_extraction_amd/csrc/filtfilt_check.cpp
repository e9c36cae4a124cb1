// Stand-alone check of the host side of the zero-phase filter (afx_filt_host.cpp: afx_butter_sos, afx_sosfiltfilt_host), built
// with AddressSanitizer + UBSan by `make filtfilt-check` and run on the CPU: every order of the design into an exactly sized
// buffer, and the executor over the boundary lengths of the block decomposition with exactly sized heap buffers for the
// samples and the result (an index past either is an ASan report).  The results are checked for what needs no reference:
// statuses, finiteness, the unit peak of the experiment mode, and that a constant is removed by a high-pass.
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
    if (!(cond)) { std::fprintf(stderr, "filtfilt_check: line %d: %s\n", __LINE__, #cond); ++g_fail; } \
  } while (0)

}  // namespace

int main() {
  int32_t geo[4] = {0, 0, 0, 0};
  CHECK(afx_filtfilt_geometry(geo) == AFX_OK);
  const int L = geo[0], tile = geo[0] * geo[1], p = 18;
  CHECK(L > 2 * p + 1 && geo[2] == 4 && geo[3] >= p);
  for (int order = 1; order <= 8; ++order)
    for (int hp = 0; hp < 2; ++hp) {
      std::vector<double> sos((size_t)((order + 1) / 2) * 6, -7.0);
      CHECK(afx_butter_sos(order, 0.018, hp, sos.data()) == AFX_OK);
      for (double v : sos) CHECK(std::isfinite(v) && v != -7.0);
    }
  std::vector<double> one(6);
  CHECK(afx_butter_sos(9, 0.1, 1, one.data()) == AFX_ERR_UNSUPPORTED);
  CHECK(afx_butter_sos(0, 0.1, 1, one.data()) == AFX_ERR_INVALID);
  CHECK(afx_butter_sos(2, 1.0, 1, one.data()) == AFX_ERR_INVALID);
  CHECK(afx_butter_sos(2, 0.1, 1, nullptr) == AFX_ERR_INVALID);

  std::vector<double> sos(18);
  CHECK(afx_butter_sos(5, 200.0 / 11025.0, 1, sos.data()) == AFX_OK);
  const int64_t lens[] = {0, 1, p, p + 1, p + 2, L - 2 * p - 1, L - 2 * p, L - 2 * p + 1, 2 * L - 2 * p + 1,
                          tile - 2 * p, tile - 2 * p + 1, 3 * (int64_t)tile + 17};
  uint32_t seed = 12345u;
  for (int64_t n : lens)
    for (int mode = 0; mode < 2; ++mode)
      for (int fmt = 0; fmt < 2; ++fmt) {
        std::vector<float> xf((size_t)(fmt == AFX_FMT_F32 ? n : 0));
        std::vector<int16_t> xs((size_t)(fmt == AFX_FMT_S16 ? n : 0));
        for (int64_t i = 0; i < n; ++i) {
          seed = seed * 1664525u + 1013904223u;
          const int v = (int)(seed >> 17) - 16384;
          if (fmt == AFX_FMT_F32) xf[i] = 0.5f + (float)v / 32768.0f; else xs[i] = (int16_t)(8192 + v / 2);
        }
        std::vector<float> out((size_t)n, -3.0f);
        double peak[2] = {-1.0, -1.0};
        int32_t st = -1;
        const void* x = fmt == AFX_FMT_F32 ? (const void*)xf.data() : (const void*)xs.data();
        CHECK(afx_sosfiltfilt_host(x, fmt, n, sos.data(), 3, p, mode, 0.98f, out.data(), peak, &st) == AFX_OK);
        if (n <= p) {
          CHECK(st == AFX_CLIP_TOO_SHORT);
          for (float v : out) CHECK(v == -3.0f);
          continue;
        }
        CHECK(st == AFX_CLIP_OK && peak[0] > 0.0 && peak[1] > 0.0);
        float mx = 0.0f;
        for (float v : out) { CHECK(std::isfinite(v)); mx = std::fmax(mx, std::fabs(v)); }
        if (mode == AFX_FILT_EXPERIMENT) CHECK(mx == 1.0f);
      }
  // a constant is a high-pass filter's steady state on both passes: the plain result is zero to rounding
  {
    const int64_t n = 3 * (int64_t)tile + 17;
    std::vector<float> x((size_t)n, 0.75f), out((size_t)n, -3.0f);
    int32_t st = -1;
    CHECK(afx_sosfiltfilt_host(x.data(), AFX_FMT_F32, n, sos.data(), 3, p, AFX_FILT_PLAIN, 0.0f, out.data(), nullptr, &st) == AFX_OK);
    CHECK(st == AFX_CLIP_OK);
    for (float v : out) CHECK(std::fabs(v) < 1e-9f);
  }
  // a NaN in the last sample; padlen 0; the largest padlen on a clip one sample longer
  {
    std::vector<float> x(300, 0.25f), out(300, -3.0f);
    x[299] = NAN;
    int32_t st = -1;
    CHECK(afx_sosfiltfilt_host(x.data(), AFX_FMT_F32, 300, sos.data(), 3, p, AFX_FILT_EXPERIMENT, 0.98f, out.data(), nullptr, &st) == AFX_OK);
    CHECK(st == AFX_CLIP_NONFINITE && out[0] == -3.0f);
    x[299] = 0.5f;
    CHECK(afx_sosfiltfilt_host(x.data(), AFX_FMT_F32, 1, sos.data(), 3, 0, AFX_FILT_PLAIN, 0.0f, out.data(), nullptr, &st) == AFX_OK);
    CHECK(st == AFX_CLIP_OK);
    std::vector<float> big((size_t)geo[3] + 1, 0.5f), bout((size_t)geo[3] + 1);
    CHECK(afx_sosfiltfilt_host(big.data(), AFX_FMT_F32, geo[3] + 1, sos.data(), 3, geo[3], AFX_FILT_EXPERIMENT, 0.98f, bout.data(), nullptr, &st) == AFX_OK);
    CHECK(st == AFX_CLIP_OK);
    CHECK(afx_sosfiltfilt_host(big.data(), AFX_FMT_F32, geo[3] + 1, sos.data(), 3, geo[3] + 1, 0, 0.0f, bout.data(), nullptr, &st) == AFX_ERR_UNSUPPORTED);
    CHECK(afx_sosfiltfilt_host(big.data(), AFX_FMT_F32, 100, sos.data(), 5, p, 0, 0.0f, bout.data(), nullptr, &st) == AFX_ERR_UNSUPPORTED);
    CHECK(afx_sosfiltfilt_host(big.data(), AFX_FMT_F32, 100, sos.data(), 3, p, 2, 0.0f, bout.data(), nullptr, &st) == AFX_ERR_INVALID);
    CHECK(afx_sosfiltfilt_host(big.data(), AFX_FMT_F32, -1, sos.data(), 3, p, 0, 0.0f, bout.data(), nullptr, &st) == AFX_ERR_INVALID);
  }
  if (g_fail) { std::fprintf(stderr, "filtfilt_check: %d check(s) failed\n", g_fail); return 1; }
  std::printf("filtfilt_check: ok\n");
  return 0;
}
