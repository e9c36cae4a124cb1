// Stand-alone check of the host executor of the beat tracker (afx_beat_host.cpp: afx_beat_track_host), built with
// AddressSanitizer + UBSan by `make beat-check` and run on the CPU: the lengths either side of the window's and the candidate
// range's boundaries, at the smallest and largest periods, with exactly sized heap buffers for the envelope and every output
// (an index past one is an ASan report) and with the optional outputs absent.  The results are checked for what needs no
// reference: the count against the flags, the gaps between beats, the backlinks' range, the refusals.
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
    if (!(cond)) { std::fprintf(stderr, "beat_check: line %d: %s\n", __LINE__, #cond); ++g_fail; } \
  } while (0)

}  // namespace

int main() {
  const double fps = 22050.0 / 512.0;
  const int fpbs[] = {1, 2, 42, 43, 768};
  uint32_t seed = 2024u;
  for (int fpb : fpbs) {
    const double bpm = 60.0 * fps / (double)fpb;
    const int lo = (int)std::nearbyint(fpb / 2.0);
    const int64_t lens[] = {0, 1, 2, 3, 63, 64, 65, 2 * (int64_t)fpb - 1, 2 * (int64_t)fpb, 2 * (int64_t)fpb + 1};
    for (int64_t T : lens)
      for (int kind = 0; kind < 3; ++kind)                 // random, an impulse train of the period, constant
        for (int trim = 0; trim < 2; ++trim)
          for (int opt = 0; opt < 2; ++opt) {
            std::vector<float> env((size_t)T);
            for (int64_t i = 0; i < T; ++i) {
              seed = seed * 1664525u + 1013904223u;
              env[i] = kind == 0 ? (float)(seed >> 8) / 16777216.0f : kind == 1 ? (i % fpb == 0 ? 1.0f : 0.0f) : 1.0f;
            }
            bool constant = true;                         // std 0: x is huge and the scores may overflow
            for (int64_t i = 1; i < T; ++i) constant &= env[i] == env[0];
            std::vector<uint8_t> mask((size_t)T, 7);
            std::vector<double> ls((size_t)(opt ? T : 0), -3.0), cum((size_t)(opt ? T : 0), -3.0);
            std::vector<int32_t> bl((size_t)(opt ? T : 0), -3);
            int64_t nb = -1;
            CHECK(afx_beat_track_host(env.data(), T, fps, bpm, 100.0, trim, mask.data(), &nb, opt ? ls.data() : nullptr,
                                      opt ? cum.data() : nullptr, opt ? bl.data() : nullptr) == AFX_OK);
            int64_t count = 0, prev = -1;
            for (int64_t i = 0; i < T; ++i) {
              CHECK(mask[i] <= 1);
              if (!mask[i]) continue;
              ++count;
              if (prev >= 0) CHECK(i - prev >= (lo > 1 ? lo : 1) && i - prev <= 2 * fpb);
              prev = i;
            }
            CHECK(count == nb);
            if (T < 2) CHECK(nb == 0);
            for (int64_t i = 0; opt && i < T; ++i) {
              CHECK(bl[i] >= -1 && bl[i] < i);
              if (!constant) CHECK(std::isfinite(ls[i]) && std::isfinite(cum[i]));
              else CHECK(!std::isnan(ls[i]));
            }
          }
  }
  // an all-zero envelope and tempo 0 have no beats; the refusals
  {
    std::vector<float> z(100, 0.0f), one(100, 0.5f);
    one[50] = 1.0f;
    std::vector<uint8_t> mask(100, 7);
    int64_t nb = -1;
    CHECK(afx_beat_track_host(z.data(), 100, fps, 120.0, 100.0, 1, mask.data(), &nb, nullptr, nullptr, nullptr) == AFX_OK && nb == 0);
    CHECK(afx_beat_track_host(one.data(), 100, fps, 0.0, 100.0, 1, mask.data(), &nb, nullptr, nullptr, nullptr) == AFX_OK && nb == 0);
    for (uint8_t m : mask) CHECK(m == 0);
    CHECK(afx_beat_track_host(one.data(), 100, fps, -1.0, 100.0, 1, mask.data(), &nb, nullptr, nullptr, nullptr) == AFX_ERR_INVALID);
    CHECK(afx_beat_track_host(one.data(), 100, fps, NAN, 100.0, 1, mask.data(), &nb, nullptr, nullptr, nullptr) == AFX_ERR_INVALID);
    CHECK(afx_beat_track_host(one.data(), 100, fps, INFINITY, 100.0, 1, mask.data(), &nb, nullptr, nullptr, nullptr) == AFX_ERR_INVALID);
    CHECK(afx_beat_track_host(one.data(), 100, NAN, 120.0, 100.0, 1, mask.data(), &nb, nullptr, nullptr, nullptr) == AFX_ERR_INVALID);
    CHECK(afx_beat_track_host(one.data(), 100, fps, 120.0, 0.0, 1, mask.data(), &nb, nullptr, nullptr, nullptr) == AFX_ERR_INVALID);
    CHECK(afx_beat_track_host(one.data(), 100, fps, 120.0, NAN, 1, mask.data(), &nb, nullptr, nullptr, nullptr) == AFX_ERR_INVALID);
    CHECK(afx_beat_track_host(one.data(), 100, fps, 60.0 * fps / 769.0, 100.0, 1, mask.data(), &nb, nullptr, nullptr, nullptr) == AFX_ERR_INVALID);
    CHECK(afx_beat_track_host(one.data(), 100, fps, 60.0 * fps / 0.4, 100.0, 1, mask.data(), &nb, nullptr, nullptr, nullptr) == AFX_ERR_INVALID);
    CHECK(afx_beat_track_host(one.data(), -1, fps, 120.0, 100.0, 1, mask.data(), &nb, nullptr, nullptr, nullptr) == AFX_ERR_INVALID);
    one[99] = NAN;
    CHECK(afx_beat_track_host(one.data(), 100, fps, 120.0, 100.0, 1, mask.data(), &nb, nullptr, nullptr, nullptr) == AFX_ERR_INVALID);
  }
  if (g_fail) { std::fprintf(stderr, "beat_check: %d check(s) failed\n", g_fail); return 1; }
  std::printf("beat_check: ok\n");
  return 0;
}
