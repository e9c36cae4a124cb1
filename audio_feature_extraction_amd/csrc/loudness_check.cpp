// Stand-alone check of the host side of the loudness meter (afx_loudness_host.cpp: afx_kweight_sos, afx_loudness_blocks,
// afx_loudness_host, afx_loudness_cost), built with AddressSanitizer + UBSan by `make loudness-check` and run on the CPU: the
// executor over the lengths around the shortest clip, both sides of the block count's rounding, a partial last block and the
// tile, at rates whose segment boundaries are and are not evenly spaced, with exactly sized heap buffers for the samples,
// z_j and the result (an index past any of them is an ASan report) and NULL optionals.  Every z_j is compared with a
// sequential restatement (the two sections sample by sample, the blocks' squares summed one by one).
// Exit status 0: every check held.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "afx.h"

namespace {

int g_fail = 0;
#define CHECK(cond)                                                              \
  do {                                                                           \
    if (!(cond)) { std::fprintf(stderr, "loudness_check: line %d: %s\n", __LINE__, #cond); ++g_fail; } \
  } while (0)

uint32_t g_seed = 2463534242u;
float noise() {
  g_seed = g_seed * 1664525u + 1013904223u;
  return (float)((int)(g_seed >> 17) - 16384) / 16384.0f;
}

// z_j the plain way
std::vector<double> plain_z(const std::vector<float>& x, int rate, double tg, int64_t nblocks) {
  double sos[12];
  CHECK(afx_kweight_sos(rate, sos) == AFX_OK);
  std::vector<double> y(x.begin(), x.end());
  for (int s = 0; s < 2; ++s) {
    const double* c = sos + 6 * s;
    double z0 = 0.0, z1 = 0.0;
    for (double& v : y) {
      const double o = c[0] * v + z0;
      z0 = c[1] * v - c[4] * o + z1;
      z1 = c[2] * v - c[5] * o;
      v = o;
    }
  }
  std::vector<double> z((size_t)nblocks);
  for (int64_t j = 0; j < nblocks; ++j) {
    const int64_t l = (int64_t)(tg * ((double)j * 0.25) * (double)rate);
    const int64_t u = std::min<int64_t>((int64_t)(tg * ((double)j * 0.25 + 1.0) * (double)rate), (int64_t)y.size());
    double a = 0.0;
    for (int64_t i = l; i < u; ++i) a += y[i] * y[i];
    z[j] = a / (tg * (double)rate);
  }
  return z;
}

void one(int rate, int64_t n, int fmt, int mode) {
  const double tg = 0.4;
  std::vector<float> x((size_t)n);
  for (float& v : x) v = 0.25f * noise();
  std::vector<int16_t> xi((size_t)n);
  for (int64_t i = 0; i < n; ++i) xi[i] = (int16_t)std::lrintf(x[i] * 32767.0f);
  if (fmt == AFX_FMT_S16) for (int64_t i = 0; i < n; ++i) x[i] = (float)xi[i] / 32768.0f;
  int64_t nb = -1;
  CHECK(afx_loudness_blocks(n, rate, tg, &nb) == AFX_OK && nb >= 0);
  const bool shortclip = (double)n < tg * rate;
  CHECK((nb == 0) == shortclip);
  double rec[AFX_LOUD_N];
  std::vector<double> z((size_t)nb, -7.0);
  std::vector<float> out((size_t)(mode == AFX_LOUD_MEASURE ? 0 : n), -7.0f);
  int32_t st = -1;
  const void* p = fmt == AFX_FMT_S16 ? (const void*)xi.data() : (const void*)x.data();
  CHECK(afx_loudness_host(p, fmt, n, rate, tg, -23.0, mode, rec, nb ? z.data() : nullptr, out.empty() ? nullptr : out.data(), &st) == AFX_OK);
  if (mode == AFX_LOUD_NORM_PEAK ? n == 0 : shortclip) {
    CHECK(st == AFX_CLIP_TOO_SHORT && std::isnan(rec[AFX_LOUD_LUFS]));
    for (float v : out) CHECK(v == -7.0f);
    return;
  }
  CHECK(st == AFX_CLIP_OK);
  if (nb > 0) {
    CHECK(rec[AFX_LOUD_BLOCKS] == (double)nb && rec[AFX_LOUD_N1] <= nb && rec[AFX_LOUD_N2] <= rec[AFX_LOUD_N1]);
    CHECK(std::isfinite(rec[AFX_LOUD_LUFS]) && rec[AFX_LOUD_LUFS] < 0.0 && rec[AFX_LOUD_LUFS] > -40.0);
    const std::vector<double> ref = plain_z(x, rate, tg, nb);
    for (int64_t j = 0; j < nb; ++j) CHECK(std::fabs(z[j] - ref[j]) <= 1e-9 * ref[j]);
  }
  if (mode != AFX_LOUD_MEASURE) {
    const float g = (float)rec[AFX_LOUD_GAIN];
    float mx = 0.0f;
    for (int64_t i = 0; i < n; ++i) { CHECK(out[i] == g * x[i]); mx = std::max(mx, std::fabs(out[i])); }
    CHECK((double)mx == rec[AFX_LOUD_PEAK_OUT]);
  }
  // second call without the optional z_j
  double rec2[AFX_LOUD_N];
  CHECK(afx_loudness_host(p, fmt, n, rate, tg, -23.0, AFX_LOUD_MEASURE, rec2, nullptr, nullptr, &st) == AFX_OK);
  if (nb > 0) CHECK(rec2[AFX_LOUD_LUFS] == rec[AFX_LOUD_LUFS]);
}

}  // namespace

int main() {
  int32_t geo[5] = {0, 0, 0, 0, 0};
  CHECK(afx_loudness_geometry(geo) == AFX_OK && geo[0] == 64 && geo[1] == 64 && geo[2] == 4000 && geo[3] == 192000 && geo[4] == 16);
  CHECK(afx_loudness_geometry(nullptr) == AFX_ERR_INVALID);
  const int tile = geo[0] * geo[1];
  double sos[12];
  CHECK(afx_kweight_sos(3999, sos) == AFX_ERR_INVALID && afx_kweight_sos(192001, sos) == AFX_ERR_INVALID && afx_kweight_sos(48000, nullptr) == AFX_ERR_INVALID);
  for (int rate : {4000, 8000, 11025, 16000, 22050, 44100, 48000, 192000}) {
    CHECK(afx_kweight_sos(rate, sos) == AFX_OK && sos[3] == 1.0 && sos[9] == 1.0);
    for (double v : sos) CHECK(std::isfinite(v));
    CHECK(std::fabs(sos[6] + sos[7] + sos[8]) < 1e-12);                   // the high pass has a zero at DC
  }
  // BS.1770's own coefficients at 48 kHz, to the figures the standard prints
  CHECK(afx_kweight_sos(48000, sos) == AFX_OK);
  CHECK(std::fabs(sos[4] + 1.69065929318241) < 2e-3 && std::fabs(sos[5] - 0.73248077421585) < 2e-3);
  CHECK(std::fabs(sos[10] + 1.99004745483398) < 1e-4 && std::fabs(sos[11] - 0.99007225036621) < 1e-4);

  int64_t nb = 0;
  const int64_t at16k[][2] = {{6399, 0}, {6400, 1}, {7199, 1}, {7200, 1}, {7201, 2}, {8799, 2}, {8800, 3}};
  for (auto& c : at16k) CHECK(afx_loudness_blocks(c[0], 16000, 0.4, &nb) == AFX_OK && nb == c[1]);
  CHECK(afx_loudness_blocks(100, 16000, 0.4, nullptr) == AFX_ERR_INVALID && afx_loudness_blocks(-1, 16000, 0.4, &nb) == AFX_ERR_INVALID);
  CHECK(afx_loudness_blocks(100, 0, 0.4, &nb) == AFX_ERR_INVALID && afx_loudness_blocks(100, 16000, 0.0, &nb) == AFX_ERR_INVALID);
  CHECK(afx_loudness_blocks(100, 2000, 0.4, &nb) == AFX_ERR_UNSUPPORTED && afx_loudness_blocks(100, 8000, 0.03, &nb) == AFX_ERR_UNSUPPORTED);

  for (int rate : {8000, 11025, 16000, 48000}) {
    const int64_t B = (int64_t)std::ceil(0.4 * rate);
    for (int64_t n : {(int64_t)0, (int64_t)1, B - 1, B, B + 1, B + B / 8 - 1, B + B / 8, B + B / 8 + 1, B + 3 * (B / 8), B + 3 * (B / 8) + 1,
                      (int64_t)tile - 1, (int64_t)tile, (int64_t)tile + 1, (int64_t)2 * tile + 77})
      for (int fmt : {AFX_FMT_F32, AFX_FMT_S16})
        for (int mode : {AFX_LOUD_MEASURE, AFX_LOUD_NORM_LOUDNESS, AFX_LOUD_NORM_PEAK}) one(rate, n, fmt, mode);
  }
  {
    // silence has no level: -inf, and the clip comes back unchanged with gain 1; a NaN is reported, nothing written
    std::vector<float> x(8000, 0.0f), out(8000, -7.0f);
    double rec[AFX_LOUD_N];
    int32_t st = -1;
    CHECK(afx_loudness_host(x.data(), AFX_FMT_F32, 8000, 16000, 0.4, -23.0, AFX_LOUD_NORM_LOUDNESS, rec, nullptr, out.data(), &st) == AFX_OK);
    CHECK(st == AFX_CLIP_OK && std::isinf(rec[AFX_LOUD_LUFS]) && rec[AFX_LOUD_LUFS] < 0 && rec[AFX_LOUD_GAIN] == 1.0 && rec[AFX_LOUD_N1] == 0);
    for (float v : out) CHECK(v == 0.0f);
    x[4321] = NAN;
    std::fill(out.begin(), out.end(), -7.0f);
    CHECK(afx_loudness_host(x.data(), AFX_FMT_F32, 8000, 16000, 0.4, -23.0, AFX_LOUD_NORM_PEAK, rec, nullptr, out.data(), &st) == AFX_OK);
    CHECK(st == AFX_CLIP_NONFINITE && std::isnan(rec[AFX_LOUD_LUFS]));
    for (float v : out) CHECK(v == -7.0f);
    CHECK(afx_loudness_host(x.data(), 7, 8000, 16000, 0.4, -23.0, AFX_LOUD_MEASURE, rec, nullptr, nullptr, &st) == AFX_ERR_INVALID);
    CHECK(afx_loudness_host(x.data(), AFX_FMT_F32, 8000, 16000, 0.4, -23.0, 3, rec, nullptr, nullptr, &st) == AFX_ERR_INVALID);
    CHECK(afx_loudness_host(x.data(), AFX_FMT_F32, 8000, 16000, 0.4, NAN, AFX_LOUD_NORM_PEAK, rec, nullptr, out.data(), &st) == AFX_ERR_INVALID);
    CHECK(afx_loudness_host(x.data(), AFX_FMT_F32, 8000, 16000, 0.4, -23.0, AFX_LOUD_NORM_PEAK, rec, nullptr, nullptr, &st) == AFX_ERR_INVALID);
    CHECK(afx_loudness_host(x.data(), AFX_FMT_F32, 8000, 1000, 0.4, -23.0, AFX_LOUD_MEASURE, rec, nullptr, nullptr, &st) == AFX_ERR_UNSUPPORTED);
    CHECK(afx_loudness_host(nullptr, AFX_FMT_F32, 8000, 16000, 0.4, -23.0, AFX_LOUD_MEASURE, rec, nullptr, nullptr, &st) == AFX_ERR_INVALID);
  }
  {
    int64_t cost[6];
    CHECK(afx_loudness_cost(AFX_FMT_S16, AFX_MEM_HOST, AFX_MEM_HOST, AFX_LOUD_NORM_LOUDNESS, cost) == AFX_OK && cost[0] == 512 && cost[2] == 6 && cost[4] == 8);
    CHECK(afx_loudness_cost(AFX_FMT_F32, AFX_MEM_DEVICE, AFX_MEM_HOST, AFX_LOUD_MEASURE, cost) == AFX_OK && cost[2] == 0);
    CHECK(afx_loudness_cost(7, AFX_MEM_HOST, AFX_MEM_HOST, 0, cost) == AFX_ERR_INVALID && afx_loudness_cost(0, 0, 0, 3, cost) == AFX_ERR_INVALID);
    CHECK(afx_loudness_cost(AFX_FMT_F32, AFX_MEM_HOST, AFX_MEM_HOST, 0, nullptr) == AFX_ERR_INVALID);
  }
  if (g_fail) { std::fprintf(stderr, "loudness_check: %d check(s) failed\n", g_fail); return 1; }
  std::printf("loudness_check: ok\n");
  return 0;
}
