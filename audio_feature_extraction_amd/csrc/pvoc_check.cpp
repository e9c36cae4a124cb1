// Stand-alone check of the host side of phase_vocoder / time_stretch (afx_pvoc_host.cpp), built with AddressSanitizer +
// UBSan (make pvoc-check): T_out against a plain count of the steps below T, the length ties, afx_pvoc_host on a stationary
// bin-centred tone at the tile edges (its output buffer is exactly T_out rows: a write past it is caught), the statuses,
// the cost records within what afx_stft_chunks takes, and the arguments refused.  CPU only; nothing is preloaded.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "afx.h"

namespace {

int g_fail = 0;
#define CHECK(cond)                                                                              \
  do {                                                                                           \
    if (!(cond)) { std::fprintf(stderr, "pvoc_check: line %d: %s\n", __LINE__, #cond); ++g_fail; } \
  } while (0)

afx_stft_opts opts(int n_fft, int hop, int center = 1, int pad_mode = AFX_PAD_CONSTANT) {
  afx_stft_opts o{};
  o.n_fft = n_fft; o.hop = hop; o.center = center; o.pad_mode = pad_mode; o.out_kind = AFX_STFT_COMPLEX;
  return o;
}

// the steps t with double(t) rate < T, counted
int64_t count_steps(int64_t T, double rate) {
  int64_t t = 0;
  while ((double)t * rate < (double)T) ++t;
  return t;
}

}  // namespace

int main() {
  const double rates[] = {1.0, 0.5, 2.0, 0.8, 1.25, 3.7, 1.0 / 3.0, 0.1, 7.0};
  const double pi = 3.14159265358979323846;
  for (double rate : rates) {
    for (int64_t T = 0; T < 200; ++T) {
      int64_t T_out = -7;
      int32_t st = -7;
      CHECK(afx_pvoc_frames(16, 4, T, rate, &T_out, &st) == AFX_OK);
      CHECK(st == (T ? AFX_CLIP_OK : AFX_CLIP_TOO_SHORT) && T_out == (T ? count_steps(T, rate) : 0));
    }
    // one clip through the definition: bin k0 of a stationary tone e^{i phi[k0] t} keeps |D| and advances phi per step
    const int n_fft = 16, hop = 4, bins = 9, k0 = 3;
    for (int64_t T : {1, 2, 31, 32, 33, 70}) {
      std::vector<float> D((size_t)T * bins * 2, 0.f);
      const double phi = 2.0 * pi * hop * k0 / n_fft;
      for (int64_t t = 0; t < T; ++t) {
        D[(size_t)(t * bins + k0) * 2] = (float)(0.5 * std::cos(phi * t + 0.3));
        D[(size_t)(t * bins + k0) * 2 + 1] = (float)(0.5 * std::sin(phi * t + 0.3));
      }
      int64_t T_out = 0;
      int32_t st = -7;
      CHECK(afx_pvoc_frames(n_fft, hop, T, rate, &T_out, &st) == AFX_OK && T_out >= 1);
      std::vector<float> P((size_t)T_out * bins * 2, 9.f);
      CHECK(afx_pvoc_host(D.data(), T, rate, n_fft, hop, P.data(), &st) == AFX_OK && st == AFX_CLIP_OK);
      for (int64_t t = 0; t < T_out; ++t) {
        const double s = (double)t * rate;
        const bool inside = (int64_t)std::floor(s) + 1 < T;         // both columns lie in the clip
        for (int b = 0; b < bins; ++b) {
          const double re = P[(size_t)(t * bins + b) * 2], im = P[(size_t)(t * bins + b) * 2 + 1];
          if (b != k0) { CHECK(re == 0.0 && im == 0.0); continue; }
          if (!inside) continue;
          CHECK(std::fabs(std::hypot(re, im) - 0.5) < 1e-6);
          const double want = phi * t + 0.3, d = std::remainder(std::atan2(im, re) - want, 2.0 * pi);
          CHECK(std::fabs(d) < 1e-5);
        }
      }
      if (T >= 2) {                                              // a NaN bin: the status, zeros out
        D[5] = std::numeric_limits<float>::quiet_NaN();
        CHECK(afx_pvoc_host(D.data(), T, rate, n_fft, hop, P.data(), &st) == AFX_OK && st == AFX_CLIP_NONFINITE);
        bool any = false;
        for (float v : P) any = any || v != 0.f;
        CHECK(!any);
      }
    }
  }
  {  // the length rule: rint(length / rate), halves to even
    const afx_stft_opts o = opts(2048, 512);
    int64_t T, To, no;
    int32_t st;
    CHECK(afx_time_stretch_samples(&o, 5, 2.0, &T, &To, &no, &st) == AFX_OK && no == 2 && st == AFX_CLIP_OK && T == 1 && To == 1);
    CHECK(afx_time_stretch_samples(&o, 7, 2.0, &T, &To, &no, &st) == AFX_OK && no == 4);
    CHECK(afx_time_stretch_samples(&o, 1, 2.0, &T, &To, &no, &st) == AFX_OK && no == 0);
    CHECK(afx_time_stretch_samples(&o, 3, 2.0, &T, &To, &no, &st) == AFX_OK && no == 2);
    CHECK(afx_time_stretch_samples(&o, 22050, 0.8, &T, &To, &no, &st) == AFX_OK && no == 27562 && T == 44 && To == 55);
    CHECK(afx_time_stretch_samples(&o, 0, 0.8, &T, &To, &no, &st) == AFX_OK && st == AFX_CLIP_TOO_SHORT && T == 0 && To == 0 && no == 0);
    const afx_stft_opts r = opts(2048, 512, 1, AFX_PAD_REFLECT);
    CHECK(afx_time_stretch_samples(&r, 1024, 0.8, &T, &To, &no, &st) == AFX_OK && st == AFX_CLIP_TOO_SHORT);
    CHECK(afx_time_stretch_samples(&o, (int64_t)1 << 31, 0.25, &T, &To, &no, &st) == AFX_ERR_INVALID);
  }
  {  // the cost records stay within what afx_stft_chunks accepts and cut a batch
    for (int n_fft : {16, 1024, 2048, 4096})
      for (int mem : {AFX_MEM_HOST, AFX_MEM_DEVICE})
        for (int omem : {AFX_MEM_HOST, AFX_MEM_DEVICE}) {
          int64_t cost[6];
          CHECK(afx_pvoc_cost(n_fft, mem, omem, cost) == AFX_OK);
          CHECK(cost[0] == 0 && cost[1] == 0 && cost[2] > 0 && cost[2] <= (1 << 20) && cost[3] > 0 && cost[3] <= (1 << 30) && cost[4] >= 1);
          const std::vector<int64_t> w = {100, 0, 5000, 7};
          std::vector<int32_t> chunk(w.size());
          CHECK(afx_stft_chunks(w.data(), (int)w.size(), cost, 1, chunk.data()) == AFX_OK);
          CHECK(chunk[0] == 0 && chunk[1] == -1 && chunk[2] == 1 && chunk[3] == 2);
          if (n_fft == 1024 || n_fft == 2048) {
            const afx_stft_opts o = opts(n_fft, n_fft / 4);
            CHECK(afx_time_stretch_cost(&o, AFX_FMT_S16, mem, omem, cost) == AFX_OK);
            CHECK(cost[0] == 0 && cost[1] == 0 && cost[2] > 0 && cost[2] <= (1 << 20) && cost[3] > 0 && cost[3] <= (1 << 30) && cost[4] >= 1);
            CHECK(afx_stft_chunks(w.data(), (int)w.size(), cost, 1, chunk.data()) == AFX_OK && chunk[3] == 2);
          }
        }
  }
  {  // hostile arguments
    int64_t T = 0, To = 0, no = 0, cost[6];
    int32_t st = 0;
    float D[18] = {0}, P[18];
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    for (double bad : {0.0, -1.0, inf, -inf, nan}) {
      CHECK(afx_pvoc_frames(16, 4, 10, bad, &To, &st) == AFX_ERR_INVALID);
      CHECK(afx_pvoc_host(D, 1, bad, 16, 4, P, &st) == AFX_ERR_INVALID);
      const afx_stft_opts o = opts(2048, 512);
      CHECK(afx_time_stretch_samples(&o, 5000, bad, &T, &To, &no, &st) == AFX_ERR_INVALID);
    }
    const int shapes[][2] = {{15, 4}, {0, 1}, {4098, 1024}, {16, 0}, {16, 17}, {-16, 4}, {1, 1}};
    for (const auto& sh : shapes) {
      CHECK(afx_pvoc_frames(sh[0], sh[1], 10, 1.0, &To, &st) == AFX_ERR_UNSUPPORTED);
      CHECK(afx_pvoc_host(D, 1, 1.0, sh[0], sh[1], P, &st) == AFX_ERR_UNSUPPORTED);
    }
    CHECK(afx_pvoc_cost(15, AFX_MEM_HOST, AFX_MEM_HOST, cost) == AFX_ERR_UNSUPPORTED);
    CHECK(afx_pvoc_cost(16, 2, AFX_MEM_HOST, cost) == AFX_ERR_INVALID);
    CHECK(afx_pvoc_cost(16, AFX_MEM_HOST, AFX_MEM_HOST, nullptr) == AFX_ERR_INVALID);
    CHECK(afx_pvoc_frames(16, 4, 10, 1.0, nullptr, &st) == AFX_ERR_INVALID);
    CHECK(afx_pvoc_frames(16, 4, 10, 1.0, &To, nullptr) == AFX_ERR_INVALID);
    CHECK(afx_pvoc_frames(16, 4, -1, 1.0, &To, &st) == AFX_ERR_INVALID);
    CHECK(afx_pvoc_frames(4096, 4, (int64_t)1 << 31, 1.0, &To, &st) == AFX_ERR_UNSUPPORTED);   // T_out x bins >= 2^31
    CHECK(afx_pvoc_frames(16, 4, 1000, 1e-9, &To, &st) == AFX_ERR_UNSUPPORTED);
    CHECK(afx_pvoc_host(nullptr, 1, 1.0, 16, 4, P, &st) == AFX_ERR_INVALID);
    CHECK(afx_pvoc_host(D, 1, 1.0, 16, 4, nullptr, &st) == AFX_ERR_INVALID);
    CHECK(afx_pvoc_host(D, 1, 1.0, 16, 4, P, nullptr) == AFX_ERR_INVALID);
    CHECK(afx_pvoc_host(nullptr, 0, 1.0, 16, 4, nullptr, &st) == AFX_OK && st == AFX_CLIP_TOO_SHORT);
    afx_stft_opts o = opts(512, 128);
    CHECK(afx_time_stretch_samples(&o, 5000, 1.0, &T, &To, &no, &st) == AFX_ERR_UNSUPPORTED);
    CHECK(afx_time_stretch_cost(&o, AFX_FMT_F32, AFX_MEM_HOST, AFX_MEM_HOST, cost) == AFX_ERR_UNSUPPORTED);
    o = opts(2048, 512);
    CHECK(afx_time_stretch_samples(nullptr, 5000, 1.0, &T, &To, &no, &st) == AFX_ERR_INVALID);
    CHECK(afx_time_stretch_samples(&o, -1, 1.0, &T, &To, &no, &st) == AFX_ERR_INVALID);
    CHECK(afx_time_stretch_samples(&o, 5000, 1.0, &T, &To, nullptr, &st) == AFX_ERR_INVALID);
    CHECK(afx_time_stretch_cost(&o, 5, AFX_MEM_HOST, AFX_MEM_HOST, cost) == AFX_ERR_INVALID);
    CHECK(afx_time_stretch_cost(&o, AFX_FMT_F32, AFX_MEM_HOST, AFX_MEM_HOST, nullptr) == AFX_ERR_INVALID);
  }
  if (g_fail) { std::fprintf(stderr, "pvoc_check: %d failure(s)\n", g_fail); return 1; }
  std::printf("pvoc_check: ok\n");
  return 0;
}
