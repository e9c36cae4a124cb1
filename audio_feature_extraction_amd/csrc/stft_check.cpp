// Stand-alone check of the host side of stft / istft (afx_stft_host.cpp: afx_stft_frames, afx_istft_samples, afx_stft_cost),
// built with AddressSanitizer + UBSan (make stft-check): the frame count and the statuses over the lengths around the frame
// and the hop against a plain restatement, istft's length rule, the cost record within what afx_stft_chunks takes, and the
// arguments refused.  CPU only; nothing is preloaded.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "afx.h"

namespace {

int g_fail = 0;
#define CHECK(cond)                                                                              \
  do {                                                                                           \
    if (!(cond)) { std::fprintf(stderr, "stft_check: line %d: %s\n", __LINE__, #cond); ++g_fail; } \
  } while (0)

afx_stft_opts opts(int n_fft, int hop, int center = 1, int pad_mode = AFX_PAD_CONSTANT, int kind = AFX_STFT_COMPLEX) {
  afx_stft_opts o{};
  o.n_fft = n_fft; o.hop = hop; o.center = center; o.pad_mode = pad_mode; o.out_kind = kind;
  return o;
}

// the definition, restated: frames of the padded clip, or -1 for a clip that is too short
int64_t want_frames(const afx_stft_opts& o, int64_t L) {
  if (L == 0) return -1;
  if (!o.center) return L < o.n_fft ? -1 : 1 + (L - o.n_fft) / o.hop;
  if (o.pad_mode == AFX_PAD_REFLECT && L <= o.n_fft / 2) return -1;
  return 1 + L / o.hop;
}

}  // namespace

int main() {
  for (int n : {1024, 2048}) {
    const int hops[] = {1, 160, 441, n / 16, n / 4, n / 2, n - 1, n};
    for (int hop : hops)
      for (int center : {0, 1})
        for (int pad : {AFX_PAD_CONSTANT, AFX_PAD_REFLECT}) {
          const afx_stft_opts o = opts(n, hop, center, pad);
          const int64_t lens[] = {0, 1, n / 2 - 1, n / 2, n / 2 + 1, n - 1, n, n + 1, n + hop - 1, n + hop, 3 * (int64_t)hop - 1,
                                  3 * (int64_t)hop, 3 * (int64_t)hop + 1, 220500, (int64_t)1 << 31};
          for (int64_t L : lens) {
            int64_t T = -7;
            int32_t st = -7;
            CHECK(afx_stft_frames(&o, L, &T, &st) == AFX_OK);
            const int64_t w = want_frames(o, L);
            CHECK(st == (w < 0 ? AFX_CLIP_TOO_SHORT : AFX_CLIP_OK) && T == (w < 0 ? 0 : w));
            if (w < 0) continue;
            // the frames fit the padded clip, and one more would not
            const int64_t padded = L + (center ? n : 0);
            CHECK((T - 1) * hop + n <= padded && T * hop + n > padded);
            // istft of those frames: the natural length, a shorter and a longer one
            const int64_t s = center ? n / 2 : 0, full = n + (int64_t)hop * (T - 1);
            int64_t nf = -1, no = -1;
            if (T > (int64_t)1 << 31) {                          // hop 1 on 2^31 samples: one frame more than istft takes
              CHECK(afx_istft_samples(&o, T, -1, &nf, &no) == AFX_ERR_INVALID);
              continue;
            }
            CHECK(afx_istft_samples(&o, T, -1, &nf, &no) == AFX_OK && nf == T && no == full - 2 * s);
            CHECK(afx_istft_samples(&o, T, -12345, &nf, &no) == AFX_OK && nf == T && no == full - 2 * s);
            CHECK(afx_istft_samples(&o, T, L, &nf, &no) == AFX_OK && no == L && nf >= 1 && nf <= T);
            CHECK(nf == T || (nf * hop >= L + 2 * s && (nf - 1) * hop < L + 2 * s));
            if (full + 99 <= (int64_t)1 << 31)
              CHECK(afx_istft_samples(&o, T, full + 99, &nf, &no) == AFX_OK && nf == T && no == full + 99);
            else
              CHECK(afx_istft_samples(&o, T, full + 99, &nf, &no) == AFX_ERR_INVALID);
            if (L > 1) {
              CHECK(afx_istft_samples(&o, T, 1, &nf, &no) == AFX_OK && no == 1 && nf >= 1 && (nf == T || (nf - 1) * hop < 1 + 2 * s));
            }
          }
          int64_t nf = -1, no = -1;
          CHECK(afx_istft_samples(&o, 0, -1, &nf, &no) == AFX_OK && nf == 0 && no == 0);
          CHECK(afx_istft_samples(&o, 1, -1, &nf, &no) == AFX_OK && nf == 1 && no == (center ? 0 : n));
          CHECK(afx_istft_samples(&o, 5, 0, &nf, &no) == AFX_OK && no == 0 && nf <= 5);
          // the cost record stays within what afx_stft_chunks accepts and cuts a batch
          for (int inverse : {0, 1})
            for (int mem : {AFX_MEM_HOST, AFX_MEM_DEVICE})
              for (int omem : {AFX_MEM_HOST, AFX_MEM_DEVICE}) {
                int64_t cost[6];
                CHECK(afx_stft_cost(&o, AFX_FMT_S16, mem, omem, inverse, cost) == AFX_OK);
                CHECK(cost[0] == 0 && cost[1] == 0 && cost[2] > 0 && cost[2] <= (1 << 20) && cost[3] > 0 && cost[3] <= (1 << 30) && cost[4] >= 1);
                const std::vector<int64_t> len = {1000, 0, 50000, 7};
                std::vector<int32_t> chunk(len.size());
                CHECK(afx_stft_chunks(len.data(), (int)len.size(), cost, 1, chunk.data()) == AFX_OK);
                CHECK(chunk[0] == 0 && chunk[1] == -1 && chunk[2] == 1 && chunk[3] == 2);
                CHECK(afx_stft_chunks(len.data(), (int)len.size(), cost, (int64_t)2 << 30, chunk.data()) == AFX_OK && chunk[3] == 0);
              }
        }
  }
  {  // hostile arguments
    int64_t T = 0, nf = 0, no = 0, cost[6];
    int32_t st = 0;
    afx_stft_opts o = opts(2048, 512);
    CHECK(afx_stft_frames(nullptr, 10, &T, &st) == AFX_ERR_INVALID);
    CHECK(afx_stft_frames(&o, 10, nullptr, &st) == AFX_ERR_INVALID);
    CHECK(afx_stft_frames(&o, 10, &T, nullptr) == AFX_ERR_INVALID);
    CHECK(afx_stft_frames(&o, -1, &T, &st) == AFX_ERR_INVALID);
    CHECK(afx_stft_frames(&o, ((int64_t)1 << 31) + 1, &T, &st) == AFX_ERR_INVALID);
    CHECK(afx_istft_samples(nullptr, 1, -1, &nf, &no) == AFX_ERR_INVALID);
    CHECK(afx_istft_samples(&o, 1, -1, nullptr, &no) == AFX_ERR_INVALID);
    CHECK(afx_istft_samples(&o, 1, -1, &nf, nullptr) == AFX_ERR_INVALID);
    CHECK(afx_istft_samples(&o, -1, -1, &nf, &no) == AFX_ERR_INVALID);
    CHECK(afx_istft_samples(&o, 1, INT64_MAX, &nf, &no) == AFX_ERR_INVALID);
    CHECK(afx_istft_samples(&o, 1, INT64_MIN, &nf, &no) == AFX_OK);
    CHECK(afx_stft_cost(nullptr, AFX_FMT_F32, AFX_MEM_HOST, AFX_MEM_HOST, 0, cost) == AFX_ERR_INVALID);
    CHECK(afx_stft_cost(&o, AFX_FMT_F32, AFX_MEM_HOST, AFX_MEM_HOST, 0, nullptr) == AFX_ERR_INVALID);
    CHECK(afx_stft_cost(&o, 5, AFX_MEM_HOST, AFX_MEM_HOST, 0, cost) == AFX_ERR_INVALID);
    CHECK(afx_stft_cost(&o, AFX_FMT_F32, 2, AFX_MEM_HOST, 0, cost) == AFX_ERR_INVALID);
    const int shapes[][2] = {{512, 128}, {2048, 0}, {2048, -512}, {2048, 2049}, {1024, 1025}, {4096, 1024}, {0, 0}, {1000, 250}, {-2048, 512}};
    for (const auto& sh : shapes) {
      o = opts(sh[0], sh[1]);
      CHECK(afx_stft_frames(&o, 5000, &T, &st) == AFX_ERR_UNSUPPORTED);
      CHECK(afx_istft_samples(&o, 5, -1, &nf, &no) == AFX_ERR_UNSUPPORTED);
      CHECK(afx_stft_cost(&o, AFX_FMT_F32, AFX_MEM_HOST, AFX_MEM_HOST, 0, cost) == AFX_ERR_UNSUPPORTED);
    }
    o = opts(2048, 512, 2);
    CHECK(afx_stft_frames(&o, 5000, &T, &st) == AFX_ERR_INVALID);
    o = opts(2048, 512, 1, 2);
    CHECK(afx_stft_frames(&o, 5000, &T, &st) == AFX_ERR_INVALID);
    o = opts(2048, 512, 1, AFX_PAD_CONSTANT, 3);
    CHECK(afx_stft_cost(&o, AFX_FMT_F32, AFX_MEM_HOST, AFX_MEM_HOST, 0, cost) == AFX_ERR_INVALID);
  }
  if (g_fail) { std::fprintf(stderr, "stft_check: %d failure(s)\n", g_fail); return 1; }
  std::printf("stft_check: ok\n");
  return 0;
}
