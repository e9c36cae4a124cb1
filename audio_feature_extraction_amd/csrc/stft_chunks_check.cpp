// Stand-alone check of the chunk cut of the STFT-based groups (afx_host.cpp: cut_stft_chunk behind afx_stft_chunks), built
// with AddressSanitizer + UBSan by `make stft-chunks-check` and run on the CPU: the caps, the exact fit and the largest
// arguments the query accepts, each result written into an exactly sized heap buffer (an index past it is an ASan report,
// a sum past 2^63 a UBSan one).  Exit status 0: every check held.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "afx.h"

namespace {

int g_fail = 0;
#define CHECK(cond)                                                              \
  do {                                                                           \
    if (!(cond)) { std::fprintf(stderr, "stft_chunks_check: line %d: %s\n", __LINE__, #cond); ++g_fail; } \
  } while (0)

std::vector<int32_t> cut(const std::vector<int64_t>& len, const int64_t (&cost)[6], int64_t budget, int expect = AFX_OK) {
  std::vector<int32_t> out(len.size(), -7);
  CHECK(afx_stft_chunks(len.data(), (int)len.size(), cost, budget, out.data()) == expect);
  return out;
}

}  // namespace

int main() {
  const int64_t hpss[6] = {1032 * 8 * 2 + 17 * 4, 0, 12, 128, 64, 65535};
  const int64_t rhythm[6] = {1040 * 4 + 128 * 4 + 4, 344 * 8, 8, 344 * 8 + 128, 16, INT32_MAX / 2};
  const int64_t most[6] = {1 << 20, 1 << 20, 1 << 20, 1 << 20, 1, INT32_MAX};
  const int64_t big = (int64_t)1 << 62;
  // 40000 clips of one sample, an empty one after every third: 32768 records, then the rest
  std::vector<int64_t> len;
  for (int i = 0; i < 40000; ++i) { len.push_back(1); if (i % 3 == 2) len.push_back(0); }
  std::vector<int32_t> c = cut(len, rhythm, big);
  int live = 0;
  for (size_t i = 0; i < len.size(); ++i) {
    if (len[i] == 0) { CHECK(c[i] == -1); continue; }
    CHECK(c[i] == (live < 32768 ? 0 : 1));
    ++live;
  }
  c = cut(len, rhythm, 1);                                   // every clip its own chunk
  CHECK(c[0] == 0 && c[1] == 1 && c[3] == -1 && c[len.size() - 1] == 39999);
  // the tile cap of afx_hpss_batch: 127 x 513 tiles fit 65535, 128 x 513 do not
  c = cut(std::vector<int64_t>(128, (int64_t)1 << 24), hpss, big);
  CHECK(c[0] == 0 && c[126] == 0 && c[127] == 1);
  // a clip that lands on the budget stays; one byte less and it starts the next chunk
  const int64_t b5000 = 10 * hpss[0] + 5000 * hpss[2] + hpss[3], b700 = 2 * hpss[0] + 700 * hpss[2] + hpss[3];
  c = cut({5000, 0, 700}, hpss, b5000 + b700);
  CHECK(c[0] == 0 && c[1] == -1 && c[2] == 0);
  c = cut({5000, 0, 700}, hpss, b5000 + b700 - 1);
  CHECK(c[0] == 0 && c[1] == -1 && c[2] == 1);
  // the largest clips at the largest costs and budget: no sum overflows
  c = cut(std::vector<int64_t>(4096, (int64_t)1 << 31), most, big);
  CHECK(c[0] == 0 && c[4095] > 0);
  c = cut({}, hpss, big);
  CHECK(c.empty());
  // refusals
  cut({-1}, hpss, 1, AFX_ERR_INVALID);
  cut({((int64_t)1 << 31) + 1}, hpss, 1, AFX_ERR_INVALID);
  cut({1}, hpss, 0, AFX_ERR_INVALID);
  cut({1}, hpss, big + 1, AFX_ERR_INVALID);
  const int64_t no_tile[6] = {1, 1, 1, 1, 0, 1};
  cut({1}, no_tile, 1, AFX_ERR_INVALID);
  // afx_denoise_batch's record through its own entry point: six clips at 400000 bytes are (5000) (12345, 700) (9000, 3000) (7000)
  int64_t dn[6] = {0, 0, 0, 0, 0, 0};
  CHECK(afx_denoise_cost(0, AFX_FMT_F32, AFX_MEM_HOST, dn) == AFX_OK && dn[0] == 1032 * 8 && dn[2] == 12 && dn[3] == 128 + 1040 * 4 + 32);
  c = cut({5000, 12345, 700, 9000, 3000, 7000}, dn, 400000);
  CHECK(c[0] == 0 && c[1] == 1 && c[2] == 1 && c[3] == 2 && c[4] == 2 && c[5] == 3);
  CHECK(afx_denoise_cost(AFX_DENOISE_VAD, AFX_FMT_S16, AFX_MEM_DEVICE, dn) == AFX_OK && dn[2] == 12 && dn[3] == 128 + 1040 * 4 + 36);
  CHECK(afx_denoise_cost(AFX_FLAG_TRIM, AFX_FMT_F32, AFX_MEM_HOST, dn) == AFX_ERR_UNSUPPORTED);
  CHECK(afx_denoise_cost(4, AFX_FMT_F32, AFX_MEM_HOST, dn) == AFX_ERR_INVALID);
  CHECK(afx_denoise_cost(0, 9, AFX_MEM_HOST, dn) == AFX_ERR_INVALID && afx_denoise_cost(0, AFX_FMT_F32, AFX_MEM_HOST, nullptr) == AFX_ERR_INVALID);
  if (g_fail) { std::fprintf(stderr, "stft_chunks_check: %d check(s) failed\n", g_fail); return 1; }
  std::printf("stft_chunks_check: ok\n");
  return 0;
}
