// Stand-alone check of the host side of spectral gating (afx_gate_host.cpp: afx_gate_params, afx_gate_cost), built with
// AddressSanitizer + UBSan (make gate-check): the tap buffers sized exactly, the largest filter the entry point takes, the
// arguments it refuses, NULL optionals.  CPU only; nothing is preloaded.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "afx.h"

namespace {

int g_fail = 0;
#define CHECK(cond)                                                                              \
  do {                                                                                           \
    if (!(cond)) { std::fprintf(stderr, "gate_check: line %d: %s\n", __LINE__, #cond); ++g_fail; } \
  } while (0)

afx_gate_opts opts(int sr, int n_fft, int hop, double hz = 500.0, double ms = 50.0) {
  afx_gate_opts o{};
  o.sr = sr; o.n_fft = n_fft; o.win_length = n_fft; o.hop = hop; o.stationary = 1; o.clip_noise = 1;
  o.padding = 30000; o.chunk_size = 600000;
  o.prop_decrease = 1.0; o.time_constant_s = 2.0; o.freq_mask_smooth_hz = hz; o.time_mask_smooth_ms = ms;
  o.thresh_n_mult = 2.0; o.sigmoid_slope = 10.0; o.n_std_thresh = 1.5;
  return o;
}

}  // namespace

int main() {
  const int rates[] = {8000, 16000, 22050, 44100, 48000, 192000};
  for (int sr : rates)
    for (int n_fft : {1024, 2048}) {
      const afx_gate_opts o = opts(sr, n_fft, n_fft / 4);
      int64_t info[4];
      double beta = 0.0;
      const int rc = afx_gate_params(&o, 32000, info, &beta, nullptr, nullptr);
      if (rc != AFX_OK) { CHECK(rc == AFX_ERR_INVALID || rc == AFX_ERR_UNSUPPORTED); continue; }
      CHECK(info[0] >= 1 && info[0] <= 128 && info[1] >= 1 && info[1] <= 64 && info[2] == 1 + (32000 + 60000) / (n_fft / 4));
      CHECK(beta > 0.0 && beta < 1.0);
      // buffers of exactly 2 n + 1 doubles
      std::vector<double> tf((size_t)(2 * info[0] + 1)), tt((size_t)(2 * info[1] + 1));
      CHECK(afx_gate_params(&o, 0, info, nullptr, tf.data(), tt.data()) == AFX_OK);
      double sf = 0.0, st = 0.0;
      for (double v : tf) { CHECK(v > 0.0); sf += v; }
      for (double v : tt) { CHECK(v > 0.0); st += v; }
      CHECK(std::fabs(sf - 1.0) < 1e-14 && std::fabs(st - 1.0) < 1e-14);
      CHECK(tf[(size_t)info[0]] >= tf[0] && tt[(size_t)info[1]] >= tt[0]);
      int64_t cost[6];
      CHECK(afx_gate_cost(&o, AFX_FMT_S16, AFX_MEM_HOST, AFX_MEM_DEVICE, 1, cost) == AFX_OK);
      CHECK(cost[0] > 0 && cost[0] <= (1 << 20) && cost[3] > 0 && cost[3] <= (1 << 30) && cost[4] >= 1);
    }
  {  // the widest filter taken: 128 bins and 64 frames a side, into buffers of exactly 257 and 129 doubles
    const afx_gate_opts o = opts(16000, 1024, 256, 128.0 * 31.25, 64.0 * 16.0);
    int64_t info[4];
    std::vector<double> tf(257), tt(129);
    CHECK(afx_gate_params(&o, 1, info, nullptr, tf.data(), tt.data()) == AFX_OK && info[0] == 128 && info[1] == 64 && info[3] == 1);
    afx_gate_opts w = opts(16000, 1024, 256, 129.0 * 31.25, 50.0);
    CHECK(afx_gate_params(&w, 1, info, nullptr, nullptr, nullptr) == AFX_ERR_UNSUPPORTED);
    w = opts(16000, 1024, 256, 500.0, 65.0 * 16.0);
    CHECK(afx_gate_params(&w, 1, info, nullptr, nullptr, nullptr) == AFX_ERR_UNSUPPORTED);
    w = opts(16000, 1024, 256, 31.25, 16.0);
    CHECK(afx_gate_params(&w, 1, info, nullptr, tf.data(), tt.data()) == AFX_OK && info[0] == 1 && info[1] == 1 && info[3] == 0);
  }
  {  // refusals
    int64_t info[4], cost[6];
    afx_gate_opts o = opts(8000, 2048, 512);
    CHECK(afx_gate_params(&o, 1, info, nullptr, nullptr, nullptr) == AFX_ERR_INVALID);
    o = opts(16000, 1024, 256);
    CHECK(afx_gate_params(nullptr, 1, info, nullptr, nullptr, nullptr) == AFX_ERR_INVALID);
    CHECK(afx_gate_params(&o, 1, nullptr, nullptr, nullptr, nullptr) == AFX_ERR_INVALID);
    CHECK(afx_gate_params(&o, -1, info, nullptr, nullptr, nullptr) == AFX_ERR_INVALID);
    CHECK(afx_gate_cost(&o, AFX_FMT_F32, AFX_MEM_HOST, AFX_MEM_HOST, 0, nullptr) == AFX_ERR_INVALID);
    CHECK(afx_gate_cost(&o, 5, AFX_MEM_HOST, AFX_MEM_HOST, 0, cost) == AFX_ERR_INVALID);
    o.win_length = 512;
    CHECK(afx_gate_params(&o, 1, info, nullptr, nullptr, nullptr) == AFX_ERR_UNSUPPORTED);
    o = opts(16000, 512, 128);
    CHECK(afx_gate_params(&o, 1, info, nullptr, nullptr, nullptr) == AFX_OK);
    CHECK(afx_gate_cost(&o, AFX_FMT_F32, AFX_MEM_HOST, AFX_MEM_HOST, 0, cost) == AFX_ERR_UNSUPPORTED);
    o = opts(16000, 1024, 256);
    o.prop_decrease = NAN;
    CHECK(afx_gate_params(&o, 1, info, nullptr, nullptr, nullptr) == AFX_ERR_INVALID);
    o = opts(16000, 1024, 256);
    o.sr = INT32_MAX; o.time_constant_s = 1e300;
    CHECK(afx_gate_params(&o, 1, info, nullptr, nullptr, nullptr) != AFX_OK || info[0] >= 1);
  }
  if (g_fail) { std::fprintf(stderr, "gate_check: %d failure(s)\n", g_fail); return 1; }
  std::printf("gate_check: ok\n");
  return 0;
}
