// The host side of spectral gating (afx_gate.h): what noisereduce derives from its arguments -- the smoothing filter's
// sizes and taps, the recurrence's coefficient, the frame count -- and the cost record of afx_gate_batch.  No device.
#include <climits>
#include <cmath>
#include <cstring>
#include <string>

#include "afx.h"
#include "afx_gate.h"
#include "afx_internal.h"

namespace afx {

// v(n) = concatenate(linspace(0, 1, n + 1, endpoint=False), linspace(1, 0, n + 2))[1:-1] / its sum, as numpy evaluates it
static void gate_taps(int n, double* v) {
  const double up = 1.0 / (double)(n + 1), down = -1.0 / (double)(n + 1);
  int m = 0;
  for (int k = 1; k <= n; ++k) v[m++] = (double)k * up;
  for (int j = 0; j <= n; ++j) v[m++] = (double)j * down + 1.0;
  double s = 0.0;
  for (int i = 0; i < m; ++i) s += v[i];
  for (int i = 0; i < m; ++i) v[i] /= s;
}

int gate_derive(const afx_gate_opts& o, GateDerived& d, const char** why) {
  auto fail = [&](int code, const char* w) { *why = w; return code; };
  if (o.sr < 1) return fail(AFX_ERR_INVALID, "sr must be positive");
  if (o.n_fft < 2 || (o.n_fft & 1) || o.hop < 1 || o.win_length < 1) return fail(AFX_ERR_INVALID, "n_fft must be even and at least 2, hop and win_length positive");
  if (o.win_length != o.n_fft) return fail(AFX_ERR_UNSUPPORTED, "win_length != n_fft is not supported");
  if (!(o.prop_decrease >= 0.0 && o.prop_decrease <= 1.0)) return fail(AFX_ERR_INVALID, "prop_decrease must be in [0, 1]");
  if (!(o.time_constant_s > 0.0) || !std::isfinite(o.time_constant_s)) return fail(AFX_ERR_INVALID, "time_constant_s must be positive and finite");
  if (!std::isfinite(o.freq_mask_smooth_hz) || !std::isfinite(o.time_mask_smooth_ms) || !std::isfinite(o.thresh_n_mult) ||
      !std::isfinite(o.sigmoid_slope) || !std::isfinite(o.n_std_thresh))
    return fail(AFX_ERR_INVALID, "the smoothing widths and thresholds must be finite");
  if (o.padding < 0 || o.chunk_size < 1) return fail(AFX_ERR_INVALID, "padding must not be negative and chunk_size positive");
  if (o.padding > kGateMaxPad || o.chunk_size > kGateMaxChunk) return fail(AFX_ERR_UNSUPPORTED, "padding above 2^20 or chunk_size above 2^24 is not supported");
  // noisereduce: int(freq_mask_smooth_hz / (sr / (n_fft / 2))), int(time_mask_smooth_ms / ((hop / sr) * 1000))
  const double nf = o.freq_mask_smooth_hz / ((double)o.sr / ((double)o.n_fft / 2.0));
  const double nt = o.time_mask_smooth_ms / (((double)o.hop / (double)o.sr) * 1000.0);
  if (!(nf >= 1.0)) return fail(AFX_ERR_INVALID, "freq_mask_smooth_hz is below one bin: sr / (n_fft / 2) Hz at least");
  if (!(nt >= 1.0)) return fail(AFX_ERR_INVALID, "time_mask_smooth_ms is below one frame: hop / sr * 1000 ms at least");
  if (nf >= (double)(kGateMaxNf + 1) || nt >= (double)(kGateMaxNt + 1)) return fail(AFX_ERR_UNSUPPORTED, "the smoothing filter spans more than 128 bins or 64 frames a side");
  d.n_f = (int)nf; d.n_t = (int)nt;
  d.smooth = !(d.n_f == 1 && d.n_t == 1);
  gate_taps(d.n_f, d.vf);
  gate_taps(d.n_t, d.vt);
  const double tf = o.time_constant_s * (double)o.sr / (double)o.hop;
  d.beta = (std::sqrt(1.0 + 4.0 * (tf * tf)) - 1.0) / (2.0 * (tf * tf));
  return AFX_OK;
}

void gate_cost(int n_fft, int stationary, int padding, int sample_fmt, int mem_kind, int out_mem_kind, int with_noise, StftCost& cost) {
  const int64_t hop = n_fft / 4, pitch = gate_pitch(n_fft), r = 512 / hop;
  // a frame: its magnitude and mask rows, the noise grid's row and the bits (stationary) or the forward pass, the time row
  const int64_t frame = pitch * 4 * 2 + (stationary ? pitch * 4 + gate_words(n_fft) * 4 : pitch * 8) + (int64_t)n_fft * 4;
  const int64_t up = mem_kind != AFX_MEM_HOST ? 0 : sample_fmt == AFX_FMT_S16 ? 2 : 4;
  cost = StftCost{};
  cost.per_frame = r * frame;                              // 1 + len / hop <= r (1 + len / 512) frames of the clip itself
  cost.per_sample = (4 + up) * (with_noise ? 2 : 1) + (out_mem_kind == AFX_MEM_HOST ? 4 : 0);
  cost.per_clip = (2 * (int64_t)padding / hop + 3) * frame + 2 * (int64_t)sizeof(GateGrid) + 2 * pitch * 8 + 8 + 128;
  cost.tile = 16;
  cost.tile_cap = INT32_MAX / 2;
}

}  // namespace afx

using namespace afx;

static bool gate_shape_ok(const afx_gate_opts& o) {
  return (o.n_fft == 1024 || o.n_fft == 2048) && o.hop == o.n_fft / 4;
}

extern "C" int afx_gate_params(const afx_gate_opts* opts, int64_t length, int64_t* info, double* beta, double* taps_f, double* taps_t) {
  if (!opts || !info) { set_error("afx_gate_params: null argument"); return AFX_ERR_INVALID; }
  if (length < 0) { set_error("afx_gate_params: negative length"); return AFX_ERR_INVALID; }
  GateDerived d;
  const char* why = "";
  const int rc = gate_derive(*opts, d, &why);
  if (rc != AFX_OK) { set_error(std::string("afx_gate_params: ") + why); return rc; }
  info[0] = d.n_f; info[1] = d.n_t; info[2] = gate_frames(length, opts->hop, opts->padding); info[3] = d.smooth ? 1 : 0;
  if (beta) *beta = d.beta;
  if (taps_f) std::memcpy(taps_f, d.vf, (size_t)(2 * d.n_f + 1) * sizeof(double));
  if (taps_t) std::memcpy(taps_t, d.vt, (size_t)(2 * d.n_t + 1) * sizeof(double));
  return AFX_OK;
}

extern "C" int afx_gate_cost(const afx_gate_opts* opts, int sample_fmt, int mem_kind, int out_mem_kind, int with_noise, int64_t* cost) {
  if (!opts || !cost) { set_error("afx_gate_cost: null argument"); return AFX_ERR_INVALID; }
  if ((sample_fmt != AFX_FMT_F32 && sample_fmt != AFX_FMT_S16) || (mem_kind != AFX_MEM_HOST && mem_kind != AFX_MEM_DEVICE) ||
      (out_mem_kind != AFX_MEM_HOST && out_mem_kind != AFX_MEM_DEVICE)) {
    set_error("afx_gate_cost: unknown sample format or memory kind");
    return AFX_ERR_INVALID;
  }
  GateDerived d;
  const char* why = "";
  const int rc = gate_derive(*opts, d, &why);
  if (rc != AFX_OK) { set_error(std::string("afx_gate_cost: ") + why); return rc; }
  if (!gate_shape_ok(*opts)) { set_error("afx_gate_cost: n_fft / hop must be 1024 / 256 or 2048 / 512"); return AFX_ERR_UNSUPPORTED; }
  StftCost c;
  gate_cost(opts->n_fft, opts->stationary, opts->padding, sample_fmt, mem_kind, out_mem_kind, with_noise, c);
  const int64_t v[6] = {c.per_frame, c.per_tile, c.per_sample, c.per_clip, c.tile, c.tile_cap};
  std::memcpy(cost, v, sizeof(v));
  return AFX_OK;
}
