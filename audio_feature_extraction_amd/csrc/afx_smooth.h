// Sample-domain smoothers with scipy semantics (scipy.signal.medfilt, scipy.signal.savgol_filter(mode='interp')) and the
// experiment extractor's energy and ZCR groups built on them (04_feature_extraction_experiment/feature_extractor.py:341-483):
// geometry, tables, the clip record, and the arithmetic the kernels of afx_smooth.hip and the host executors of
// afx_smooth_host.cpp share.  Internal to libafx.so; include/afx.h (afx_medfilt_batch, afx_savgol_batch, afx_energy_zcr_batch,
// their host executors, afx_savgol_tables, afx_smooth_geometry) is the ABI.
//
// A tile is kSmTile consecutive samples of one clip; a workgroup stages it once into LDS with a halo of half the window on
// both sides, every index checked against the clip's own range (zeros outside), and each lane then produces the outputs
// e, e + 256, .. of the tile from LDS.
//   median   the result is one of the inputs or the padding's 0, so any selection gives the same value; a zero result is
//            always +0 (v + 0.0f), which makes it the same bits as well.
//   savgol   float32 samples widened to float64, one chain of fused multiply-adds from 0 over the taps in ascending order
//            (sg_dot), one rounding to float32.  The first and last W / 2 outputs of a clip are the same chain over the
//            clip's first / last W samples with a row of the edge matrices.
// The group statistics are sums in one fixed order: a lane's own terms in ascending order, then a halving tree over the lanes
// (sm_tree_sum); the host executor walks the same order.
#pragma once
#include <cmath>
#include <cstdint>

#include "afx_filt.h"

namespace afx {

constexpr int kSmTile = 2048;                  // samples of a tile
constexpr int kSmThreads = 256;                // lanes of a workgroup: 8 outputs each
constexpr int kSmMaxK = 31;                    // largest median kernel and Savitzky-Golay window
constexpr int kSmMaxHalo = kSmMaxK / 2;
constexpr int kSgMaxP = 5, kSgMaxDeriv = 2;
constexpr int kSgRow = 32;                     // row stride of the tables
constexpr int kEzStatLanes = 256;              // lanes of the per-clip statistics (partials of sm_tree_sum)
constexpr int kEzFrameLanes = 64;              // lanes of a frame's sum of squares
constexpr int kEzWin = 10;                     // window of the local stability

// one clip of a chunk as the kernels see it (FiltClip's layout: the fused call hands the same records to the filter)
using SmClip = FiltClip;

// c: interior taps in convolution order (scipy.signal.savgol_coeffs): y[i] = sum_k c[k] x[i + W / 2 - k].  left[r] / right[r]:
// output r / n - W / 2 + r as weights over the clip's first / last W samples in ascending order.  t[k] = c[W - 1 - k]: the
// taps as the chain walks them.
struct SgTab {
  double t[kSgRow];
  double left[kSmMaxHalo][kSgRow];
  double right[kSmMaxHalo][kSgRow];
  int32_t W, h;
};

struct SmSrc { const void* in; int64_t off; int fmt; };     // AFX_FMT_*
AFX_HD inline float sm_raw(const SmSrc& s, int64_t i) {
  if (s.fmt == 1) return (float)((const int16_t*)s.in)[s.off + i] * (1.0f / 32768.0f);
  return ((const float*)s.in)[s.off + i];
}

AFX_HD inline float sm_min(float a, float b) { return a < b ? a : b; }
AFX_HD inline float sm_max(float a, float b) { return a < b ? b : a; }
AFX_HD inline float sm_med3(float a, float b, float c) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_fmed3f(a, b, c);
#else
  return sm_max(sm_min(a, b), sm_min(sm_max(a, b), c));
#endif
}
// the lowest and the highest of a, b, c, d cannot be the median of five
AFX_HD inline float sm_med5(float a, float b, float c, float d, float e) {
  const float f = sm_max(sm_min(a, b), sm_min(c, d));
  const float g = sm_min(sm_max(a, b), sm_max(c, d));
  return sm_med3(e, f, g);
}
// the element of w[0 .. K) with fewer than K / 2 + 1 elements below it and more than K / 2 not above it
template <typename WP>
AFX_HD inline float sm_med_rank(WP w, int K) {
  const int h = K / 2;
  float r = 0.0f;
  for (int j = 0; j < K; ++j) {
    const float v = w[j];
    int lt = 0, le = 0;
    for (int k = 0; k < K; ++k) { const float u = w[k]; lt += u < v ? 1 : 0; le += u <= v ? 1 : 0; }
    if (lt <= h && h < le) r = v;
  }
  return r;
}
// w: the K samples around the output (zeros outside the clip)
template <typename WP>
AFX_HD inline float sm_median(WP w, int K) {
  float r;
  if (K == 1) r = w[0];
  else if (K == 3) r = sm_med3(w[0], w[1], w[2]);
  else if (K == 5) r = sm_med5(w[0], w[1], w[2], w[3], w[4]);
  else r = sm_med_rank(w, K);
  return r + 0.0f;
}

// sum_k t[k] x[k], k ascending, every product fused into the sum
template <typename TP, typename XP>
AFX_HD inline double sg_dot(TP t, XP x, int W) {
  double a = 0.0;
  for (int k = 0; k < W; ++k) a = fma(t[k], (double)x[k], a);
  return a;
}
struct SmSrcAt {                               // x[k] = sample first + k of a source
  SmSrc s; int64_t first;
  AFX_HD float operator[](int k) const { return sm_raw(s, first + k); }
};
// a clip-edge output i (i < h or i >= n - h) of a clip of n >= W samples
template <typename TabP>
AFX_HD inline float sg_edge(TabP tab, const SmSrc& s, int64_t n, int64_t i) {
  const int W = tab->W, h = tab->h;
  if (i < h) return (float)sg_dot(tab->left[i], SmSrcAt{s, 0}, W);
  return (float)sg_dot(tab->right[i - (n - h)], SmSrcAt{s, n - W}, W);
}

// ---- the energy and ZCR groups ----
// per-clip framing (feature_extractor.py:42-60, 352-353)
struct EzFrame { int32_t fl, hop; int64_t T; };
AFX_HD inline EzFrame ez_framing(int64_t n, int frame_length, int hop_length) {
  EzFrame f;
  f.fl = frame_length;
  if (n < frame_length) {
    int p = 1;
    while ((int64_t)2 * p <= n) p *= 2;
    f.fl = p < 64 ? 64 : p;
  }
  f.hop = hop_length < f.fl / 4 ? hop_length : f.fl / 4;
  f.T = 1 + n / f.hop;
  return f;
}

// the halving tree over L partials (L a power of two): p[j] += p[j + w] for j < w, w = L / 2 .. 1
inline double sm_tree_sum(double* p, int L) {
  for (int w = L / 2; w > 0; w >>= 1)
    for (int j = 0; j < w; ++j) p[j] = p[j] + p[j + w];
  return p[0];
}

// sign bit of a smoothed sample after librosa.util.normalize and the 1e-10 clip of librosa.zero_crossings: a peak below
// tiny(float32) leaves the signal unscaled, and every sample of such a signal is within the clip
AFX_HD inline bool ez_neg(float s, float peak) {
  if (!(peak >= 1.17549435e-38f)) return false;
  if (fabs((double)s / (double)peak) <= 1e-10) return false;
  return s < 0.0f;
}

// population standard deviation of r[0 .. w): sequential sums
template <typename RP>
AFX_HD inline double ez_window_std(RP r, int w) {
  double a = 0.0;
  for (int k = 0; k < w; ++k) a = a + r[k];
  const double m = a / (double)w;
  double v = 0.0;
  for (int k = 0; k < w; ++k) { const double d = r[k] - m; v = fma(d, d, v); }
  return sqrt(v / (double)w);
}

// numpy's linear percentile from the two order statistics around the virtual index (numpy.lib._function_base_impl._lerp)
AFX_HD inline double ez_lerp(double a, double b, double g) {
  AFX_FILT_NO_CONTRACT
  const double d = b - a;
  if (g >= 0.5) { const double u = d * (1.0 - g); return b - u; }
  const double u = d * g;
  return a + u;
}
AFX_HD inline void ez_p10_index(int64_t T, int64_t* k0, int64_t* k1, double* g) {
  AFX_FILT_NO_CONTRACT
  const double v = (double)(T - 1) * 0.1;
  const double f = floor(v);
  *k0 = (int64_t)f;
  *k1 = *k0 + 1 < T ? *k0 + 1 : T - 1;
  *g = v - f;
}

// record slots of afx_energy_zcr_batch (AFX_EZ_* of afx.h)
constexpr int kEzN = 12;

// afx_smooth_host.cpp (host-only)
// nullptr, or why (window_length, polyorder, deriv, delta) is refused; *code: AFX_ERR_INVALID / AFX_ERR_UNSUPPORTED
const char* savgol_refusal(int W, int P, int deriv, double delta, int* code);
void savgol_build_tab(int W, int P, int deriv, double delta, SgTab& t);
const char* medfilt_refusal(int K, int* code);
const char* ez_refusal(int sr, int frame_length, int hop_length, int flags, int* code);

}  // namespace afx

#if defined(__HIP_PLATFORM_AMD__) && !defined(AFX_FILT_HOST_ONLY)
#include <hip/hip_runtime_api.h>
namespace afx {
// afx_smooth.hip.  clips, bad, tab: device memory; n: clip records; n_tiles: tiles of all records.  bad[c * bad_stride] != 0:
// clip c holds a NaN / inf sample and none of its outputs is written
hipError_t launch_sm_check(hipStream_t s, const void* in, int fmt, const SmClip* clips, int n, uint32_t* bad);
hipError_t launch_medfilt(hipStream_t s, const void* in, int fmt, int K, const SmClip* clips, int n, int n_tiles,
                          const uint32_t* bad, int bad_stride, float* out);
// clips shorter than min_n are copied (the ZCR chain's guard); the public entry point never hands one over
hipError_t launch_savgol(hipStream_t s, const void* in, int fmt, const SgTab* tab, int64_t min_n, const SmClip* clips, int n,
                         int n_tiles, const uint32_t* bad, int bad_stride, float* out);

// one clip of the fused call: its samples at y_off of the groups' input and at off of the workspace signals, its T frames at
// first_frame of the two row buffers
struct EzClip { int64_t y_off, off, n, T, first_frame; int32_t fl, hop; };
static_assert(sizeof(EzClip) == 48, "EzClip layout");
// peak[c] = max |s| of the smoothed signal
hipError_t launch_ez_peak(hipStream_t s, const float* sig, const EzClip* clips, int n, const uint32_t* bad, int bad_stride,
                          float* peak);
// neg[off + i] = ez_neg(sig[off + i], peak[c]); clips: tile records with in_off == out_off == the clip's off
hipError_t launch_ez_sign(hipStream_t s, const float* sig, const SmClip* clips, int n, int n_tiles, const uint32_t* bad,
                          int bad_stride, const float* peak, uint8_t* neg);
// energy[first_frame + t] = sqrt(mean square of frame t of y) (y != nullptr), rate[first_frame + t] = crossings / fl
// (neg != nullptr); n_frames: frames of all records
hipError_t launch_ez_frames(hipStream_t s, const void* y, int y_fmt, const uint8_t* neg, const EzClip* clips, int n,
                            int64_t n_frames, const uint32_t* bad, int bad_stride, double* energy, double* rate);
// rec[c][kEzN]: the statistics slots (the others are the host's)
hipError_t launch_ez_stats(hipStream_t s, const EzClip* clips, int n, const uint32_t* bad, int bad_stride, int flags,
                           const double* energy, const double* rate, double* rec);
}  // namespace afx
#endif
