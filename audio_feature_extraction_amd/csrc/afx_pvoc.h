// librosa-style phase_vocoder and effects.time_stretch (afx_pvoc.hip, afx_pvoc_host.cpp).  The step
// rule and the phase increment the host and the kernels share, the clip record, the cost records and the launchers.
// Internal to libafx.so.
#pragma once
#include <cmath>
#include <cstdint>

#include <hip/hip_runtime_api.h>

#include "afx.h"
#include "afx_hpss.h"
#include "afx_stft.h"

namespace afx {

constexpr int kPvocTile = AFX_PVOC_TILE;   // output steps per tile: the unit of the fixed summation order
constexpr double kTwoPi = 6.283185307179586476925286766559;

// Step t of a stretch by `rate`: s_t = t rate in float64, the column j = floor(s_t) and the weight a = s_t - j of column
// j + 1.  The one place the step positions come from (a caller's table of positions would replace this alone).
__host__ __device__ inline void pvoc_step(int64_t t, double rate, int64_t* j, double* a) {
  const double s = (double)t * rate;
  const double f = floor(s);
  *j = (int64_t)f;
  *a = s - f;
}

// d - 2 pi rint(d / 2 pi), halves to even; the product is rounded before the difference
__host__ __device__ inline double pvoc_wrap(double d) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  const double r = rint(d / kTwoPi);
  const double p = kTwoPi * r;
  return d - p;
}

// phi[k] = 2 pi hop k / n_fft
__host__ __device__ inline double pvoc_phi(int hop, int n_fft, int k) { return kTwoPi * (double)hop * (double)k / (double)n_fft; }

// What step t adds to the accumulator of a bin: phi + wrapped (angle(c1) - angle(c0) - phi), with phi reduced to
// [-pi, pi] in the first term (phi_r = pvoc_wrap(phi)): only acc mod 2 pi is observable
__host__ __device__ inline double pvoc_inc(double ang0, double ang1, double phi, double phi_r) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  const double d = (ang1 - ang0) - phi;
  return phi_r + pvoc_wrap(d);
}

// (1 - a) |c0| + a |c1| in float32: two products and a sum, each rounded once
__host__ __device__ inline float pvoc_mag(float m0, float m1, double a) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  const float w1 = (float)a, w0 = (float)(1.0 - a);
  const float p0 = w0 * m0;
  const float p1 = w1 * m1;
  return p0 + p1;
}

// One clip of a chunk of afx_pvoc_batch / afx_time_stretch_batch (host-built)
struct PvocClip {
  int64_t spec_off;     // row 0 of D, in complex64 elements
  int64_t row_base;     // first of the clip's T rows in the angle and magnitude planes
  int64_t out_off;      // row 0 of the result, in complex64 elements
  int64_t tile_base;    // first of the clip's ceil(T_out / kPvocTile) tiles
  double rate;
  int32_t T, T_out;     // input rows; output rows written
  int32_t clip;         // the clip's place in the chunk (its flag is bad[clip])
  int32_t pad_;
};

// AFX_OK, or AFX_ERR_UNSUPPORTED with `why` set: n_fft even in [2, 4096], hop in [1, n_fft]
int pvoc_check(int n_fft, int hop, const char** why);
// rate finite and > 0
bool pvoc_rate_ok(double rate);
// T_out = ceil(T / rate) in float64 for T >= 1; false when T_out bins >= 2^31
bool pvoc_frames(int n_fft, int64_t T, double rate, int64_t* T_out);
// L_out = rint(length / rate), halves to even; false beyond 2^31
bool stretch_length(int64_t length, double rate, int64_t* n_out);
// what cut_stft_chunk is handed as a clip's length: rows in + rows out (afx_pvoc_batch); with the hops of the samples in
// and out as well (afx_time_stretch_batch)
inline int64_t pvoc_weight(int64_t T, int64_t T_out) { return T + T_out; }
inline int64_t stretch_weight(const afx_stft_opts& o, int64_t length, int64_t T, int64_t T_out, int64_t n_out) {
  return T + T_out + (length + o.hop - 1) / o.hop + (n_out + o.hop - 1) / o.hop;
}
void pvoc_cost(int n_fft, int mem_kind, int out_mem_kind, StftCost& cost);
void stretch_cost(const afx_stft_opts& o, int sample_fmt, int mem_kind, int out_mem_kind, StftCost& cost);

// angle (float64) and |c| (float32) of every input element, once; bad[clip] = 1 for a clip with a NaN / inf bin
hipError_t launch_pvoc_prep(hipStream_t s, int bins, const float2* spec, const PvocClip* clips, int n, int64_t n_rows,
                            double* ang, float* mag, uint32_t* bad);
// the sum of a tile's increments per bin, in increasing t from 0.0
hipError_t launch_pvoc_tiles(hipStream_t s, int n_fft, int hop, const PvocClip* clips, int n, int64_t n_tiles, const double* ang,
                             double* sums);
// sums[tile] becomes the accumulator at the tile's first step: acc_0 = angle(D[:, 0]), then tile after tile, reduced to
// [-pi, pi] after every tile
hipError_t launch_pvoc_carry(hipStream_t s, int bins, const PvocClip* clips, int n, const double* ang, double* sums);
// out[:, t] = mag (cos, sin)(acc_t), acc_t = the tile's accumulator + the increments before t in the tile; zeros for a
// clip whose flag is set
hipError_t launch_pvoc_apply(hipStream_t s, int n_fft, int hop, const PvocClip* clips, int n, int64_t n_tiles, const double* ang,
                             const float* mag, const double* carry, const uint32_t* bad, float2* out);

}  // namespace afx
