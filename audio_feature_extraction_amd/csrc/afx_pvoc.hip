// librosa-style phase_vocoder (afx_pvoc.h).  Rows are frame after frame with the bins contiguous
// (section 26's layout); lanes run along the bins in every kernel, so every access is coalesced.  The recurrence along time
// is a prefix sum in a fixed order: within a tile of kPvocTile output steps in increasing t from 0.0, across the tiles of a
// clip one after another.
//   k_pvoc_prep    one workgroup per input row: angle = atan2(double im, double re) as float64 and |c| as float32, once per
//                  input element (a stretch by rate < 1 reads every column several times); bad[clip] = 1 for a NaN / inf bin
//   k_pvoc_tiles   one thread per (tile, bin): the sum of the tile's increments
//   k_pvoc_carry   one thread per (clip, bin): the serial carry over the clip's tile totals, in place, kept in [-pi, pi]
//   k_pvoc_apply   one thread per (tile, bin): walks the tile again and writes mag x (cos, sin)(carry + partial sum)
// No atomics, no barriers and no LDS: a lane past the last bin has nothing to wait for and leaves.  The summation order is a
// function of (bin, t) alone, and a clip reads nothing of another.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "afx.h"
#include "afx_pvoc.h"

namespace afx {

namespace {

// |c| as one fixed rounding sequence (hp_abs): two products, one sum, one square root
__device__ __forceinline__ float pv_abs(float2 x) {
#pragma clang fp contract(off)
  const float a = x.x * x.x;
  const float b = x.y * x.y;
  return sqrtf(a + b);
}

// the clip of a tile and the tile's steps [t0, t1)
__device__ __forceinline__ PvocClip pv_tile(const PvocClip* __restrict__ clips, int n, int64_t tile, int64_t* t0, int64_t* t1) {
  const int ci = hp_find(n, tile, [&](int i) { return clips[i].tile_base; });
  const PvocClip c = clips[ci];
  *t0 = (tile - c.tile_base) * kPvocTile;
  *t1 = *t0 + kPvocTile < c.T_out ? *t0 + kPvocTile : c.T_out;
  return c;
}

// angle of column j of the clip at bin b; columns T and beyond are +0 + 0i, whose angle is 0
__device__ __forceinline__ double pv_ang(const double* __restrict__ ang, const PvocClip& c, int bins, int b, int64_t j) {
  return j < c.T ? ang[(c.row_base + j) * bins + b] : 0.0;
}

}  // namespace

__global__ __launch_bounds__(256) void k_pvoc_prep(int bins, const float2* __restrict__ spec, const PvocClip* __restrict__ clips,
                                                   int n, double* __restrict__ ang, float* __restrict__ mag,
                                                   uint32_t* __restrict__ bad) {
  const int64_t row = blockIdx.x;
  const int ci = hp_find(n, row, [&](int i) { return clips[i].row_base; });
  const PvocClip c = clips[ci];
  const int64_t r = row - c.row_base;
  if (r >= c.T) return;                                          // (never: the rows of a chunk are exactly its clips')
  const float2* __restrict__ src = spec + c.spec_off + r * bins;
  bool flag = false;
  for (int b = threadIdx.x; b < bins; b += 256) {
    const float2 x = src[b];
    flag |= !(isfinite(x.x) && isfinite(x.y));
    ang[row * bins + b] = atan2((double)x.y, (double)x.x);
    mag[row * bins + b] = pv_abs(x);
  }
  if (flag) bad[c.clip] = 1u;                                    // every writer writes the same word
}

__global__ __launch_bounds__(256) void k_pvoc_tiles(int n_fft, int hop, const PvocClip* __restrict__ clips, int n,
                                                    const double* __restrict__ ang, double* __restrict__ sums) {
  const int bins = n_fft / 2 + 1;
  const int b = blockIdx.y * 256 + threadIdx.x;
  if (b >= bins) return;
  const int64_t tile = blockIdx.x;
  int64_t t0, t1;
  const PvocClip c = pv_tile(clips, n, tile, &t0, &t1);
  const double phi = pvoc_phi(hop, n_fft, b), phi_r = pvoc_wrap(phi);
  double sum = 0.0;
  for (int64_t t = t0; t < t1; ++t) {
    int64_t j;
    double a;
    pvoc_step(t, c.rate, &j, &a);
    sum += pvoc_inc(pv_ang(ang, c, bins, b, j), pv_ang(ang, c, bins, b, j + 1), phi, phi_r);
  }
  sums[tile * bins + b] = sum;
}

__global__ __launch_bounds__(256) void k_pvoc_carry(int bins, const PvocClip* __restrict__ clips, const double* __restrict__ ang,
                                                    double* __restrict__ sums) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= bins) return;
  const PvocClip c = clips[blockIdx.y];
  const int64_t nt = ((int64_t)c.T_out + kPvocTile - 1) / kPvocTile;
  double acc = ang[c.row_base * bins + b];                       // T >= 1 for every clip of a chunk
  for (int64_t k = 0; k < nt; ++k) {
    double* p = sums + (c.tile_base + k) * bins + b;
    const double s = *p;
    *p = acc;
    acc = pvoc_wrap(acc + s);
  }
}

__global__ __launch_bounds__(256) void k_pvoc_apply(int n_fft, int hop, const PvocClip* __restrict__ clips, int n,
                                                    const double* __restrict__ ang, const float* __restrict__ mag,
                                                    const double* __restrict__ carry, const uint32_t* __restrict__ bad,
                                                    float2* __restrict__ out) {
  const int bins = n_fft / 2 + 1;
  const int b = blockIdx.y * 256 + threadIdx.x;
  if (b >= bins) return;
  const int64_t tile = blockIdx.x;
  int64_t t0, t1;
  const PvocClip c = pv_tile(clips, n, tile, &t0, &t1);
  float2* __restrict__ dst = out + c.out_off + b;
  if (bad[c.clip]) {
    for (int64_t t = t0; t < t1; ++t) dst[t * bins] = float2{0.f, 0.f};
    return;
  }
  const double phi = pvoc_phi(hop, n_fft, b), phi_r = pvoc_wrap(phi);
  const double acc0 = carry[tile * bins + b];
  double sum = 0.0;
  for (int64_t t = t0; t < t1; ++t) {
    int64_t j;
    double a;
    pvoc_step(t, c.rate, &j, &a);
    const float m0 = j < c.T ? mag[(c.row_base + j) * bins + b] : 0.f;
    const float m1 = j + 1 < c.T ? mag[(c.row_base + j + 1) * bins + b] : 0.f;
    const float m = pvoc_mag(m0, m1, a);
    double sn, cs;
    sincos(acc0 + sum, &sn, &cs);
    dst[t * bins] = float2{(float)((double)m * cs), (float)((double)m * sn)};
    sum += pvoc_inc(pv_ang(ang, c, bins, b, j), pv_ang(ang, c, bins, b, j + 1), phi, phi_r);
  }
}

// ---------------------------------------------------------------------------------------------------------------------
hipError_t launch_pvoc_prep(hipStream_t s, int bins, const float2* spec, const PvocClip* clips, int n, int64_t n_rows,
                            double* ang, float* mag, uint32_t* bad) {
  if (n <= 0 || n_rows <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_pvoc_prep, dim3((unsigned)n_rows), dim3(256), 0, s, bins, spec, clips, n, ang, mag, bad);
  return hipGetLastError();
}

hipError_t launch_pvoc_tiles(hipStream_t s, int n_fft, int hop, const PvocClip* clips, int n, int64_t n_tiles, const double* ang,
                             double* sums) {
  if (n <= 0 || n_tiles <= 0) return hipSuccess;
  const dim3 grid((unsigned)n_tiles, (unsigned)((n_fft / 2 + 1 + 255) / 256));
  hipLaunchKernelGGL(k_pvoc_tiles, grid, dim3(256), 0, s, n_fft, hop, clips, n, ang, sums);
  return hipGetLastError();
}

hipError_t launch_pvoc_carry(hipStream_t s, int bins, const PvocClip* clips, int n, const double* ang, double* sums) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_pvoc_carry, dim3((unsigned)((bins + 255) / 256), (unsigned)n), dim3(256), 0, s, bins, clips, ang, sums);
  return hipGetLastError();
}

hipError_t launch_pvoc_apply(hipStream_t s, int n_fft, int hop, const PvocClip* clips, int n, int64_t n_tiles, const double* ang,
                             const float* mag, const double* carry, const uint32_t* bad, float2* out) {
  if (n <= 0 || n_tiles <= 0) return hipSuccess;
  const dim3 grid((unsigned)n_tiles, (unsigned)((n_fft / 2 + 1 + 255) / 256));
  hipLaunchKernelGGL(k_pvoc_apply, grid, dim3(256), 0, s, n_fft, hop, clips, n, ang, mag, carry, bad, out);
  return hipGetLastError();
}

}  // namespace afx
