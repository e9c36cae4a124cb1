// What the two DTW kernel files share (k_dtw in afx_dtw.hip, k_dtw_steps in afx_dtw_steps.hip): the (dim, metric) ->
// instantiation dispatch, the DPP lane shifts of a double, the per-pair NaN / zero-norm test, the local cost of one cell
// and the back-track.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "afx.h"
#include "afx_dtw.h"

namespace afx {

// Host side: f(std::integral_constant<int, DIMP>) for the compiled width that serves `dim` (dtw_dimp is this list) ...
template <class F>
auto dtw_with_dimp(int dim, F&& f) {
  if (dim <= 8) return f(std::integral_constant<int, 8>{});
  if (dim <= 16) return f(std::integral_constant<int, 16>{});
  if (dim <= 24) return f(std::integral_constant<int, 24>{});
  if (dim <= 40) return f(std::integral_constant<int, 40>{});
  if (dim <= 64) return f(std::integral_constant<int, 64>{});
  return f(std::integral_constant<int, 128>{});
}
// ... and f(DIMP, METRIC), both as integral constants, for the kernels that are templates over the metric too
template <class F>
auto dtw_dispatch(int dim, int metric, F&& f) {
  return dtw_with_dimp(dim, [&](auto dimp) {
    if (metric == AFX_DTW_EUCLIDEAN) return f(dimp, std::integral_constant<int, AFX_DTW_EUCLIDEAN>{});
    if (metric == AFX_DTW_SQEUCLIDEAN) return f(dimp, std::integral_constant<int, AFX_DTW_SQEUCLIDEAN>{});
    return f(dimp, std::integral_constant<int, AFX_DTW_COSINE>{});
  });
}

constexpr double kDtwInf = __builtin_huge_val();
typedef float dtw_f2 __attribute__((ext_vector_type(2)));   // v_pk_add_f32 / v_pk_fma_f32 operands

__device__ __forceinline__ double dtw_shr1(double v, double lane0) {
  // lane l <- lane l-1 (wave_shr:1, DPP control 0x138); lane 0 keeps `lane0`
  const int lo = __builtin_amdgcn_update_dpp(__double2loint(lane0), __double2loint(v), 0x138, 0xf, 0xf, false);
  const int hi = __builtin_amdgcn_update_dpp(__double2hiint(lane0), __double2hiint(v), 0x138, 0xf, 0xf, false);
  return __hiloint2double(hi, lo);
}

__device__ __forceinline__ double dtw_shl1(double v) {
  // lane l <- lane l+1 (wave_shl:1, DPP control 0x130)
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), 0x130, 0xf, 0xf, false);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), 0x130, 0xf, 0xf, false);
  return __hiloint2double(hi, lo);
}

// NaN / inf anywhere in X or Y, or a zero-norm frame under cosine (librosa raises): true in every lane of the wave
template <int DIMP, int METRIC>
__device__ __forceinline__ bool dtw_pair_nonfinite(const float* __restrict__ feats, const float* __restrict__ norms,
                                                   const DtwPair& P, int l) {
  bool bad = false;
  const float* fx = feats + P.x_frame * DIMP;
  const float* fy = feats + P.y_frame * DIMP;
  const int64_t nx = (int64_t)P.n * DIMP, ny = (int64_t)P.m * DIMP;
  for (int64_t e = l; e < nx; e += 64) bad |= !isfinite(fx[e]);
  for (int64_t e = l; e < ny; e += 64) bad |= !isfinite(fy[e]);
  if (METRIC == AFX_DTW_COSINE) {
    for (int t = l; t < P.n; t += 64) bad |= !(norms[P.x_frame + t] > 0.f);
    for (int t = l; t < P.m; t += 64) bad |= !(norms[P.y_frame + t] > 0.f);
  }
  return __any(bad);
}

// the local cost of the lane's x row (xr, norm nx) against the y column in ring slot `slot` (stride S = DIMP + 4 floats,
// the column's norm in float DIMP): float32, direct differences, as scipy's cdist.
// XR: an array of DIMP / 2 register pairs, or anything indexed the same way that reads the row from LDS.  The LDS form
// runs in pieces of eight 16-byte units: the accumulator and an offset that is always zero pass through an empty asm
// between pieces, so a piece's reads cannot be issued before the piece before it is summed.  Left alone, the scheduler
// issues all 64 reads of a 128-wide cell before the first subtraction and needs 256 registers to land them.
template <int DIMP, int METRIC, class XR>
__device__ __forceinline__ float dtw_local_cost(const XR& xr, float nx, const float* ys, int slot) {
  constexpr int S = DIMP + 4;
  constexpr bool kLdsRow = !std::is_array<XR>::value;
  const float4* yp = reinterpret_cast<const float4*>(ys + slot * S);
  int off = 0;
  dtw_f2 acc = dtw_f2{0.f, 0.f};          // cosine: the dot product; otherwise the sum of squared differences
#pragma unroll
  for (int q = 0; q < DIMP / 4; ++q) {
    if constexpr (kLdsRow) {
      if (q > 0 && q % 8 == 0) asm volatile("" : "+v"(acc.x), "+v"(acc.y), "+v"(off));
    }
    const float4 y = yp[q + off];
    const dtw_f2 x0 = xr[2 * (q + off)], x1 = xr[2 * (q + off) + 1];
    if (METRIC == AFX_DTW_COSINE) {
      if constexpr (DIMP <= 64) {
        acc = __builtin_elementwise_fma(x0, dtw_f2{y.x, y.y}, acc);
        acc = __builtin_elementwise_fma(x1, dtw_f2{y.z, y.w}, acc);
      } else {
        acc.x = fmaf(x0.x, y.x, acc.x); acc.y = fmaf(x0.y, y.y, acc.y);
        acc.x = fmaf(x1.x, y.z, acc.x); acc.y = fmaf(x1.y, y.w, acc.y);
      }
    } else {
      if constexpr (DIMP <= 64) {
        const dtw_f2 d0 = x0 - dtw_f2{y.x, y.y}, d1 = x1 - dtw_f2{y.z, y.w};
        acc = __builtin_elementwise_fma(d0, d0, acc);
        acc = __builtin_elementwise_fma(d1, d1, acc);
      } else {     // scalar ops: the packed form's aligned register pairs push the 128-wide instance into spills
        const float d0 = x0.x - y.x, d1 = x0.y - y.y, d2 = x1.x - y.z, d3 = x1.y - y.w;
        acc.x = fmaf(d0, d0, acc.x); acc.y = fmaf(d1, d1, acc.y);
        acc.x = fmaf(d2, d2, acc.x); acc.y = fmaf(d3, d3, acc.y);
      }
    }
  }
  float c;
  if (METRIC == AFX_DTW_COSINE) {
    const float ny = ys[slot * S + DIMP];
    const float cs = fminf(1.f, fmaxf(-1.f, (acc.x + acc.y) / (nx * ny)));
    c = 1.f - cs;
  } else {
    c = acc.x + acc.y;
    if (METRIC == AFX_DTW_EUCLIDEAN) c = sqrtf(c);
  }
  return c;
}

// The back-track of both kernels, one lane per pair: from (N-1, end[p]), or (N-1, M-1) without `end`, along the recorded
// steps to (0, 0), or to the first cell of row 0 (row0_ends).  BITS: the width of a step code, 32 / BITS wavefront steps
// per word, layout [strip][word][lane].  back(code, i, j) takes one step back; false on a code that no step wrote.
// path[2k], path[2k+1] = i, j; len[p] = L (0 for a failed pair).
template <int BITS, class Back>
__device__ __forceinline__ void dtw_backtrack_walk(const DtwPair* __restrict__ pairs, int n_pairs,
                                                   const uint32_t* __restrict__ codes, const int32_t* __restrict__ status,
                                                   const int32_t* __restrict__ end, bool row0_ends,
                                                   int32_t* __restrict__ path, int32_t* __restrict__ len, Back back) {
  constexpr int PER = 32 / BITS;           // steps per word: 16 or 8
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_pairs) return;
  const DtwPair P = pairs[p];
  if (status[p] != AFX_DTW_OK) { len[p] = 0; return; }
  const uint32_t* cw = codes + P.codes;
  int2* out = reinterpret_cast<int2*>(path) + P.path;
  int i = P.n - 1, j = end ? end[p] : P.m - 1, k = 0;
  const int kmax = P.n + P.m - 1;
  while (k < kmax && j >= 0 && j < P.m) {
    out[k++] = make_int2(i, j);
    if (i == 0 && (row0_ends || j == 0)) break;
    const unsigned l = i & 63, s = j + l;
    const uint32_t w = cw[((int64_t)(i >> 6) * P.qn + s / PER) * 64 + l];
    // neither can happen on a finite D: an unwritten code would spin a corrupted walk, a step out of the matrix leave bounds
    if (!back((w >> (BITS * (s % PER))) & ((1u << BITS) - 1u), i, j) || i < 0 || j < 0) break;
  }
  len[p] = k;
}

}  // namespace afx
