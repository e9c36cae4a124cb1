// Batched polyphase resampler for gfx950 (layout and arithmetic: afx_resample.h).  No atomics: every output sample is
// written once, by one lane, from one fixed order of float64 fused multiply-adds.
#include <hip/hip_runtime.h>

#include "afx.h"
#include "afx_device.h"
#include "afx_resample.h"
#include "afx_wave.h"

namespace afx {

// Tables every lane of a wave reads at the same address (tap groups, clip records) are read through the constant address
// space: the compiler then issues scalar loads whatever it can prove about aliasing with the output stores, and the taps
// reach v_fma_f64 as scalar operands.  (Loads only: nothing is ever written through these pointers.)
template <typename T> using rs_const = const __attribute__((address_space(4))) T*;
template <typename T> __device__ __forceinline__ rs_const<T> rs_as_const(const T* p) { return (rs_const<T>)(uintptr_t)p; }

// the clip whose block range holds block b: the last clip with first_block <= b (clips without blocks share their
// successor's first_block and are never chosen)
__device__ __forceinline__ int rs_find_clip(rs_const<RsClip> clips, int n_clips, int b) {
  int lo = 0, hi = n_clips - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (clips[mid].first_block <= b) lo = mid; else hi = mid - 1;
  }
  return lo;
}

__device__ __forceinline__ RsClip rs_clip(rs_const<RsClip> clips, int c) {
  RsClip cl;
  cl.in_off = clips[c].in_off; cl.in_len = clips[c].in_len; cl.out_off = clips[c].out_off; cl.out_len = clips[c].out_len;
  cl.first_block = clips[c].first_block; cl.pad_ = 0;
  return cl;
}

template <int FMT>
__global__ void __launch_bounds__(1024) k_resample(const void* __restrict__ in, float* __restrict__ out,
                                                   const RsClip* __restrict__ clips, int n_clips,
                                                   const double* __restrict__ G, const int32_t* __restrict__ tstart,
                                                   const RsParams p) {
  extern __shared__ __align__(16) float xs[];          // [rows][stride]: row r holds x[(sp0 - r_back + r) * rw ..)
  const int b = blockIdx.x;
  const rs_const<RsClip> cclips = rs_as_const(clips);
  const RsClip cl = rs_clip(cclips, rs_find_clip(cclips, n_clips, b));
  const int64_t sp0 = (int64_t)(b - cl.first_block) * p.tile_sp;
  const int64_t x0 = (sp0 - p.r_back) * p.rw;          // clip-relative index of the tile's first sample (may be < 0)
  const unsigned total = (unsigned)p.rows * (unsigned)p.rw;
  for (unsigned e = threadIdx.x; e < total; e += blockDim.x) {
    const unsigned row = e / (unsigned)p.rw, col = e - row * (unsigned)p.rw;
    const int64_t i = x0 + e;
    // samples outside the clip are zero: a neighbour in the packed buffer is never read
    xs[row * p.stride + col] = (i >= 0 && i < cl.in_len) ? ld_raw<FMT>(in, cl.in_off + i) : 0.0f;
  }
  __syncthreads();

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int units = p.n_groups * p.tc;
  const int skip = p.stride - p.rw;                    // row padding stepped over when t crosses a row
  for (int u = wave; u < units; u += p.n_waves) {              // p.n_waves == blockDim.x / 64: u stays in a scalar register
    const int g = u % p.n_groups, pass = u / p.n_groups;
    const int t0 = rs_as_const(tstart)[g] + p.r_back * p.rw;        // >= 0
    const int row0 = t0 / p.rw;
    int col = t0 - row0 * p.rw;
    const int spl = pass * p.lanes + (lane < p.lanes ? lane : p.lanes - 1);
    const float* xp = xs + (spl + row0) * p.stride + col;
    rs_const<double> gp = rs_as_const(G) + (size_t)g * p.n_steps * kRsGroup;
    double acc[kRsGroup];
#pragma unroll
    for (int j = 0; j < kRsGroup; ++j) acc[j] = 0.0;
    int left = p.n_steps;
    while (left > 0) {
      const int seg = min(left, p.rw - col);
#pragma unroll 4
      for (int k = 0; k < seg; ++k) {
        const double xv = (double)xp[k];
#pragma unroll
        for (int j = 0; j < kRsGroup; ++j) acc[j] = fma(xv, gp[k * kRsGroup + j], acc[j]);
      }
      xp += seg + skip;
      gp += (size_t)seg * kRsGroup;
      left -= seg;
      col = 0;
    }
    if (lane < p.lanes) {
      const int64_t m0 = (sp0 + spl) * p.opp + (int64_t)g * kRsGroup;
      const int o_left = p.opp - g * kRsGroup;
#pragma unroll
      for (int j = 0; j < kRsGroup; ++j)
        if (j < o_left && m0 + j < cl.out_len) out[cl.out_off + m0 + j] = (float)acc[j];
    }
  }
}

template <int FMT>
__global__ void __launch_bounds__(256) k_resample_copy(const void* __restrict__ in, float* __restrict__ out,
                                                       const RsClip* __restrict__ clips, int n_clips) {
  const int b = blockIdx.x;
  const rs_const<RsClip> cclips = rs_as_const(clips);
  const RsClip cl = rs_clip(cclips, rs_find_clip(cclips, n_clips, b));
  const int64_t i0 = (int64_t)(b - cl.first_block) * kRsCopyChunk;
  for (int e = threadIdx.x; e < kRsCopyChunk; e += 256) {
    const int64_t i = i0 + e;
    if (i < cl.in_len) out[cl.out_off + i] = ld_raw<FMT>(in, cl.in_off + i);
  }
}

hipError_t launch_resample(hipStream_t s, const void* in, int fmt, float* out, const RsClip* clips, int n_clips,
                           int n_blocks, const double* G, const int32_t* tstart, const RsParams& p) {
  if (n_blocks <= 0) return hipSuccess;
  const size_t lds = (size_t)p.rows * p.stride * sizeof(float);
  auto kern = fmt == AFX_FMT_S16 ? k_resample<AFX_FMT_S16> : k_resample<AFX_FMT_F32>;
  hipError_t e = set_lds_limit(kern, lds);      // every launch: the bytes follow the resampling ratio
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kern, dim3(n_blocks), dim3(64 * p.n_waves), lds, s, in, out, clips, n_clips, G, tstart, p);
  return hipGetLastError();
}

hipError_t launch_resample_copy(hipStream_t s, const void* in, int fmt, float* out, const RsClip* clips, int n_clips,
                                int n_blocks) {
  if (n_blocks <= 0) return hipSuccess;
  if (fmt == AFX_FMT_S16) hipLaunchKernelGGL(k_resample_copy<AFX_FMT_S16>, dim3(n_blocks), dim3(256), 0, s, in, out, clips, n_clips);
  else hipLaunchKernelGGL(k_resample_copy<AFX_FMT_F32>, dim3(n_blocks), dim3(256), 0, s, in, out, clips, n_clips);
  return hipGetLastError();
}

}  // namespace afx
