// Zero-phase IIR filtering for gfx950 (decomposition, tables and the shared arithmetic: afx_filt.h; the same chain on the
// CPU: afx_filt_host.cpp).  No atomics: every value is written once, by one lane, from one fixed order of float64 fused
// multiply-adds, and the peaks are maxima.  A tile belongs to one clip, and every index into the caller's samples is
// checked against that clip's length: a neighbour in the packed buffer is never read.
//
// The block walks are dependent float64 chains (5 S fused operations per sample, S sections): one lane walks one block of
// kFiltL samples, a wave a tile of kFiltB blocks held in LDS as float64 rows of kFiltStride -- 33 KiB, four workgroups of one
// wave per CU.  The tile moves between memory and LDS with the lanes on adjacent samples (coalesced); the walk reads a
// column, lane i on row i, which the odd row stride keeps off shared banks.
#include <cfloat>

#include <hip/hip_runtime.h>

#include "afx.h"
#include "afx_filt.h"

namespace afx {

// Tables and records every lane reads at one address go through the constant address space: scalar loads, and the
// coefficients reach v_fma_f64 as scalar operands.  (Loads only.)
template <typename T> using ft_const = const __attribute__((address_space(4))) T*;
template <typename T> __device__ __forceinline__ ft_const<T> ft_as_const(const T* p) { return (ft_const<T>)(uintptr_t)p; }

struct FtClip { int64_t in_off, out_off, n; int first_tile, n_tiles, c; };

// the record whose tile range holds tile g (every record has at least one tile)
__device__ __forceinline__ FtClip ft_find(const FiltClip* clips, int n, int g) {
  const ft_const<FiltClip> cc = ft_as_const(clips);
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (cc[mid].first_tile <= g) lo = mid; else hi = mid - 1;
  }
  FtClip r;
  r.in_off = cc[lo].in_off; r.out_off = cc[lo].out_off; r.n = cc[lo].n; r.first_tile = cc[lo].first_tile;
  r.n_tiles = cc[lo].n_tiles; r.c = lo;
  return r;
}

template <int S>
__device__ __forceinline__ void ft_sections(const FiltTab* tab, FiltSec* sec) {
  const ft_const<FiltTab> t = ft_as_const(tab);
#pragma unroll
  for (int s = 0; s < S; ++s) { sec[s].b0 = t->sec[s].b0; sec[s].b1 = t->sec[s].b1; sec[s].b2 = t->sec[s].b2; sec[s].a1 = t->sec[s].a1; sec[s].a2 = t->sec[s].a2; }
}

__global__ void __launch_bounds__(256) k_filt_peak(const void* __restrict__ in, int fmt, const FiltClip* __restrict__ clips,
                                                   FiltState* __restrict__ st) {
  __shared__ float s_max[256];
  __shared__ unsigned s_bad[256];
  const FiltClip cl = clips[blockIdx.x];
  FiltIn f{};
  f.in = in; f.off = cl.in_off; f.n = cl.n; f.fmt = fmt;
  float mx = 0.0f;
  unsigned bad = 0;
  for (int64_t i = threadIdx.x; i < cl.n; i += 256) {
    const float a = fabsf(filt_raw(f, i));
    if (!(a <= FLT_MAX)) bad = 1;
    mx = fmaxf(mx, a);
  }
  s_max[threadIdx.x] = mx; s_bad[threadIdx.x] = bad;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (threadIdx.x < w) {
      s_max[threadIdx.x] = fmaxf(s_max[threadIdx.x], s_max[threadIdx.x + w]);
      s_bad[threadIdx.x] |= s_bad[threadIdx.x + w];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) { st[blockIdx.x].peak_in = s_max[0]; st[blockIdx.x].bad = s_bad[0]; st[blockIdx.x].peak_out = 0.0; }
}

// Samples past the clip's extended length are zeros and blocks past its last one are walked like any other: their outputs
// and end states land in the tile-granular workspace and are never read.
template <int S>
__global__ void __launch_bounds__(64) k_filt_forward(const void* __restrict__ in, int fmt, int mode, float coef, int padlen,
                                                     const FiltTab* __restrict__ tab, const FiltClip* __restrict__ clips, int n,
                                                     const FiltState* __restrict__ st, double* __restrict__ W,
                                                     double* __restrict__ carry) {
  __shared__ double tile[kFiltB * kFiltStride];
  const FtClip cl = ft_find(clips, n, blockIdx.x);
  if (st[cl.c].bad) return;
  FiltIn f{};
  f.in = in; f.off = cl.in_off; f.n = cl.n; f.fmt = fmt; f.mode = mode; f.coef = coef; f.padlen = padlen;
  f.peak = st[cl.c].peak_in;
  f.norm = mode == kFiltModeExperiment && f.peak >= FLT_MIN;
  const int64_t N = cl.n + 2 * (int64_t)padlen;
  const int lane = threadIdx.x;
  const int64_t j0 = (int64_t)(blockIdx.x - cl.first_tile) * kFiltTile;
  for (int q = 0; q < kFiltB; ++q) {
    const int64_t j = j0 + q * kFiltL + lane;
    tile[q * kFiltStride + lane] = j < N ? filt_e(f, j) : 0.0;
  }
  __syncthreads();
  FiltSec sec[S];
  ft_sections<S>(tab, sec);
  double z[2 * S];
#pragma unroll
  for (int j = 0; j < 2 * S; ++j) z[j] = 0.0;
  if (j0 == 0 && lane == 0) {                  // the clip's first block: the steady state under e[0]
    const double e0 = tile[0];
#pragma unroll
    for (int j = 0; j < 2 * S; ++j) z[j] = ft_as_const(tab)->zi[j] * e0;
  }
  double* row = tile + lane * kFiltStride;
  for (int m = 0; m < kFiltL; ++m) row[m] = filt_cascade<S>(sec, row[m], z);
  double* c = carry + ((int64_t)blockIdx.x * kFiltB + lane) * kFiltZ;
#pragma unroll
  for (int j = 0; j < 2 * S; ++j) c[j] = z[j];
  __syncthreads();
  double* w = W + (int64_t)blockIdx.x * kFiltTile;
  for (int q = 0; q < kFiltB; ++q) w[q * kFiltL + lane] = tile[q * kFiltStride + lane];
}

// One lane per clip, its blocks in pass order: the end state in carry[block] is replaced by the correction entering the
// block.  The loads of kScanAhead blocks are issued together, ahead of the dependent updates.
constexpr int kScanAhead = 8;
template <int S>
__global__ void __launch_bounds__(64) k_filt_scan(int padlen, const FiltTab* __restrict__ tab, const FiltClip* __restrict__ clips,
                                                  int n, const FiltState* __restrict__ st, double* __restrict__ carry,
                                                  int backward) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  if (c >= n || st[c].bad) return;
  const int64_t nb = (clips[c].n + 2 * (int64_t)padlen + kFiltL - 1) / kFiltL;
  double* base = carry + (int64_t)clips[c].first_tile * kFiltB * kFiltZ;
  const ft_const<FiltTab> t = ft_as_const(tab);
  double z[2 * S];
#pragma unroll
  for (int j = 0; j < 2 * S; ++j) z[j] = 0.0;
  for (int64_t q0 = 0; q0 < nb; q0 += kScanAhead) {
    double fin[kScanAhead][2 * S];
#pragma unroll
    for (int u = 0; u < kScanAhead; ++u) {
      const int64_t q = q0 + u < nb ? q0 + u : nb - 1;
      const double* p = base + (backward ? nb - 1 - q : q) * kFiltZ;
#pragma unroll
      for (int j = 0; j < 2 * S; ++j) fin[u][j] = p[j];
    }
#pragma unroll
    for (int u = 0; u < kScanAhead; ++u) {
      if (q0 + u < nb) {
        double* p = base + (backward ? nb - 1 - (q0 + u) : q0 + u) * kFiltZ;
#pragma unroll
        for (int j = 0; j < 2 * S; ++j) p[j] = z[j];
        filt_carry<S>(t->T, z, fin[u]);
      }
    }
  }
}

template <int S>
__global__ void __launch_bounds__(64) k_filt_backward(int padlen, const FiltTab* __restrict__ tab, const FiltClip* __restrict__ clips,
                                                      int n, const FiltState* __restrict__ st, double* __restrict__ W,
                                                      double* __restrict__ carry) {
  __shared__ double tile[kFiltB * kFiltStride];
  const FtClip cl = ft_find(clips, n, blockIdx.x);
  if (st[cl.c].bad) return;
  const int64_t N = cl.n + 2 * (int64_t)padlen;
  const int lane = threadIdx.x;
  const int64_t j0 = (int64_t)(blockIdx.x - cl.first_tile) * kFiltTile;
  double* w = W + (int64_t)blockIdx.x * kFiltTile;
  for (int q = 0; q < kFiltB; ++q) tile[q * kFiltStride + lane] = w[q * kFiltL + lane];
  __syncthreads();
  FiltSec sec[S];
  ft_sections<S>(tab, sec);
  const ft_const<FiltTab> t = ft_as_const(tab);
  double* c = carry + ((int64_t)blockIdx.x * kFiltB + lane) * kFiltZ;
  const int64_t start = j0 + (int64_t)lane * kFiltL;
  const int len = (int)(N - start < kFiltL ? (N - start < 0 ? 0 : N - start) : kFiltL);
  const bool last = start < N && start + kFiltL >= N;      // the clip's last block: the backward pass begins here
  double zin[2 * S], z[2 * S];
#pragma unroll
  for (int j = 0; j < 2 * S; ++j) { zin[j] = c[j]; z[j] = 0.0; }
  double* row = tile + lane * kFiltStride;
  for (int m = kFiltL - 1; m >= 0; --m) {
    if (m < len) {
      const double v = filt_correct<S>(row[m], t->R[m], zin);
      if (last && m == len - 1) {
#pragma unroll
        for (int j = 0; j < 2 * S; ++j) z[j] = t->zi[j] * v;
      }
      row[m] = filt_cascade<S>(sec, v, z);
    }
  }
#pragma unroll
  for (int j = 0; j < 2 * S; ++j) c[j] = z[j];
  __syncthreads();
  for (int q = 0; q < kFiltB; ++q) w[q * kFiltL + lane] = tile[q * kFiltStride + lane];
}

// thread t of 256 takes the tile's samples t, t + 256, ..: always step t & 63 of a block, so its row of R is read once
template <int S>
__global__ void __launch_bounds__(256) k_filt_final(int padlen, const FiltTab* __restrict__ tab, const FiltClip* __restrict__ clips,
                                                    int n, const FiltState* __restrict__ st, double* __restrict__ W,
                                                    const double* __restrict__ carry, double* __restrict__ tile_max,
                                                    float* __restrict__ out) {
  __shared__ double s_max[256];
  const FtClip cl = ft_find(clips, n, blockIdx.x);
  if (st[cl.c].bad) return;
  const int64_t j0 = (int64_t)(blockIdx.x - cl.first_tile) * kFiltTile;
  const int m = threadIdx.x & (kFiltL - 1);
  double Rm[2 * S];
#pragma unroll
  for (int j = 0; j < 2 * S; ++j) Rm[j] = tab->R[kFiltL - 1 - m][j];
  double* w = W + (int64_t)blockIdx.x * kFiltTile;
  const double* cb = carry + (int64_t)blockIdx.x * kFiltB * kFiltZ;
  double mx = 0.0;
  for (int e = threadIdx.x; e < kFiltTile; e += 256) {
    const int64_t i = j0 + e - padlen;         // the clip's own sample index
    if (i < 0 || i >= cl.n) continue;
    const double y = filt_correct<S>(w[e], Rm, cb + (e >> 6) * kFiltZ);
    mx = fmax(mx, fabs(y));
    if (out) out[cl.out_off + i] = (float)y;
    else w[e] = y;
  }
  s_max[threadIdx.x] = mx;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (threadIdx.x < h) s_max[threadIdx.x] = fmax(s_max[threadIdx.x], s_max[threadIdx.x + h]);
    __syncthreads();
  }
  if (threadIdx.x == 0) tile_max[blockIdx.x] = s_max[0];
}

__global__ void __launch_bounds__(64) k_filt_clipmax(const FiltClip* __restrict__ clips, const double* __restrict__ tile_max,
                                                     FiltState* __restrict__ st) {
  __shared__ double s_max[64];
  const FiltClip cl = clips[blockIdx.x];
  if (st[blockIdx.x].bad) return;
  double mx = 0.0;
  for (int q = threadIdx.x; q < cl.n_tiles; q += 64) mx = fmax(mx, tile_max[cl.first_tile + q]);
  s_max[threadIdx.x] = mx;
  __syncthreads();
  for (int h = 32; h > 0; h >>= 1) {
    if (threadIdx.x < h) s_max[threadIdx.x] = fmax(s_max[threadIdx.x], s_max[threadIdx.x + h]);
    __syncthreads();
  }
  if (threadIdx.x == 0) st[blockIdx.x].peak_out = s_max[0];
}

__global__ void __launch_bounds__(256) k_filt_scale(int padlen, const FiltClip* __restrict__ clips, int n,
                                                    const FiltState* __restrict__ st, const double* __restrict__ W,
                                                    float* __restrict__ out) {
  const FtClip cl = ft_find(clips, n, blockIdx.x);
  if (st[cl.c].bad) return;
  const double peak = st[cl.c].peak_out;
  const bool scale = peak >= DBL_MIN;
  const int64_t j0 = (int64_t)(blockIdx.x - cl.first_tile) * kFiltTile;
  const double* w = W + (int64_t)blockIdx.x * kFiltTile;
  for (int e = threadIdx.x; e < kFiltTile; e += 256) {
    const int64_t i = j0 + e - padlen;
    if (i < 0 || i >= cl.n) continue;
    out[cl.out_off + i] = (float)(scale ? w[e] / peak : w[e]);
  }
}

#define FILT_DISPATCH(S, CALL)                   \
  switch (S) {                                   \
    case 1: { constexpr int kS = 1; CALL; } break; \
    case 2: { constexpr int kS = 2; CALL; } break; \
    case 3: { constexpr int kS = 3; CALL; } break; \
    default: { constexpr int kS = 4; CALL; } break; \
  }

hipError_t launch_filt_peak(hipStream_t s, const void* in, int fmt, const FiltClip* clips, int n, FiltState* st) {
  hipLaunchKernelGGL(k_filt_peak, dim3(n), dim3(256), 0, s, in, fmt, clips, st);
  return hipGetLastError();
}

hipError_t launch_filt_forward(hipStream_t s, const void* in, int fmt, int mode, float coef, int padlen, int S,
                               const FiltTab* tab, const FiltClip* clips, int n, int n_tiles, const FiltState* st, double* W,
                               double* carry) {
  FILT_DISPATCH(S, hipLaunchKernelGGL(k_filt_forward<kS>, dim3(n_tiles), dim3(64), 0, s, in, fmt, mode, coef, padlen, tab, clips,
                                      n, st, W, carry));
  return hipGetLastError();
}

hipError_t launch_filt_scan(hipStream_t s, int padlen, int S, const FiltTab* tab, const FiltClip* clips, int n,
                            const FiltState* st, double* carry, bool backward) {
  FILT_DISPATCH(S, hipLaunchKernelGGL(k_filt_scan<kS>, dim3((n + 63) / 64), dim3(64), 0, s, padlen, tab, clips, n, st, carry,
                                      backward ? 1 : 0));
  return hipGetLastError();
}

hipError_t launch_filt_backward(hipStream_t s, int padlen, int S, const FiltTab* tab, const FiltClip* clips, int n, int n_tiles,
                                const FiltState* st, double* W, double* carry) {
  FILT_DISPATCH(S, hipLaunchKernelGGL(k_filt_backward<kS>, dim3(n_tiles), dim3(64), 0, s, padlen, tab, clips, n, st, W, carry));
  return hipGetLastError();
}

hipError_t launch_filt_final(hipStream_t s, int padlen, int S, const FiltTab* tab, const FiltClip* clips, int n, int n_tiles,
                             const FiltState* st, double* W, const double* carry, double* tile_max, float* out) {
  FILT_DISPATCH(S, hipLaunchKernelGGL(k_filt_final<kS>, dim3(n_tiles), dim3(256), 0, s, padlen, tab, clips, n, st, W, carry,
                                      tile_max, out));
  return hipGetLastError();
}

hipError_t launch_filt_clipmax(hipStream_t s, const FiltClip* clips, int n, const double* tile_max, FiltState* st) {
  hipLaunchKernelGGL(k_filt_clipmax, dim3(n), dim3(64), 0, s, clips, tile_max, st);
  return hipGetLastError();
}

hipError_t launch_filt_scale(hipStream_t s, int padlen, const FiltClip* clips, int n, int n_tiles, const FiltState* st,
                             const double* W, float* out) {
  hipLaunchKernelGGL(k_filt_scale, dim3(n_tiles), dim3(256), 0, s, padlen, clips, n, st, W, out);
  return hipGetLastError();
}

}  // namespace afx
