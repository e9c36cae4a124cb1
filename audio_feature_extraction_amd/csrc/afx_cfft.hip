// Batched complex DFT of arbitrary length in float64 for gfx950, by Bluestein's algorithm over a power of two, and the
// reduction of a pair's two magnitude spectra to the spectral term of the PESQ-like score (layout and the plan:
// afx_cfft.h; definitions: include/afx.h).  No atomics; every sum is taken in an order that depends on the pair alone.
#include <hip/hip_runtime.h>

#include <cmath>

#include "afx.h"
#include "afx_cfft.h"

namespace afx {

typedef double2 cf_c;

__device__ __forceinline__ cf_c cf_mul(cf_c a, cf_c b) { return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
// a conj(b)
__device__ __forceinline__ cf_c cf_mulc(cf_c a, cf_c b) { return make_double2(a.x * b.x + a.y * b.y, a.y * b.x - a.x * b.y); }
// exp(i pi t)
__device__ __forceinline__ cf_c cf_cispi(double t) {
  double s, c;
  sincospi(t, &s, &c);
  return make_double2(c, s);
}
// the chirp w_k = exp(-i pi k^2 / n), the phase reduced in integers: k < 2^22, so k^2 fits 64 bits with room
__device__ __forceinline__ cf_c cf_chirp(int64_t k, int64_t n) {
  const uint64_t r = ((uint64_t)k * (uint64_t)k) % (uint64_t)(2 * n);
  return cf_cispi(-(double)r / (double)n);
}
// point j of the filter: conj(w_j) at j and at M - j for j < n, zero between (M >= 2 n - 1: the two ranges do not meet)
__device__ __forceinline__ cf_c cf_filter(int64_t j, int64_t n, int64_t M) {
  const int64_t k = j < n ? j : M - j;
  if (k >= n) return make_double2(0.0, 0.0);
  const cf_c w = cf_chirp(k, n);
  return make_double2(w.x, -w.y);
}

template <int FMT>
__device__ __forceinline__ float cf_sample(const void* __restrict__ p, int64_t j) {
  if constexpr (FMT == AFX_FMT_S16) return (float)((const int16_t*)p)[j] * 0x1p-15f;
  else return ((const float*)p)[j];
}
// point j of a job's input: (r_j + i d_j) w_j for j < n, zero behind.  flags: kCfBad for a NaN / inf sample, kCfDiffers
// for a pair whose two sides differ here
template <int FMT>
__device__ __forceinline__ cf_c cf_signal(const CfJob& jb, const void* __restrict__ ref, const void* __restrict__ deg, int64_t j,
                                          int& flags) {
  if (j >= jb.n) return make_double2(0.0, 0.0);
  const float x = cf_sample<FMT>(ref, jb.r_off + j), y = jb.d_off >= 0 ? cf_sample<FMT>(deg, jb.d_off + j) : 0.f;
  if (!(isfinite(x) && isfinite(y))) flags |= kCfBad;
  if (jb.d_off >= 0 && x != y) flags |= kCfDiffers;
  return cf_mul(make_double2((double)x, (double)y), cf_chirp(j, jb.n));
}

// Transforms of length 2^logL along the high index of a tile x[(pos << logC) | c], nb butterflies per stage in all (half
// the tile's points): forwards by decimation in frequency, natural order in, bit-reversed out.  With logC = 0 and a tile
// longer than 2^logL the tile is a run of rows, each transformed.  tw: exp(-2 pi i j / 4096).  Barriers in front and behind.
__device__ __forceinline__ void cf_dif(cf_c* x, int nb, int logL, int logC, const cf_c* __restrict__ tw) {
  __syncthreads();
  for (int h = logL - 1; h >= 0; --h) {
    for (int t = threadIdx.x; t < nb; t += kCfLanes) {
      const int c = t & ((1 << logC) - 1), u = t >> logC, j = u & ((1 << h) - 1), g = u >> h;
      const int i0 = ((((g << (h + 1)) | j)) << logC) | c, i1 = i0 + (1 << (h + logC));
      const cf_c a = x[i0], b = x[i1], w = tw[j << (kCfTileLog - 1 - h)];
      x[i0] = make_double2(a.x + b.x, a.y + b.y);
      x[i1] = cf_mul(make_double2(a.x - b.x, a.y - b.y), w);
    }
    __syncthreads();
  }
}
// ... and backwards by decimation in time, bit-reversed in, natural out, not scaled: cf_dit(cf_dif(x)) = 2^logL x
__device__ __forceinline__ void cf_dit(cf_c* x, int nb, int logL, int logC, const cf_c* __restrict__ tw) {
  __syncthreads();
  for (int h = 0; h < logL; ++h) {
    for (int t = threadIdx.x; t < nb; t += kCfLanes) {
      const int c = t & ((1 << logC) - 1), u = t >> logC, j = u & ((1 << h) - 1), g = u >> h;
      const int i0 = ((((g << (h + 1)) | j)) << logC) | c, i1 = i0 + (1 << (h + logC));
      const cf_c a = x[i0], b = cf_mulc(x[i1], tw[j << (kCfTileLog - 1 - h)]);
      x[i0] = make_double2(a.x + b.x, a.y + b.y);
      x[i1] = make_double2(a.x - b.x, a.y - b.y);
    }
    __syncthreads();
  }
}

// a job's two flag words: one plain store per lane that saw the condition (all store the same value)
__device__ __forceinline__ void cf_raise(int32_t* __restrict__ flags, int job, int seen) {
  if (seen & kCfBad) flags[2 * job] = 1;
  if (seen & kCfDiffers) flags[2 * job + 1] = 1;
}

// the job whose range of workgroups holds b: the last one with blk_base <= b
__device__ __forceinline__ int cf_find(const CfJob* __restrict__ jobs, int n, int64_t b) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (jobs[mid].blk_base <= b) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// ---- M <= 4096: the whole chain in one workgroup ----
template <int FMT, bool FILTER>
__global__ void __launch_bounds__(kCfLanes) k_cfft_small(const void* __restrict__ ref, const void* __restrict__ deg,
                                                         const CfJob* __restrict__ jobs, const cf_c* __restrict__ tw,
                                                         const cf_c* __restrict__ filt_in, cf_c* __restrict__ out,
                                                         int32_t* __restrict__ flags) {
  __shared__ cf_c x[kCfTile];
  const CfJob jb = jobs[blockIdx.x];
  const int tid = threadIdx.x, M = 1 << jb.logM;
  int seen = 0;
  for (int i = tid; i < M; i += kCfLanes) x[i] = FILTER ? cf_filter(i, jb.n, M) : cf_signal<FMT>(jb, ref, deg, i, seen);
  cf_dif(x, M >> 1, jb.logM, 0, tw);
  if constexpr (FILTER) {
    for (int i = tid; i < M; i += kCfLanes) out[jb.work_off + i] = x[i];
  } else {
    cf_raise(flags, blockIdx.x, seen);
    for (int i = tid; i < M; i += kCfLanes) x[i] = cf_mul(x[i], filt_in[jb.filt_off + i]);
    cf_dit(x, M >> 1, jb.logM, 0, tw);
    const double scale = 1.0 / (double)M;
    for (int i = tid; i < jb.n; i += kCfLanes) {
      const cf_c v = cf_mul(x[i], cf_chirp(i, jb.n));
      out[jb.work_off + i] = make_double2(v.x * scale, v.y * scale);
    }
  }
}

// ---- M > 4096: the four-step form.  Workgroup b of a pass works on tile b - blk_base of its job. ----
// columns forwards: points (n1, c0 + c), n1 < M1, c < C = 4096 / M1
template <int FMT, bool FILTER>
__global__ void __launch_bounds__(kCfLanes) k_cfft_cols_fwd(const void* __restrict__ ref, const void* __restrict__ deg,
                                                            const CfJob* __restrict__ jobs, int n_jobs, int job0,
                                                            const cf_c* __restrict__ tw, cf_c* __restrict__ out,
                                                            int32_t* __restrict__ flags) {
  __shared__ cf_c x[kCfTile];
  const int q = cf_find(jobs, n_jobs, blockIdx.x);
  const CfJob jb = jobs[q];
  const int tid = threadIdx.x, logM2 = jb.logM - jb.logM1, logC = kCfTileLog - jb.logM1;
  const int64_t M = (int64_t)1 << jb.logM, c0 = ((int64_t)blockIdx.x - jb.blk_base) << logC;
  int seen = 0;
  for (int i = tid; i < kCfTile; i += kCfLanes) {
    const int64_t e = ((int64_t)(i >> logC) << logM2) + c0 + (i & ((1 << logC) - 1));
    x[i] = FILTER ? cf_filter(e, jb.n, M) : cf_signal<FMT>(jb, ref, deg, e, seen);
  }
  cf_dif(x, kCfTile / 2, jb.logM1, logC, tw);
  if constexpr (!FILTER) cf_raise(flags, job0 + q, seen);
  for (int i = tid; i < kCfTile; i += kCfLanes) {
    const int64_t e = ((int64_t)(i >> logC) << logM2) + c0 + (i & ((1 << logC) - 1));
    out[jb.work_off + e] = x[i];
  }
}

// rows: 4096 adjacent points = 4096 / M2 rows.  Row p1 holds k1 = the bit reversal of p1 (cf_dif's output order).
template <bool FILTER>
__global__ void __launch_bounds__(kCfLanes) k_cfft_rows(const CfJob* __restrict__ jobs, int n_jobs, const cf_c* __restrict__ tw,
                                                        const cf_c* __restrict__ filt_in, cf_c* __restrict__ data) {
  __shared__ cf_c x[kCfTile];
  constexpr int K = kCfTile / kCfLanes;
  const CfJob jb = jobs[cf_find(jobs, n_jobs, blockIdx.x)];
  const int tid = threadIdx.x, logM2 = jb.logM - jb.logM1;
  const int64_t e0 = ((int64_t)blockIdx.x - jb.blk_base) << kCfTileLog;
  const double inv = 2.0 / (double)((int64_t)1 << jb.logM);
  cf_c t[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int i = tid + kCfLanes * k;
    const int64_t e = e0 + i;
    const uint32_t p1 = (uint32_t)(e >> logM2), n2 = (uint32_t)(e & (((int64_t)1 << logM2) - 1));
    const uint32_t k1 = __brev(p1) >> (32 - jb.logM1);
    t[k] = cf_cispi(-(double)((uint64_t)n2 * k1) * inv);             // n2 k1 < M: the fraction is exact
    x[i] = cf_mul(data[jb.work_off + e], t[k]);
  }
  cf_dif(x, kCfTile / 2, logM2, 0, tw);
  if constexpr (FILTER) {
#pragma unroll
    for (int k = 0; k < K; ++k) data[jb.work_off + e0 + tid + kCfLanes * k] = x[tid + kCfLanes * k];
  } else {
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int i = tid + kCfLanes * k;
      x[i] = cf_mul(x[i], filt_in[jb.filt_off + e0 + i]);
    }
    cf_dit(x, kCfTile / 2, logM2, 0, tw);
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int i = tid + kCfLanes * k;
      data[jb.work_off + e0 + i] = cf_mulc(x[i], t[k]);
    }
  }
}

// columns backwards; the N points of the DFT are kept
__global__ void __launch_bounds__(kCfLanes) k_cfft_cols_inv(const CfJob* __restrict__ jobs, int n_jobs, const cf_c* __restrict__ tw,
                                                            cf_c* __restrict__ work) {
  __shared__ cf_c x[kCfTile];
  const CfJob jb = jobs[cf_find(jobs, n_jobs, blockIdx.x)];
  const int tid = threadIdx.x, logM2 = jb.logM - jb.logM1, logC = kCfTileLog - jb.logM1;
  const int64_t c0 = ((int64_t)blockIdx.x - jb.blk_base) << logC;
  for (int i = tid; i < kCfTile; i += kCfLanes) {
    const int64_t e = ((int64_t)(i >> logC) << logM2) + c0 + (i & ((1 << logC) - 1));
    x[i] = work[jb.work_off + e];
  }
  cf_dit(x, kCfTile / 2, jb.logM1, logC, tw);
  const double scale = 1.0 / (double)((int64_t)1 << jb.logM);
  for (int i = tid; i < kCfTile; i += kCfLanes) {
    const int64_t e = ((int64_t)(i >> logC) << logM2) + c0 + (i & ((1 << logC) - 1));
    if (e < jb.n) {
      const cf_c v = cf_mul(x[i], cf_chirp(e, jb.n));
      work[jb.work_off + e] = make_double2(v.x * scale, v.y * scale);
    }
  }
}

// ---- the record of a pair: one workgroup.  Z = DFT(r + i d): R_k = (Z_k + conj Z_{N-k}) / 2, D_k = (Z_k - conj Z_{N-k}) / 2i.
// Lane l of the 1024 adds the bins l, l + 1024, ... in that order; the lanes of a wave are joined by a butterfly, the
// sixteen waves in wave order.  A pair whose sides are equal sample for sample has D = R by definition, not to rounding: its distance is
// exactly 0, as the reference's is.
__global__ void __launch_bounds__(kCfTailLanes) k_specdist_tail(const CfJob* __restrict__ jobs, const cf_c* __restrict__ work,
                                                                const int32_t* __restrict__ flags, double* __restrict__ rec) {
  constexpr int W = kCfTailLanes / 64;
  __shared__ double red[W * 3];
  const int tid = threadIdx.x, c = blockIdx.x;
  const int64_t n = jobs[c].n;
  const cf_c* Z = work + jobs[c].work_off;
  const bool differs = flags[2 * c + 1] != 0;
  double a[3] = {0.0, 0.0, 0.0};
  for (int64_t k = tid; k < n; k += kCfTailLanes) {
    const cf_c p = Z[k], m = Z[k == 0 ? 0 : n - k];
    const double rr = 0.5 * (p.x + m.x), ri = 0.5 * (p.y - m.y), dr = 0.5 * (p.y + m.y), di = 0.5 * (m.x - p.x);
    const double R2 = rr * rr + ri * ri, D2 = differs ? dr * dr + di * di : R2, R = sqrt(R2), D = sqrt(D2);
    a[0] += fabs(R - D) / (R + 1e-10);
    a[1] += R2;
    a[2] += D2;
  }
#pragma unroll
  for (int q = 0; q < 3; ++q) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) a[q] += __shfl_xor(a[q], m, 64);
    if ((tid & 63) == 0) red[W * q + (tid >> 6)] = a[q];
  }
  __syncthreads();
  if (tid == 0) {
    double* out = rec + (size_t)c * AFX_SPECDIST_N;
    const bool isbad = flags[2 * c] != 0;
    const double nan = __builtin_nan("");
    out[0] = isbad ? nan : (double)n;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      double v = red[W * q];
#pragma unroll
      for (int w = 1; w < W; ++w) v += red[W * q + w];
      out[1 + q] = isbad ? nan : v;
    }
  }
}

hipError_t launch_cfft_filters(hipStream_t s, const CfJob* jobs, int n_small, int n_large, int large_blocks,
                               const double* tw, double* filt) {
  const cf_c* t = (const cf_c*)tw;
  cf_c* f = (cf_c*)filt;
  if (n_small > 0) {
    hipLaunchKernelGGL((k_cfft_small<AFX_FMT_F32, true>), dim3(n_small), dim3(kCfLanes), 0, s, nullptr, nullptr, jobs, t, nullptr, f, nullptr);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  if (n_large > 0 && large_blocks > 0) {
    const CfJob* lj = jobs + n_small;
    hipLaunchKernelGGL((k_cfft_cols_fwd<AFX_FMT_F32, true>), dim3(large_blocks), dim3(kCfLanes), 0, s, nullptr, nullptr, lj, n_large, n_small, t, f, nullptr);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_cfft_rows<true>, dim3(large_blocks), dim3(kCfLanes), 0, s, lj, n_large, t, nullptr, f);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t launch_cfft(hipStream_t s, const void* ref, const void* deg, int sample_fmt, const CfJob* jobs, int n_small,
                       int n_large, int large_blocks, const double* tw, const double* filt, double* work, int32_t* flags) {
  const cf_c* t = (const cf_c*)tw;
  const cf_c* f = (const cf_c*)filt;
  cf_c* w = (cf_c*)work;
  hipError_t e;
  if (n_small > 0) {
    if (sample_fmt == AFX_FMT_S16)
      hipLaunchKernelGGL((k_cfft_small<AFX_FMT_S16, false>), dim3(n_small), dim3(kCfLanes), 0, s, ref, deg, jobs, t, f, w, flags);
    else
      hipLaunchKernelGGL((k_cfft_small<AFX_FMT_F32, false>), dim3(n_small), dim3(kCfLanes), 0, s, ref, deg, jobs, t, f, w, flags);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  if (n_large > 0 && large_blocks > 0) {
    const CfJob* lj = jobs + n_small;
    if (sample_fmt == AFX_FMT_S16)
      hipLaunchKernelGGL((k_cfft_cols_fwd<AFX_FMT_S16, false>), dim3(large_blocks), dim3(kCfLanes), 0, s, ref, deg, lj, n_large, n_small, t, w, flags);
    else
      hipLaunchKernelGGL((k_cfft_cols_fwd<AFX_FMT_F32, false>), dim3(large_blocks), dim3(kCfLanes), 0, s, ref, deg, lj, n_large, n_small, t, w, flags);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_cfft_rows<false>, dim3(large_blocks), dim3(kCfLanes), 0, s, lj, n_large, t, f, w);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_cfft_cols_inv, dim3(large_blocks), dim3(kCfLanes), 0, s, lj, n_large, t, w);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t launch_specdist_tail(hipStream_t s, const CfJob* jobs, int n_jobs, const double* work, const int32_t* flags,
                                double* rec) {
  if (n_jobs <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_specdist_tail, dim3(n_jobs), dim3(kCfTailLanes), 0, s, jobs, (const cf_c*)work, flags, rec);
  return hipGetLastError();
}

}  // namespace afx
