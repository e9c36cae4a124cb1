// Median and Savitzky-Golay filtering of ragged batches and the experiment extractor's energy and ZCR groups for gfx950
// (geometry, tables and the shared arithmetic: afx_smooth.h; the same chains on the CPU: afx_smooth_host.cpp).
// Every output sample and every statistic is written once, by one lane, from one fixed order of operations; the only
// atomics are integer counts in LDS (the radix select of the energy percentile), whose totals do not depend on their
// order.  A tile belongs to one clip, and every index into a clip's samples is checked against that clip's length: a
// neighbour in the packed buffer is never read.
#include <cfloat>

#include <hip/hip_runtime.h>

#include "afx.h"
#include "afx_smooth.h"

namespace afx {

template <typename T> using sm_const = const __attribute__((address_space(4))) T*;
template <typename T> __device__ __forceinline__ sm_const<T> sm_as_const(const T* p) { return (sm_const<T>)(uintptr_t)p; }

struct SmTile { int64_t in_off, out_off, n, j0; int c; };

// the record whose tile range holds tile g (every record has at least one tile), and the tile's first sample
__device__ __forceinline__ SmTile sm_find(const SmClip* clips, int n, int g) {
  const sm_const<SmClip> cc = sm_as_const(clips);
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (cc[mid].first_tile <= g) lo = mid; else hi = mid - 1;
  }
  SmTile r;
  r.in_off = cc[lo].in_off; r.out_off = cc[lo].out_off; r.n = cc[lo].n; r.c = lo;
  r.j0 = (int64_t)(g - cc[lo].first_tile) * kSmTile;
  return r;
}

// tile[q] = sample j0 - h + q of the clip, 0 <= q < kSmTile + 2 h; zeros outside [0, n): the lanes on adjacent samples
__device__ __forceinline__ void sm_stage(float* tile, const SmSrc& src, const SmTile& t, int h) {
  for (int q = threadIdx.x; q < kSmTile + 2 * h; q += kSmThreads) {
    const int64_t j = t.j0 - h + q;
    tile[q] = j >= 0 && j < t.n ? sm_raw(src, j) : 0.0f;
  }
  __syncthreads();
}

__global__ void __launch_bounds__(kSmThreads) k_sm_check(const void* __restrict__ in, int fmt, const SmClip* __restrict__ clips,
                                                         uint32_t* __restrict__ bad) {
  __shared__ unsigned s_bad[kSmThreads];
  const SmClip cl = clips[blockIdx.x];
  const SmSrc src{in, cl.in_off, fmt};
  unsigned b = 0;
  for (int64_t i = threadIdx.x; i < cl.n; i += kSmThreads)
    if (!(fabsf(sm_raw(src, i)) <= FLT_MAX)) b = 1;
  s_bad[threadIdx.x] = b;
  __syncthreads();
  for (int w = kSmThreads / 2; w > 0; w >>= 1) {
    if (threadIdx.x < w) s_bad[threadIdx.x] |= s_bad[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) bad[blockIdx.x] = s_bad[0];
}

// KT: the kernel size compiled in (1, 3, 5), or 0 for the rank count over any odd K
template <int KT>
__global__ void __launch_bounds__(kSmThreads) k_medfilt(const void* __restrict__ in, int fmt, int K_, const SmClip* __restrict__ clips,
                                                        int n, const uint32_t* __restrict__ bad, int bad_stride,
                                                        float* __restrict__ out) {
  __shared__ float tile[kSmTile + 2 * kSmMaxHalo];
  const SmTile t = sm_find(clips, n, blockIdx.x);
  if (bad[(int64_t)t.c * bad_stride]) return;
  const int K = KT ? KT : K_;
  sm_stage(tile, SmSrc{in, t.in_off, fmt}, t, K / 2);
  for (int e = threadIdx.x; e < kSmTile; e += kSmThreads) {
    const int64_t i = t.j0 + e;
    if (i >= t.n) break;
    out[t.out_off + i] = sm_median(tile + e, K);
  }
}

__global__ void __launch_bounds__(kSmThreads) k_savgol(const void* __restrict__ in, int fmt, const SgTab* __restrict__ tab_,
                                                       int64_t min_n, const SmClip* __restrict__ clips, int n,
                                                       const uint32_t* __restrict__ bad, int bad_stride, float* __restrict__ out) {
  __shared__ float tile[kSmTile + 2 * kSmMaxHalo];
  const SmTile t = sm_find(clips, n, blockIdx.x);
  if (bad[(int64_t)t.c * bad_stride]) return;
  const sm_const<SgTab> tab = sm_as_const(tab_);
  const int W = tab->W, h = tab->h;
  const SmSrc src{in, t.in_off, fmt};
  sm_stage(tile, src, t, h);
  for (int e = threadIdx.x; e < kSmTile; e += kSmThreads) {
    const int64_t i = t.j0 + e;
    if (i >= t.n) break;
    float y;
    if (t.n < min_n) y = tile[e + h];
    else if (i < h || i >= t.n - h) y = sg_edge(tab, src, t.n, i);
    else y = (float)sg_dot(tab->t, tile + e, W);
    out[t.out_off + i] = y;
  }
}

// ---- the energy and ZCR groups ----

__device__ __forceinline__ int ez_find(const EzClip* clips, int n, int64_t g) {
  const sm_const<EzClip> cc = sm_as_const(clips);
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (cc[mid].first_frame <= g) lo = mid; else hi = mid - 1;
  }
  return lo;
}

__global__ void __launch_bounds__(kSmThreads) k_ez_peak(const float* __restrict__ sig, const EzClip* __restrict__ clips,
                                                        const uint32_t* __restrict__ bad, int bad_stride, float* __restrict__ peak) {
  __shared__ float s_max[kSmThreads];
  if (bad[(int64_t)blockIdx.x * bad_stride]) return;
  const EzClip cl = clips[blockIdx.x];
  float mx = 0.0f;
  for (int64_t i = threadIdx.x; i < cl.n; i += kSmThreads) mx = fmaxf(mx, fabsf(sig[cl.off + i]));
  s_max[threadIdx.x] = mx;
  __syncthreads();
  for (int w = kSmThreads / 2; w > 0; w >>= 1) {
    if (threadIdx.x < w) s_max[threadIdx.x] = fmaxf(s_max[threadIdx.x], s_max[threadIdx.x + w]);
    __syncthreads();
  }
  if (threadIdx.x == 0) peak[blockIdx.x] = s_max[0];
}

__global__ void __launch_bounds__(kSmThreads) k_ez_sign(const float* __restrict__ sig, const SmClip* __restrict__ clips, int n,
                                                        const uint32_t* __restrict__ bad, int bad_stride,
                                                        const float* __restrict__ peak, uint8_t* __restrict__ neg) {
  const SmTile t = sm_find(clips, n, blockIdx.x);
  if (bad[(int64_t)t.c * bad_stride]) return;
  const float pk = peak[t.c];
  for (int e = threadIdx.x; e < kSmTile; e += kSmThreads) {
    const int64_t i = t.j0 + e;
    if (i >= t.n) break;
    neg[t.out_off + i] = ez_neg(sig[t.out_off + i], pk) ? 1 : 0;
  }
}

// one wave per frame: frame t holds the samples t hop - fl / 2 + k, 0 <= k < fl (fl >= 64: every lane has terms)
__global__ void __launch_bounds__(256) k_ez_frames(const void* __restrict__ y, int y_fmt, const uint8_t* __restrict__ neg,
                                                   const EzClip* __restrict__ clips, int n, int64_t n_frames,
                                                   const uint32_t* __restrict__ bad, int bad_stride, double* __restrict__ energy,
                                                   double* __restrict__ rate) {
  const int lane = threadIdx.x & 63;
  const int64_t g = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (g >= n_frames) return;
  const int c = ez_find(clips, n, g);
  if (bad[(int64_t)c * bad_stride]) return;
  const EzClip cl = clips[c];
  const int64_t t = g - cl.first_frame;
  const int64_t g0 = t * cl.hop - cl.fl / 2;
  if (y) {
    // librosa.feature.rms: centred, zero padding; squares of float32 are exact in float64
    const SmSrc src{y, cl.y_off, y_fmt};
    double a = 0.0;
    for (int k = lane; k < cl.fl; k += kEzFrameLanes) {
      const int64_t j = g0 + k;
      const double v = j >= 0 && j < cl.n ? (double)sm_raw(src, j) : 0.0;
      a = fma(v, v, a);
    }
#pragma unroll
    for (int w = kEzFrameLanes / 2; w > 0; w >>= 1) a = a + __shfl_down(a, w);
    if (lane == 0) energy[cl.first_frame + t] = sqrt(a / (double)cl.fl);
  }
  if (neg) {
    // librosa.feature.zero_crossing_rate: centred, edge padding; the frame's first sample is never a crossing
    const uint8_t* s = neg + cl.off;
    auto at = [&](int64_t j) -> int { return s[j < 0 ? 0 : (j >= cl.n ? cl.n - 1 : j)]; };
    int cnt = 0;
    for (int k = lane; k < cl.fl; k += kEzFrameLanes)
      if (k > 0) cnt += at(g0 + k) != at(g0 + k - 1) ? 1 : 0;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) cnt += __shfl_xor(cnt, o);
    if (lane == 0) rate[cl.first_frame + t] = (double)cnt / (double)cl.fl;
  }
}

// sum over t of term(t) in the order of sm_tree_sum: lane j takes t = j, j + 256, .. in ascending order
template <typename F>
__device__ __forceinline__ double ez_block_sum(double* p, int64_t T, F term) {
  double a = 0.0;
  for (int64_t t = threadIdx.x; t < T; t += kEzStatLanes) a = term(a, t);
  __syncthreads();                               // p may still be read from the sum before
  p[threadIdx.x] = a;
  __syncthreads();
  for (int w = kEzStatLanes / 2; w > 0; w >>= 1) {
    if (threadIdx.x < w) p[threadIdx.x] = p[threadIdx.x] + p[threadIdx.x + w];
    __syncthreads();
  }
  return p[0];
}

// the k-th smallest (0-based) of v[0 .. T), all >= +0: a radix select over the bit patterns, most significant byte first
__device__ __forceinline__ double ez_select(const double* v, int64_t T, int64_t k, unsigned* hist, unsigned long long* pick) {
  unsigned long long prefix = 0;
  for (int b = 7; b >= 0; --b) {
    __syncthreads();
    hist[threadIdx.x] = 0;
    __syncthreads();
    const unsigned long long mask = b == 7 ? 0ull : ~0ull << (8 * (b + 1));
    for (int64_t t = threadIdx.x; t < T; t += kEzStatLanes) {
      const unsigned long long u = (unsigned long long)__double_as_longlong(v[t]);
      if ((u & mask) == prefix) atomicAdd(&hist[(u >> (8 * b)) & 255], 1u);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      int64_t below = 0;
      int bin = 0;
      for (; bin < 255; ++bin) {
        if (below + hist[bin] > k) break;
        below += hist[bin];
      }
      pick[0] = (unsigned long long)bin;
      pick[1] = (unsigned long long)below;
    }
    __syncthreads();
    prefix |= pick[0] << (8 * b);
    k -= (int64_t)pick[1];
  }
  return __longlong_as_double((long long)prefix);
}

__global__ void __launch_bounds__(kEzStatLanes) k_ez_stats(const EzClip* __restrict__ clips, const uint32_t* __restrict__ bad,
                                                           int bad_stride, int flags, const double* __restrict__ energy,
                                                           const double* __restrict__ rate, double* __restrict__ rec) {
  __shared__ double p[kEzStatLanes];
  __shared__ unsigned hist[kEzStatLanes];
  __shared__ unsigned long long pick[2];
  if (bad[(int64_t)blockIdx.x * bad_stride]) return;
  const EzClip cl = clips[blockIdx.x];
  const int64_t T = cl.T;
  double* r = rec + (int64_t)blockIdx.x * kEzN;
  auto mean_std = [&](const double* v, double* mean, double* sd) {
    const double m = ez_block_sum(p, T, [&](double a, int64_t t) { return a + v[t]; }) / (double)T;
    const double q = ez_block_sum(p, T, [&](double a, int64_t t) { const double d = v[t] - m; return fma(d, d, a); });
    *mean = m; *sd = sqrt(q / (double)T);
  };
  if (flags & AFX_EZ_ENERGY) {
    const double* v = energy + cl.first_frame;
    double m, sd;
    mean_std(v, &m, &sd);
    int64_t k0, k1;
    double g;
    ez_p10_index(T, &k0, &k1, &g);
    const double a = ez_select(v, T, k0, hist, pick);
    const double b = ez_select(v, T, k1, hist, pick);
    if (threadIdx.x == 0) { r[AFX_EZ_ENERGY_MEAN] = m; r[AFX_EZ_ENERGY_STD] = sd; r[AFX_EZ_ENERGY_P10] = ez_lerp(a, b, g); }
  }
  if (flags & AFX_EZ_ZCR) {
    const double* v = rate + cl.first_frame;
    double m, sd;
    mean_std(v, &m, &sd);
    const int w = T < kEzWin ? (int)T : kEzWin;
    double local = sd;
    if (w > 1) {
      const int64_t nw = T - w + 1;
      local = ez_block_sum(p, nw, [&](double a, int64_t i) { return a + ez_window_std(v + i, w); }) / (double)nw;
    }
    if (threadIdx.x == 0) { r[AFX_EZ_ZCR_MEAN] = m; r[AFX_EZ_ZCR_STD] = sd; r[AFX_EZ_ZCR_LOCAL] = local; }
  }
}

hipError_t launch_sm_check(hipStream_t s, const void* in, int fmt, const SmClip* clips, int n, uint32_t* bad) {
  hipLaunchKernelGGL(k_sm_check, dim3(n), dim3(kSmThreads), 0, s, in, fmt, clips, bad);
  return hipGetLastError();
}

hipError_t launch_medfilt(hipStream_t s, const void* in, int fmt, int K, const SmClip* clips, int n, int n_tiles,
                          const uint32_t* bad, int bad_stride, float* out) {
  switch (K) {
    case 1: hipLaunchKernelGGL(k_medfilt<1>, dim3(n_tiles), dim3(kSmThreads), 0, s, in, fmt, K, clips, n, bad, bad_stride, out); break;
    case 3: hipLaunchKernelGGL(k_medfilt<3>, dim3(n_tiles), dim3(kSmThreads), 0, s, in, fmt, K, clips, n, bad, bad_stride, out); break;
    case 5: hipLaunchKernelGGL(k_medfilt<5>, dim3(n_tiles), dim3(kSmThreads), 0, s, in, fmt, K, clips, n, bad, bad_stride, out); break;
    default: hipLaunchKernelGGL(k_medfilt<0>, dim3(n_tiles), dim3(kSmThreads), 0, s, in, fmt, K, clips, n, bad, bad_stride, out); break;
  }
  return hipGetLastError();
}

hipError_t launch_savgol(hipStream_t s, const void* in, int fmt, const SgTab* tab, int64_t min_n, const SmClip* clips, int n,
                         int n_tiles, const uint32_t* bad, int bad_stride, float* out) {
  hipLaunchKernelGGL(k_savgol, dim3(n_tiles), dim3(kSmThreads), 0, s, in, fmt, tab, min_n, clips, n, bad, bad_stride, out);
  return hipGetLastError();
}

hipError_t launch_ez_peak(hipStream_t s, const float* sig, const EzClip* clips, int n, const uint32_t* bad, int bad_stride,
                          float* peak) {
  hipLaunchKernelGGL(k_ez_peak, dim3(n), dim3(kSmThreads), 0, s, sig, clips, bad, bad_stride, peak);
  return hipGetLastError();
}

hipError_t launch_ez_sign(hipStream_t s, const float* sig, const SmClip* clips, int n, int n_tiles, const uint32_t* bad,
                          int bad_stride, const float* peak, uint8_t* neg) {
  hipLaunchKernelGGL(k_ez_sign, dim3(n_tiles), dim3(kSmThreads), 0, s, sig, clips, n, bad, bad_stride, peak, neg);
  return hipGetLastError();
}

hipError_t launch_ez_frames(hipStream_t s, const void* y, int y_fmt, const uint8_t* neg, const EzClip* clips, int n,
                            int64_t n_frames, const uint32_t* bad, int bad_stride, double* energy, double* rate) {
  hipLaunchKernelGGL(k_ez_frames, dim3((unsigned)((n_frames + 3) / 4)), dim3(256), 0, s, y, y_fmt, neg, clips, n, n_frames, bad,
                     bad_stride, energy, rate);
  return hipGetLastError();
}

hipError_t launch_ez_stats(hipStream_t s, const EzClip* clips, int n, const uint32_t* bad, int bad_stride, int flags,
                           const double* energy, const double* rate, double* rec) {
  hipLaunchKernelGGL(k_ez_stats, dim3(n), dim3(kEzStatLanes), 0, s, clips, bad, bad_stride, flags, energy, rate, rec);
  return hipGetLastError();
}

}  // namespace afx
