// The recording screen and the compare sums for gfx950 (layout: afx_assess.h; definitions: include/afx.h).  Streaming
// kernels: every sample is read from HBM once, as 16-byte loads where the clip's address allows.  Squares of float32 samples
// are exact in float64 and are summed there, in orders that depend on the clip alone: no atomics, nothing depends on the
// rest of the batch.
#include <hip/hip_runtime.h>

#include <cmath>

#include "afx.h"
#include "afx_assess.h"

namespace afx {

template <typename T> using as_const = const __attribute__((address_space(4))) T*;

// the record whose span range holds workgroup b: the last one with span_base <= b (every record has at least one span)
template <typename R>
__device__ __forceinline__ int as_find(as_const<R> recs, int n, int64_t b) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (recs[mid].span_base <= b) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// samples j .. j + 3 of a span of ns samples at p (zeros from ns on): one 16-byte (S16: 8-byte) load where `wide` says the
// span's first sample is aligned to it and all four are inside, else one load per sample.  Either way the same values.
template <int FMT>
__device__ __forceinline__ float4 as_load4(const void* __restrict__ p, int j, int ns, bool wide) {
  float v[4] = {0.f, 0.f, 0.f, 0.f};
  if constexpr (FMT == AFX_FMT_S16) {
    const int16_t* q = (const int16_t*)p + j;
    if (wide && j + 4 <= ns) {
      const uint2 w = *(const uint2*)q;
      v[0] = (float)(int16_t)(w.x & 0xffffu) * 0x1p-15f; v[1] = (float)(int16_t)(w.x >> 16) * 0x1p-15f;
      v[2] = (float)(int16_t)(w.y & 0xffffu) * 0x1p-15f; v[3] = (float)(int16_t)(w.y >> 16) * 0x1p-15f;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) if (j + e < ns) v[e] = (float)q[e] * 0x1p-15f;
    }
  } else {
    const float* q = (const float*)p + j;
    if (wide && j + 4 <= ns) {
      const float4 w = *(const float4*)q;
      v[0] = w.x; v[1] = w.y; v[2] = w.z; v[3] = w.w;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) if (j + e < ns) v[e] = q[e];
    }
  }
  return make_float4(v[0], v[1], v[2], v[3]);
}

template <int FMT>
__device__ __forceinline__ bool as_is_wide(const void* p) {
  return ((uintptr_t)p & (FMT == AFX_FMT_S16 ? 7 : 15)) == 0;
}

__device__ __forceinline__ double as_wave_sum(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}
__device__ __forceinline__ double as_wave_max(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = fmax(v, __shfl_xor(v, m, 64));
  return v;
}
// the workgroup's sum in every lane: the four waves' sums added in wave order.  red: 4 doubles; two barriers
__device__ __forceinline__ double as_block_sum(double v, double* red) {
  v = as_wave_sum(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  const double s = ((red[0] + red[1]) + red[2]) + red[3];
  __syncthreads();
  return s;
}
__device__ __forceinline__ double as_block_max(double v, double* red) {
  v = as_wave_max(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  const double s = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
  __syncthreads();
  return s;
}

// N sums at once, each as as_block_sum forms it (the four waves' sums added in wave order).  red: 4 N doubles; two barriers
template <int N>
__device__ __forceinline__ void as_block_sums(double (&v)[N], double* red) {
#pragma unroll
  for (int q = 0; q < N; ++q) {
    v[q] = as_wave_sum(v[q]);
    if ((threadIdx.x & 63) == 0) red[4 * q + (threadIdx.x >> 6)] = v[q];
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < N; ++q) v[q] = ((red[4 * q] + red[4 * q + 1]) + red[4 * q + 2]) + red[4 * q + 3];
  __syncthreads();
}

__device__ __forceinline__ double as_sq(float x) { return (double)x * (double)x; }

// The pieces of one framing that lie in span i = [s0, s0 + ns) of a clip, from the span's LDS image: piece (t, i) goes to
// P[t + i].  Who sums a piece depends on fl alone (the workgroup, a wave or a lane), and each sums in one fixed order.
__device__ __forceinline__ void as_pieces(const float* sx, int64_t s0, int ns, int64_t i, int32_t fl, double* __restrict__ P,
                                          double* red) {
  const int64_t h = fl / 2;
  const int64_t t0 = (s0 + h) / fl, t1 = (s0 + ns - 1 + h) / fl;
  const int np = (int)(t1 - t0 + 1);                                   // <= ns + 1
  const int tid = threadIdx.x;
  auto bounds = [&](int p, int& lo, int& hi) {
    const int64_t a = (t0 + p) * fl - h;
    lo = (int)(a > s0 ? a - s0 : 0);
    hi = (int)(a + fl < s0 + ns ? a + fl - s0 : ns);
  };
  if (fl >= kAsWide) {
    for (int p = 0; p < np; ++p) {
      int lo, hi;
      bounds(p, lo, hi);
      double a = 0.0;
      for (int j = lo + tid; j < hi; j += kAsLanes) a += as_sq(sx[j]);
      a = as_block_sum(a, red);
      if (tid == 0) P[t0 + p + i] = a;
    }
  } else if (fl >= kAsNarrow) {
    for (int p = tid >> 6; p < np; p += kAsLanes / 64) {
      int lo, hi;
      bounds(p, lo, hi);
      double a = 0.0;
      for (int j = lo + (tid & 63); j < hi; j += 64) a += as_sq(sx[j]);
      a = as_wave_sum(a);
      if ((tid & 63) == 0) P[t0 + p + i] = a;
    }
  } else {
    for (int p = tid; p < np; p += kAsLanes) {
      int lo, hi;
      bounds(p, lo, hi);
      double a = 0.0;
      for (int j = lo; j < hi; ++j) a += as_sq(sx[j]);
      P[t0 + p + i] = a;
    }
  }
}

template <int FMT>
__global__ void __launch_bounds__(kAsLanes) k_assess_spans(const void* __restrict__ samples, const AsClip* __restrict__ clips,
                                                           int n_clips, double* __restrict__ pieces, AsSpan* __restrict__ spans) {
  __shared__ __attribute__((aligned(16))) float sx[kAsSpan];
  __shared__ double red[4];
  __shared__ float red_pk[4];
  __shared__ uint32_t red_bad[4];
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x;
  const as_const<AsClip> cc = (as_const<AsClip>)(uintptr_t)clips;
  const int c = as_find(cc, n_clips, b);
  const int64_t len = cc[c].len, nw = cc[c].nw, i = b - cc[c].span_base, s0 = i << kAsSpanLog;
  const int32_t fs = cc[c].fs, fl = cc[c].fl;
  const int ns = (int)(len - s0 < kAsSpan ? len - s0 : kAsSpan);       // >= 1: the clip has exactly ceil(len / kAsSpan) spans
  const void* p = FMT == AFX_FMT_S16 ? (const void*)((const int16_t*)samples + cc[c].in_off + s0)
                                     : (const void*)((const float*)samples + cc[c].in_off + s0);
  const bool wide = as_is_wide<FMT>(p);
  float pk = 0.f;
  bool bad = false;
#pragma unroll
  for (int k = 0; k < kAsSpan / (4 * kAsLanes); ++k) {
    const int j = 4 * (tid + kAsLanes * k);
    const float4 v = as_load4<FMT>(p, j, ns, wide);
    *(float4*)(sx + j) = v;
    pk = fmaxf(fmaxf(pk, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
    bad = bad || !(isfinite(v.x) && isfinite(v.y) && isfinite(v.z) && isfinite(v.w));
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) pk = fmaxf(pk, __shfl_xor(pk, m, 64));
  const bool wbad = __any(bad);
  if ((tid & 63) == 0) { red_pk[tid >> 6] = pk; red_bad[tid >> 6] = wbad ? 1u : 0u; }
  __syncthreads();                                                     // the span is in LDS
  // the span's part of the noise window [0, nw)
  const int m = (int)(nw - s0 <= 0 ? 0 : nw - s0 < ns ? nw - s0 : ns);
  double noise = 0.0;
  if (m > 0) {                                                         // the same in every lane
    for (int j = tid; j < m; j += kAsLanes) noise += as_sq(sx[j]);
    noise = as_block_sum(noise, red);
  }
  if (tid == 0) {
    AsSpan r;
    r.noise = noise;
    r.peak = fmaxf(fmaxf(red_pk[0], red_pk[1]), fmaxf(red_pk[2], red_pk[3]));
    r.bad = red_bad[0] | red_bad[1] | red_bad[2] | red_bad[3];
    spans[b] = r;
  }
  as_pieces(sx, s0, ns, i, fs, pieces + cc[c].ps_off, red);
  as_pieces(sx, s0, ns, i, fl, pieces + cc[c].pl_off, red);
}

// the sum of squares of frame t (the collector as_frames(len, fl) included): its pieces in increasing span order
__device__ __forceinline__ double as_frame_ss(const double* __restrict__ P, int64_t t, int32_t fl, int64_t len) {
  int64_t a = t * fl - fl / 2, e = a + fl < len ? a + fl : len;
  if (a < 0) a = 0;
  if (e <= a) return 0.0;
  const int64_t i0 = a >> kAsSpanLog, i1 = (e - 1) >> kAsSpanLog;
  double s = 0.0;
  for (int64_t i = i0; i <= i1; ++i) s += P[t + i];
  return s;
}

// One workgroup per clip.  Lane l owns the frames [l per, (l + 1) per) of either framing, per = ceil(frames / 256): its
// maximum, its sums and the summary of its silent runs (count, leading run, trailing run, longest run inside); the 256
// summaries are joined by one lane, so the run scan of T frames costs T / 256 + 256 steps.
__global__ void __launch_bounds__(kAsLanes) k_assess_finish(const AsClip* __restrict__ clips, const double* __restrict__ pieces,
                                                            const AsSpan* __restrict__ spans, double thr_ratio,
                                                            double* __restrict__ rec, int32_t* __restrict__ bad) {
  __shared__ double red[4];
  __shared__ int64_t s_cnt[kAsLanes], s_pre[kAsLanes], s_suf[kAsLanes], s_best[kAsLanes];
  const int tid = threadIdx.x, c = blockIdx.x;
  const as_const<AsClip> cc = (as_const<AsClip>)(uintptr_t)clips;
  const int64_t len = cc[c].len, nw = cc[c].nw, sb = cc[c].span_base;
  const int32_t fs = cc[c].fs, fl = cc[c].fl;
  const int64_t n_spans = (len + kAsSpan - 1) >> kAsSpanLog;
  double* out = rec + (size_t)c * AFX_ASSESS_N;
  // the span records: peak, flag, the noise window's sum in span order within a lane, lanes in a fixed tree
  double pk = 0.0, isbad = 0.0, noise = 0.0;
  const int64_t n_noise = (nw + kAsSpan - 1) >> kAsSpanLog;
  for (int64_t i = tid; i < n_spans; i += kAsLanes) {
    const AsSpan r = spans[sb + i];
    pk = fmax(pk, (double)r.peak);
    if (r.bad) isbad = 1.0;
    if (i < n_noise) noise += r.noise;
  }
  pk = as_block_max(pk, red);
  isbad = as_block_max(isbad, red);
  noise = as_block_sum(noise, red);
  if (isbad != 0.0) {                                                  // the same in every lane
    if (tid < AFX_ASSESS_N) out[tid] = __builtin_nan("");
    if (tid == 0) bad[c] = 1;
    return;
  }
  // ---- the short framing ----
  const double* Ps = pieces + cc[c].ps_off;
  const int64_t T = as_frames(len, fs), per = (T + kAsLanes - 1) / kAsLanes;
  const int64_t f0 = tid * per < T ? tid * per : T, f1 = f0 + per < T ? f0 + per : T;
  double mx = 0.0, tot = 0.0;
  for (int64_t t = f0; t < f1; ++t) {
    const double ss = as_frame_ss(Ps, t, fs, len);
    mx = fmax(mx, ss);
    tot += ss;
  }
  if (tid == kAsLanes - 1) tot += as_frame_ss(Ps, T, fs, len);         // the samples behind the last frame
  mx = as_block_max(mx, red);
  tot = as_block_sum(tot, red);
  // silent: rms_db < threshold_db with rms_db = 10 log10(max(amin^2, p)) - 10 log10(max(amin^2, pmax)), p = ss / fs, clamped
  // at -80 from below: max(amin^2, p) < max(amin^2, pmax) 10^(threshold_db / 10), and never when threshold_db <= -80
  const double a2 = 1e-10, pmax = mx / (double)fs;
  const double lim = fmax(a2, pmax) * thr_ratio;
  int64_t cnt = 0, pre = 0, run = 0, best = 0;
  bool open = true;                                                    // no loud frame seen yet: the run is the leading one
  for (int64_t t = f0; t < f1; ++t) {
    const bool silent = thr_ratio >= 0.0 && fmax(a2, as_frame_ss(Ps, t, fs, len) / (double)fs) < lim;
    if (silent) {
      ++cnt; ++run;
    } else {
      if (open) { pre = run; open = false; }
      best = run > best ? run : best;
      run = 0;
    }
  }
  if (open) pre = run;                                                 // all silent (or no frames): cnt == pre == suf
  s_cnt[tid] = cnt; s_pre[tid] = pre; s_suf[tid] = run; s_best[tid] = best;
  __syncthreads();
  if (tid == 0) {
    int64_t total = 0, longest = 0, carry = 0;
    for (int l = 0; l < kAsLanes; ++l) {
      const int64_t a = l * per < T ? l * per : T, e = a + per < T ? a + per : T;
      if (e == a) break;
      total += s_cnt[l];
      if (s_cnt[l] == e - a) { carry += e - a; continue; }             // silent throughout: the run goes on
      carry += s_pre[l];
      longest = carry > longest ? carry : longest;
      longest = s_best[l] > longest ? s_best[l] : longest;
      carry = s_suf[l];
    }
    longest = carry > longest ? carry : longest;                       // a run that reaches the last frame counts
    out[0] = (double)T;
    out[1] = (double)total;
    out[2] = (double)longest;
    out[3] = sqrt(pmax);
    out[4] = tot / (double)len;
    out[5] = pk;
    out[6] = nw > 0 ? noise / (double)nw : __builtin_nan("");
    bad[c] = 0;
  }
  // ---- the long framing: mean and population deviation of the frames' RMS, the deviation around the mean ----
  const double* Pl = pieces + cc[c].pl_off;
  const int64_t TL = as_frames(len, fl), perl = (TL + kAsLanes - 1) / kAsLanes;
  const int64_t g0 = tid * perl < TL ? tid * perl : TL, g1 = g0 + perl < TL ? g0 + perl : TL;
  double sum = 0.0;
  for (int64_t t = g0; t < g1; ++t) sum += sqrt(as_frame_ss(Pl, t, fl, len) / (double)fl);
  const double mean = as_block_sum(sum, red) / (double)TL;
  double dev = 0.0;
  for (int64_t t = g0; t < g1; ++t) {
    const double d = sqrt(as_frame_ss(Pl, t, fl, len) / (double)fl) - mean;
    dev += d * d;
  }
  dev = as_block_sum(dev, red);
  if (tid == 0) {
    out[7] = (double)TL;
    out[8] = mean;
    out[9] = sqrt(dev / (double)TL);
  }
}

// ---- the compare sums: one workgroup per span of a pair, then one wave per pair ----
// A span's raw sums, then -- its 16 samples per lane still in registers -- the sums centred on the span's own means.  The
// finishing kernel joins the spans' centred sums around the pair's means (M2 = sum M2_i + n_i (mean_i - mean)^2, every
// term >= 0), so the correlation of a pair with a large offset does not cancel.
template <int FMT>
__global__ void __launch_bounds__(kAsLanes) k_compare_spans(const void* __restrict__ ref, const void* __restrict__ deg,
                                                            const CmpPair* __restrict__ pairs, int n_pairs,
                                                            double* __restrict__ part) {
  __shared__ double red[4 * 6];
  constexpr int K = kAsSpan / (4 * kAsLanes);
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x;
  const as_const<CmpPair> pp = (as_const<CmpPair>)(uintptr_t)pairs;
  const int c = as_find(pp, n_pairs, b);
  const int64_t s0 = (b - pp[c].span_base) << kAsSpanLog, n = pp[c].n;
  const int ns = (int)(n - s0 < kAsSpan ? n - s0 : kAsSpan);
  const void* pr = FMT == AFX_FMT_S16 ? (const void*)((const int16_t*)ref + pp[c].r_off + s0) : (const void*)((const float*)ref + pp[c].r_off + s0);
  const void* pd = FMT == AFX_FMT_S16 ? (const void*)((const int16_t*)deg + pp[c].d_off + s0) : (const void*)((const float*)deg + pp[c].d_off + s0);
  const bool wr = as_is_wide<FMT>(pr), wd = as_is_wide<FMT>(pd);
  float r[4 * K], d[4 * K];
  double a[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  bool bad = false;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int j = 4 * (tid + kAsLanes * k);
    const float4 r4 = as_load4<FMT>(pr, j, ns, wr), d4 = as_load4<FMT>(pd, j, ns, wd);
    r[4 * k] = r4.x; r[4 * k + 1] = r4.y; r[4 * k + 2] = r4.z; r[4 * k + 3] = r4.w;
    d[4 * k] = d4.x; d[4 * k + 1] = d4.y; d[4 * k + 2] = d4.z; d[4 * k + 3] = d4.w;
#pragma unroll
    for (int e = 0; e < 4; ++e) {                                      // samples behind the pair's end are zeros: they add nothing
      const double x = (double)r[4 * k + e], y = (double)d[4 * k + e];
      const double z = (double)(d[4 * k + e] - r[4 * k + e]);          // the difference in float32, as numpy's
      a[0] += x; a[1] += y; a[2] += x * x; a[3] += y * y; a[4] += x * y; a[5] += z * z;
      bad = bad || !(isfinite(r[4 * k + e]) && isfinite(d[4 * k + e]));
    }
  }
  const bool anybad = __syncthreads_or(bad);
  double* out = part + (size_t)b * kCmpSpanDoubles;
  as_block_sums(a, red);
#pragma unroll
  for (int q = 0; q < 6; ++q) if (tid == 0) out[q] = a[q];
  const double mr = a[0] / (double)ns, md = a[1] / (double)ns;
  double m[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int k = 0; k < K; ++k)
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (4 * (tid + kAsLanes * k) + e < ns) {
        const double x = (double)r[4 * k + e] - mr, y = (double)d[4 * k + e] - md;
        m[0] += x * x; m[1] += y * y; m[2] += x * y;
      }
  as_block_sums(m, red);
#pragma unroll
  for (int q = 0; q < 3; ++q) if (tid == 0) out[6 + q] = m[q];
  if (tid == 0) out[9] = anybad ? 1.0 : 0.0;
}

__global__ void __launch_bounds__(64) k_compare_finish(const CmpPair* __restrict__ pairs, const double* __restrict__ part,
                                                       double* __restrict__ rec, int32_t* __restrict__ bad) {
  const int lane = threadIdx.x, c = blockIdx.x;
  const int64_t n = pairs[c].n, n_spans = (n + kAsSpan - 1) >> kAsSpanLog;
  const double* P = part + (size_t)pairs[c].span_base * kCmpSpanDoubles;
  double a[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};                   // the six raw sums, the flag
  for (int64_t i = lane; i < n_spans; i += 64) {
#pragma unroll
    for (int q = 0; q < 6; ++q) a[q] += P[i * kCmpSpanDoubles + q];
    a[6] += P[i * kCmpSpanDoubles + 9];
  }
#pragma unroll
  for (int q = 0; q < 7; ++q) a[q] = as_wave_sum(a[q]);
  const double mr = a[0] / (double)n, md = a[1] / (double)n;
  double m[3] = {0.0, 0.0, 0.0};
  for (int64_t i = lane; i < n_spans; i += 64) {
    const double ni = (double)(n - (i << kAsSpanLog) < kAsSpan ? n - (i << kAsSpanLog) : kAsSpan);
    const double dr = P[i * kCmpSpanDoubles] / ni - mr, dd = P[i * kCmpSpanDoubles + 1] / ni - md;
    m[0] += P[i * kCmpSpanDoubles + 6] + ni * dr * dr;
    m[1] += P[i * kCmpSpanDoubles + 7] + ni * dd * dd;
    m[2] += P[i * kCmpSpanDoubles + 8] + ni * dr * dd;
  }
#pragma unroll
  for (int q = 0; q < 3; ++q) m[q] = as_wave_sum(m[q]);
  if (lane == 0) {
    double* out = rec + (size_t)c * AFX_COMPARE_N;
    const bool isbad = a[6] != 0.0;
    const double nan = __builtin_nan("");
    out[0] = isbad ? nan : (double)n;
#pragma unroll
    for (int q = 0; q < 6; ++q) out[1 + q] = isbad ? nan : a[q];
#pragma unroll
    for (int q = 0; q < 3; ++q) out[7 + q] = isbad ? nan : m[q];
    bad[c] = isbad ? 1 : 0;
  }
}

hipError_t launch_assess(hipStream_t s, const void* samples, int sample_fmt, const AsClip* clips, int n_clips, int n_blocks,
                         double thr_ratio, double* pieces, AsSpan* spans, double* rec, int32_t* bad) {
  if (n_clips <= 0 || n_blocks <= 0) return hipSuccess;
  if (sample_fmt == AFX_FMT_S16)
    hipLaunchKernelGGL(k_assess_spans<AFX_FMT_S16>, dim3(n_blocks), dim3(kAsLanes), 0, s, samples, clips, n_clips, pieces, spans);
  else
    hipLaunchKernelGGL(k_assess_spans<AFX_FMT_F32>, dim3(n_blocks), dim3(kAsLanes), 0, s, samples, clips, n_clips, pieces, spans);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_assess_finish, dim3(n_clips), dim3(kAsLanes), 0, s, clips, pieces, spans, thr_ratio, rec, bad);
  return hipGetLastError();
}

hipError_t launch_compare(hipStream_t s, const void* ref, const void* deg, int sample_fmt, const CmpPair* pairs, int n_pairs,
                          int n_blocks, double* part, double* rec, int32_t* bad) {
  if (n_pairs <= 0 || n_blocks <= 0) return hipSuccess;
  if (sample_fmt == AFX_FMT_S16)
    hipLaunchKernelGGL(k_compare_spans<AFX_FMT_S16>, dim3(n_blocks), dim3(kAsLanes), 0, s, ref, deg, pairs, n_pairs, part);
  else
    hipLaunchKernelGGL(k_compare_spans<AFX_FMT_F32>, dim3(n_blocks), dim3(kAsLanes), 0, s, ref, deg, pairs, n_pairs, part);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_compare_finish, dim3(n_pairs), dim3(64), 0, s, pairs, part, rec, bad);
  return hipGetLastError();
}

}  // namespace afx
