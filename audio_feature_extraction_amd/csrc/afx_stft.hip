// librosa-style stft / istft at n_fft 1024 and 2048, any hop in [1, n_fft], any window table (afx_stft.h).
//   k_stft_frames<NFFT, KIND>  one wave per unit (a 2048 frame, or two 1024 frames packed into one complex transform), four
//                              waves per workgroup, one 8 KB LDS image per wave: the samples through the pad rule (zeros, or
//                              the folded index of np.pad's reflect), x window, hp_fft1024, the real-FFT split (2048) or the
//                              a + i b separation (1024), the packed row: complex64, |D| or |D|^2
//   k_istft_frames<NFFT>       the rows back: merge (2048) or a + i b packing (1024), hp_fft1024, x window / n_fft, as time
//                              rows of n_fft floats in a workspace.  A row with a NaN / inf bin is taken out of the transform
//                              and its time row set to NaN, so that at 1024 it cannot reach the frame it is packed with
//   k_istft_ola                overlap-add as a gather in increasing frame order, the overlap-added window^2 beside it,
//                              / where that exceeds FLT_MIN, zeros beyond the last frame
// The samples come from k_hpss_prep (float32 and the non-finite flag per clip).  No atomics in any sum; a clip reads nothing
// of another.  Rows of 1025 / 513 complex64 are 8-byte but not 16-byte aligned: stores are v2, never wider.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>

#include "afx.h"
#include "afx_hpss_dev.h"
#include "afx_stft.h"

namespace afx {

namespace {

// |D| and |D|^2 as one fixed rounding sequence (hp_abs / gt_abs): two products, one sum, one square root
template <int KIND>
__device__ __forceinline__ float st_mag(v2 x) {
#pragma clang fp contract(off)
  const float a = x.x * x.x;
  const float b = x.y * x.y;
  return KIND == AFX_STFT_POWER ? a + b : sqrtf(a + b);
}

template <int KIND>
__device__ __forceinline__ void st_store(void* __restrict__ out, int64_t e, v2 x) {
  if constexpr (KIND == AFX_STFT_COMPLEX) ((v2*)out)[e] = x;
  else ((float*)out)[e] = st_mag<KIND>(x);
}

// sample i of the padded clip's own axis (i < 0 and i >= len lie in the padding): zero, or np.pad's reflect, which for
// len > n_fft / 2 folds once
__device__ __forceinline__ float st_sample(const float* __restrict__ y, const StftClip& c, int64_t i, bool reflect, bool zero) {
  if (reflect) i = i < 0 ? -i : i >= c.len ? 2 * (c.len - 1) - i : i;
  return (!zero && i >= 0 && i < c.len) ? y[c.y_off + i] : 0.f;
}

__device__ __forceinline__ bool st_bad(v2 x) { return !(isfinite(x.x) && isfinite(x.y)); }

}  // namespace

template <int NFFT, int KIND>
__global__ __launch_bounds__(256) void k_stft_frames(const float* __restrict__ y, const StftClip* __restrict__ clips,
                                                     const uint32_t* __restrict__ bad, int n, int64_t n_units, int hop, int shift,
                                                     int reflect, StftTabs tb, void* __restrict__ out) {
  constexpr int BINS = stft_bins(NFFT);
  __shared__ v2 lds[4][1024];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t u = (int64_t)blockIdx.x * 4 + wave;
  const bool live = u < n_units;                                 // a wave past the end transforms zeros and stores nothing
  const int64_t uu = live ? u : n_units - 1;
  const int ci = hp_find(n, uu, [&](int i) { return clips[i].unit_base; });
  const StftClip c = clips[ci];
  const bool zero = !live || bad[c.clip] != 0;
  const bool refl = reflect != 0;
  v2* buf = lds[wave];
  const v2* W1 = (const v2*)tb.w1024;

  if constexpr (NFFT == 2048) {
    const int64_t t = uu - c.unit_base;
    const int64_t s0 = t * hop - shift;
#pragma unroll 4
    for (int q = 0; q < 16; ++q) {
      const int m = lane + 64 * q;
      buf[m] = v2{tb.window[2 * m] * st_sample(y, c, s0 + 2 * m, refl, zero),
                  tb.window[2 * m + 1] * st_sample(y, c, s0 + 2 * m + 1, refl, zero)};
    }
    hp_fft1024(buf, W1, lane);
    const v2* W = (const v2*)tb.w2048;
    const int64_t row = c.out_off + t * BINS;
#pragma unroll 4
    for (int q = 0; q < 8; ++q) {
      const int k = lane + 64 * q;
      const v2 zk = buf[k], zn = buf[(1024 - k) & 1023];
      const v2 xk = hp_split(zk, zn, W[k]);
      const v2 xn = k ? hp_split(zn, zk, W[(1024 - k) & 1023]) : v2{zk.x - zk.y, 0.f};
      if (live) { st_store<KIND>(out, row + k, xk); st_store<KIND>(out, row + 1024 - k, xn); }
    }
    if (lane == 0 && live) {
      const v2 zm = buf[512];
      st_store<KIND>(out, row + 512, hp_split(zm, zm, W[512]));
    }
  } else {
    // two real frames a, b as z = a + i b: A[k] = (Z[k] + conj Z[N - k]) / 2, B[k] = (Z[k] - conj Z[N - k]) / 2i; the last
    // unit of a clip with an odd frame count has no frame b
    const int64_t ta = 2 * (uu - c.unit_base);
    const bool has_b = ta + 1 < c.T;
    const int64_t sa = ta * hop - shift, sb = sa + hop;
#pragma unroll 4
    for (int q = 0; q < 16; ++q) {
      const int m = lane + 64 * q;
      const float w = tb.window[m];
      buf[m] = v2{w * st_sample(y, c, sa + m, refl, zero), w * st_sample(y, c, sb + m, refl, zero || !has_b)};
    }
    hp_fft1024(buf, W1, lane);
    const int64_t rowa = c.out_off + ta * BINS, rowb = rowa + BINS;          // rowb is never touched without a frame b
#pragma unroll 4
    for (int q = 0; q < 8; ++q) {
      const int k = lane + 64 * q;
      const v2 zk = buf[k], zn = buf[(1024 - k) & 1023];
      const v2 A = v2{zk.x + zn.x, zk.y - zn.y} * 0.5f;
      const v2 B = v2{zk.y + zn.y, zn.x - zk.x} * 0.5f;
      if (live) {
        st_store<KIND>(out, rowa + k, A);
        if (has_b) st_store<KIND>(out, rowb + k, B);
      }
    }
    if (lane == 0 && live) {
      const v2 z = buf[512];
      st_store<KIND>(out, rowa + 512, v2{z.x, 0.f});
      if (has_b) st_store<KIND>(out, rowb + 512, v2{z.y, 0.f});
    }
  }
}

template <int NFFT>
__global__ __launch_bounds__(256) void k_istft_frames(const v2* __restrict__ spec, const IstftClip* __restrict__ clips, int n,
                                                      int64_t n_units, StftTabs tb, float* __restrict__ rows) {
  constexpr int BINS = stft_bins(NFFT);
  __shared__ v2 lds[4][1024];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t u = (int64_t)blockIdx.x * 4 + wave;
  const bool live = u < n_units;
  const int64_t uu = live ? u : n_units - 1;
  const int ci = hp_find(n, uu, [&](int i) { return clips[i].unit_base; });
  const IstftClip c = clips[ci];
  v2* buf = lds[wave];
  const v2* W1 = (const v2*)tb.w1024;
  const v2 z0 = v2{0.f, 0.f};
  const float qnan = __builtin_nanf("");

  if constexpr (NFFT == 2048) {
    const int64_t t = uu - c.unit_base;
    const v2* X = spec + c.spec_off + t * BINS;
    v2 xk[8], xn[8];
    bool flag = false;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int k = lane + 64 * q;
      xk[q] = live ? X[k] : z0;
      xn[q] = live ? X[1024 - k] : z0;
      if (k == 0) { xk[q].y = 0.f; xn[q].y = 0.f; }              // numpy's irfft ignores the imaginary parts of bins 0 and n / 2
      flag |= st_bad(xk[q]) || st_bad(xn[q]);
    }
    v2 xm = (live && lane == 0) ? X[512] : z0;
    flag |= st_bad(xm);
    const bool nf = __ballot(flag) != 0;                         // wave-uniform: the row holds a NaN / inf
    const v2* W = (const v2*)tb.w2048;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int k = lane + 64 * q;
      const v2 a = nf ? z0 : xk[q], b = nf ? z0 : xn[q];
      buf[k] = hp_merge(a, b, W[k]);
      if (k) buf[1024 - k] = hp_merge(b, a, W[(1024 - k) & 1023]);
    }
    if (lane == 0) {
      if (nf) xm = z0;
      buf[512] = hp_merge(xm, xm, W[512]);
    }
    hp_fft1024(buf, W1, lane);
    if (!live) return;
    const float sc = 1.0f / 2048.0f;
    v2* row = (v2*)(rows + (c.row_base + t) * NFFT);
#pragma unroll 4
    for (int q = 0; q < 16; ++q) {
      const int m = lane + 64 * q;
      const v2 z = buf[m];
      row[m] = nf ? v2{qnan, qnan} : v2{tb.window[2 * m] * (z.x * sc), tb.window[2 * m + 1] * (-z.y * sc)};
    }
  } else {
    // Y = Ya + i Yb with both extended Hermitian; buf takes conj Y, whose forward FFT is the conjugate of N times the inverse
    const int64_t ta = 2 * (uu - c.unit_base);
    const bool has_b = ta + 1 < c.n_frames;
    const v2* Xa = spec + c.spec_off + ta * BINS;
    const v2* Xb = Xa + (has_b ? BINS : 0);
    v2 ya[8], yb[8];
    bool fa = false, fb = false;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int k = lane + 64 * q;
      ya[q] = live ? Xa[k] : z0;
      yb[q] = (live && has_b) ? Xb[k] : z0;
      if (k == 0) { ya[q].y = 0.f; yb[q].y = 0.f; }
      fa |= st_bad(ya[q]);
      fb |= st_bad(yb[q]);
    }
    float ma = (live && lane == 0) ? Xa[512].x : 0.f;
    float mb = (live && has_b && lane == 0) ? Xb[512].x : 0.f;
    fa |= !isfinite(ma);
    fb |= !isfinite(mb);
    const bool nfa = __ballot(fa) != 0, nfb = __ballot(fb) != 0;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int k = lane + 64 * q;
      const v2 Ya = nfa ? z0 : ya[q], Yb = nfb ? z0 : yb[q];
      buf[k] = v2{Ya.x - Yb.y, -(Ya.y + Yb.x)};
      if (k) buf[1024 - k] = v2{Ya.x + Yb.y, Ya.y - Yb.x};
    }
    if (lane == 0) buf[512] = v2{nfa ? 0.f : ma, -(nfb ? 0.f : mb)};
    hp_fft1024(buf, W1, lane);
    if (!live) return;
    const float sc = 1.0f / 1024.0f;
    float* rowa = rows + (c.row_base + ta) * NFFT;
    float* rowb = rowa + (has_b ? NFFT : 0);
#pragma unroll 4
    for (int q = 0; q < 16; ++q) {
      const int m = lane + 64 * q;
      const v2 z = buf[m];
      const float w = tb.window[m];
      const float vb = nfb ? qnan : w * (-z.y * sc);
      rowa[m] = nfa ? qnan : w * (z.x * sc);
      if (has_b) rowb[m] = vb;
    }
  }
}

__global__ __launch_bounds__(256) void k_istft_ola(const float* __restrict__ rows, const IstftClip* __restrict__ clips, int n_fft,
                                                   int hop, int shift, StftTabs tb, float* __restrict__ out) {
#pragma clang fp contract(off)
  const IstftClip c = clips[blockIdx.y];
  const int64_t full = (int64_t)n_fft + (int64_t)hop * (c.n_frames - 1);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int64_t i = (int64_t)blockIdx.x * 1024 + k * 256 + threadIdx.x;
    if (i >= c.n_out) break;
    const int64_t m = i + shift;
    float acc = 0.f, wss = 0.f;
    if (m < full) {
      const int64_t tlo = m - n_fft + 1 <= 0 ? 0 : (m - n_fft + hop) / hop;
      const int64_t thi = std::min<int64_t>(m / hop, c.n_frames - 1);
      for (int64_t t = tlo; t <= thi; ++t) {
        const int j = (int)(m - t * hop);                        // 0 <= j < n_fft by tlo and thi
        acc += rows[(c.row_base + t) * n_fft + j];
        const float w = tb.window[j];
        wss += w * w;
      }
    }
    out[c.out_off + i] = wss > FLT_MIN ? acc / wss : acc;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
template <int NFFT>
static void launch_stft_kind(hipStream_t s, const afx_stft_opts& o, dim3 grid, const float* y, const StftClip* clips,
                             const uint32_t* bad, int n, int64_t n_units, StftTabs tb, void* out) {
  const int shift = o.center ? NFFT / 2 : 0, reflect = o.center && o.pad_mode == AFX_PAD_REFLECT;
  if (o.out_kind == AFX_STFT_MAG)
    hipLaunchKernelGGL((k_stft_frames<NFFT, AFX_STFT_MAG>), grid, dim3(256), 0, s, y, clips, bad, n, n_units, o.hop, shift, reflect, tb, out);
  else if (o.out_kind == AFX_STFT_POWER)
    hipLaunchKernelGGL((k_stft_frames<NFFT, AFX_STFT_POWER>), grid, dim3(256), 0, s, y, clips, bad, n, n_units, o.hop, shift, reflect, tb, out);
  else
    hipLaunchKernelGGL((k_stft_frames<NFFT, AFX_STFT_COMPLEX>), grid, dim3(256), 0, s, y, clips, bad, n, n_units, o.hop, shift, reflect, tb, out);
}

hipError_t launch_stft_frames(hipStream_t s, const afx_stft_opts& o, const float* y, const StftClip* clips, const uint32_t* bad,
                              int n, int64_t n_units, StftTabs tb, void* out) {
  if (n_units <= 0) return hipSuccess;
  const dim3 grid((unsigned)((n_units + 3) / 4));
  if (o.n_fft == 1024) launch_stft_kind<1024>(s, o, grid, y, clips, bad, n, n_units, tb, out);
  else launch_stft_kind<2048>(s, o, grid, y, clips, bad, n, n_units, tb, out);
  return hipGetLastError();
}

hipError_t launch_istft_frames(hipStream_t s, int n_fft, const float2* spec, const IstftClip* clips, int n, int64_t n_units,
                               StftTabs tb, float* rows) {
  if (n_units <= 0) return hipSuccess;
  const dim3 grid((unsigned)((n_units + 3) / 4));
  if (n_fft == 1024) hipLaunchKernelGGL(k_istft_frames<1024>, grid, dim3(256), 0, s, (const v2*)spec, clips, n, n_units, tb, rows);
  else hipLaunchKernelGGL(k_istft_frames<2048>, grid, dim3(256), 0, s, (const v2*)spec, clips, n, n_units, tb, rows);
  return hipGetLastError();
}

hipError_t launch_istft_ola(hipStream_t s, const afx_stft_opts& o, const float* rows, const IstftClip* clips, int n,
                            int64_t max_out, StftTabs tb, float* out) {
  if (n <= 0 || max_out <= 0) return hipSuccess;
  const dim3 grid((unsigned)((max_out + 1023) / 1024), (unsigned)n);
  hipLaunchKernelGGL(k_istft_ola, grid, dim3(256), 0, s, rows, clips, o.n_fft, o.hop, o.center ? o.n_fft / 2 : 0, tb, out);
  return hipGetLastError();
}

}  // namespace afx
