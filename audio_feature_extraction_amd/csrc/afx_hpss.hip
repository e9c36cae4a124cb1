// Harmonic-percussive separation: librosa.effects.hpss / harmonic / percussive at librosa 0.11's defaults (kernel_size 31,
// power 2, margin 1) on the 2048 / 512 periodic-Hann STFT, centred with zero padding.  Five kernels on one stream:
//   k_hpss_prep   the chunk's clips as float32 (S16 / pre-emphasis applied), one NaN / inf flag per clip
//   k_hpss_stft   one wave per frame: window, 1024-point complex FFT (radix-4 Stockham in LDS), real-FFT split
//                 (its power-output instantiation is the front end of afx_chroma.hip)
//   k_hpss_mask   64 x 64 cells per workgroup: |X| with a 15-cell halo in LDS, the two medians of 31 as sorted sliding
//                 windows per lane, the soft masks, Yh = X mh (and Yp = X mp)
//   k_hpss_irfft  one wave per frame, in place: irfft x window
//   k_hpss_ola    overlap-add as a gather (each sample reads its <= 4 frames, no atomics), window-sum-square
//                 normalisation, cut to length
//   k_hpss_stats  per clip, float64 in a fixed order: sum h^2, sum y^2, mean / std of h's spectral centroid frames
// The centroid frames themselves come from the existing k_frames3s<DESC> run on the device-resident h (afx_api.cpp).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cstdint>

#include "afx.h"
#include "afx_hpss.h"
#include "afx_hpss_dev.h"

namespace afx {

namespace {

constexpr int kSP = 95;                    // LDS pitch of the |X| tile (94 x 94 cells; odd: the transposed walk is conflict-free)
constexpr int kHP = 64;                    // LDS pitch of the harmonic-median tile

// |x| as one fixed sequence of roundings (the tile load and the mask stage must agree bit for bit)
__device__ __forceinline__ float hp_abs(v2 x) {
#pragma clang fp contract(off)
  const float a = x.x * x.x;
  const float b = x.y * x.y;
  return sqrtf(a + b);
}

// scipy.ndimage 'reflect' (d c b a | a b c d | d c b a), repeated with period 2n when the window is longer than the row
__device__ __forceinline__ int hp_refl(int i, int n) {
  const int p = 2 * n;
  int m = i % p;
  if (m < 0) m += p;
  return m < n ? m : p - 1 - m;
}

// librosa.util.softmask(H, P, power=2, split_zeros=True) and softmask(P, H, ...), in librosa's float32 order
__device__ __forceinline__ void hp_softmask(float hm, float pm, float& mh, float& mp) {
#pragma clang fp contract(off)
  const float z = hm > pm ? hm : pm;
  if (z < FLT_MIN) { mh = 0.5f; mp = 0.5f; return; }
  float a = hm / z, b = pm / z;
  a = a * a; b = b * b;
  mh = a / (a + b);
  mp = b / (b + a);
}

// 16 consecutive medians of 31: out[o] = median(src[(o + j) * ss], j < 31).  The window is kept sorted in 31 registers;
// a step deletes the leaving value (30 compares + 30 selects: everything from its first occurrence on shifts down) and
// inserts the arriving one (31 v_med3_f32: slot k becomes med3(a[k-1], v, a[k]) with a[-1] = -inf, a[30] = +inf).
template <int DS>
__device__ __forceinline__ void hp_median16(const float* src, int ss, float* out) {
  float a[31];
#pragma unroll
  for (int k = 0; k < 31; ++k) a[k] = INFINITY;
#pragma unroll
  for (int j = 0; j < 31; ++j) {              // insertion sort of the first window: value j touches slots 0 .. j
    const float v = src[j * ss];
    float prev = -INFINITY;
#pragma unroll
    for (int k = 0; k <= j; ++k) { const float cur = a[k]; a[k] = __builtin_amdgcn_fmed3f(prev, v, cur); prev = cur; }
  }
  out[0] = a[15];
#pragma unroll
  for (int o = 1; o < 16; ++o) {
    const float old = src[(o - 1) * ss], v = src[(o + 30) * ss];
#pragma unroll
    for (int k = 0; k < 30; ++k) a[k] = a[k] < old ? a[k] : a[k + 1];
    a[30] = INFINITY;
    float prev = -INFINITY;
#pragma unroll
    for (int k = 0; k < 31; ++k) { const float cur = a[k]; a[k] = __builtin_amdgcn_fmed3f(prev, v, cur); prev = cur; }
    out[o * DS] = a[15];
  }
}

}  // namespace

__global__ __launch_bounds__(256) void k_hpss_prep(const void* __restrict__ in, int fmt, int flags, float b1,
                                                   const HpssClip* __restrict__ clips, float* __restrict__ y,
                                                   uint32_t* __restrict__ bad) {
  const HpssClip c = clips[blockIdx.y];
  const bool pre = (flags & AFX_FLAG_PREEMPH) != 0;
  bool nf = false;
  for (int64_t i0 = (int64_t)blockIdx.x * 1024; i0 < c.len; i0 += (int64_t)gridDim.x * 1024) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t i = i0 + u * 256 + threadIdx.x;
      if (i >= c.len) break;
      const float v = ld_sample(in, fmt, c.in_off + i);
      nf |= !isfinite(v);
      float o = v;
      if (pre) {
        if (i == 0) o = c.len > 1 ? preemph0(v, ld_sample(in, fmt, c.in_off + 1)) : v;
        else o = preemph1(v, ld_sample(in, fmt, c.in_off + i - 1), b1);
      }
      y[c.y_off + i] = o;
    }
  }
  if (nf) atomicOr(&bad[blockIdx.y], 1u);
}

// POW: |X|^2 as float32 rows of kHpssPowPitch (the pad behind bin 1024 zeroed) instead of the complex rows
template <bool POW>
__global__ __launch_bounds__(256) void k_hpss_stft(const float* __restrict__ y, const HpssClip* __restrict__ clips,
                                                   const uint32_t* __restrict__ bad, int n, int64_t n_frames, HpssTabs tb,
                                                   void* __restrict__ out) {
  __shared__ v2 lds[4][1024];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t g = (int64_t)blockIdx.x * 4 + wave;
  const bool live = g < n_frames;
  const int64_t gg = live ? g : n_frames - 1;
  const int ci = hp_find(n, gg, [&](int i) { return clips[i].frame_base; });
  const HpssClip c = clips[ci];
  const bool zero = !live || bad[ci] != 0;
  const int64_t s0 = (gg - c.frame_base) * 512 - 1024;          // clip sample of frame sample 0
  v2* buf = lds[wave];
#pragma unroll 4
  for (int q = 0; q < 16; ++q) {
    const int m = lane + 64 * q;
    const int64_t i0 = s0 + 2 * m, i1 = i0 + 1;
    const float a = (!zero && i0 >= 0 && i0 < c.len) ? y[c.y_off + i0] : 0.f;
    const float b = (!zero && i1 >= 0 && i1 < c.len) ? y[c.y_off + i1] : 0.f;
    buf[m] = v2{tb.window[2 * m] * a, tb.window[2 * m + 1] * b};
  }
  hp_fft1024(buf, (const v2*)tb.w1024, lane);
  // real-FFT split: hp_split's expression written out (a call changes how the compiler packs it, not what it computes;
  // written out, the kernel's instructions are the ones it has always had)
  const v2* W = (const v2*)tb.w2048;
  v2* row = (v2*)out + gg * kHpssPitch;
  float* prow = (float*)out + gg * kHpssPowPitch;
#pragma unroll 4
  for (int q = 0; q < 16; ++q) {
    const int k = lane + 64 * q;
    const v2 zk = buf[k], zn = buf[(1024 - k) & 1023];
    const v2 A = v2{zk.x + zn.x, zk.y - zn.y} * 0.5f;
    const v2 B = v2{zk.x - zn.x, zk.y + zn.y} * 0.5f;
    const v2 wb = hp_cmul(W[k], B);
    v2 xk = v2{A.x + wb.y, A.y - wb.x};
    if (zero) xk = v2{0.f, 0.f};
    if (POW) { if (live) prow[k] = xk.x * xk.x + xk.y * xk.y; }
    else if (live) row[k] = xk;
  }
  if (POW) {
    if (live && lane < kHpssPowPitch - 1024) {
      const v2 z0 = buf[0];
      const float ny = z0.x - z0.y;
      prow[1024 + lane] = (zero || lane > 0) ? 0.f : ny * ny;
    }
  } else if (live && lane == 0) {
    const v2 z0 = buf[0];
    row[1024] = zero ? v2{0.f, 0.f} : v2{z0.x - z0.y, 0.f};
  }
}

__global__ __launch_bounds__(256) void k_hpss_mask(const v2* __restrict__ X, const HpssClip* __restrict__ clips, int n,
                                                   v2* __restrict__ Yh, v2* __restrict__ Yp, float* __restrict__ spec) {
  __shared__ float S[94 * kSP];            // |X| of frames t0 - 15 .. t0 + 78, bins b0 - 15 .. b0 + 78 (reflected)
  __shared__ float Hs[64 * kHP];           // harmonic medians; then the percussive ones in S's place
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int ci = hp_find(n, blockIdx.y, [&](int i) { return (int64_t)clips[i].tile_base; });
  const HpssClip c = clips[ci];
  const int T = c.T, t0 = ((int)blockIdx.y - c.tile_base) * kHpssTile, b0 = (int)blockIdx.x * kHpssTile;
  const v2* Xc = X + c.frame_base * kHpssPitch;
  for (int i = tid; i < 94 * 94; i += 256) {
    const int r = i / 94, q = i - r * 94;
    const int t = hp_refl(t0 - kHpssHalo + r, T), b = hp_refl(b0 - kHpssHalo + q, kHpssBins);
    S[r * kSP + q] = hp_abs(Xc[(int64_t)t * kHpssPitch + b]);
  }
  __syncthreads();
  // Hm = median_filter(S, size=(1, 31)) along time: wave = 16 frames, lane = bin
  hp_median16<kHP>(&S[(16 * wave) * kSP + lane + kHpssHalo], kSP, &Hs[(16 * wave) * kHP + lane]);
  // Pm = median_filter(S, size=(31, 1)) along frequency: wave = 16 bins, lane = frame
  float pm[16];
  hp_median16<1>(&S[(lane + kHpssHalo) * kSP + 16 * wave], 1, pm);
  __syncthreads();
  float* Ps = S;                           // 64 x 65
#pragma unroll
  for (int o = 0; o < 16; ++o) Ps[lane * 65 + 16 * wave + o] = pm[o];
  __syncthreads();
  float* sp = spec ? spec + c.spec_off : nullptr;
  for (int i = tid; i < 64 * 64; i += 256) {
    const int tl = i >> 6, bl = i & 63, t = t0 + tl, b = b0 + bl;
    if (t >= T || b >= kHpssBins) continue;
    const float hm = Hs[tl * kHP + bl], pmv = Ps[tl * 65 + bl];
    float mh, mp;
    hp_softmask(hm, pmv, mh, mp);
    const int64_t at = (c.frame_base + t) * kHpssPitch + b;
    const v2 x = X[at];
    Yh[at] = x * mh;
    if (Yp) Yp[at] = x * mp;
    if (sp) {
      sp[(int64_t)b * T + t] = hp_abs(x);
      sp[(int64_t)(kHpssBins + b) * T + t] = hm;
      sp[(int64_t)(2 * kHpssBins + b) * T + t] = pmv;
    }
  }
}

__global__ __launch_bounds__(256) void k_hpss_irfft(v2* __restrict__ Yh, v2* __restrict__ Yp, int64_t n_frames, HpssTabs tb) {
  __shared__ v2 lds[4][1024];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t g = (int64_t)blockIdx.x * 4 + wave;
  const bool live = g < n_frames;
  v2* row = (blockIdx.y ? Yp : Yh) + (live ? g : 0) * kHpssPitch;
  v2* buf = lds[wave];
  const v2* W = (const v2*)tb.w2048;
  // conj Z' of hp_merge; the imaginary parts of X[0] and X[1024] are ignored (numpy's irfft)
#pragma unroll 4
  for (int q = 0; q < 16; ++q) {
    const int k = lane + 64 * q;
    v2 zc = v2{0.f, 0.f};
    if (live) {
      v2 xk = row[k], xn = row[1024 - k];
      if (k == 0) { xk.y = 0.f; xn.y = 0.f; }
      zc = hp_merge(xk, xn, W[k]);
    }
    buf[k] = zc;
  }
  hp_fft1024(buf, (const v2*)tb.w1024, lane);
  if (!live) return;
  const float sc = 1.0f / 2048.0f;
#pragma unroll 4
  for (int q = 0; q < 16; ++q) {
    const int m = lane + 64 * q;
    const v2 z = buf[m];
    row[m] = v2{tb.window[2 * m] * (z.x * sc), tb.window[2 * m + 1] * (-z.y * sc)};
  }
}

__global__ __launch_bounds__(256) void k_hpss_ola(const v2* __restrict__ Yh, const v2* __restrict__ Yp,
                                                  const HpssClip* __restrict__ clips, HpssTabs tb, float* __restrict__ h,
                                                  float* __restrict__ p) {
  const HpssClip c = clips[blockIdx.y];
  const float* src = (const float*)(blockIdx.z ? Yp : Yh) + c.frame_base * 2 * kHpssPitch;
  float* dst = (blockIdx.z ? p : h) + c.y_off;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int64_t i = (int64_t)blockIdx.x * 1024 + u * 256 + threadIdx.x;
    if (i >= c.len) break;
    const int64_t m = i + 1024;                                  // sample of the centred (padded) signal
    const int64_t tlo = m >= 2048 ? (m - 2048) / 512 + 1 : 0;
    const int64_t thi = (m / 512) < (int64_t)(c.T - 1) ? m / 512 : (int64_t)(c.T - 1);
    float acc = 0.f, wss = 0.f;
    for (int64_t t = tlo; t <= thi; ++t) {                       // frames in increasing order, as librosa adds them
      const int j = (int)(m - 512 * t);
      acc += src[t * 2 * kHpssPitch + j];
      const float w = tb.window[j];
      wss += w * w;
    }
    if (wss > FLT_MIN) acc /= wss;
    dst[i] = acc;
  }
}

__device__ __forceinline__ double hp_block_sum(double v, double* red) {
  red[threadIdx.x] = v;
  __syncthreads();
#pragma unroll
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}

__global__ __launch_bounds__(256) void k_hpss_stats(const float* __restrict__ y, const float* __restrict__ h,
                                                    const HpssClip* __restrict__ clips, const float* __restrict__ desc,
                                                    const int64_t* __restrict__ desc_off, double* __restrict__ stats) {
  __shared__ double red[256];
  const HpssClip c = clips[blockIdx.x];
  double sh = 0.0, sy = 0.0;
  for (int64_t i = threadIdx.x; i < c.len; i += 256) {
    const double a = h[c.y_off + i], b = y[c.y_off + i];
    sh += a * a; sy += b * b;
  }
  sh = hp_block_sum(sh, red);
  sy = hp_block_sum(sy, red);
  const float* d = desc + desc_off[blockIdx.x];
  double sc = 0.0;
  for (int t = threadIdx.x; t < c.T; t += 256) sc += (double)d[(int64_t)t * 17];
  const double mean = hp_block_sum(sc, red) / c.T;
  double sv = 0.0;
  for (int t = threadIdx.x; t < c.T; t += 256) { const double e = (double)d[(int64_t)t * 17] - mean; sv += e * e; }
  const double var = hp_block_sum(sv, red) / c.T;
  if (threadIdx.x == 0) {
    double* o = stats + 4 * (int64_t)blockIdx.x;
    o[0] = sh; o[1] = sy; o[2] = mean; o[3] = sqrt(var);
  }
}

// ---------------------------------------------------------------------------------------------------------------------
hipError_t launch_hpss_prep(hipStream_t s, const void* in, int fmt, int flags, float preemph_b1, const HpssClip* clips,
                            int n, int64_t max_len, float* y, uint32_t* bad) {
  const int gx = (int)std::min<int64_t>(std::max<int64_t>((max_len + 1023) / 1024, 1), 1024);
  hipLaunchKernelGGL(k_hpss_prep, dim3(gx, n), dim3(256), 0, s, in, fmt, flags, preemph_b1, clips, y, bad);
  return hipGetLastError();
}

hipError_t launch_hpss_stft(hipStream_t s, const float* y, const HpssClip* clips, const uint32_t* bad, int n,
                            int64_t n_frames, HpssTabs tb, float2* X) {
  hipLaunchKernelGGL(k_hpss_stft<false>, dim3((unsigned)((n_frames + 3) / 4)), dim3(256), 0, s, y, clips, bad, n, n_frames,
                     tb, (void*)X);
  return hipGetLastError();
}

hipError_t launch_hpss_stft_power(hipStream_t s, const float* y, const HpssClip* clips, const uint32_t* bad, int n,
                                  int64_t n_frames, HpssTabs tb, float* S) {
  hipLaunchKernelGGL(k_hpss_stft<true>, dim3((unsigned)((n_frames + 3) / 4)), dim3(256), 0, s, y, clips, bad, n, n_frames,
                     tb, (void*)S);
  return hipGetLastError();
}

hipError_t launch_hpss_mask(hipStream_t s, const float2* X, const HpssClip* clips, int n, int n_tiles, float2* Yh,
                            float2* Yp, float* spec) {
  hipLaunchKernelGGL(k_hpss_mask, dim3(kHpssBinTiles, n_tiles), dim3(256), 0, s, (const v2*)X, clips, n, (v2*)Yh, (v2*)Yp,
                     spec);
  return hipGetLastError();
}

hipError_t launch_hpss_irfft(hipStream_t s, float2* Yh, float2* Yp, int64_t n_frames, HpssTabs tb) {
  hipLaunchKernelGGL(k_hpss_irfft, dim3((unsigned)((n_frames + 3) / 4), Yp ? 2 : 1), dim3(256), 0, s, (v2*)Yh, (v2*)Yp,
                     n_frames, tb);
  return hipGetLastError();
}

hipError_t launch_hpss_ola(hipStream_t s, const float2* Yh, const float2* Yp, const HpssClip* clips, int n, int64_t max_len,
                           HpssTabs tb, float* h, float* p) {
  const unsigned gx = (unsigned)std::max<int64_t>((max_len + 1023) / 1024, 1);
  hipLaunchKernelGGL(k_hpss_ola, dim3(gx, n, Yp ? 2 : 1), dim3(256), 0, s, (const v2*)Yh, (const v2*)Yp, clips, tb, h, p);
  return hipGetLastError();
}

hipError_t launch_hpss_stats(hipStream_t s, const float* y, const float* h, const HpssClip* clips, int n,
                             const float* desc, const int64_t* desc_off, double* stats) {
  hipLaunchKernelGGL(k_hpss_stats, dim3(n), dim3(256), 0, s, y, h, clips, desc, desc_off, stats);
  return hipGetLastError();
}

}  // namespace afx
