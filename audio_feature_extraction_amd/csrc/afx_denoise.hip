// STFT-domain noise reduction on the 2048 / 512 periodic-Hann centred STFT (afx_hpss_dev.h): spectral subtraction, the
// Wiener filter, and the aligner's preprocess (RMS gain, subtraction of the whole profile, energy VAD).  Frames of a clip
// are coupled only through the clip's noise profile, so a frame's spectrum never leaves its wave's LDS image:
//   k_dn_gain     per clip: sum y^2 in float64 (fixed order), the gain to RMS 0.1 as one float32
//   k_dn_profile  per clip: the first n frames through window -> FFT -> split, |X| or |X|^2 summed in increasing t
//   k_dn_frames   one wave per frame: window, FFT, split, gain, merge, FFT of the conjugate, x window / 2048; the 2048
//                 time samples go out as the rows k_hpss_ola reads
//   k_dn_vad_e    one wave per VAD frame: its RMS over the zero-padded denoised signal
//   k_dn_vad_thr  per clip: the mean of the energies in a fixed order, the threshold, the frames above it
//   k_dn_finish   in place: the VAD's copy windows as a gather, zeros behind L' = 512 (len / 512) and for a bad clip
// The overlap-add between k_dn_frames and the VAD is launch_hpss_ola.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>

#include "afx.h"
#include "afx_denoise.h"
#include "afx_hpss_dev.h"

namespace afx {

namespace {

// sum of a block's 256 values in a fixed order (k_hpss_stats' tree)
__device__ __forceinline__ double dn_block_sum(double v, double* red) {
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

// |x|^2 and |x| as one fixed sequence of roundings (the profile and the gain must agree on what a zero is)
__device__ __forceinline__ float dn_pow(v2 x) {
#pragma clang fp contract(off)
  const float a = x.x * x.x;
  const float b = x.y * x.y;
  return a + b;
}
__device__ __forceinline__ float dn_abs(v2 x) { return sqrtf(dn_pow(x)); }

// Y = X max(|X| - beta N, 0) / |X|, 0 where |X| = 0 (the reference's angle / exp have magnitude 0 there)
__device__ __forceinline__ v2 dn_specsub(v2 x, float noise, float beta) {
#pragma clang fp contract(off)
  const float m = dn_abs(x);
  if (!(m > 0.f)) return v2{0.f, 0.f};
  const float t = beta * noise;
  const float c = fmaxf(m - t, 0.f);
  return x * (c / m);
}

// Y = X P / (P + Np + eps), eps = 2^-52 added in float32: P = Np = 0 gives 0
__device__ __forceinline__ v2 dn_wiener(v2 x, float noise) {
#pragma clang fp contract(off)
  const float p = dn_pow(x);
  const float den = (p + noise) + 0x1p-52f;
  return x * (p / den);
}

// the windowed frame whose sample 0 is clip sample s0, scaled by g, as 1024 float2 in buf
__device__ __forceinline__ void dn_load(v2* buf, const float* __restrict__ y, const HpssClip& c, int64_t s0, bool zero, float g,
                                        const float* __restrict__ window, int lane) {
#pragma unroll 4
  for (int q = 0; q < 16; ++q) {
    const int m = lane + 64 * q;
    const int64_t i0 = s0 + 2 * m, i1 = i0 + 1;
    const float a = (!zero && i0 >= 0 && i0 < c.len) ? y[c.y_off + i0] * g : 0.f;
    const float b = (!zero && i1 >= 0 && i1 < c.len) ? y[c.y_off + i1] * g : 0.f;
    buf[m] = v2{window[2 * m] * a, window[2 * m + 1] * b};
  }
}

}  // namespace

__global__ __launch_bounds__(256) void k_dn_gain(const float* __restrict__ y, const HpssClip* __restrict__ clips, int rms_gain,
                                                 double* __restrict__ info) {
  __shared__ double red[256];
  const HpssClip c = clips[blockIdx.x];
  double g = 1.0;
  if (rms_gain) {
    double sy = 0.0;
    for (int64_t i = threadIdx.x; i < c.len; i += 256) { const double a = y[c.y_off + i]; sy += a * a; }
    sy = dn_block_sum(sy, red);
    g = (double)(float)(0.1 / (sqrt(sy / (double)c.len) + 1e-6));
  }
  if (threadIdx.x == 0) {
    double* o = info + kDnInfo * (int64_t)blockIdx.x;
    o[0] = g; o[1] = NAN; o[2] = 0.0; o[3] = 0.0;
  }
}

// One workgroup per clip, a wave per frame, four frames a round.  A round leaves its four magnitude rows in LDS and every
// thread adds them to its bins in the order of the frames, so the sum runs over t = 0, 1, 2, .. whatever the launch is.
template <bool POW>
__global__ __launch_bounds__(256) void k_dn_profile(const float* __restrict__ y, const HpssClip* __restrict__ clips,
                                                    const uint32_t* __restrict__ bad, int noise_frames,
                                                    const double* __restrict__ info, HpssTabs tb, float* __restrict__ prof) {
  __shared__ v2 lds[4][1024];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const HpssClip c = clips[blockIdx.x];
  const bool dead = bad[blockIdx.x] != 0;
  const float g = dead ? 0.f : (float)info[kDnInfo * (int64_t)blockIdx.x];
  const int n = c.T < noise_frames ? c.T : noise_frames;
  const v2* W = (const v2*)tb.w2048;
  v2* buf = lds[wave];
  float* mag = (float*)buf;                                    // 1025 floats of the wave's own image
  float acc[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
  for (int t0 = 0; t0 < n; t0 += 4) {                          // block-uniform: every wave runs every round
    const int t = t0 + wave;
    const bool zero = dead || t >= n;
    dn_load(buf, y, c, (int64_t)t * 512 - 1024, zero, g, tb.window, lane);
    hp_fft1024(buf, (const v2*)tb.w1024, lane);
    // a lane takes the pairs (k, 1024 - k): both bins come from Z[k] and Z[1024 - k], which no other lane touches
    float mk[8], mn[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int k = lane + 64 * q;
      const v2 zk = buf[k], zn = buf[(1024 - k) & 1023];
      const v2 xk = hp_split(zk, zn, W[k]);
      const v2 xn = k ? hp_split(zn, zk, W[(1024 - k) & 1023]) : v2{zk.x - zk.y, 0.f};
      mk[q] = POW ? dn_pow(xk) : dn_abs(xk);
      mn[q] = POW ? dn_pow(xn) : dn_abs(xn);
    }
    const v2 zm = buf[512];
    const v2 xm = hp_split(zm, zm, W[512]);
    const float mm = POW ? dn_pow(xm) : dn_abs(xm);
    // the wave's image is read by this wave alone until the barrier, so the magnitudes may overwrite it after the reads
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int q = 0; q < 8; ++q) { const int k = lane + 64 * q; mag[k] = mk[q]; mag[1024 - k] = mn[q]; }
    if (lane == 0) mag[512] = mm;
    __syncthreads();
    const int live = n - t0 < 4 ? n - t0 : 4;
    for (int w = 0; w < live; ++w) {
      const float* mw = (const float*)lds[w];
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] += mw[threadIdx.x + 256 * j];
      if (threadIdx.x == 0) acc[4] += mw[1024];
    }
    __syncthreads();
  }
  float* row = prof + (int64_t)blockIdx.x * kDnProfPitch;
  const float inv = (float)n;
#pragma unroll
  for (int j = 0; j < 4; ++j) row[threadIdx.x + 256 * j] = dead ? 0.f : acc[j] / inv;
  if (threadIdx.x == 0) row[1024] = dead ? 0.f : acc[4] / inv;
  if (threadIdx.x >= 1 && threadIdx.x < kDnProfPitch - 1024) row[1024 + threadIdx.x] = 0.f;
}

template <bool WIENER>
__global__ __launch_bounds__(256) void k_dn_frames(const float* __restrict__ y, const HpssClip* __restrict__ clips,
                                                   const uint32_t* __restrict__ bad, int n, int64_t n_frames, float beta,
                                                   const double* __restrict__ info, const float* __restrict__ prof, HpssTabs tb,
                                                   v2* __restrict__ rows) {
  __shared__ v2 lds[4][1024];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t g = (int64_t)blockIdx.x * 4 + wave;
  const bool live = g < n_frames;
  const int64_t gg = live ? g : n_frames - 1;
  const int ci = hp_find(n, gg, [&](int i) { return clips[i].frame_base; });
  const HpssClip c = clips[ci];
  const bool zero = !live || bad[ci] != 0;
  const float gain = zero ? 0.f : (float)info[kDnInfo * (int64_t)ci];
  v2* buf = lds[wave];
  dn_load(buf, y, c, (gg - c.frame_base) * 512 - 1024, zero, gain, tb.window, lane);
  hp_fft1024(buf, (const v2*)tb.w1024, lane);
  const v2* W = (const v2*)tb.w2048;
  const float* N = prof + (int64_t)ci * kDnProfPitch;
  auto apply = [&](v2 x, float nz) { return WIENER ? dn_wiener(x, nz) : dn_specsub(x, nz, beta); };
  // split, gain and merge of the pair (k, 1024 - k) in place: X[k] and X[1024 - k] come from Z[k] and Z[1024 - k], and so
  // do Z'[k] and Z'[1024 - k] from Y[k] and Y[1024 - k]; no other lane touches either slot
#pragma unroll 4
  for (int q = 0; q < 8; ++q) {
    const int k = lane + 64 * q;
    const v2 zk = buf[k], zn = buf[(1024 - k) & 1023];
    const v2 xk = hp_split(zk, zn, W[k]);
    const v2 xn = k ? hp_split(zn, zk, W[(1024 - k) & 1023]) : v2{zk.x - zk.y, 0.f};
    v2 yk = apply(xk, N[k]), yn = apply(xn, N[1024 - k]);
    if (k == 0) { yk.y = 0.f; yn.y = 0.f; }                   // numpy's irfft ignores them
    buf[k] = hp_merge(yk, yn, W[k]);
    if (k) buf[1024 - k] = hp_merge(yn, yk, W[(1024 - k) & 1023]);
  }
  if (lane == 0) {
    const v2 zm = buf[512];
    const v2 ym = apply(hp_split(zm, zm, W[512]), N[512]);
    buf[512] = hp_merge(ym, ym, W[512]);
  }
  hp_fft1024(buf, (const v2*)tb.w1024, lane);
  if (!live) return;
  const float sc = 1.0f / 2048.0f;
  v2* row = rows + gg * kHpssPitch;
#pragma unroll 4
  for (int q = 0; q < 16; ++q) {
    const int m = lane + 64 * q;
    const v2 z = buf[m];
    row[m] = zero ? v2{0.f, 0.f} : v2{tb.window[2 * m] * (z.x * sc), tb.window[2 * m + 1] * (-z.y * sc)};
  }
}

// e of VAD frame i: sqrt(mean d[j]^2), j in [i hop - fl / 2, .. + fl), zeros outside [0, L').  One wave per frame, float64
// partial sums per lane in the order of j, then the wave's tree.
__global__ __launch_bounds__(256) void k_dn_vad_e(const float* __restrict__ d, const HpssClip* __restrict__ clips,
                                                  const uint32_t* __restrict__ bad, DnVad vad, float* __restrict__ e) {
  const HpssClip c = clips[blockIdx.y];
  const int64_t Lp = 512 * (c.len / 512);
  const int64_t F = bad[blockIdx.y] ? 0 : dn_vad_frames(Lp, vad.fl, vad.hop);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int64_t i = (int64_t)blockIdx.x * 4 + wave; i < F; i += (int64_t)gridDim.x * 4) {   // wave-uniform
    const int64_t j0 = i * vad.hop - vad.fl / 2;
    double s = 0.0;
    for (int u = lane; u < vad.fl; u += 64) {
      const int64_t j = j0 + u;
      const double v = (j >= 0 && j < Lp) ? (double)d[c.y_off + j] : 0.0;
      s += v * v;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) e[c.y_off + blockIdx.y + i] = (float)sqrt(s / (double)vad.fl);
  }
}

__global__ __launch_bounds__(256) void k_dn_vad_thr(const HpssClip* __restrict__ clips, const uint32_t* __restrict__ bad,
                                                    DnVad vad, const float* __restrict__ e, double* __restrict__ info) {
  __shared__ double red[256];
  const HpssClip c = clips[blockIdx.x];
  const int64_t F = bad[blockIdx.x] ? 0 : dn_vad_frames(512 * (c.len / 512), vad.fl, vad.hop);
  if (F == 0) return;                                          // block-uniform: info keeps NaN, 0, 0
  const float* ec = e + c.y_off + blockIdx.x;
  double s = 0.0;
  for (int64_t i = threadIdx.x; i < F; i += 256) s += (double)ec[i];
  s = dn_block_sum(s, red);
  const float thr = (float)(0.5 * (s / (double)F));
  double cnt = 0.0;
  for (int64_t i = threadIdx.x; i < F; i += 256) cnt += ec[i] > thr ? 1.0 : 0.0;
  cnt = dn_block_sum(cnt, red);
  if (threadIdx.x == 0) {
    double* o = info + kDnInfo * (int64_t)blockIdx.x;
    o[1] = (double)thr; o[2] = cnt; o[3] = (double)F;
  }
}

__global__ __launch_bounds__(256) void k_dn_finish(float* __restrict__ d, const HpssClip* __restrict__ clips,
                                                   const uint32_t* __restrict__ bad, DnVad vad, const float* __restrict__ e,
                                                   const double* __restrict__ info) {
  const HpssClip c = clips[blockIdx.y];
  const bool dead = bad[blockIdx.y] != 0;
  const int64_t Lp = 512 * (c.len / 512);
  const int64_t F = vad.fl ? dn_vad_frames(Lp, vad.fl, vad.hop) : 0;
  const float thr = vad.fl ? (float)info[kDnInfo * (int64_t)blockIdx.y + 1] : 0.f;
  const float* ec = e ? e + c.y_off + blockIdx.y : nullptr;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int64_t j = (int64_t)blockIdx.x * 1024 + u * 256 + threadIdx.x;
    if (j >= c.len) break;
    bool keep = !dead && j < Lp;
    if (keep && vad.fl) {
      // the speech frames i with i hop <= j < i hop + fl whose window ends inside the signal
      keep = false;
      const int64_t ihi = j / vad.hop < F - 1 ? j / vad.hop : F - 1;
      for (int64_t i = ihi; i >= 0 && i * vad.hop + vad.fl > j; --i)
        if (i * vad.hop + vad.fl <= Lp && ec[i] > thr) { keep = true; break; }
    }
    if (!keep) d[c.y_off + j] = 0.f;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
hipError_t launch_dn_gain(hipStream_t s, const float* y, const HpssClip* clips, int n, bool rms_gain, double* info) {
  hipLaunchKernelGGL(k_dn_gain, dim3(n), dim3(256), 0, s, y, clips, rms_gain ? 1 : 0, info);
  return hipGetLastError();
}

hipError_t launch_dn_profile(hipStream_t s, const float* y, const HpssClip* clips, const uint32_t* bad, int n, int noise_frames,
                             bool power, const double* info, HpssTabs tb, float* prof) {
  if (power) hipLaunchKernelGGL(k_dn_profile<true>, dim3(n), dim3(256), 0, s, y, clips, bad, noise_frames, info, tb, prof);
  else hipLaunchKernelGGL(k_dn_profile<false>, dim3(n), dim3(256), 0, s, y, clips, bad, noise_frames, info, tb, prof);
  return hipGetLastError();
}

hipError_t launch_dn_frames(hipStream_t s, const float* y, const HpssClip* clips, const uint32_t* bad, int n, int64_t n_frames,
                            bool wiener, float beta, const double* info, const float* prof, HpssTabs tb, float2* rows) {
  const dim3 grid((unsigned)((n_frames + 3) / 4));
  if (wiener) hipLaunchKernelGGL(k_dn_frames<true>, grid, dim3(256), 0, s, y, clips, bad, n, n_frames, beta, info, prof, tb, (v2*)rows);
  else hipLaunchKernelGGL(k_dn_frames<false>, grid, dim3(256), 0, s, y, clips, bad, n, n_frames, beta, info, prof, tb, (v2*)rows);
  return hipGetLastError();
}

hipError_t launch_dn_vad(hipStream_t s, const float* d, const HpssClip* clips, const uint32_t* bad, int n, int64_t max_len,
                         DnVad vad, float* e, double* info) {
  const int64_t maxf = std::max<int64_t>(dn_vad_frames(512 * (max_len / 512), vad.fl, vad.hop), 1);
  const unsigned gx = (unsigned)std::min<int64_t>((maxf + 3) / 4, 65535);
  hipLaunchKernelGGL(k_dn_vad_e, dim3(gx, n), dim3(256), 0, s, d, clips, bad, vad, e);
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) return err;
  hipLaunchKernelGGL(k_dn_vad_thr, dim3(n), dim3(256), 0, s, clips, bad, vad, (const float*)e, info);
  return hipGetLastError();
}

hipError_t launch_dn_finish(hipStream_t s, float* d, const HpssClip* clips, const uint32_t* bad, int n, int64_t max_len,
                            DnVad vad, const float* e, const double* info) {
  const unsigned gx = (unsigned)std::max<int64_t>((max_len + 1023) / 1024, 1);
  hipLaunchKernelGGL(k_dn_finish, dim3(gx, n), dim3(256), 0, s, d, clips, bad, vad, e, info);
  return hipGetLastError();
}

}  // namespace afx
