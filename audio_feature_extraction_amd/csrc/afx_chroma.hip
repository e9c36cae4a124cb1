// Chroma, tuning estimate and mel power: librosa.feature.chroma_stft (librosa.estimate_tuning / piptrack when no tuning is
// given) and librosa.feature.melspectrogram at librosa's defaults, on the float32 power rows of k_hpss_stft<true>
// (tests/chroma_ref.py is the spec).  Four kernels on one stream behind HPSS's prep + STFT:
//   k_chroma_peaks    one wave per frame: the frame maximum, piptrack's peak test and parabolic interpolation in its
//                     150 .. 4000 Hz band, the tuning residual's histogram bin -- dense per (frame, band bin)
//   k_chroma_tuning   one workgroup per clip: the exact median of the peak magnitudes (radix select over the float bits,
//                     8 bits a pass, integer LDS atomics), the 100-bin count of the peaks at or above it, its first maximum
//   k_chroma_apply    one wave per 16 frames: the 12 (16) x 1040 filterbank of the clip's tuning times the rows as exact-f32
//                     MFMA, every frame divided by its maximum; the banded mel contraction of the same rows; per-frame sums
//   k_chroma_stats    per clip, float64 in a fixed order: mean / std of the mel and the chroma matrix
// No float atomics anywhere; nothing depends on the order in which waves run.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cstdint>

#include "afx_chroma.h"
#include "afx_wave.h"

namespace afx {

typedef float f32x4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(256) void k_chroma_peaks(const float* __restrict__ S, int64_t n_frames, ChromaBand band,
                                                      float* __restrict__ mag, uint8_t* __restrict__ bin) {
#pragma clang fp contract(off)
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t g = (int64_t)blockIdx.x * 4 + wave;
  if (g >= n_frames) return;
  const float* row = S + g * kHpssPowPitch;
  float m = 0.f;
  for (int i = lane; i < kHpssPowPitch / 4; i += 64) {
    const float4 v = reinterpret_cast<const float4*>(row)[i];
    m = fmaxf(fmaxf(m, fmaxf(v.x, v.y)), fmaxf(v.z, v.w));
  }
  const float thr = 0.1f * wave_max(m);
  for (int j = lane; j < band.nr; j += 64) {
    const int k = band.kmin + j;
    const float lo = row[k - 1], mid = row[k], hi = row[k + 1];
    const float s0 = lo > thr ? lo : 0.f, s1 = mid > thr ? mid : 0.f, s2 = hi > thr ? hi : 0.f;
    float mg = 0.f;
    int bn = 255;
    if (s1 > s0 && s1 >= s2) {
      const float b = (hi - lo) * 0.5f, a = hi + lo - 2.f * mid;
      const float shift = fabsf(b) >= fabsf(a) ? 0.f : -b / a;
      mg = mid + 0.5f * b * shift;
      const float pitch = ((float)k + shift) * band.hz_per_bin;
      float r = 12.f * log2f(pitch / 27.5f);
      r -= floorf(r);
      if (r >= 0.5f) r -= 1.f;
      bn = (int)floorf((r + 0.5f) * 100.f);
      bn = bn < 0 ? 0 : (bn > 99 ? 99 : bn);
    }
    mag[g * band.nr + j] = mg;
    bin[g * band.nr + j] = (uint8_t)bn;
  }
}

// A peak's magnitude is positive (it is at least S[k], which exceeds a tenth of the frame maximum), so the float bits order
// as unsigned integers and 0 marks "no peak".
__global__ __launch_bounds__(1024) void k_chroma_tuning(const HpssClip* __restrict__ clips, ChromaBand band,
                                                        const float* __restrict__ mag, const uint8_t* __restrict__ bin,
                                                        int32_t* __restrict__ slot, int32_t* __restrict__ hist) {
  __shared__ unsigned cnt[256];
  __shared__ unsigned sh_prefix, sh_rank, sh_n, sh_le, sh_gt;
  const int tid = threadIdx.x;
  const HpssClip c = clips[blockIdx.x];
  const int64_t base = c.frame_base * band.nr, N = (int64_t)c.T * band.nr;
  const uint32_t* mg = reinterpret_cast<const uint32_t*>(mag) + base;
  const uint8_t* bn = bin + base;
  int32_t* out = hist + (int64_t)blockIdx.x * kChromaHist;
  unsigned prefix = 0, mask = 0, n = 0;
  for (int pass = 0; pass < 4; ++pass) {                 // the element of rank (n - 1) / 2, one byte of it per pass
    const int sh = 24 - 8 * pass;
    if (tid < 256) cnt[tid] = 0;
    __syncthreads();
    for (int64_t i = tid; i < N; i += 1024) {
      const uint32_t u = mg[i];
      if (u != 0 && (u & mask) == prefix) atomicAdd(&cnt[(u >> sh) & 255], 1u);
    }
    __syncthreads();
    if (tid == 0) {
      unsigned rank;
      if (pass == 0) {
        unsigned tot = 0;
        for (int b = 0; b < 256; ++b) tot += cnt[b];
        sh_n = tot;
        rank = tot ? (tot - 1) / 2 : 0;
      } else {
        rank = sh_rank;
      }
      unsigned cum = 0;
      int b = 0;
      for (; b < 255; ++b) {
        if (cum + cnt[b] > rank) break;
        cum += cnt[b];
      }
      sh_prefix = prefix | ((unsigned)b << sh);
      sh_rank = rank - cum;
    }
    __syncthreads();
    prefix = sh_prefix; n = sh_n;
    mask |= 255u << sh;
    if (n == 0) break;
  }
  if (n == 0) {                                          // no peak: tuning 0.0
    if (tid < kChromaHist) out[tid] = 0;
    if (tid == 0) slot[blockIdx.x] = kChromaGrid / 2;
    return;
  }
  float thr = __uint_as_float(prefix);
  if ((n & 1) == 0) {                                    // even: the mean of ranks n / 2 - 1 (found) and n / 2
    if (tid == 0) { sh_le = 0; sh_gt = 0xffffffffu; }
    __syncthreads();
    unsigned le = 0, gt = 0xffffffffu;
    for (int64_t i = tid; i < N; i += 1024) {
      const uint32_t u = mg[i];
      if (u == 0) continue;
      if (u <= prefix) ++le; else gt = u < gt ? u : gt;
    }
    atomicAdd(&sh_le, le);
    atomicMin(&sh_gt, gt);
    __syncthreads();
    const unsigned upper = sh_le > n / 2 ? prefix : sh_gt;
    thr = (thr + __uint_as_float(upper)) * 0.5f;
  }
  if (tid < 256) cnt[tid] = 0;
  __syncthreads();
  for (int64_t i = tid; i < N; i += 1024) {
    const uint32_t u = mg[i];
    if (u != 0 && __uint_as_float(u) >= thr) atomicAdd(&cnt[bn[i] < kChromaGrid ? bn[i] : kChromaGrid - 1], 1u);
  }
  __syncthreads();
  if (tid < kChromaGrid) out[2 + tid] = (int32_t)cnt[tid];
  if (tid == 0) {
    unsigned kept = 0, best = 0;
    int arg = 0;
    for (int b = 0; b < kChromaGrid; ++b) {
      kept += cnt[b];
      if (cnt[b] > best) { best = cnt[b]; arg = b; }
    }
    out[0] = (int32_t)n; out[1] = (int32_t)kept;
    slot[blockIdx.x] = arg;
  }
}

template <bool MEL>
__global__ __launch_bounds__(256) void k_chroma_apply(const float* __restrict__ S, const HpssClip* __restrict__ clips, int n,
                                                      int n_tiles, const int32_t* __restrict__ slot,
                                                      const float* __restrict__ grid, const float* __restrict__ extra,
                                                      ChromaMel mel, float* __restrict__ chroma_out,
                                                      float* __restrict__ mel_out, double* __restrict__ parts) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int g = (int)blockIdx.x * 4 + wave;
  if (g >= n_tiles) return;
  const int ci = hp_find(n, g, [&](int i) { return (int64_t)clips[i].tile_base; });
  const HpssClip c = clips[ci];
  const int f = lane & 15, q = lane >> 4, t = (g - c.tile_base) * 16 + f;
  const bool valid = t < c.T;
  // a lane past the clip's last frame reads that last frame again (never another clip's rows) and stores nothing
  const float* row = S + (c.frame_base + (valid ? t : c.T - 1)) * kHpssPowPitch + 4 * q;
  const int sl = slot[ci];
  const float* A = (sl < kChromaGrid ? grid + (int64_t)sl * kChromaImg : extra + (int64_t)(sl - kChromaGrid) * kChromaImg) + lane;
  f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 5
  for (int s = 0; s < kChromaSteps; ++s) {
    const float4 x = *reinterpret_cast<const float4*>(row + 16 * s);
    a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(A[(4 * s + 0) * 64], x.x, a0, 0, 0, 0);
    a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(A[(4 * s + 1) * 64], x.y, a1, 0, 0, 0);
    a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(A[(4 * s + 2) * 64], x.z, a0, 0, 0, 0);
    a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(A[(4 * s + 3) * 64], x.w, a1, 0, 0, 0);
  }
  f32x4 ch = a0 + a1;                                    // rows 4 q + {0..3} of frame f; rows 12 .. 15 are zero
  float m = fmaxf(fmaxf(fabsf(ch[0]), fabsf(ch[1])), fmaxf(fabsf(ch[2]), fabsf(ch[3])));
  m = fmaxf(m, __shfl_xor(m, 16));
  m = fmaxf(m, __shfl_xor(m, 32));
  double cs = 0.0, cq = 0.0;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    if (m >= FLT_MIN) ch[r] = ch[r] / m;
    cs += (double)ch[r]; cq += (double)ch[r] * (double)ch[r];
  }
  if (chroma_out && valid && q < 3) {
    float* o = chroma_out + 12 * c.frame_base + (int64_t)(4 * q) * c.T + t;
#pragma unroll
    for (int r = 0; r < 4; ++r) o[(int64_t)r * c.T] = ch[r];
  }
  double ms = 0.0, mq = 0.0;
  if (MEL) {
    float* o = mel_out ? mel_out + (int64_t)mel.n_mels * c.frame_base + t : nullptr;
#pragma unroll
    for (int gi = 0; gi < kChromaMelGroups; ++gi) {
      if (gi >= mel.n_groups) break;
      const float* M = mel.img + (int64_t)mel.off[gi] * 256 + lane;
      f32x4 b0 = {0.f, 0.f, 0.f, 0.f}, b1 = {0.f, 0.f, 0.f, 0.f};
      for (int s = mel.s0[gi]; s < mel.s1[gi]; ++s, M += 256) {
        const float4 x = *reinterpret_cast<const float4*>(row + 16 * s);
        b0 = __builtin_amdgcn_mfma_f32_16x16x4f32(M[0], x.x, b0, 0, 0, 0);
        b1 = __builtin_amdgcn_mfma_f32_16x16x4f32(M[64], x.y, b1, 0, 0, 0);
        b0 = __builtin_amdgcn_mfma_f32_16x16x4f32(M[128], x.z, b0, 0, 0, 0);
        b1 = __builtin_amdgcn_mfma_f32_16x16x4f32(M[192], x.w, b1, 0, 0, 0);
      }
      const f32x4 v = b0 + b1;                           // filters 16 gi + 4 q + {0..3}; those past n_mels are zero
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int k = 16 * gi + 4 * q + r;
        ms += (double)v[r]; mq += (double)v[r] * (double)v[r];
        if (o && valid && k < mel.n_mels) o[(int64_t)k * c.T] = v[r];
      }
    }
  }
  if (parts) {                                           // the frame's four sums: over this lane's rows, then over q
    cs += __shfl_xor(cs, 16); cq += __shfl_xor(cq, 16); ms += __shfl_xor(ms, 16); mq += __shfl_xor(mq, 16);
    cs += __shfl_xor(cs, 32); cq += __shfl_xor(cq, 32); ms += __shfl_xor(ms, 32); mq += __shfl_xor(mq, 32);
    if (valid && q == 0) {
      double* p = parts + 4 * (c.frame_base + t);
      p[0] = cs; p[1] = cq; p[2] = ms; p[3] = mq;
    }
  }
}

__device__ __forceinline__ double ch_block_sum(double v, double* red) {
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

__global__ __launch_bounds__(256) void k_chroma_stats(const HpssClip* __restrict__ clips, int n_mels,
                                                      const double* __restrict__ parts, double* __restrict__ stats) {
  __shared__ double red[256];
  const HpssClip c = clips[blockIdx.x];
  double v[4] = {0.0, 0.0, 0.0, 0.0};
  for (int t = threadIdx.x; t < c.T; t += 256) {
    const double* p = parts + 4 * (c.frame_base + t);
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] += p[k];
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) v[k] = ch_block_sum(v[k], red);
  if (threadIdx.x == 0) {
    const double nc = 12.0 * c.T, nm = (double)n_mels * c.T;
    const double cm = v[0] / nc, mm = v[2] / nm;
    const double cv = v[1] / nc - cm * cm, mv = v[3] / nm - mm * mm;
    double* o = stats + 4 * (int64_t)blockIdx.x;
    o[0] = mm; o[1] = sqrt(mv > 0.0 ? mv : 0.0); o[2] = cm; o[3] = sqrt(cv > 0.0 ? cv : 0.0);
  }
}

// ---------------------------------------------------------------------------------------------------------------------
hipError_t launch_chroma_peaks(hipStream_t s, const float* S, int64_t n_frames, ChromaBand band, float* mag, uint8_t* bin) {
  hipLaunchKernelGGL(k_chroma_peaks, dim3((unsigned)((n_frames + 3) / 4)), dim3(256), 0, s, S, n_frames, band, mag, bin);
  return hipGetLastError();
}

hipError_t launch_chroma_tuning(hipStream_t s, const HpssClip* clips, int n, ChromaBand band, const float* mag,
                                const uint8_t* bin, int32_t* slot, int32_t* hist) {
  hipLaunchKernelGGL(k_chroma_tuning, dim3(n), dim3(1024), 0, s, clips, band, mag, bin, slot, hist);
  return hipGetLastError();
}

hipError_t launch_chroma_apply(hipStream_t s, const float* S, const HpssClip* clips, int n, int n_tiles, const int32_t* slot,
                               const float* grid, const float* extra, ChromaMel mel, bool want_mel, float* chroma_out,
                               float* mel_out, double* parts) {
  const dim3 gr((unsigned)((n_tiles + 3) / 4));
  if (want_mel) hipLaunchKernelGGL(k_chroma_apply<true>, gr, dim3(256), 0, s, S, clips, n, n_tiles, slot, grid, extra, mel, chroma_out, mel_out, parts);
  else hipLaunchKernelGGL(k_chroma_apply<false>, gr, dim3(256), 0, s, S, clips, n, n_tiles, slot, grid, extra, mel, chroma_out, mel_out, parts);
  return hipGetLastError();
}

hipError_t launch_chroma_stats(hipStream_t s, const HpssClip* clips, int n, int n_mels, const double* parts, double* stats) {
  hipLaunchKernelGGL(k_chroma_stats, dim3(n), dim3(256), 0, s, clips, n_mels, parts, stats);
  return hipGetLastError();
}

}  // namespace afx
