// The DCT stage of libafx.so (gfx950): power_to_db's clip-global top_db clamp + ortho DCT-II of the log-mel tiles ->
// MFCC rows, on the matrix pipe as exact-f32 MFMA (reference call site: feature_extractor.py:127, librosa.feature.mfcc).
//   k_dct<NCG>      any n_mels / n_mfcc
//   k_dct16<NCG>    n_mels % 16 == 0, the DCT matrix in registers
//   k_dct16l<NCG>   the same for more than 16 coefficients, the matrix in LDS
// FM: the frame-major spill of the wave-level frame kernels instead of the [mel/4][frame][mel%4] tiles of k_frames.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "afx_device.h"
#include "afx_devenv.h"
#include "afx_wave.h"

namespace afx {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------------------
// k_dct: clamp at (clip max - top_db), ortho DCT-II on the matrix pipe.
// One wave per 16-frame log-mel tile: the tile's [mel][16 frames] layout is exactly the
// MFMA B-operand order, so each k-step is one coalesced 256-byte load.
// ---------------------------------------------------------------------------
template <int NCG, bool FM>
__global__ __launch_bounds__(256) void k_dct(const ClipDesc* __restrict__ clips,
                                             const ClipInfo* __restrict__ info,
                                             const float* __restrict__ dctA, KParams kp,
                                             const float* __restrict__ logmel,
                                             float* __restrict__ mfcc, int spec) {
  const int clip = blockIdx.y;
  const ClipInfo ci = info[clip];
  if (ci.status != AFX_CLIP_OK) return;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int t0 = (blockIdx.x * 4 + wave) * 16;
  if (t0 >= ci.T) return;
  const ClipDesc cd = clips[clip];
  const int M = kp.n_mels, K = kp.n_mfcc, NI = M >> 2;
  const float theta = ord2f(ci.lmax_ord) - kp.top_db;
  const int f = lane & 15, q = lane >> 4;
  // tile layout [mel/4][frame][mel%4]: B[k = q][j = f] of k-step i is at 64 i + 4 f + q (one 256-B row per step)
  // FM (k_frames3's spill): frame-major [frame][mel], B[k = q][j = f] of k-step i is mel 4 i + q of frame t0 + f
  // spec: the spill holds absolute frames (k_frames3 ran before the trim decision); trimmed frame t is frame start / hop + t
  const int g0 = spec ? (int)(ci.start / kp.hop) : 0;
  const float* tile = FM ? logmel + (cd.frame_base + g0 + t0 + f) * (int64_t)M + q
                         : logmel + (cd.frame_base + t0) * (int64_t)M + f * 4 + q;
  f32x4 acc[NCG];
#pragma unroll
  for (int c = 0; c < NCG; ++c) acc[c] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
  for (int i = 0; i < NI; ++i) {
    const float Lc = fmaxf(tile[FM ? i * 4 : i * 64], theta);
#pragma unroll
    for (int c = 0; c < NCG; ++c)
      acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(dctA[((int64_t)c * NI + i) * 64 + lane], Lc, acc[c], 0, 0, 0);
  }
  if (t0 + f < ci.T) {
    float* out = mfcc + cd.frame_base * (int64_t)K + t0 + f;
#pragma unroll
    for (int c = 0; c < NCG; ++c)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int k = c * 16 + q * 4 + r;
        if (k < K) out[(int64_t)k * cd.tpad] = acc[c][r];
      }
  }
}

// k_dct16<NCG>: the same for n_mels % 16 == 0 and n_mfcc <= 16 NCG <= 48 (the reference's 128 / 13).  A wave takes kDctTiles
// tiles; lane (f, q) fetches filters 16 s + 4 q + {0..3} of frame f with one 16-byte load (a wave-load is 1 KB
// contiguous), all loads of its tiles issued before the first use; the DCT matrix sits in registers.
constexpr int kDctTiles = 1;
template <int NCG, bool FM>
__global__ __launch_bounds__(256) void k_dct16(const ClipDesc* __restrict__ clips,
                                               const ClipInfo* __restrict__ info,
                                               const float* __restrict__ dctP, KParams kp,
                                               const float* __restrict__ logmel,
                                               float* __restrict__ mfcc, int spec) {
  const int clip = blockIdx.y;
  const ClipInfo ci = info[clip];
  if (ci.status != AFX_CLIP_OK) return;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int tile0 = (blockIdx.x * 4 + wave) * kDctTiles;
  if (tile0 * 16 >= ci.T) return;
  const ClipDesc cd = clips[clip];
  const int M = kp.n_mels, K = kp.n_mfcc, S = M >> 4;         // S <= 8
  const float theta = ord2f(ci.lmax_ord) - kp.top_db;
  const int f = lane & 15, q = lane >> 4;
  float4 x[kDctTiles][8];
#pragma unroll
  for (int j = 0; j < kDctTiles; ++j) {
    const int t0 = (tile0 + j) * 16;
    // tiles past the clip's last frame are not read (t0 is wave-uniform); [mel/4][frame][mel%4]: quad row 4 s + q
    // FM: frame-major [frame][mel] -- the same four filters 16 s + 4 q + {0..3} of frame f, 16 bytes at mel offset 16 s + 4 q
    const float* tile = FM ? logmel + (cd.frame_base + (spec ? (int)(ci.start / kp.hop) : 0) + t0 + f) * (int64_t)M + q * 4
                           : logmel + (cd.frame_base + t0) * (int64_t)M + (q * 16 + f) * 4;
#pragma unroll
    for (int s = 0; s < 8; ++s)
      x[j][s] = (s < S && t0 < ci.T) ? *reinterpret_cast<const float4*>(tile + s * (FM ? 16 : 256)) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  float a[NCG][8][4];
#pragma unroll
  for (int g = 0; g < NCG; ++g)
#pragma unroll
    for (int s = 0; s < 8; ++s)
#pragma unroll
      for (int c = 0; c < 4; ++c) a[g][s][c] = s < S ? dctP[((g * S + s) * 4 + c) * 64 + lane] : 0.f;
#pragma unroll
  for (int j = 0; j < kDctTiles; ++j) {
    const int t0 = (tile0 + j) * 16;
    if (t0 >= ci.T) break;
    f32x4 acc[NCG][2];
#pragma unroll
    for (int g = 0; g < NCG; ++g) { acc[g][0] = f32x4{0.f, 0.f, 0.f, 0.f}; acc[g][1] = f32x4{0.f, 0.f, 0.f, 0.f}; }
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      if (s < S) {
        const float b0 = fmaxf(x[j][s].x, theta), b1 = fmaxf(x[j][s].y, theta);
        const float b2 = fmaxf(x[j][s].z, theta), b3 = fmaxf(x[j][s].w, theta);
#pragma unroll
        for (int g = 0; g < NCG; ++g) {
          acc[g][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[g][s][0], b0, acc[g][0], 0, 0, 0);
          acc[g][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[g][s][1], b1, acc[g][1], 0, 0, 0);
          acc[g][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[g][s][2], b2, acc[g][0], 0, 0, 0);
          acc[g][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[g][s][3], b3, acc[g][1], 0, 0, 0);
        }
      }
    }
    if (t0 + f < ci.T) {
      float* out = mfcc + cd.frame_base * (int64_t)K + t0 + f;
#pragma unroll
      for (int g = 0; g < NCG; ++g) {
        const f32x4 r4 = acc[g][0] + acc[g][1];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int k = g * 16 + q * 4 + r;
          if (k < K) out[(int64_t)k * cd.tpad] = r4[r];
        }
      }
    }
  }
}

// k_dct16l<NCG>: k_dct16 for more than 16 coefficients (NCG = 2, 3).  There the coefficient images are 64 / 96 registers
// per lane, re-read from memory by every wave for every 16-frame tile (96 loads in front of 96 MFMAs: 0.30 ms for the
// 40 coefficients of the 16 kHz configuration, against 0.13 ms of spill traffic).  Here a workgroup copies the images
// to LDS once (NCG x 8 KB), walks many tiles of its clip, and fetches each MFMA's A operand with one ds_read_b32;
// the next tile's frames are in flight while the current one is multiplied.
template <int NCG, bool FM>
__global__ __launch_bounds__(256) void k_dct16l(const ClipDesc* __restrict__ clips,
                                                const ClipInfo* __restrict__ info,
                                                const float* __restrict__ dctP, KParams kp,
                                                const float* __restrict__ logmel,
                                                float* __restrict__ mfcc, int spec) {
  extern __shared__ float dct_tab[];                     // [(g S + s) 4 + c][64 lanes]
  const int clip = blockIdx.y;
  const ClipInfo ci = info[clip];
  if (ci.status != AFX_CLIP_OK) return;                  // uniform per workgroup
  const int M = kp.n_mels, K = kp.n_mfcc, S = M >> 4;    // S <= 8
  for (int i = threadIdx.x; i < NCG * S * 4 * 64; i += 256) dct_tab[i] = dctP[i];
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const ClipDesc cd = clips[clip];
  const float theta = ord2f(ci.lmax_ord) - kp.top_db;
  const int f = lane & 15, q = lane >> 4;
  const int ntiles = (ci.T + 15) >> 4, tstep = gridDim.x * 4;
  const int g0 = spec ? (int)(ci.start / kp.hop) : 0;
  auto load_tile = [&](int tile, float4 (&x)[8]) {
    const int t0 = tile * 16;
    const float* src = FM ? logmel + (cd.frame_base + g0 + t0 + f) * (int64_t)M + q * 4
                          : logmel + (cd.frame_base + t0) * (int64_t)M + (q * 16 + f) * 4;
#pragma unroll
    for (int s = 0; s < 8; ++s)
      x[s] = (s < S && tile < ntiles) ? *reinterpret_cast<const float4*>(src + s * (FM ? 16 : 256)) : make_float4(0.f, 0.f, 0.f, 0.f);
  };
  float4 xc[8], xn[8];
  int tile = blockIdx.x * 4 + wave;
  load_tile(tile, xc);
  for (; tile < ntiles; tile += tstep) {
    load_tile(tile + tstep, xn);
    f32x4 acc[NCG][2];
#pragma unroll
    for (int g = 0; g < NCG; ++g) { acc[g][0] = f32x4{0.f, 0.f, 0.f, 0.f}; acc[g][1] = f32x4{0.f, 0.f, 0.f, 0.f}; }
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      if (s < S) {
        const float b0 = fmaxf(xc[s].x, theta), b1 = fmaxf(xc[s].y, theta);
        const float b2 = fmaxf(xc[s].z, theta), b3 = fmaxf(xc[s].w, theta);
#pragma unroll
        for (int g = 0; g < NCG; ++g) {
          const float* a = dct_tab + ((g * S + s) * 4) * 64 + lane;
          acc[g][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[0], b0, acc[g][0], 0, 0, 0);
          acc[g][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[64], b1, acc[g][1], 0, 0, 0);
          acc[g][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[128], b2, acc[g][0], 0, 0, 0);
          acc[g][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[192], b3, acc[g][1], 0, 0, 0);
        }
      }
    }
    const int t0 = tile * 16;
    if (t0 + f < ci.T) {
      float* out = mfcc + cd.frame_base * (int64_t)K + t0 + f;
#pragma unroll
      for (int g = 0; g < NCG; ++g) {
        const f32x4 r4 = acc[g][0] + acc[g][1];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int k = g * 16 + q * 4 + r;
          if (k < K) out[(int64_t)k * cd.tpad] = r4[r];
        }
      }
    }
#pragma unroll
    for (int s = 0; s < 8; ++s) xc[s] = xn[s];
  }
}

template <bool FM>
static hipError_t launch_dct_t(hipStream_t s, const ClipDesc* clips, const ClipInfo* info, const DevTables& tb,
                               const KParams& kp, const float* logmel, float* mfcc, int n_clips, int max_tmax, int spec) {
  if (tb.dctP && kp.n_mels % 16 == 0 && kp.n_mels <= 128 && kp.n_mfcc <= 48) {
    dim3 g16(((max_tmax + 15) / 16 + 4 * kDctTiles - 1) / (4 * kDctTiles), n_clips);
    const int ncg = (kp.n_mfcc + 15) / 16;
    if (ncg == 1) hipLaunchKernelGGL((k_dct16<1, FM>), g16, dim3(256), 0, s, clips, info, tb.dctP, kp, logmel, mfcc, spec);
    else {
      // a workgroup per 64 tiles of a clip (16 per wave): the table copy is paid once per 512 KB of frames
      const int tiles = (max_tmax + 15) / 16;
      dim3 gl(std::max(1, (tiles + 63) / 64), n_clips);
      const size_t lds = (size_t)ncg * (kp.n_mels / 16) * 4 * 64 * sizeof(float);
      if (dev_env().no_dct16l) {
        if (ncg == 2) hipLaunchKernelGGL((k_dct16<2, FM>), g16, dim3(256), 0, s, clips, info, tb.dctP, kp, logmel, mfcc, spec);
        else hipLaunchKernelGGL((k_dct16<3, FM>), g16, dim3(256), 0, s, clips, info, tb.dctP, kp, logmel, mfcc, spec);
      } else if (ncg == 2) hipLaunchKernelGGL((k_dct16l<2, FM>), gl, dim3(256), lds, s, clips, info, tb.dctP, kp, logmel, mfcc, spec);
      else hipLaunchKernelGGL((k_dct16l<3, FM>), gl, dim3(256), lds, s, clips, info, tb.dctP, kp, logmel, mfcc, spec);
    }
    return hipGetLastError();
  }
  dim3 grid(((max_tmax + 15) / 16 + 3) / 4, n_clips);
  switch (tb.n_cgroups) {
    case 1: hipLaunchKernelGGL((k_dct<1, FM>), grid, dim3(256), 0, s, clips, info, tb.dctA, kp, logmel, mfcc, spec); break;
    case 2: hipLaunchKernelGGL((k_dct<2, FM>), grid, dim3(256), 0, s, clips, info, tb.dctA, kp, logmel, mfcc, spec); break;
    case 3: hipLaunchKernelGGL((k_dct<3, FM>), grid, dim3(256), 0, s, clips, info, tb.dctA, kp, logmel, mfcc, spec); break;
    case 4: hipLaunchKernelGGL((k_dct<4, FM>), grid, dim3(256), 0, s, clips, info, tb.dctA, kp, logmel, mfcc, spec); break;
    case 5: hipLaunchKernelGGL((k_dct<5, FM>), grid, dim3(256), 0, s, clips, info, tb.dctA, kp, logmel, mfcc, spec); break;
    case 6: hipLaunchKernelGGL((k_dct<6, FM>), grid, dim3(256), 0, s, clips, info, tb.dctA, kp, logmel, mfcc, spec); break;
    case 7: hipLaunchKernelGGL((k_dct<7, FM>), grid, dim3(256), 0, s, clips, info, tb.dctA, kp, logmel, mfcc, spec); break;
    case 8: hipLaunchKernelGGL((k_dct<8, FM>), grid, dim3(256), 0, s, clips, info, tb.dctA, kp, logmel, mfcc, spec); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t launch_dct(hipStream_t s, const ClipDesc* clips, const ClipInfo* info, const DevTables& tb,
                      const KParams& kp, const float* logmel, float* mfcc, int n_clips, int max_tmax, bool frame_major,
                      bool spec) {
  return frame_major ? launch_dct_t<true>(s, clips, info, tb, kp, logmel, mfcc, n_clips, max_tmax, spec ? 1 : 0)
                     : launch_dct_t<false>(s, clips, info, tb, kp, logmel, mfcc, n_clips, max_tmax, 0);
}

}  // namespace afx
