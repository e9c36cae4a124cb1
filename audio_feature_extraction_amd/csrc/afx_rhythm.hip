// Onset strength, tempogram and tempo: librosa.onset.onset_strength, librosa.feature.tempogram (win_length = int(8 sr) //
// 512, what beat_track asks of it) and librosa.feature.tempo's decision at librosa's defaults, on the float32 power rows of
// k_hpss_stft<true> (tests/rhythm_ref.py is the spec).  Four kernels on one stream behind HPSS's prep + STFT:
//   k_rhythm_mel         one wave per 16 frames: the banded mel contraction of afx_chroma.h's ChromaMel images as exact-f32
//                        MFMA, stored as float32 dB; the clip's largest mel power by an integer atomic max of its bits
//   k_rhythm_env         one wave per frame: both dB rows clamped at the clip maximum - 80, the rectified difference, the
//                        mean over the bands
//   k_rhythm_tempogram   one workgroup per 16 frames, a wave per 4 of them: the padded envelope and the window in LDS, the
//                        windowed frame in a zero-extended LDS row of the wave's own; a lane owns L consecutive lags and
//                        slides its operands through registers: L broadcast values and L new values (vector reads, no bank
//                        conflict at the lane stride L) feed L x L FMAs; wave maximum, division, float64 sums per lag
//   k_rhythm_reduce      per clip, float64 in a fixed order: the mean tempogram, the first maximum of log1p(1e6 acmean) +
//                        logprior, mean / std of the envelope
// No float atomics anywhere; nothing depends on the order in which waves run.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <climits>
#include <cstdint>

#include "afx_rhythm.h"
#include "afx_wave.h"

namespace afx {

typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float rh_db(float p) { return 10.0f * log10f(fmaxf(1e-10f, p)); }

__global__ __launch_bounds__(256) void k_rhythm_mel(const float* __restrict__ S, const HpssClip* __restrict__ clips, int n,
                                                    int n_tiles, ChromaMel mel, float* __restrict__ db,
                                                    uint32_t* __restrict__ clip_max) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int g = (int)blockIdx.x * 4 + wave;
  if (g >= n_tiles) return;
  const int ci = hp_find(n, g, [&](int i) { return (int64_t)clips[i].tile_base; });
  const HpssClip c = clips[ci];
  const int f = lane & 15, q = lane >> 4, t = (g - c.tile_base) * 16 + f;
  const bool valid = t < c.T;
  // a lane past the clip's last frame reads that last frame again (never another clip's rows) and stores nothing
  const float* row = S + (c.frame_base + (valid ? t : c.T - 1)) * kHpssPowPitch + 4 * q;
  float* o = db + (c.frame_base + t) * kRhMels + 4 * q;
  float m = 0.f;
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
    const f32x4 v = b0 + b1;                             // filters 16 gi + 4 q + {0..3}; those past n_mels are zero
    m = fmaxf(fmaxf(m, fmaxf(v[0], v[1])), fmaxf(v[2], v[3]));
    if (valid) *reinterpret_cast<float4*>(o + 16 * gi) = make_float4(rh_db(v[0]), rh_db(v[1]), rh_db(v[2]), rh_db(v[3]));
  }
  // the mel power is non-negative, so its float bits order as unsigned integers
  m = wave_max(valid ? m : 0.f);
  if (lane == 0) atomicMax(clip_max + ci, __float_as_uint(m));
}

__global__ __launch_bounds__(256) void k_rhythm_env(const float* __restrict__ db, const uint32_t* __restrict__ clip_max,
                                                    const HpssClip* __restrict__ clips, int n, int64_t n_frames, int n_mels,
                                                    float* __restrict__ env) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t g = (int64_t)blockIdx.x * 4 + wave;
  if (g >= n_frames) return;
  const int ci = hp_find(n, g, [&](int i) { return clips[i].frame_base; });
  const int64_t t = g - clips[ci].frame_base;
  if (t < kRhOnsetLag) {
    if (lane == 0) env[g] = 0.f;
    return;
  }
  const float floor_db = rh_db(__uint_as_float(clip_max[ci])) - 80.0f;
  const float* a = db + (g - kRhOnsetLag) * kRhMels;     // dB[:, t - 3], then dB[:, t - 2]
  const float* b = a + kRhMels;
  float s = 0.f;
#pragma unroll
  for (int m = lane; m < kRhMels; m += 64)
    if (m < n_mels) s += fmaxf(0.f, fmaxf(b[m], floor_db) - fmaxf(a[m], floor_db));
  s = wave_sum(s);
  if (lane == 0) env[g] = s / (float)n_mels;
}

// L floats from an address that is a multiple of 4 L bytes: ds_read_b128 (L a multiple of 4) or ds_read_b64 (L even)
template <int L>
__device__ __forceinline__ void rh_load(const float* p, float (&v)[L]) {
  if constexpr (L % 4 == 0) {
#pragma unroll
    for (int q = 0; q < L / 4; ++q) {
      const float4 a = reinterpret_cast<const float4*>(p)[q];
      v[4 * q] = a.x; v[4 * q + 1] = a.y; v[4 * q + 2] = a.z; v[4 * q + 3] = a.w;
    }
  } else {
#pragma unroll
    for (int q = 0; q < L / 2; ++q) {
      const float2 a = reinterpret_cast<const float2*>(p)[q];
      v[2 * q] = a.x; v[2 * q + 1] = a.y;
    }
  }
}

// Lane l owns lags l L .. l L + L - 1 (64 L >= win).  Step i of the autocorrelation needs x[i] in every lane (one address:
// a broadcast read) and x[i + l L + j], j < L, in lane l: of those, L - 1 are the previous step's, so L steps at a time take
// L broadcast values and L new values per lane for L x L FMAs.  x is zero from win on, which ends every lag's sum where it
// must.  Partial sums are folded into the total every F steps of L (about 48 products): the float32 sum of up to 768
// non-negative products then carries the rounding of sqrt(48) + sqrt(16) additions, not of sqrt(768).
template <int L>
__global__ __launch_bounds__(256) void k_rhythm_tempogram(const float* __restrict__ env, const HpssClip* __restrict__ clips,
                                                          int n, int n_tiles, RhythmTab tab, double* __restrict__ parts,
                                                          float* __restrict__ tg) {
  constexpr int F = 48 / L;                              // steps of L between two folds
  constexpr int XS = 130 * L + 64;                       // floats of a wave's row: reads reach below win + F L + 65 L
  __shared__ __attribute__((aligned(16))) float rows[4 * XS];
  __shared__ float seg[kRhMaxWin + kRhTile];
  __shared__ float win[kRhMaxWin];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int g = (int)blockIdx.x;
  const int ci = hp_find(n, g, [&](int i) { return (int64_t)clips[i].tile_base; });
  const HpssClip c = clips[ci];
  const int w = tab.win, h = w / 2, T = c.T, t0 = (g - c.tile_base) * kRhTile;
  const float* e = env + c.frame_base;
  // the tile's span of the envelope padded by h on both sides: numpy's linear_ramp to 0 (the left ramp starts from env[0],
  // which is 0; the right one is float32(m * (float64(env[T - 1]) / h)), m = h - 1 .. 0)
  for (int q = tid; q < w + kRhTile - 1; q += 256) {
    const int j = t0 + q;
    float p = 0.f;
    if (j >= h && j < h + T) p = e[j - h];
    else if (j >= h + T && j < T + 2 * h) p = (float)((double)(T + 2 * h - 1 - j) * ((double)e[T - 1] / (double)h));
    seg[q] = p;
  }
  for (int i = tid; i < w; i += 256) win[i] = tab.window[i];
  float* x = rows + wave * XS;
  for (int i = w + lane; i < XS; i += 64) x[i] = 0.f;
  __syncthreads();
  double dsum[L];
#pragma unroll
  for (int j = 0; j < L; ++j) dsum[j] = 0.0;
  const int nblk = (w + F * L - 1) / (F * L);
  for (int fr = 0; fr < 4; ++fr) {
    const int tl = wave * 4 + fr, t = t0 + tl;
    const bool active = t < T;                           // the same in every lane of the wave
    if (active)
      for (int i = lane; i < w; i += 64) x[i] = win[i] * seg[tl + i];
    __syncthreads();
    if (active) {
      float tot[L], r[L];
#pragma unroll
      for (int j = 0; j < L; ++j) tot[j] = 0.f;
      rh_load<L>(x + lane * L, r);
      for (int b = 0; b < nblk; ++b) {
        float acc[L];
#pragma unroll
        for (int j = 0; j < L; ++j) acc[j] = 0.f;
#pragma unroll
        for (int u8 = 0; u8 < F; ++u8) {
          const int i0 = (b * F + u8) * L;
          float xb[L], nw[L];
          rh_load<L>(x + i0, xb);
          rh_load<L>(x + i0 + (lane + 1) * L, nw);
#pragma unroll
          for (int u = 0; u < L; ++u)
#pragma unroll
            for (int j = 0; j < L; ++j) acc[j] = fmaf(xb[u], u + j < L ? r[u + j] : nw[u + j - L], acc[j]);
#pragma unroll
          for (int j = 0; j < L; ++j) r[j] = nw[j];
        }
#pragma unroll
        for (int j = 0; j < L; ++j) tot[j] += acc[j];
      }
      float m = 0.f;
#pragma unroll
      for (int j = 0; j < L; ++j)
        if (lane * L + j < w) m = fmaxf(m, fabsf(tot[j]));
      m = wave_max(m);
#pragma unroll
      for (int j = 0; j < L; ++j) {
        const int k = lane * L + j;
        if (k < w) {
          const float v = m >= FLT_MIN ? tot[j] / m : tot[j];
          dsum[j] += (double)v;
          if (tg) tg[(int64_t)w * c.frame_base + (int64_t)k * T + t] = v;
        }
      }
    }
    __syncthreads();
  }
  // the tile's sums: the four waves' in wave order (the rows are free now: every wave is past its last read)
  double* slab = reinterpret_cast<double*>(rows);
#pragma unroll
  for (int j = 0; j < L; ++j)
    if (lane * L + j < w) slab[wave * w + lane * L + j] = dsum[j];
  __syncthreads();
  for (int k = tid; k < w; k += 256) parts[(int64_t)g * w + k] = ((slab[k] + slab[w + k]) + slab[2 * w + k]) + slab[3 * w + k];
}

__device__ __forceinline__ double rh_block_sum(double v, double* red) {
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

__global__ __launch_bounds__(256) void k_rhythm_reduce(const float* __restrict__ env, const HpssClip* __restrict__ clips,
                                                       RhythmTab tab, const double* __restrict__ parts,
                                                       double* __restrict__ acmean, double* __restrict__ res) {
  __shared__ double red[256];
  __shared__ int redi[256];
  const int tid = threadIdx.x;
  const HpssClip c = clips[blockIdx.x];
  const int w = tab.win, T = c.T, nt = (T + kRhTile - 1) / kRhTile;
  const double* p = parts + (int64_t)c.tile_base * w;
  double best = -INFINITY;
  int arg = INT_MAX;
  for (int k = tid; k < w; k += 256) {                   // ascending k and a strict comparison: the thread's first maximum
    double s = 0.0;
    for (int i = 0; i < nt; ++i) s += p[(int64_t)i * w + k];
    const double am = s / (double)T;
    acmean[(int64_t)blockIdx.x * w + k] = am;
    const double score = log1p(1e6 * am) + tab.logprior[k];
    if (arg == INT_MAX || score > best) { best = score; arg = k; }
  }
  red[tid] = best; redi[tid] = arg;
  __syncthreads();
#pragma unroll
  for (int s = 128; s > 0; s >>= 1) {                    // the larger score; of equal scores the smaller lag
    if (tid < s) {
      const double o = red[tid + s];
      const int oi = redi[tid + s];
      if (o > red[tid] || (o == red[tid] && oi < redi[tid])) { red[tid] = o; redi[tid] = oi; }
    }
    __syncthreads();
  }
  const int lag = redi[0];
  __syncthreads();
  const float* e = env + c.frame_base;
  double s = 0.0;
  int nz = 0;
  for (int t = tid; t < T; t += 256) { s += (double)e[t]; nz |= e[t] != 0.f; }
  nz = __syncthreads_or(nz);
  const double mean = rh_block_sum(s, red) / (double)T;
  double v = 0.0;
  for (int t = tid; t < T; t += 256) { const double d = (double)e[t] - mean; v += d * d; }
  v = rh_block_sum(v, red) / (double)T;
  if (tid == 0) {
    double* o = res + 4 * (int64_t)blockIdx.x;
    o[0] = nz ? tab.bpm[lag] : 0.0; o[1] = mean; o[2] = sqrt(v); o[3] = nz ? (double)lag : 0.0;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
hipError_t launch_rhythm_mel(hipStream_t s, const float* S, const HpssClip* clips, int n, int n_tiles, ChromaMel mel,
                             float* db, uint32_t* clip_max) {
  hipLaunchKernelGGL(k_rhythm_mel, dim3((unsigned)((n_tiles + 3) / 4)), dim3(256), 0, s, S, clips, n, n_tiles, mel, db, clip_max);
  return hipGetLastError();
}

hipError_t launch_rhythm_env(hipStream_t s, const float* db, const uint32_t* clip_max, const HpssClip* clips, int n,
                             int64_t n_frames, int n_mels, float* env) {
  hipLaunchKernelGGL(k_rhythm_env, dim3((unsigned)((n_frames + 3) / 4)), dim3(256), 0, s, db, clip_max, clips, n, n_frames, n_mels, env);
  return hipGetLastError();
}

hipError_t launch_rhythm_tempogram(hipStream_t s, const float* env, const HpssClip* clips, int n, int n_tiles, RhythmTab tab,
                                   double* parts, float* tg) {
  if (tab.win < 2 || tab.win > kRhMaxWin) return hipErrorInvalidValue;
  const dim3 gr((unsigned)n_tiles), bl(256);
  const int lanes = (tab.win + 63) / 64;                 // lags per lane, rounded up to an even count
#define AFX_RH_TG(L) hipLaunchKernelGGL(k_rhythm_tempogram<L>, gr, bl, 0, s, env, clips, n, n_tiles, tab, parts, tg)
  switch ((lanes + 1) / 2) {
    case 1: AFX_RH_TG(2); break;
    case 2: AFX_RH_TG(4); break;
    case 3: AFX_RH_TG(6); break;
    case 4: AFX_RH_TG(8); break;
    case 5: AFX_RH_TG(10); break;
    default: AFX_RH_TG(12); break;
  }
#undef AFX_RH_TG
  return hipGetLastError();
}

hipError_t launch_rhythm_reduce(hipStream_t s, const float* env, const HpssClip* clips, int n, RhythmTab tab,
                                const double* parts, double* acmean, double* res) {
  hipLaunchKernelGGL(k_rhythm_reduce, dim3(n), dim3(256), 0, s, env, clips, tab, parts, acmean, res);
  return hipGetLastError();
}

}  // namespace afx
