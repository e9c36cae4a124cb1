// The kernels of the fused pass over the spectral, harmonic, timbre and rhythm groups (afx_groups.h, afx_groups_batch):
// everything here reads rows the existing kernels left on the device -- the complex or power rows of k_hpss_stft, the dB
// rows of k_rhythm_mel -- and writes scalars.  No float atomics, no LDS but the per-clip float64 reductions; every sum has
// one fixed order, so a clip's record depends neither on its neighbours nor on how the batch was cut.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdint>

#include "afx_groups.h"
#include "afx_wave.h"

namespace afx {

namespace {

typedef float gv2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ double gr_block_sum(double v, double* red) {
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

__device__ __forceinline__ double gr_block_max(double v, double* red) {
  red[threadIdx.x] = v;
  __syncthreads();
#pragma unroll
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] = fmax(red[threadIdx.x], red[threadIdx.x + s]);
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}

// librosa.power_to_db(ref=1.0, amin=1e-10) of one value, before the clamp
__device__ __forceinline__ double gr_db(double p) { return 10.0 * log10(fmax(1e-10, p)); }

}  // namespace

// |x|^2 as k_hpss_stft<true> rounds it: there the compiler squares (re, im) with one packed multiply and adds the halves,
// two rounded products and a rounded sum, never a fused multiply-add.  Written out so that it cannot be contracted here.
__device__ __forceinline__ float gr_power(float re, float im) {
#pragma clang fp contract(off)
  const float a = re * re;
  const float b = im * im;
  return a + b;
}

// One thread per float4 of a power row (260 of them), from the complex rows of k_hpss_stft<false>: the same xk, the same
// roundings (gr_power), so the rows are launch_hpss_stft_power's bit for bit; the Nyquist bin is a single product there.
__global__ __launch_bounds__(256) void k_groups_square(const gv2* __restrict__ X, int64_t n_frames, float* __restrict__ S) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_frames * (kHpssPowPitch / 4)) return;
  const int64_t g = i / (kHpssPowPitch / 4);
  const int j = (int)(i - g * (kHpssPowPitch / 4));
  float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
  const gv2* row = X + g * kHpssPitch;
  if (j < 256) {
    const float4 a = *reinterpret_cast<const float4*>(row + 4 * j), b = *reinterpret_cast<const float4*>(row + 4 * j + 2);
    o = make_float4(gr_power(a.x, a.y), gr_power(a.z, a.w), gr_power(b.x, b.y), gr_power(b.z, b.w));
  } else if (j == 256) {
    const float ny = row[1024].x;
    o.x = ny * ny;
  }
  *reinterpret_cast<float4*>(S + g * kHpssPowPitch + 4 * j) = o;
}

// One wave per frame.  Lane l holds the magnitudes of bins 4 (l + 64 q) + c, q < 4, c < 4 (slot 4 q + c: four coalesced
// 16-byte loads of the row's first 256 float4) and lane 0 bin 1024 in slot 16.
template <bool FULL>
__global__ __launch_bounds__(256) void k_spec_rows(const float* __restrict__ S, int64_t n_frames, SpecBands sb,
                                                   float* __restrict__ desc) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t g = (int64_t)blockIdx.x * 4 + wave;
  if (g >= n_frames) return;
  const float* row = S + g * kHpssPowPitch;
  float mg[17];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const float4 p4 = *reinterpret_cast<const float4*>(row + 4 * (lane + 64 * q));
    mg[4 * q] = sqrtf(p4.x); mg[4 * q + 1] = sqrtf(p4.y); mg[4 * q + 2] = sqrtf(p4.z); mg[4 * q + 3] = sqrtf(p4.w);
  }
  mg[16] = lane == 0 ? sqrtf(row[1024]) : 0.f;
  auto bin = [&](int j) -> int { return j < 16 ? 4 * (lane + 64 * (j >> 2)) + (j & 3) : 1024; };
  const float hz = sb.hz_per_bin;
  float s0 = 0.f, s1 = 0.f;
#pragma unroll
  for (int j = 0; j < 17; ++j) { s0 += mg[j]; s1 = fmaf(mg[j], (float)bin(j) * hz, s1); }
  const float tot = wave_sum(s0);
  const float len = tot < FLT_MIN ? 1.0f : tot;          // librosa.util.normalize(norm=1): a column below tiny keeps its scale
  const float cen = wave_sum(s1) / len;
  float* const dst = desc + g * kSpecFloats;
  if constexpr (!FULL) {
    if (lane == 0) dst[0] = cen;
    return;
  } else {
    float s2 = 0.f;
#pragma unroll
    for (int j = 0; j < 17; ++j) { const float d = (float)bin(j) * hz - cen; s2 = fmaf(mg[j], d * d, s2); }
    const float bw = sqrtf(wave_sum(s2) / len);
    // roll-off: the lowest bin whose running sum reaches 85 % of the total.  The running sum goes through the four
    // 256-bin segments in bin order: inside a lane, across the lanes (inclusive scan), then the segments before it.
    const float thr = sb.roll_percent * tot;
    int kroll = 1 << 20;
    float segbase = 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float r0 = mg[4 * q], r1 = r0 + mg[4 * q + 1], r2 = r1 + mg[4 * q + 2], r3 = r2 + mg[4 * q + 3];
      float pre = r3;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) { const float t = __shfl_up(pre, o); if (lane >= o) pre += t; }
      const float base = segbase + (pre - r3);
      const int k0 = 4 * (lane + 64 * q);
      int k = 1 << 20;
      if (base + r3 >= thr) k = k0 + 3;
      if (base + r2 >= thr) k = k0 + 2;
      if (base + r1 >= thr) k = k0 + 1;
      if (base + r0 >= thr) k = k0;
      kroll = k < kroll ? k : kroll;
      segbase += __shfl(pre, 63);
    }
    if (lane == 0 && segbase + mg[16] >= thr && kroll > 1024) kroll = 1024;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { const int t = __shfl_xor(kroll, o); kroll = t < kroll ? t : kroll; }
    const float roll = (kroll < (1 << 20) ? (float)kroll : 0.f) * hz;
    if (lane == 0) { dst[0] = cen; dst[1] = bw; dst[2] = roll; }
    // contrast bands: repeated extraction of the band's smallest (largest) remaining magnitude, as k_frames3s<DESC>
#pragma unroll 1
    for (int bnd = 0; bnd < 7; ++bnd) {
      const int lo = sb.lo[bnd], hi = sb.hi[bnd], cnt = sb.cnt[bnd];
      unsigned inb = 0;
#pragma unroll
      for (int j = 0; j < 17; ++j) { const int k = bin(j); if (k >= lo && k <= hi && (j < 16 || lane == 0)) inb |= 1u << j; }
#pragma unroll 1
      for (int side = 0; side < 2; ++side) {             // 0: valley (smallest), 1: peak (largest)
        unsigned avail = inb;
        float total = 0.f;
#pragma unroll 1
        for (int r = 0; r < cnt; ++r) {
          float m = side ? -1.f : INFINITY;
          int jm = 0;
#pragma unroll
          for (int j = 0; j < 17; ++j) {
            const bool ok = (avail >> j) & 1u;
            const bool better = ok && (side ? mg[j] > m : mg[j] < m);
            m = better ? mg[j] : m; jm = better ? j : jm;
          }
          const float best = side ? wave_max(m) : wave_min(m);
          const bool have = side ? m >= 0.f : m < INFINITY;      // the lane still had a candidate
          const unsigned long long holders = __ballot(have && m == best);
          if (holders == 0ull) break;                    // band exhausted
          const int owner = __ffsll((long long)holders) - 1;
          if (lane == owner) avail &= ~(1u << jm);
          total += best;
        }
        if (lane == 0) dst[3 + 7 * side + bnd] = cnt > 0 ? total / (float)cnt : 0.f;     // [3..9] valley, [10..16] peak
      }
    }
  }
}

// One workgroup per clip.  Pass one: the clip's largest peak and valley (their dB floors); pass two: the four means, the
// contrast as power_to_db(peak) - power_to_db(valley) with both clamps; pass three: the squared deviations.
__global__ __launch_bounds__(256) void k_spec_stats(const float* __restrict__ desc, const HpssClip* __restrict__ clips,
                                                    double* __restrict__ stats) {
  __shared__ double red[256];
  const HpssClip c = clips[blockIdx.x];
  const float* d = desc + c.frame_base * kSpecFloats;
  double mp = 0.0, mv = 0.0;
  for (int t = threadIdx.x; t < c.T; t += 256) {
    const float* r = d + (int64_t)t * kSpecFloats;
#pragma unroll
    for (int k = 0; k < 7; ++k) { mv = fmax(mv, (double)r[3 + k]); mp = fmax(mp, (double)r[10 + k]); }
  }
  const double floor_p = gr_db(gr_block_max(mp, red)) - 80.0, floor_v = gr_db(gr_block_max(mv, red)) - 80.0;
  double mean[4];
  for (int pass = 0; pass < 2; ++pass) {
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int t = threadIdx.x; t < c.T; t += 256) {
      const float* r = d + (int64_t)t * kSpecFloats;
      if (pass == 0) {
        acc[0] += (double)r[0]; acc[1] += (double)r[1]; acc[2] += (double)r[2];
      } else {
#pragma unroll
        for (int k = 0; k < 3; ++k) { const double e = (double)r[k] - mean[k]; acc[k] += e * e; }
      }
#pragma unroll
      for (int k = 0; k < 7; ++k) {
        const double con = fmax(gr_db((double)r[10 + k]), floor_p) - fmax(gr_db((double)r[3 + k]), floor_v);
        if (pass == 0) acc[3] += con;
        else { const double e = con - mean[3]; acc[3] += e * e; }
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[k] = gr_block_sum(acc[k], red) / ((k == 3 ? 7.0 : 1.0) * (double)c.T);
    if (pass == 0) {
#pragma unroll
      for (int k = 0; k < 4; ++k) mean[k] = acc[k];
    } else if (threadIdx.x == 0) {
      double* o = stats + 8 * (int64_t)blockIdx.x;
#pragma unroll
      for (int k = 0; k < 4; ++k) { o[2 * k] = mean[k]; o[2 * k + 1] = sqrt(acc[k]); }
    }
  }
}

// A wave walks kGroupsMfccFrames consecutive rows of the chunk with its share of the table in registers: lane l holds
// columns l and l + 64 of the 13 rows.  Per frame: both dB values clamped at the clip's floor, 13 wave sums (float32,
// fixed order), the frame's sum and sum of squares in float64.
__global__ __launch_bounds__(256) void k_mfcc_rows(const float* __restrict__ db, const uint32_t* __restrict__ clip_max,
                                                   const HpssClip* __restrict__ clips, int n, int64_t n_frames,
                                                   int n_mels, const float* __restrict__ dct, double* __restrict__ parts) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t g0 = ((int64_t)blockIdx.x * 4 + wave) * kGroupsMfccFrames;
  if (g0 >= n_frames) return;
  float w0[kGroupsMfcc], w1[kGroupsMfcc];
#pragma unroll
  for (int k = 0; k < kGroupsMfcc; ++k) { w0[k] = dct[k * kRhMels + lane]; w1[k] = dct[k * kRhMels + 64 + lane]; }
  for (int u = 0; u < kGroupsMfccFrames; ++u) {
    const int64_t g = g0 + u;
    if (g >= n_frames) break;
    const int ci = hp_find(n, g, [&](int i) { return clips[i].frame_base; });
    const float floor_db = 10.0f * log10f(fmaxf(1e-10f, __uint_as_float(clip_max[ci]))) - 80.0f;
    const float* r = db + g * kRhMels;
    // bands past n_mels were never written (their table columns are zero, but 0 x NaN is not)
    const float a = lane < n_mels ? fmaxf(r[lane], floor_db) : 0.f, b = 64 + lane < n_mels ? fmaxf(r[64 + lane], floor_db) : 0.f;
    double s = 0.0, q = 0.0;
#pragma unroll
    for (int k = 0; k < kGroupsMfcc; ++k) {
      const float ck = wave_sum(fmaf(w1[k], b, w0[k] * a));
      s += (double)ck; q += (double)ck * (double)ck;
    }
    if (lane == 0) { parts[2 * g] = s; parts[2 * g + 1] = q; }
  }
}

__global__ __launch_bounds__(256) void k_mfcc_stats(const double* __restrict__ parts, const HpssClip* __restrict__ clips,
                                                    double* __restrict__ stats) {
  __shared__ double red[256];
  const HpssClip c = clips[blockIdx.x];
  double s = 0.0, q = 0.0;
  for (int t = threadIdx.x; t < c.T; t += 256) {
    const double* p = parts + 2 * (c.frame_base + t);
    s += p[0]; q += p[1];
  }
  s = gr_block_sum(s, red);
  q = gr_block_sum(q, red);
  if (threadIdx.x == 0) {
    const double cnt = (double)kGroupsMfcc * c.T, mean = s / cnt, var = q / cnt - mean * mean;
    stats[2 * (int64_t)blockIdx.x] = mean;
    stats[2 * (int64_t)blockIdx.x + 1] = sqrt(var > 0.0 ? var : 0.0);
  }
}

__global__ __launch_bounds__(256) void k_groups_mark_bad(const FiltState* __restrict__ st, int n, uint32_t* __restrict__ bad) {
  const int c = (int)(blockIdx.x * 256 + threadIdx.x);
  if (c < n && st[c].bad) bad[c] = 1u;
}

__global__ __launch_bounds__(256) void k_groups_record(GroupsSrc src, const HpssClip* __restrict__ clips,
                                                       const uint32_t* __restrict__ bad, int n, double* __restrict__ rec,
                                                       int32_t* __restrict__ ints) {
  const int c = (int)(blockIdx.x * 256 + threadIdx.x);
  if (c >= n) return;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  double v[kGroupsStats];
#pragma unroll
  for (int k = 0; k < kGroupsStats; ++k) v[k] = nan;
  int32_t slot = 50, lag = 0;
  if (!bad[c]) {
    const bool one = clips[c].len < 2;                   // a clip of one sample has no centroid (afx_hpss_batch, afx_spectral_batch)
    if (src.spec && !one)
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] = src.spec[8 * (int64_t)c + k];
    if (src.harm) {
#pragma unroll
      for (int k = 0; k < 4; ++k) v[8 + k] = src.harm[4 * (int64_t)c + k];
      if (one) v[10] = v[11] = nan;
    }
    if (src.chroma)
#pragma unroll
      for (int k = 0; k < 4; ++k) v[12 + k] = src.chroma[4 * (int64_t)c + k];
    if (src.mfcc) { v[16] = src.mfcc[2 * (int64_t)c]; v[17] = src.mfcc[2 * (int64_t)c + 1]; }
    if (src.slot) slot = src.slot[c];
    if (src.rhythm) {
      const double* r = src.rhythm + 4 * (int64_t)c;
      lag = (int32_t)r[3];
      v[18] = r[0]; v[19] = r[1]; v[20] = r[2];
      v[21] = src.acmean[(int64_t)src.win * c + lag];
    }
    v[22] = src.filt ? (double)src.filt[c].peak_in : 0.0;
    v[23] = src.filt ? src.filt[c].peak_out : 0.0;
  }
#pragma unroll
  for (int k = 0; k < kGroupsStats; ++k) rec[kGroupsStats * (int64_t)c + k] = v[k];
  ints[2 * c] = slot; ints[2 * c + 1] = lag;
}

// ---------------------------------------------------------------------------------------------------------------------
hipError_t launch_groups_square(hipStream_t s, const float2* X, int64_t n_frames, float* S) {
  const int64_t items = n_frames * (kHpssPowPitch / 4);
  hipLaunchKernelGGL(k_groups_square, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, s, (const gv2*)X, n_frames, S);
  return hipGetLastError();
}

hipError_t launch_spec_rows(hipStream_t s, const float* S, int64_t n_frames, const SpecBands& sb, bool full, float* desc) {
  const dim3 gr((unsigned)((n_frames + 3) / 4));
  if (full) hipLaunchKernelGGL(k_spec_rows<true>, gr, dim3(256), 0, s, S, n_frames, sb, desc);
  else hipLaunchKernelGGL(k_spec_rows<false>, gr, dim3(256), 0, s, S, n_frames, sb, desc);
  return hipGetLastError();
}

hipError_t launch_spec_stats(hipStream_t s, const float* desc, const HpssClip* clips, int n, double* stats) {
  hipLaunchKernelGGL(k_spec_stats, dim3(n), dim3(256), 0, s, desc, clips, stats);
  return hipGetLastError();
}

hipError_t launch_mfcc_rows(hipStream_t s, const float* db, const uint32_t* clip_max, const HpssClip* clips, int n,
                            int64_t n_frames, int n_mels, const float* dct, double* parts) {
  const int64_t waves = (n_frames + kGroupsMfccFrames - 1) / kGroupsMfccFrames;
  hipLaunchKernelGGL(k_mfcc_rows, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, s, db, clip_max, clips, n, n_frames, n_mels, dct, parts);
  return hipGetLastError();
}

hipError_t launch_mfcc_stats(hipStream_t s, const double* parts, const HpssClip* clips, int n, double* stats) {
  hipLaunchKernelGGL(k_mfcc_stats, dim3(n), dim3(256), 0, s, parts, clips, stats);
  return hipGetLastError();
}

hipError_t launch_groups_mark_bad(hipStream_t s, const FiltState* st, int n, uint32_t* bad) {
  hipLaunchKernelGGL(k_groups_mark_bad, dim3((n + 255) / 256), dim3(256), 0, s, st, n, bad);
  return hipGetLastError();
}

hipError_t launch_groups_record(hipStream_t s, const GroupsSrc& src, const HpssClip* clips, const uint32_t* bad, int n,
                                double* rec, int32_t* ints) {
  hipLaunchKernelGGL(k_groups_record, dim3((n + 255) / 256), dim3(256), 0, s, src, clips, bad, n, rec, ints);
  return hipGetLastError();
}

}  // namespace afx
