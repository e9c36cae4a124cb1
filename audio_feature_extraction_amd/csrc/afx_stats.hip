// k_stats of libafx.so (gfx950): Savitzky-Golay delta / delta2 rows (width 9, 'interp' edges) and the per-clip mean /
// std / ptp reductions (reference call sites: feature_extractor.py:137-150, 171-178).
#include <hip/hip_runtime.h>

#include "afx_device.h"
#include "afx_wave.h"

namespace afx {

// ---------------------------------------------------------------------------
// k_stats: one wave per (clip, row); rows 0..K-1 = MFCC coefficients, row K = RMS
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_stats(const ClipDesc* __restrict__ clips,
                                               const ClipInfo* __restrict__ info, KParams kp,
                                               const float* __restrict__ mfcc,
                                               const float* __restrict__ rms_rows,
                                               float* __restrict__ stats,
                                               float* __restrict__ frames_out,
                                               const int64_t* __restrict__ frame_offsets,
                                               ClipInfo* __restrict__ info_out) {
  const int clip = blockIdx.y;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int K = kp.n_mfcc;
  const int row = blockIdx.x * 4 + wave;
  if (row > K) return;
  const ClipInfo ci = info[clip];
  if (info_out && row == K && lane == 0) info_out[clip] = ci;      // the caller's copy (host memory the device can write)
  float* st = stats + (int64_t)clip * (4 * K + 3);
  const ClipDesc cd = clips[clip];
  // a clip with fewer than 9 frames fails the MFCC rows (librosa.feature.delta raises) but still has an RMS row:
  // extract_energy (F:153-179) only calls librosa.feature.rms
  const bool energy_only = ci.status == AFX_CLIP_TOO_SHORT && cd.len >= 2 && ci.T >= 1;   // RMS rows from the sub-block sums, or from k_trim_decide
  if (ci.status != AFX_CLIP_OK && !(energy_only && row == K)) {
    if (lane == 0) {
      if (row < K) { st[row] = 0.f; st[K + row] = 0.f; st[2 * K + row] = 0.f; st[3 * K + row] = 0.f; }
      else { st[4 * K] = 0.f; st[4 * K + 1] = 0.f; st[4 * K + 2] = 0.f; }
    }
    return;
  }
  const int T = ci.T;
  const double invT = 1.0 / (double)T;
  float* fo = frames_out ? frames_out + frame_offsets[clip] : nullptr;
  const int64_t fstride = cd.tmax;
  if (row < K) {
    const float* x = mfcc + cd.frame_base * (int64_t)K + (int64_t)row * cd.tpad;
    // the nine frames at either end, for the delta means below: fetched now, one per lane, handed to lane 0 later
    const float ev = x[lane < 9 ? lane : (lane < 18 ? T - 18 + lane : 0)];
    // one pass: sum and sum of squares in float64 (values up to ~1e3, T ~ 1e3: the squares' sum is exact to 1e-8 of
    // a variance term of 1e4 or more); sum (x - c)^2 = ss - 2 c s + T c^2 about the float32 mean c, as numpy's std
    double s = 0.0, ss = 0.0;
#pragma unroll 8
    for (int t = lane; t < T; t += 64) { const double v = (double)x[t]; s += v; ss = fma(v, v, ss); }
    s = wave_sum_d(s); ss = wave_sum_d(ss);
    const double mean = s * invT;
    const float meanf = (float)mean;
    const double c = (double)meanf;
    const double s2 = fmax(ss - 2.0 * c * s + (double)T * c * c, 0.0);
    if (fo) {
#pragma unroll 2
      for (int t = lane; t < T; t += 64) {
        // savgol_filter(width 9, polyorder=deriv=order, mode='interp'): interior taps; the
        // fitted edge polynomial has a constant derivative, so frames 0..3 / T-4..T-1 repeat
        // frame 4 / frame T-5.
        const int tc = t < 4 ? 4 : (t > T - 5 ? T - 5 : t);
        const float* cc = x + tc;
        const double d1 = (4.0 * ((double)cc[4] - (double)cc[-4]) + 3.0 * ((double)cc[3] - (double)cc[-3]) +
                           2.0 * ((double)cc[2] - (double)cc[-2]) + ((double)cc[1] - (double)cc[-1])) * (1.0 / 60.0);
        const double d2 = (28.0 * ((double)cc[4] + (double)cc[-4]) + 7.0 * ((double)cc[3] + (double)cc[-3]) -
                           8.0 * ((double)cc[2] + (double)cc[-2]) - 17.0 * ((double)cc[1] + (double)cc[-1]) -
                           20.0 * (double)cc[0]) * (1.0 / 462.0);
        fo[(int64_t)row * fstride + t] = x[t];
        fo[(int64_t)(K + row) * fstride + t] = (float)d1;
        fo[(int64_t)(2 * K + row) * fstride + t] = (float)d2;
      }
    }
    // Means of the two delta rows without the rows: both filters are differences, so their sum over the frames
    // telescopes to the nine frames at either end (the first filter) and the second one's weights cancel the bulk of
    // the row exactly (28 + 7 - 8 - 17 = 10 on either side of -20).  Frames 0..3 and T-4..T-1 repeat frame 4 / T-5.
    double h[9], g[9];                                    // h[i] = x[i], g[i] = x[T - 9 + i]
#pragma unroll
    for (int i = 0; i < 9; ++i) { h[i] = (double)__shfl(ev, i); g[i] = (double)__shfl(ev, 9 + i); }
    if (lane == 0) {
      auto D1 = [](const double* c) {
        return (4.0 * (c[4] - c[-4]) + 3.0 * (c[3] - c[-3]) + 2.0 * (c[2] - c[-2]) + (c[1] - c[-1])) * (1.0 / 60.0);
      };
      auto D2 = [](const double* c) {
        return (28.0 * (c[4] + c[-4]) + 7.0 * (c[3] + c[-3]) - 8.0 * (c[2] + c[-2]) - 17.0 * (c[1] + c[-1]) - 20.0 * c[0]) * (1.0 / 462.0);
      };
      const double w2[5] = {0.0, -17.0, -8.0, 7.0, 28.0};
      double sd1 = 0.0, sd2 = 0.0;
#pragma unroll
      for (int k = 1; k <= 4; ++k) {
        double head = 0.0, tail = 0.0, hl = 0.0, hr = 0.0, tl = 0.0, tr = 0.0;
#pragma unroll
        for (int i = 4 - k; i <= 3 + k; ++i) head += h[i];          // x[4 - k .. 3 + k]
#pragma unroll
        for (int i = 5 - k; i <= 4 + k; ++i) tail += g[i];          // x[T - 4 - k .. T - 5 + k]
#pragma unroll
        for (int i = 4 - k; i <= 3; ++i) hl += h[i];
#pragma unroll
        for (int i = 4; i <= 3 + k; ++i) hr += h[i];
#pragma unroll
        for (int i = 5 - k; i <= 4; ++i) tl += g[i];
#pragma unroll
        for (int i = 5; i <= 4 + k; ++i) tr += g[i];
        sd1 += (double)k * (tail - head);
        sd2 += w2[k] * ((hl - hr) + (tr - tl));
      }
      sd1 = sd1 * (1.0 / 60.0) + 4.0 * ((double)(float)D1(h + 4) + (double)(float)D1(g + 4));
      sd2 = sd2 * (1.0 / 462.0) + 4.0 * ((double)(float)D2(h + 4) + (double)(float)D2(g + 4));
      st[row] = meanf;
      st[K + row] = (float)sqrt(s2 * invT);
      st[2 * K + row] = (float)(sd1 * invT);
      st[3 * K + row] = (float)(sd2 * invT);
    }
  } else {
    const float* r = rms_rows + cd.frame_base;
    double s = 0.0;
    float mx = -INFINITY, mn = INFINITY;
    for (int t = lane; t < T; t += 64) {
      const float v = r[t];
      s += (double)v; mx = fmaxf(mx, v); mn = fminf(mn, v);
      if (fo) fo[(int64_t)(3 * K) * fstride + t] = v;
    }
    const double mean = wave_sum_d(s) * invT;
    const float meanf = (float)mean;
    mx = wave_max(mx); mn = wave_min(mn);
    double s2 = 0.0;
    for (int t = lane; t < T; t += 64) { const float d = r[t] - meanf; s2 += (double)d * (double)d; }
    s2 = wave_sum_d(s2);
    if (lane == 0) {
      st[4 * K] = meanf;
      st[4 * K + 1] = (float)sqrt(s2 * invT);
      st[4 * K + 2] = mx - mn;
    }
  }
}

hipError_t launch_stats(hipStream_t s, const ClipDesc* clips, const ClipInfo* info, const KParams& kp,
                        const float* mfcc, const float* rms_rows, float* stats, float* frames_out,
                        const int64_t* frame_offsets, int n_clips, ClipInfo* info_out) {
  dim3 grid((kp.n_mfcc + 1 + 3) / 4, n_clips);
  hipLaunchKernelGGL(k_stats, grid, dim3(256), 0, s, clips, info, kp, mfcc, rms_rows, stats, frames_out,
                     frame_offsets, info_out);
  return hipGetLastError();
}

}  // namespace afx
