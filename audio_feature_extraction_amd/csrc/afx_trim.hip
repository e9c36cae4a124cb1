// The trim stage of libafx.so (gfx950): what librosa.effects.trim(top_db) needs and what follows from its answer
// (reference call site: audio_feature_extraction_toolkit/core/feature_extractor.py:69-72).
//   k_trim_blocks    pre-emphasis on the fly, sum of squares per trim block (or per hop-sized sub-block of it)
//   k_trim_decide    one workgroup per clip: threshold search -> [start, end), T, status; RMS rows; the clip's block records
// The search, the RMS rows (afx_trim_dev.h) and the block record (make_block, afx_device.h) exist once; afx_trim3.hip
// holds the decision that follows a speculative frame pass.
#include <hip/hip_runtime.h>

#include "afx_device.h"
#include "afx_trim_dev.h"
#include "afx_wave.h"

namespace afx {

// ---------------------------------------------------------------------------
// k_trim_blocks: sums of squares of the (pre-emphasised) samples per trim block -- the only full pass over the
// samples besides the frame kernel.  A wave owns kTrimPerWave consecutive trim blocks of one clip; when they are
// all interior, float32 and 16-byte aligned it issues every load of its span before the first use.
// ---------------------------------------------------------------------------
constexpr int kTrimPerWave = 4;

__device__ __forceinline__ float sumsq4(float v0, float v1, float v2, float v3) {
#pragma clang fp contract(off)      // one rounding sequence wherever this is inlined
  float s4 = v0 * v0; s4 += v1 * v1; s4 += v2 * v2; s4 += v3 * v3;
  return s4;
}
__device__ __forceinline__ float sq4(float y0, float y1, float y2, float y3, float prev, bool pre, float b1) {
  float v0 = y0, v1 = y1, v2 = y2, v3 = y3;
  if (pre) {
    v0 = preemph1(y0, prev, b1); v1 = preemph1(y1, y0, b1);
    v2 = preemph1(y2, y1, b1); v3 = preemph1(y3, y2, b1);
  }
  return sumsq4(v0, v1, v2, v3);
}

__global__ __launch_bounds__(256) void k_trim_blocks(const void* __restrict__ samples,
                                                     const ClipDesc* __restrict__ clips,
                                                     ClipInfo* __restrict__ info,
                                                     float* __restrict__ bsum, KParams kp) {
  const int clip = blockIdx.y;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const ClipDesc cd = clips[clip];
  const int64_t N = cd.len;
  const int th = kp.trim_hop;
  const int64_t nb = (N + th - 1) / th;
  const int64_t bfirst = ((int64_t)blockIdx.x * 4 + wave) * kTrimPerWave;
  if (bfirst >= nb) return;
  const bool pre = (kp.flags & AFX_FLAG_PREEMPH) != 0;
  const float b1 = kp.preemph_b1;
  // per > 1: a block's sum is kept as `per` sub-block sums of 256 samples (RMS rows are built from them)
  const int per = kp.rms_sub > 0 ? kp.rms_sub : 1;
  const float* base = (const float*)samples + cd.off;
  int nf = 0;

  // fast route: the wave's whole span is inside the clip, aligned, and made of 256-sample runs
  const int64_t s0 = bfirst * th, s1 = s0 + (int64_t)kTrimPerWave * th;
  const bool fast = (th == 256 || th == 512) && s0 > 0 && s1 <= N && (((cd.off + s0) & 3) == 0);
  if (fast) {
    constexpr int MAXR = kTrimPerWave * 2;
    const int nr = kTrimPerWave * (th >> 8);
    float4 q[MAXR];
    if (kp.fmt == AFX_FMT_F32) {
#pragma unroll
      for (int r = 0; r < MAXR; ++r)
        if (r < nr) q[r] = *reinterpret_cast<const float4*>(base + s0 + 256 * r + 4 * lane);
    } else {                                                    // int16: 8-byte loads, /32768 as libsndfile
      const int16_t* b16 = (const int16_t*)samples + cd.off;
      const float sc = 1.0f / 32768.0f;
#pragma unroll
      for (int r = 0; r < MAXR; ++r)
        if (r < nr) {
          const int2 w = *reinterpret_cast<const int2*>(b16 + s0 + 256 * r + 4 * lane);
          q[r] = make_float4((float)(short)(w.x & 0xffff) * sc, (float)(short)(w.x >> 16) * sc,
                             (float)(short)(w.y & 0xffff) * sc, (float)(short)(w.y >> 16) * sc);
        }
    }
    float carry = ld_sample(samples, kp.fmt, cd.off + s0 - 1);   // sample before the span (lane 0 of run 0)
    float acc = 0.f;
#pragma unroll
    for (int r = 0; r < MAXR; ++r) {
      if (r < nr) {
        float prev = __shfl_up(q[r].w, 1);
        if (lane == 0) prev = carry;
        carry = __shfl(q[r].w, 63);
        nf |= !(isfinite(q[r].x) && isfinite(q[r].y) && isfinite(q[r].z) && isfinite(q[r].w));
        const float s4 = sq4(q[r].x, q[r].y, q[r].z, q[r].w, prev, pre, b1);
        if (per > 1 || th == 256) {                             // every run is its own sum
          const float t = wave_sum(s4);
          if (lane == 0) bsum[(cd.tblk_base + bfirst) * per + r] = t;
        } else {                                                // th == 512, one sum per block
          acc += s4;
          if (r & 1) {
            const float t = wave_sum(acc);
            if (lane == 0) bsum[cd.tblk_base + bfirst + (r >> 1)] = t;
            acc = 0.f;
          }
        }
      }
    }
    nf = __any(nf);
    if (lane == 0 && nf) atomicOr(&info[clip].nonfinite, 1u);
    return;
  }

  // general route (clip head and tail, int16 input, unaligned packing): same order of additions as above --
  // lane l takes samples 4l .. 4l+3 of every 256-sample run -- so the sums, and everything derived from them,
  // do not depend on how the clips were packed.
  for (int k = 0; k < kTrimPerWave; ++k) {
    const int64_t b = bfirst + k;
    if (b >= nb) break;
    const int64_t i0 = b * th;
    const int64_t i1 = (i0 + th < N) ? i0 + th : N;
    float* const dst = bsum + (cd.tblk_base + b) * per;
    float sum = 0.f;
    int j = 0;
    for (int64_t r0 = i0; r0 < i1; r0 += 256, ++j) {
      const int64_t i = r0 + 4 * lane;
      float y0 = 0.f, y1 = 0.f, y2 = 0.f, y3 = 0.f, prev = 0.f;
      if (i < i1) y0 = ld_sample(samples, kp.fmt, cd.off + i);
      if (i + 1 < i1) y1 = ld_sample(samples, kp.fmt, cd.off + i + 1);
      if (i + 2 < i1) y2 = ld_sample(samples, kp.fmt, cd.off + i + 2);
      if (i + 3 < i1) y3 = ld_sample(samples, kp.fmt, cd.off + i + 3);
      if (i > 0 && i < i1) prev = ld_sample(samples, kp.fmt, cd.off + i - 1);
      nf |= !(isfinite(y0) && isfinite(y1) && isfinite(y2) && isfinite(y3));
      float s4;
      if (pre && (i == 0 || i + 3 >= i1)) {                     // clip sample 0 / the clip end inside this quad
        float v0 = preemph1(y0, prev, b1), v1 = preemph1(y1, y0, b1), v2 = preemph1(y2, y1, b1), v3 = preemph1(y3, y2, b1);
        if (i == 0) v0 = (N > 1) ? preemph0(y0, y1) : y0;
        v0 = (i < i1) ? v0 : 0.f; v1 = (i + 1 < i1) ? v1 : 0.f;
        v2 = (i + 2 < i1) ? v2 : 0.f; v3 = (i + 3 < i1) ? v3 : 0.f;
        s4 = sumsq4(v0, v1, v2, v3);
      } else {
        s4 = sq4(y0, y1, y2, y3, prev, pre, b1);
      }
      if (per > 1) {                       // th == 256 * per: this run is sub-block j
        s4 = wave_sum(s4);
        if (lane == 0) dst[j] = s4;
      } else {
        sum += s4;
      }
    }
    if (per > 1) {                         // a short last block: its missing sub-blocks are empty
      for (int kk = j; kk < per; ++kk) if (lane == 0) dst[kk] = 0.f;
    } else {
      sum = wave_sum(sum);
      if (lane == 0) dst[0] = sum;
    }
  }
  nf = __any(nf);
  if (lane == 0 && nf) atomicOr(&info[clip].nonfinite, 1u);
}

// ---------------------------------------------------------------------------
// k_trim_decide: one workgroup per clip
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_trim_decide(const ClipDesc* __restrict__ clips,
                                                     ClipInfo* __restrict__ info,
                                                     const float* __restrict__ bsum,
                                                     BlockDesc* __restrict__ blocks,
                                                     float* __restrict__ rms_rows, KParams kp,
                                                     const void* __restrict__ samples) {
  __shared__ float red_f[4];
  __shared__ long long red_a[4], red_b[4];
  const int clip = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const ClipDesc cd = clips[clip];
  const int64_t N = cd.len;
  int status = AFX_CLIP_OK;
  if (N < 2) status = AFX_CLIP_TOO_SHORT;
  else if (info[clip].nonfinite) status = AFX_CLIP_NONFINITE;
  int64_t start = 0, end = N;
  if ((kp.flags & AFX_FLAG_TRIM) && status == AFX_CLIP_OK) {   // uniform per workgroup
    const int per = kp.rms_sub > 0 ? kp.rms_sub : 1;
    trim_search(bsum + cd.tblk_base * per, N, kp, per, red_f, red_a, red_b, false, start, end);
  }
  const int T = (int)(1 + (end - start) / kp.hop);
  if (status == AFX_CLIP_OK && T < 9) status = AFX_CLIP_TOO_SHORT;   // librosa.feature.delta width 9
  if (tid == 0) {
    ClipInfo ci;
    ci.start = start; ci.end = end; ci.T = T; ci.status = status; ci.lmax_ord = 0u;
    ci.nonfinite = info[clip].nonfinite;
    info[clip] = ci;
  }
  // RMS rows from the sub-block sums
  // (also for a clip too short for the width-9 delta: extract_energy only needs librosa.feature.rms, F:164)
  if (kp.rms_sub > 0 && rms_rows && (status == AFX_CLIP_OK || (status == AFX_CLIP_TOO_SHORT && N >= 2)))
    trim_rms_rows(bsum + cd.tblk_base * kp.rms_sub, start, end, T, kp, rms_rows + cd.frame_base);
  // Shapes whose RMS rows come from the frame kernel (rms_sub == 0): a clip too short for the width-9 delta is skipped
  // by that kernel (inactive blocks), but extract_energy only calls librosa.feature.rms (F:164) and must still get its
  // statistics -- its fewer than nine frames are summed here, straight from the samples.
  if (kp.rms_sub == 0 && rms_rows && samples && status == AFX_CLIP_TOO_SHORT && N >= 2 && T >= 1) {
    const bool pre = (kp.flags & AFX_FLAG_PREEMPH) != 0;
    const float inv_n = 1.0f / (float)kp.n_fft;
    for (int t = wave; t < T; t += 4) {
      float acc = 0.f;
      for (int j = lane; j < kp.n_fft; j += 64) {
        const int64_t i = start + (int64_t)t * kp.hop - kp.n_fft / 2 + j;
        float v = 0.f;
        if (i >= start && i < end) {
          const float y = ld_sample(samples, kp.fmt, cd.off + i);
          v = y;
          if (pre) v = (i == 0) ? preemph0(y, ld_sample(samples, kp.fmt, cd.off + 1))
                                : preemph1(y, ld_sample(samples, kp.fmt, cd.off + i - 1), kp.preemph_b1);
        }
        acc = fmaf(v, v, acc);
      }
      acc = wave_sum(acc);
      if (lane == 0) rms_rows[cd.frame_base + t] = sqrtf(acc * inv_n);
    }
  }
  // block descriptors of this clip for k_frames
  for (int fb = tid; fb < cd.tpad / kFramesPerBlock; fb += 256) {
    const int t0 = fb * kFramesPerBlock;
    const int64_t g0 = start + (int64_t)t0 * kp.hop - kp.n_fft / 2;
    blocks[cd.blk_base + fb] = make_block(cd, clip, g0, t0, start, end, N, t0, T, status == AFX_CLIP_OK && t0 < T, 0, 0);
  }
}

hipError_t launch_trim_blocks(hipStream_t s, const void* samples, const ClipDesc* clips, ClipInfo* info,
                              float* bsum, int n_clips, int max_tblocks, const KParams& kp) {
  dim3 grid((max_tblocks + 4 * kTrimPerWave - 1) / (4 * kTrimPerWave), n_clips);
  hipLaunchKernelGGL(k_trim_blocks, grid, dim3(256), 0, s, samples, clips, info, bsum, kp);
  return hipGetLastError();
}

hipError_t launch_trim_decide(hipStream_t s, const ClipDesc* clips, ClipInfo* info, const float* bsum,
                              BlockDesc* blocks, float* rms_rows, int n_clips, const KParams& kp, const void* samples) {
  hipLaunchKernelGGL(k_trim_decide, dim3(n_clips), dim3(256), 0, s, clips, info, bsum, blocks, rms_rows, kp, samples);
  return hipGetLastError();
}

}  // namespace afx
