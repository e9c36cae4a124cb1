// The trim decision's device functions, shared by k_trim_decide and k_trim_decide3 (afx_trim.hip): librosa.effects.trim's
// threshold search over the sums of squares k_trim_blocks or a speculative frame pass left in bsum, and the RMS rows
// from the same sums.  Include from .hip files only.
#pragma once
#include "afx_device.h"
#include "afx_wave.h"

namespace afx {

// RMS of trim frame t (trim_frame samples centred on t * trim_hop); bs holds `per` sums per trim block
__device__ __forceinline__ float trim_frame_rms(const float* bs, int64_t t, int64_t nb, int half, int per, float inv_n) {
  float s = 0.f;
  for (int64_t b = (t - half) * per; b < (t + half) * per; ++b)
    if (b >= 0 && b < nb * per) s += bs[b];
  return sqrtf(s * inv_n);
}

// librosa.effects.trim(top_db) of one clip of N samples by a 256-thread workgroup (feature_extractor.py:72): the kept
// span [start, end), 0 .. 0 when no frame reaches the threshold.  bs: the clip's sums, `per` per trim block.  Call it
// under a workgroup-uniform condition.  reuse_red_f: the caller writes red_f again afterwards, so the merged maximum is
// read under a barrier of its own.
__device__ __forceinline__ void trim_search(const float* bs, int64_t N, const KParams& kp, int per, float* red_f,
                                            long long* red_a, long long* red_b, bool reuse_red_f, int64_t& start, int64_t& end) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int th = kp.trim_hop, half = (kp.trim_frame / th) / 2;
  const int64_t nb = (N + th - 1) / th, nt = 1 + N / th;
  const float inv_n = 1.0f / (float)kp.trim_frame;
  float mx = 0.f;
  for (int64_t t = tid; t < nt; t += 256) mx = fmaxf(mx, trim_frame_rms(bs, t, nb, half, per, inv_n));
  mx = wave_max(mx);
  if (lane == 0) red_f[wave] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(red_f[0], red_f[1]), fmaxf(red_f[2], red_f[3]));
  if (reuse_red_f) __syncthreads();
  // amplitude_to_db(mse, ref=np.max, amin=1e-5, top_db=None), float32
  const float ref_db = 10.0f * log10f(fmaxf(1e-10f, mx * mx));
  long long first = (long long)1 << 62, last = -1;
  for (int64_t t = tid; t < nt; t += 256) {
    const float r = trim_frame_rms(bs, t, nb, half, per, inv_n);
    const float db = 10.0f * log10f(fmaxf(1e-10f, r * r)) - ref_db;
    if (db > -kp.trim_top_db) { if (t < first) first = t; if (t > last) last = t; }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const long long f2 = __shfl_xor(first, o), l2 = __shfl_xor(last, o);
    first = f2 < first ? f2 : first; last = l2 > last ? l2 : last;
  }
  if (lane == 0) { red_a[wave] = first; red_b[wave] = last; }
  __syncthreads();
  first = red_a[0]; last = red_b[0];
#pragma unroll
  for (int w = 1; w < 4; ++w) { first = red_a[w] < first ? red_a[w] : first; last = red_b[w] > last ? red_b[w] : last; }
  if (last >= 0) {
    start = first * th;
    end = (last + 1) * th < N ? (last + 1) * th : N;
  } else { start = 0; end = 0; }
}

// RMS rows from the sub-block sums (feature_extractor.py:164, librosa.feature.rms center=True): frame t
// covers kept samples [start + t*hop - n_fft/2, + n_fft); start is a multiple of the sub-block (= hop),
// `end` is a multiple of it or the clip end, so the frame is a run of whole sub-blocks clipped to the kept span.
// bs: the clip's sums, one per hop; rows: the clip's first RMS row.
__device__ __forceinline__ void trim_rms_rows(const float* bs, int64_t start, int64_t end, int T, const KParams& kp, float* rows) {
  const int64_t s_lo = start / kp.hop, s_hi = (end + kp.hop - 1) / kp.hop;
  const int nsb = kp.n_fft / kp.hop, back = nsb / 2;
  const float inv_n = 1.0f / (float)kp.n_fft;
  for (int t = threadIdx.x; t < T; t += 256) {
    float sacc = 0.f;
    for (int k = 0; k < nsb; ++k) {
      const int64_t sb = s_lo + t - back + k;
      if (sb >= s_lo && sb < s_hi) sacc += bs[sb];
    }
    rows[t] = sqrtf(sacc * inv_n);
  }
}

}  // namespace afx
