// The small kernels of libafx.so (gfx950) around the pipeline: k_preemph (preprocess_audio's signal itself), k_f0_prep
// (the signal librosa.pyin is handed) and k_finish (the last kernel of a batch).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "afx_device.h"
#include "afx_f0.h"
#include "afx_wave.h"

namespace afx {

// preprocess_audio(y): the pre-emphasised signal itself (F:69), one clip
__global__ __launch_bounds__(256) void k_preemph(const float* __restrict__ y, float* __restrict__ out,
                                                 int64_t n, float b1) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  out[i] = (i == 0) ? ((n > 1) ? preemph0(y[0], y[1]) : y[0]) : preemph1(y[i], y[i - 1], b1);
}

constexpr int kF0PrepPerThread = 8;
// extract_f0 staging: the preprocessed signal itself (pre-emphasised, trimmed span moved to the clip's
// offset) as float32 -- what the reference hands to librosa.pyin (feature_extractor.py:195).
__global__ __launch_bounds__(256) void k_f0_prep(const void* __restrict__ samples,
                                                 const ClipDesc* __restrict__ clips,
                                                 const ClipInfo* __restrict__ info,
                                                 float* __restrict__ ysig, KParams kp) {
  const int clip = blockIdx.y;
  const ClipInfo ci = info[clip];
  const ClipDesc cd = clips[clip];
  const int64_t np = ci.end - ci.start;
  const bool pre = (kp.flags & AFX_FLAG_PREEMPH) != 0;
  // a workgroup takes kF0PrepPerThread runs of 256 consecutive samples (a wave per sample and a workgroup per 256 of them was
  // bound by the number of workgroups: 3.4 M waves for 1000 ten-second clips, 0.68 ms for 1.8 GB of traffic)
  for (int64_t n0 = (int64_t)blockIdx.x * (256 * kF0PrepPerThread); n0 < np; n0 += (int64_t)gridDim.x * (256 * kF0PrepPerThread)) {
#pragma unroll
    for (int u = 0; u < kF0PrepPerThread; ++u) {
      const int64_t n = n0 + u * 256 + threadIdx.x;
      if (n >= np) break;
      const int64_t i = ci.start + n;
      const float y = ld_sample(samples, kp.fmt, cd.off + i);
      float v = y;
      if (pre) {
        if (i == 0) v = (cd.len > 1) ? preemph0(y, ld_sample(samples, kp.fmt, cd.off + 1)) : y;
        else v = preemph1(y, ld_sample(samples, kp.fmt, cd.off + i - 1), kp.preemph_b1);
      }
      ysig[cd.off + n] = v;
    }
  }
}

// k_finish: the last kernel of a batch.  Clears what the next batch expects cleared (the clip records and the list /
// ticket counters: two fill commands less in front of every batch), then stores the batch's sequence number to a
// completion flag in host memory the device can write -- the host can spin on that word instead of asking the
// runtime (hipEventSynchronize on a stream that already holds the next batch's commands was measured to return late).
__global__ __launch_bounds__(1024) void k_finish(uint4* info, int n_info16, int* counters, unsigned* flag, unsigned seq) {
  for (int i = threadIdx.x; i < n_info16; i += 1024) info[i] = uint4{0u, 0u, 0u, 0u};
  if (counters && threadIdx.x < 4) counters[threadIdx.x] = 0;
  __syncthreads();
  if (flag && threadIdx.x == 0) __hip_atomic_store(flag, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
hipError_t launch_finish(hipStream_t s, ClipInfo* info, int n_clips, int* counters, unsigned* flag_dev, unsigned seq) {
  static_assert(sizeof(ClipInfo) == 32, "k_finish clears ClipInfo as two 16-byte words");
  hipLaunchKernelGGL(k_finish, dim3(1), dim3(1024), 0, s, (uint4*)info, n_clips * 2, counters, flag_dev, seq);
  return hipGetLastError();
}

hipError_t launch_preemph(hipStream_t s, const float* y, float* out, int64_t n, float b1) {
  hipLaunchKernelGGL(k_preemph, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, y, out, n, b1);
  return hipGetLastError();
}

hipError_t launch_f0_prep(hipStream_t s, const void* samples, const ClipDesc* clips, const ClipInfo* info,
                          float* ysig, int n_clips, int64_t max_len, const KParams& kp) {
  const int64_t per_wg = 256 * kF0PrepPerThread;
  const int gx = (int)std::min<int64_t>(std::max<int64_t>((max_len + per_wg - 1) / per_wg, 1), 1024);
  hipLaunchKernelGGL(k_f0_prep, dim3(gx, n_clips), dim3(256), 0, s, samples, clips, info, ysig, kp);
  return hipGetLastError();
}

}  // namespace afx
