// The trim stage behind a speculative frame pass (afx_frames3*.hip), gfx950:
//   k_trim_decide3   the decision of k_trim_decide (afx_trim.hip) from the sums that pass left; clip maximum over the
//                    blocks the cut leaves untouched, redo items for the ones it touches
//   k_build_blocks3  the speculative pass's block records, from the clip records
// Built with the wave-level frame kernels' compiler flags, as these two kernels always were.
#include <hip/hip_runtime.h>

#include "afx_device.h"
#include "afx_frames3.h"
#include "afx_trim_dev.h"
#include "afx_wave.h"

namespace afx {

// ---------------------------------------------------------------------------
// k_trim_decide3: the trim decision AFTER the speculative frame pass.  One workgroup per clip:
//   * librosa.effects.trim(top_db) on the sub-block sums k_frames3<SPEC> left in bsum (feature_extractor.py:72), the
//     search k_trim_decide runs (trim_search) -> [start, end), T, status; RMS rows from the same sums (:164);
//   * the clip's log-mel maximum (power_to_db's top_db reference) over the blocks the cut leaves untouched;
//   * the frames the cut does touch -- the two frames whose window crosses `start`, the two that cross `end`, and
//     the rest of their 16-frame blocks (a block maximum cannot be taken apart) -- as a list of up to-16-frame items
//     for the second k_frames3 launch.
// Frame t of the trimmed clip is absolute frame start / hop + t: later kernels read the spill at that offset.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_trim_decide3(const ClipDesc* __restrict__ clips, ClipInfo* __restrict__ info,
                                                      const float* __restrict__ bsum, const float* __restrict__ blockmax,
                                                      BlockDesc* __restrict__ items, int* __restrict__ n_items, int max_items,
                                                      float* __restrict__ rms_rows, KParams kp) {
  __shared__ float red_f[4];
  __shared__ long long red_a[4], red_b[4];
  const int clip = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const ClipDesc cd = clips[clip];
  const int64_t N = cd.len;
  const uint32_t nonfinite = info[clip].nonfinite;
  int status = AFX_CLIP_OK;
  if (N < 2) status = AFX_CLIP_TOO_SHORT;
  else if (nonfinite) status = AFX_CLIP_NONFINITE;
  int64_t start = 0, end = N;
  const int per = kp.rms_sub;
  if ((kp.flags & AFX_FLAG_TRIM) && status == AFX_CLIP_OK)     // uniform per workgroup
    trim_search(bsum + cd.tblk_base * per, N, kp, per, red_f, red_a, red_b, true, start, end);   // red_f is written again below
  const int hop = kp.hop;
  const int T = (int)(1 + (end - start) / hop);
  if (status == AFX_CLIP_OK && T < 9) status = AFX_CLIP_TOO_SHORT;   // librosa.feature.delta width 9
  // ---- which blocks of the speculative pass stand
  const int g0 = (int)(start / hop), glast = g0 + T - 1;
  const int nblk = cd.tpad / kFramesPerBlock;
  const bool cutL = start > 0, cutR = end < N;
  const int bLo = cutL ? (g0 + 2 + 15) >> 4 : 0;
  const int bHi = cutR ? (glast >= 17 ? (glast - 17) >> 4 : -1) : nblk - 1;
  float cm = -INFINITY;
  if (status == AFX_CLIP_OK)
    for (int b = bLo + tid; b <= bHi; b += 256) cm = fmaxf(cm, blockmax[cd.blk_base + b]);
  cm = wave_max(cm);
  if (lane == 0) red_f[wave] = cm;
  __syncthreads();
  cm = fmaxf(fmaxf(red_f[0], red_f[1]), fmaxf(red_f[2], red_f[3]));
  if (tid == 0) {
    ClipInfo ci;
    ci.start = start; ci.end = end; ci.T = T; ci.status = status;
    ci.lmax_ord = cm > -INFINITY ? f2ord(cm) : 0u;
    ci.nonfinite = nonfinite;
    info[clip] = ci;
    // ---- frames to redo: [g0, 16 bLo) on a cut left side, [16 (bHi + 1), glast] on a cut right side
    if (status == AFX_CLIP_OK && (cutL || cutR)) {
      int r0[2], r1[2], nr = 0;
      if (bLo > bHi) { r0[0] = g0; r1[0] = glast + 1; nr = 1; }
      else {
        if (cutL && 16 * bLo > g0) { r0[nr] = g0; r1[nr] = 16 * bLo < glast + 1 ? 16 * bLo : glast + 1; ++nr; }
        if (cutR && 16 * (bHi + 1) <= glast) { r0[nr] = 16 * (bHi + 1) > g0 ? 16 * (bHi + 1) : g0; r1[nr] = glast + 1; ++nr; }
      }
      int cnt = 0;
      for (int r = 0; r < nr; ++r) cnt += (r1[r] - r0[r] + 15) / 16;
      if (cnt > 0) {
        const int at = atomicAdd(n_items, cnt);
        int k = 0;
        for (int r = 0; r < nr; ++r)
          for (int gf = r0[r]; gf < r1[r]; gf += 16, ++k) {
            if (at + k >= max_items) break;                 // cannot happen: the list holds 6 items per clip
            const int nfr = r1[r] - gf < 16 ? r1[r] - gf : 16;
            items[at + k] = make_block(cd, clip, (int64_t)gf * hop - kp.n_fft / 2, gf, start, end, N, 0, nfr, true, 0, 0);
          }
      }
    }
  }
  // ---- RMS rows from the sub-block sums, trimmed frame index
  if (rms_rows && (status == AFX_CLIP_OK || (status == AFX_CLIP_TOO_SHORT && N >= 2)))      // extract_energy needs no delta
    trim_rms_rows(bsum + cd.tblk_base * per, start, end, T, kp, rms_rows + cd.frame_base);
}

// ---------------------------------------------------------------------------
// k_build_blocks3: the speculative launch's block list, built on the device from the batch's clip records.
// reference call site: audio_feature_extraction_toolkit/core/feature_extractor.py:228-235 -- batch_process never sees the
// same clip lengths twice, so nothing per batch may be built block by block on the host: the host uploads one 48-byte
// ClipDesc per clip and this kernel writes the 64-byte record of every absolute 16-frame block (one wave per clip).  54 000 records (3.5 MB) for 1000 ten-second clips.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_build_blocks3(const ClipDesc* __restrict__ clips, int n_clips,
                                                      BlockDesc* __restrict__ blocks, int n_fft, int hop, int trim_hop, int per) {
  // one wave per clip: its record is read once (scalar), its blocks written lane by lane -- no search for the clip of a block
  const int clip = blockIdx.x;
  if (clip >= n_clips) return;
  const ClipDesc c = clips[clip];
  const int nb = c.tpad / kFramesPerBlock;
  const int64_t ntb = (c.len + trim_hop - 1) / trim_hop;
  for (int b = threadIdx.x; b < nb; b += 64) {
    const int64_t gs = (int64_t)b * kFramesPerBlock * hop - n_fft / 2;       // clip sample of staged index 0
    const int t0 = b * kFramesPerBlock;
    blocks[c.blk_base + b] = make_block(c, clip, gs, t0, 0, c.len, c.len, t0, c.tmax, c.len >= 2 && t0 < c.tmax,
                                        (int32_t)(c.tblk_base * per), (int32_t)(ntb * per));
  }
}

hipError_t launch_build_blocks3(hipStream_t s, const ClipDesc* clips, int n_clips, int nblocks, BlockDesc* blocks,
                                const KParams& kp) {
  if (nblocks <= 0 || n_clips <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_build_blocks3, dim3(n_clips), dim3(64), 0, s, clips, n_clips, blocks,
                     kp.n_fft, kp.hop, kp.trim_hop, kp.rms_sub);
  return hipGetLastError();
}

hipError_t launch_trim_decide3(hipStream_t s, const ClipDesc* clips, ClipInfo* info, const float* bsum, const float* blockmax,
                               BlockDesc* items, int* n_items, int max_items, float* rms_rows, int n_clips, const KParams& kp) {
  hipLaunchKernelGGL(k_trim_decide3, dim3(n_clips), dim3(256), 0, s, clips, info, bsum, blockmax, items, n_items, max_items,
                     rms_rows, kp);
  return hipGetLastError();
}

}  // namespace afx
