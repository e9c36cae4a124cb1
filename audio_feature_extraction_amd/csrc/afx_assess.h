// The recording screen and the denoising scores (afx_assess.hip, afx_assess_host.cpp): the per-clip reductions of
// 00_audio_data_collection_experiment/audio_format_assessment.py:143-300 (detect_silence, check_volume_levels,
// check_amplitude_stability, estimate_snr) and the sums behind audio_quality_assessment.py:150-280 (SNR of the difference,
// Pearson correlation, MSE).  Records, geometry, the cost record and the launchers.  Internal to libafx.so; include/afx.h
// (afx_assess_batch, afx_compare_batch) is the ABI.
//
// Work layout.  A clip is cut into spans of kAsSpan samples from its own sample 0, one workgroup per span, whatever else
// the batch holds.  The workgroup reads its span from HBM once into LDS and leaves
//   - one record per span: max |y|, whether a sample was NaN / inf, the span's share of the noise window's sum of squares;
//   - for each of the two framings one float64 sum of squares per PIECE, a piece being the part of one frame that lies in
//     one span.  Frame t = (j + fl / 2) / fl of sample j and span i = j / kAsSpan both grow with j, and from one piece to
//     the next at least one of them grows by one, so piece (t, i) has the slot t + i to itself; a frame's pieces are
//     adjacent slots.  The two framings share nothing but the LDS image: every sample is in one piece of each.
// Frame as_frames(len, fl), which librosa does not have, collects the samples behind the last frame (centred frames of hop fl
// cover [0, frames fl - fl / 2) only), so that the short framing's pieces also add up to the clip's sum of squares.
// A second kernel, one workgroup per clip, adds the pieces of each frame in increasing span order and does everything
// that needs the whole clip: the maximum, the threshold decisions, the run scan, mean and deviation.
#pragma once
#include <cstdint>

#include "afx.h"
#include "afx_hpss.h"

namespace afx {

constexpr int kAsLanes = 256;                 // lanes of a workgroup of either kernel
constexpr int kAsSpanLog = 12;
constexpr int kAsSpan = 1 << kAsSpanLog;      // samples per workgroup: 16 per lane, 16 KiB of LDS
constexpr int kAsWide = 1024;                 // frames at least this long: the whole workgroup sums a piece
constexpr int kAsNarrow = 64;                 // frames shorter than this: one lane sums a piece; between: one wave
constexpr int kCmpSpanDoubles = 10;           // per span of a pair: the six raw sums, the three centred ones, the non-finite flag

// one clip as the kernels see it
struct AsClip {
  int64_t in_off;       // element offset of sample 0 in the buffer the kernels read
  int64_t len;          // samples, >= 1
  int64_t nw;           // samples of the noise window: min(int(0.1 len), noise_cap)
  int64_t ps_off;       // first slot of the short framing's pieces in the chunk's piece buffer
  int64_t pl_off;       // ... of the long framing's
  int64_t span_base;    // first span (= workgroup) of the clip in the chunk
  int32_t fs, fl;       // frame_short, frame_long
};
static_assert(sizeof(AsClip) == 56, "AsClip layout");

struct AsSpan {
  double noise;         // sum of y^2 over the span's part of the noise window
  float peak;           // max |y|
  uint32_t bad;         // a NaN / inf sample
};
static_assert(sizeof(AsSpan) == 16, "AsSpan layout");

// one pair of afx_compare_batch
struct CmpPair {
  int64_t r_off, d_off; // element offsets of the two sides in the buffers the kernel reads
  int64_t n;            // min of the two lengths, >= 1
  int64_t span_base;
};
static_assert(sizeof(CmpPair) == 32, "CmpPair layout");

// frames of librosa.feature.rms(frame_length = hop_length = fl, center=True): fl / 2 zeros on either side, then whole frames;
// 1 + len / fl for an even fl, 1 + (len - 1) / fl for an odd one (len >= 1)
#ifdef __HIPCC__
__host__ __device__
#endif
inline int64_t as_frames(int64_t len, int32_t fl) { return 1 + (len + 2 * (int64_t)(fl / 2) - fl) / fl; }
inline int64_t as_spans(int64_t len) { return (len + kAsSpan - 1) >> kAsSpanLog; }
// slots of one framing of a clip: frames 0 .. as_frames (the collector included) plus spans, never more than needed + 1
inline int64_t as_slots(int64_t len, int32_t fl) { return as_frames(len, fl) + 1 + as_spans(len); }

// What a clip costs a chunk (afx_assess_host.cpp; no device).  what: 0 afx_assess_batch, 1 afx_compare_batch.  The frame
// lengths are the caller's and at least 1, so a clip of L samples has at most L + 2 slots of frames and L / 4096 + 1 of
// spans in each framing: 16 L + 16 L / 4096 + 64 <= 17 L + 64 bytes of pieces, whatever the rates of the batch.
void assess_cost(int what, int sample_fmt, int mem_kind, StftCost& cost);

// the arguments the batch and the host entry points refuse alike; nullptr when there is nothing to refuse
const char* assess_refusal(int64_t len, int32_t frame_short, int32_t frame_long, double threshold_db, int64_t noise_cap);

}  // namespace afx

#ifdef __HIP_PLATFORM_AMD__
#include <hip/hip_runtime_api.h>
namespace afx {
// afx_assess.hip.  n_blocks: spans of the chunk.  thr_ratio: 10^(threshold_db / 10), or -1 when no frame can be silent
// (threshold_db <= -80, the top_db clamp).  rec: AFX_ASSESS_N doubles per clip (NaN for a bad one), bad: 1 per bad clip.
hipError_t launch_assess(hipStream_t s, const void* samples, int sample_fmt, const AsClip* clips, int n_clips, int n_blocks,
                         double thr_ratio, double* pieces, AsSpan* spans, double* rec, int32_t* bad);
// part: kCmpSpanDoubles per span; rec: AFX_COMPARE_N doubles per pair
hipError_t launch_compare(hipStream_t s, const void* ref, const void* deg, int sample_fmt, const CmpPair* pairs, int n_pairs,
                          int n_blocks, double* part, double* rec, int32_t* bad);
}  // namespace afx
#endif
