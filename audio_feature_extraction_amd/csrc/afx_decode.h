// Sample conversion and channel mix-down of raw WAVE data on the device (wavio.to_float32 + wavio.to_mono): the clip
// record and the kernel launcher.  Internal to libafx.so; include/afx.h (afx_decode_batch) is the ABI.
//
// Work layout.  A lane owns 4 consecutive sample frames of one clip.  With bpf bytes per frame (sample bytes times
// channels) those are 4 * bpf bytes = bpf whole 4-byte words from the clip's 16-byte-aligned base, whatever the sample
// width and channel count: the lane loads them with the widest loads that alignment allows (16 bytes when bpf is a multiple
// of 4, 8 when it is even, else 4), converts and mixes in registers and writes its 4 results as one 16-byte store.  A
// workgroup of 256 lanes takes kDcFrames = 1024 consecutive frames; the block -> clip map is the resampler's (a record per
// clip with its first block, found by binary search).  Every (kind, channels) pair is its own fully unrolled code path
// (word and byte positions are compile-time constants: nothing is indexed at run time, nothing spills).
#pragma once
#include <cstdint>

namespace afx {

constexpr int kDcLanes = 256;                  // lanes of a workgroup
constexpr int kDcFrames = 4 * kDcLanes;        // sample frames per workgroup
constexpr int kDcMaxChannels = 7;              // numpy's mean is the sequential sum only below 8 channels

// one clip as k_decode sees it
struct DcClip {
  int64_t in_off;                              // bytes, multiple of 16
  int64_t out_off;                             // floats, multiple of 4
  int64_t frames;
  int32_t kind, channels;                      // AFX_SMP_*, 1 .. kDcMaxChannels
  int32_t first_block, pad_;
};
static_assert(sizeof(DcClip) == 40, "DcClip layout");

inline int decode_sample_bytes(int kind) {     // AFX_SMP_U8 .. AFX_SMP_F64; 0 for an unknown kind
  constexpr int b[6] = {1, 2, 3, 4, 4, 8};
  return kind >= 0 && kind < 6 ? b[kind] : 0;
}

}  // namespace afx

#ifdef __HIP_PLATFORM_AMD__
#include <hip/hip_runtime_api.h>
namespace afx {
// afx_decode.hip
hipError_t launch_decode(hipStream_t s, const void* raw, float* out, const DcClip* clips, int n_clips, int n_blocks);
}  // namespace afx
#endif
