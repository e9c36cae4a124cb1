// Sample conversion and channel mix-down for gfx950 (layout: afx_decode.h; arithmetic: include/afx.h, afx_decode_batch).
// A streaming kernel: every input byte is read once, every output written once by one lane; no LDS, no atomics.
#include <hip/hip_runtime.h>

#include "afx.h"
#include "afx_decode.h"

namespace afx {

// clip records are read at the same address by every lane of a workgroup: through the constant address space, as scalar loads
template <typename T> using dc_const = const __attribute__((address_space(4))) T*;

// the clip whose block range holds block b: the last clip with first_block <= b (clips without blocks share their
// successor's first_block and are never chosen)
__device__ __forceinline__ int dc_find_clip(dc_const<DcClip> clips, int n_clips, int b) {
  int lo = 0, hi = n_clips - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (clips[mid].first_block <= b) lo = mid; else hi = mid - 1;
  }
  return lo;
}

constexpr int dc_bytes(int kind) {
  return kind == AFX_SMP_U8 ? 1 : kind == AFX_SMP_S16 ? 2 : kind == AFX_SMP_S24 ? 3 : kind == AFX_SMP_F64 ? 8 : 4;
}

// sample s of the lane's words as float32 (s is a constant once the callers' loops are unrolled).  The scale factors are
// powers of two: whether or not the compiler contracts scale and add into an FMA, the sum is rounded once from the same value.
template <int KIND>
__device__ __forceinline__ float dc_sample(const uint32_t* w, int s) {
  if constexpr (KIND == AFX_SMP_U8) {
    return (float)((int)((w[s >> 2] >> (8 * (s & 3))) & 0xffu) - 128) * 0x1p-7f;
  } else if constexpr (KIND == AFX_SMP_S16) {
    return (float)(int)(int16_t)(w[s >> 1] >> (16 * (s & 1))) * 0x1p-15f;
  } else if constexpr (KIND == AFX_SMP_S24) {
    const int b = 3 * s, d = b >> 2, sh = 8 * (b & 3);
    uint32_t v = w[d] >> sh;
    if (sh > 8) v |= w[d + 1] << (32 - sh);          // the sample crosses into the next word (which the lane holds: 3 s + 3 <= 4 NW)
    return (float)((int32_t)(v << 8) >> 8) * 0x1p-23f;
  } else if constexpr (KIND == AFX_SMP_S32) {
    return (float)(int32_t)w[s] * 0x1p-31f;          // v_cvt_f32_i32: round to nearest even
  } else if constexpr (KIND == AFX_SMP_F32) {
    return __uint_as_float(w[s]);
  } else {
    return (float)__hiloint2double((int)w[2 * s + 1], (int)w[2 * s]);     // v_cvt_f32_f64: nearest even, +-inf beyond float32
  }
}

// frames 4 g .. 4 g + 3 of one clip
template <int KIND, int CH>
__device__ __forceinline__ void dc_lane(const uint8_t* __restrict__ raw, float* __restrict__ out, const DcClip& cl, int64_t g) {
  constexpr int NW = dc_bytes(KIND) * CH;            // 4 frames: 4 * bytes per frame / 4
  constexpr int AL = NW % 4 == 0 ? 16 : NW % 2 == 0 ? 8 : 4;
  const int64_t left = cl.frames - 4 * g;            // >= 1
  const uint32_t* p = (const uint32_t*)(raw + cl.in_off) + g * NW;
  uint32_t w[NW];
  if (left >= 4) {
    __builtin_memcpy(w, __builtin_assume_aligned(p, AL), NW * sizeof(uint32_t));
  } else {                                           // the clip's last lane: only the words that hold its frames
    const int nw = ((int)left * NW + 3) >> 2;        // left * bytes per frame, rounded up to words
#pragma unroll
    for (int d = 0; d < NW; ++d) w[d] = d < nw ? p[d] : 0u;
  }
  float r[4];
#pragma unroll
  for (int f = 0; f < 4; ++f) {
    float a = dc_sample<KIND>(w, f * CH);
#pragma unroll
    for (int c = 1; c < CH; ++c) a += dc_sample<KIND>(w, f * CH + c);
    if constexpr (CH > 1) a = a / (float)CH;         // IEEE division: a reciprocal multiply differs for 3, 5, 6, 7
    r[f] = f < left ? a : 0.0f;
  }
  *(float4*)(out + cl.out_off + 4 * g) = make_float4(r[0], r[1], r[2], r[3]);
}

__global__ void __launch_bounds__(kDcLanes) k_decode(const uint8_t* __restrict__ raw, float* __restrict__ out,
                                                     const DcClip* __restrict__ clips, int n_clips) {
  const int b = blockIdx.x;
  const dc_const<DcClip> cc = (dc_const<DcClip>)(uintptr_t)clips;
  const int c = dc_find_clip(cc, n_clips, b);
  DcClip cl;
  cl.in_off = cc[c].in_off; cl.out_off = cc[c].out_off; cl.frames = cc[c].frames;
  cl.kind = cc[c].kind; cl.channels = cc[c].channels; cl.first_block = cc[c].first_block; cl.pad_ = 0;
  const int64_t g = (int64_t)(b - cl.first_block) * kDcLanes + threadIdx.x;
  if (4 * g >= cl.frames) return;
#define DC_CASE(K, C) case (K) * 8 + (C): dc_lane<K, C>(raw, out, cl, g); break;
#define DC_KIND(K) DC_CASE(K, 1) DC_CASE(K, 2) DC_CASE(K, 3) DC_CASE(K, 4) DC_CASE(K, 5) DC_CASE(K, 6) DC_CASE(K, 7)
  switch (cl.kind * 8 + cl.channels) {               // the same in every lane of the workgroup
    DC_KIND(AFX_SMP_U8) DC_KIND(AFX_SMP_S16) DC_KIND(AFX_SMP_S24) DC_KIND(AFX_SMP_S32) DC_KIND(AFX_SMP_F32) DC_KIND(AFX_SMP_F64)
    default: break;                                  // afx_decode_batch admits no other record
  }
#undef DC_KIND
#undef DC_CASE
}

hipError_t launch_decode(hipStream_t s, const void* raw, float* out, const DcClip* clips, int n_clips, int n_blocks) {
  if (n_blocks <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_decode, dim3(n_blocks), dim3(kDcLanes), 0, s, (const uint8_t*)raw, out, clips, n_clips);
  return hipGetLastError();
}

}  // namespace afx
