// Device primitives every kernel file of libafx.so shares: DPP moves, wave reductions, the order-preserving float image,
// pre-emphasis as scipy.signal.lfilter rounds it, sample loads by format.  These bodies hold the rounding rules parity
// rests on (fp contract(off), bit-cast not convert), so each exists once, here.  Include from .hip files only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "afx.h"

namespace afx {

// DPP move of a float / an int: lane <- the lane `ctrl` names (0xB1 quad_perm [1,0,3,2], 0x4E quad_perm [2,3,0,1], 0x141
// row_half_mirror, 0x140 row_mirror, 0x124 / 0x128 row_ror 4 / 8).  bc = bound_ctrl: where every lane has a source it
// changes nothing but spares the v_mov_b32 that would otherwise initialise the destination with the `old` value (0).
#define AFX_DPP_I(v, ctrl, bc) __builtin_amdgcn_update_dpp(0, (v), (ctrl), 0xf, 0xf, (bc))
#define AFX_DPP_F(v, ctrl, bc) __int_as_float(AFX_DPP_I(__float_as_int(v), ctrl, bc))

// Wave-wide reductions without LDS: DPP butterflies inside each 16-lane row, then one readlane per
// row (__shfl_xor would lower to six dependent ds_bpermute round trips).
template <typename Op>
__device__ __forceinline__ float row_reduce(float v, Op op) {      // every lane ends with its row's total
  v = op(v, AFX_DPP_F(v, 0xB1, false));     // quad_perm [1,0,3,2]
  v = op(v, AFX_DPP_F(v, 0x4E, false));     // quad_perm [2,3,0,1]
  v = op(v, AFX_DPP_F(v, 0x141, false));    // row_half_mirror
  v = op(v, AFX_DPP_F(v, 0x140, false));    // row_mirror
  return v;
}
// row r's total of a row_reduce result, as a uniform value (readlane is an int builtin: bit-cast, do not convert)
__device__ __forceinline__ float row_total(float v, int r) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 16 * r));
}
template <typename Op>
__device__ __forceinline__ float wave_reduce(float v, Op op) {     // uniform result: (r0 op r1) op (r2 op r3)
  v = row_reduce(v, op);
  const float r0 = row_total(v, 0), r1 = row_total(v, 1), r2 = row_total(v, 2), r3 = row_total(v, 3);
  return op(op(r0, r1), op(r2, r3));
}
struct OpAdd { __device__ float operator()(float a, float b) const { return a + b; } };
struct OpMax { __device__ float operator()(float a, float b) const { return fmaxf(a, b); } };
struct OpMin { __device__ float operator()(float a, float b) const { return fminf(a, b); } };
__device__ __forceinline__ float wave_sum(float v) { return wave_reduce(v, OpAdd()); }
__device__ __forceinline__ float wave_max(float v) { return wave_reduce(v, OpMax()); }
__device__ __forceinline__ float wave_min(float v) { return wave_reduce(v, OpMin()); }
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// order-preserving uint image of a float (atomicMax on floats of either sign) and back
__device__ __forceinline__ uint32_t f2ord(float f) {
  uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ord2f(uint32_t o) {
  uint32_t u = (o & 0x80000000u) ? (o & 0x7fffffffu) : ~o;
  return __uint_as_float(u);
}

// out[n] = y[n] + b1*y[n-1] exactly as scipy.signal.lfilter evaluates it in
// float32: the product is rounded, then the sum (no FMA contraction).
__device__ __forceinline__ float preemph1(float y, float prev, float b1) {
#pragma clang fp contract(off)   // HIP's __fmul_rn/__fadd_rn are plain * and + and would fuse
  const float p = b1 * prev;
  return y + p;
}
// librosa's default zi = 2*y[0] - y[1]  ->  out[0] = zi + y[0]
__device__ __forceinline__ float preemph0(float y0, float y1) {
#pragma clang fp contract(off)
  const float t = 2.0f * y0;
  const float zi = t - y1;
  return zi + y0;
}

// sample idx of the packed buffer as float32; int16 is scaled by 1 / 32768 as libsndfile does
__device__ __forceinline__ float ld_sample(const void* samples, int fmt, int64_t idx) {
  if (fmt == AFX_FMT_S16) return (float)((const int16_t*)samples)[idx] * (1.0f / 32768.0f);
  return ((const float*)samples)[idx];
}
// the same with the format known at compile time: by 64-bit element index, and as a row load -- typed base pointer
// (wave-uniform) + 32-bit lane offset (global_load ... s[base] offset:imm)
template <int FMT> using sample_of = typename std::conditional<FMT == AFX_FMT_S16, int16_t, float>::type;
template <int FMT>
__device__ __forceinline__ float ld_raw(const void* samples, int64_t idx) {
  if constexpr (FMT == AFX_FMT_S16) return (float)((const int16_t*)samples)[idx] * (1.0f / 32768.0f);
  else return ((const float*)samples)[idx];
}
template <int FMT>
__device__ __forceinline__ float ld_row(const sample_of<FMT>* base, unsigned idx) {
  if constexpr (FMT == AFX_FMT_S16) return (float)base[idx] * (1.0f / 32768.0f);
  else return base[idx];
}

}  // namespace afx
