// Device-side pieces of the 2048 / 512 STFT that afx_hpss.hip and afx_denoise.hip share: the 1024-point complex FFT of one
// wave's LDS image and the two halves of the real-FFT split (forward: Z -> X, inverse: X -> conj Z').
// Include from .hip files only.
#pragma once
#include <hip/hip_runtime.h>

#include "afx_frames3_dev.h"
#include "afx_hpss.h"

namespace afx {

__device__ __forceinline__ v2 hp_cmul(v2 a, v2 b) { return v2{a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x}; }

// forward 1024-point complex FFT of buf (one wave's 1024 float2 in LDS), natural order in and out: five radix-4 Stockham
// stages, four butterflies per lane.  Every wave of the workgroup calls it (the exchanges use workgroup barriers).
__device__ __forceinline__ void hp_fft1024(v2* buf, const v2* __restrict__ w1024, int lane) {
#pragma unroll
  for (int st = 0; st < 5; ++st) {
    const int ns = 1 << (2 * st), ts = 256 >> (2 * st);
    __syncthreads();
    v2 v[4][4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int j = lane + 64 * q, k = j & (ns - 1);
#pragma unroll
      for (int r = 0; r < 4; ++r) v[q][r] = buf[j + 256 * r];
      if (st > 0) {
#pragma unroll
        for (int r = 1; r < 4; ++r) v[q][r] = hp_cmul(v[q][r], w1024[r * k * ts]);
      }
      f3_dft4(v[q][0], v[q][1], v[q][2], v[q][3]);
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int j = lane + 64 * q, k = j & (ns - 1), base = (j - k) * 4 + k;
#pragma unroll
      for (int r = 0; r < 4; ++r) buf[base + r * ns] = v[q][r];
    }
  }
  __syncthreads();
}

// real-FFT split: X[k] = (Z[k] + conj Z[N-k]) / 2 - i W2048^k (Z[k] - conj Z[N-k]) / 2, zk = Z[k], zn = Z[(N - k) mod N],
// w = W2048^k, k < 1024 (bin 1024 is Z[0].x - Z[0].y)
__device__ __forceinline__ v2 hp_split(v2 zk, v2 zn, v2 w) {
  const v2 A = v2{zk.x + zn.x, zk.y - zn.y} * 0.5f;
  const v2 B = v2{zk.x - zn.x, zk.y + zn.y} * 0.5f;
  const v2 wb = hp_cmul(w, B);
  return v2{A.x + wb.y, A.y - wb.x};
}

// its inverse, conjugated: conj Z'[k], Z'[k] = (X[k] + conj X[N-k]) + i conj(W2048^k) (X[k] - conj X[N-k]), xk = X[k],
// xn = X[1024 - k] (for k = 0 the caller clears both imaginary parts, as numpy's irfft ignores them).  The forward FFT of
// conj Z' is the conjugate of the inverse.
__device__ __forceinline__ v2 hp_merge(v2 xk, v2 xn, v2 w) {
  const v2 e = v2{xk.x + xn.x, xk.y - xn.y}, d = v2{xk.x - xn.x, xk.y + xn.y};
  const v2 o = hp_cmul(d, v2{w.x, -w.y});
  return v2{e.x - o.y, -(e.y + o.x)};
}

}  // namespace afx
