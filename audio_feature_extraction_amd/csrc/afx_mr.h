// Mixed-radix real FFT of the frame lengths that are not powers of two (n_fft = 400 at 16 kHz: 25 ms frames, the speech
// front end of 04_feature_extraction_experiment/feature_extraction.py:35-41): the supported set, the radix schedule and
// the butterflies.  One body for the host executor (afx_rfft_host, afx_host.cpp) and the kernel (k_frames_mr,
// afx_frames_mr.hip), so both walk the same passes in the same operation order.
//
// n_fft real samples are taken as N2 = n_fft / 2 complex points z[n] = x[2n] + i x[2n+1]; Z = FFT_N2(z) by Stockham
// autosort passes of radix 3, 5, 4, 8 (in that order: see mr_schedule); X[k] from Z[k] and Z[N2 - k] (mr_split2).
// Pass with radix R after passes of product NS (butterfly j < N2 / R, jm = j mod NS):
//   x[r] = in[j + r * N2 / R] * tw[jm * r * N2 / (NS * R)],  X = DFT_R(x),  out[(j - jm) * R + jm + r * NS] = X[r]
// tw[n] = exp(-2 pi i n / N2) is the plan's table (HostTables::tw); nothing is computed on the fly.
#pragma once
#include <hip/hip_runtime_api.h>

namespace afx {

constexpr int kMrMaxPasses = 8;

// frame_length is accepted iff it is a multiple of 16 in [256, 2048] whose only prime factors are 2, 3 and 5
__host__ __device__ inline bool mr_supported(int n_fft) {
  if (n_fft < 256 || n_fft > 2048 || (n_fft % 16) != 0) return false;
  int n = n_fft;
  while (n % 2 == 0) n /= 2;
  while (n % 3 == 0) n /= 3;
  while (n % 5 == 0) n /= 5;
  return n == 1;
}

struct MrSchedule {
  int n;                       // passes
  unsigned packed;             // radix of pass p in bits [4 p, 4 p + 4): no array, so the device keeps it in registers
  __host__ __device__ int radix(int p) const { return (int)((packed >> (4 * p)) & 15u); }
  __host__ __device__ void push(int r) { packed |= (unsigned)r << (4 * n); ++n; }
};

// N2 (a multiple of 8 with prime factors 2, 3, 5; at most 1024) as passes of radix 3.., 5.., then the power of two 2^k as
// (4 | 4 4) 8..: at most six passes.  n = 0: N2 has another prime factor or is no multiple of 8.
// No radix-2 pass: n_fft is a multiple of 16, so k >= 3, and k mod 3 == 1 means k in {4, 7, 10}, which is 4 4 8..
// Odd radices go first: the first pass writes with stride R, and 2 R dwords with R odd walk all 32 banks (an 8-first
// schedule would put 16 lanes on two bank pairs); the power-of-two passes then run on NS >= 3 contiguous points.
__host__ __device__ inline MrSchedule mr_schedule(int N2) {
  MrSchedule s;
  s.n = 0; s.packed = 0;
  int n = N2;
  while (n % 3 == 0 && s.n < kMrMaxPasses) { s.push(3); n /= 3; }
  while (n % 5 == 0 && s.n < kMrMaxPasses) { s.push(5); n /= 5; }
  int k = 0;
  while (n % 2 == 0) { ++k; n /= 2; }
  if (n == 1 && k % 3 == 1 && k >= 4 && s.n + 2 <= kMrMaxPasses) { s.push(4); s.push(4); k -= 4; }
  else if (n == 1 && k % 3 == 2 && s.n < kMrMaxPasses) { s.push(4); k -= 2; }
  while (n == 1 && k >= 3 && s.n < kMrMaxPasses) { s.push(8); k -= 3; }
  if (n != 1 || k != 0) { s.n = 0; s.packed = 0; }
  return s;
}

struct alignas(8) mrc { float x, y; };     // one complex point (an 8-byte LDS access on the device)

__host__ __device__ inline mrc mr_mk(float x, float y) { mrc r; r.x = x; r.y = y; return r; }
__host__ __device__ inline mrc mr_mul(mrc a, mrc b) { return mr_mk(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__host__ __device__ inline mrc mr_add(mrc a, mrc b) { return mr_mk(a.x + b.x, a.y + b.y); }
__host__ __device__ inline mrc mr_sub(mrc a, mrc b) { return mr_mk(a.x - b.x, a.y - b.y); }
__host__ __device__ inline mrc mr_mi(mrc a) { return mr_mk(a.y, -a.x); }           // a * (-i)

__host__ __device__ inline void mr_dft4(mrc& x0, mrc& x1, mrc& x2, mrc& x3) {
  const mrc a = mr_add(x0, x2), b = mr_sub(x0, x2), c = mr_add(x1, x3), d = mr_mi(mr_sub(x1, x3));
  x0 = mr_add(a, c); x1 = mr_add(b, d); x2 = mr_sub(a, c); x3 = mr_sub(b, d);
}

// forward DFT of R points in place (exp(-2 pi i / R))
template <int R> __host__ __device__ inline void mr_dft(mrc* x);
// radix 2: the butterfly only.  No schedule of the supported set has a radix-2 pass (see mr_schedule), so neither the
// kernel nor the host executor instantiates one; a set widened to multiples of 4 would add the case to their switches.
template <> __host__ __device__ inline void mr_dft<2>(mrc* x) {
  const mrc a = x[0], b = x[1];
  x[0] = mr_add(a, b); x[1] = mr_sub(a, b);
}
template <> __host__ __device__ inline void mr_dft<3>(mrc* x) {
  const float s = 0.86602540378443864676f;                     // sin(2 pi / 3)
  const mrc t = mr_add(x[1], x[2]), d = mr_sub(x[1], x[2]);
  const mrc m = mr_mk(x[0].x - 0.5f * t.x, x[0].y - 0.5f * t.y);
  const mrc q = mr_mk(s * d.y, -s * d.x);                      // -i s d
  x[0] = mr_add(x[0], t); x[1] = mr_add(m, q); x[2] = mr_sub(m, q);
}
template <> __host__ __device__ inline void mr_dft<4>(mrc* x) { mr_dft4(x[0], x[1], x[2], x[3]); }
template <> __host__ __device__ inline void mr_dft<5>(mrc* x) {
  const float c1 = 0.30901699437494742410f, c2 = -0.80901699437494742410f;    // cos(2 pi / 5), cos(4 pi / 5)
  const float s1 = 0.95105651629515357212f, s2 = 0.58778525229247312917f;     // sin(2 pi / 5), sin(4 pi / 5)
  const mrc a1 = mr_add(x[1], x[4]), a2 = mr_add(x[2], x[3]), b1 = mr_sub(x[1], x[4]), b2 = mr_sub(x[2], x[3]);
  const mrc p1 = mr_mk(x[0].x + c1 * a1.x + c2 * a2.x, x[0].y + c1 * a1.y + c2 * a2.y);
  const mrc p2 = mr_mk(x[0].x + c2 * a1.x + c1 * a2.x, x[0].y + c2 * a1.y + c1 * a2.y);
  const mrc q1 = mr_mk(s1 * b1.x + s2 * b2.x, s1 * b1.y + s2 * b2.y);
  const mrc q2 = mr_mk(s2 * b1.x - s1 * b2.x, s2 * b1.y - s1 * b2.y);
  x[0] = mr_add(x[0], mr_add(a1, a2));
  x[1] = mr_mk(p1.x + q1.y, p1.y - q1.x);                      // p1 - i q1
  x[4] = mr_mk(p1.x - q1.y, p1.y + q1.x);
  x[2] = mr_mk(p2.x + q2.y, p2.y - q2.x);
  x[3] = mr_mk(p2.x - q2.y, p2.y + q2.x);
}
template <> __host__ __device__ inline void mr_dft<8>(mrc* x) {
  mrc e0 = x[0], e1 = x[2], e2 = x[4], e3 = x[6];
  mrc o0 = x[1], o1 = x[3], o2 = x[5], o3 = x[7];
  mr_dft4(e0, e1, e2, e3);
  mr_dft4(o0, o1, o2, o3);
  const float h = 0.70710678118654752440f;
  o1 = mr_mk((o1.x + o1.y) * h, (o1.y - o1.x) * h);            // * W8^1
  o2 = mr_mi(o2);                                              // * W8^2
  o3 = mr_mk((o3.y - o3.x) * h, (-o3.x - o3.y) * h);           // * W8^3
  x[0] = mr_add(e0, o0); x[1] = mr_add(e1, o1); x[2] = mr_add(e2, o2); x[3] = mr_add(e3, o3);
  x[4] = mr_sub(e0, o0); x[5] = mr_sub(e1, o1); x[6] = mr_sub(e2, o2); x[7] = mr_sub(e3, o3);
}

// butterfly j of a pass: twiddles (NS > 1), DFT_R; x holds in[j + r * N2 / R] on entry, out[.. + r * NS] on return
template <int R>
__host__ __device__ inline void mr_butterfly(mrc* x, const mrc* tw, int jm, int step, bool first) {
  if (!first) {
#pragma unroll
    for (int r = 1; r < R; ++r) x[r] = mr_mul(x[r], tw[jm * r * step]);
  }
  mr_dft<R>(x);
}

// real-FFT split: twice X[k] (0 <= k < N2) from z = Z[k], m = Z[(N2 - k) mod N2], w = exp(-2 pi i k / n_fft)
__host__ __device__ inline mrc mr_split2(mrc z, mrc m, mrc w) {
  const float e2r = z.x + m.x, e2i = z.y - m.y;
  const float o2r = z.y + m.y, o2i = m.x - z.x;
  return mr_mk(e2r + w.x * o2r - w.y * o2i, e2i + w.x * o2i + w.y * o2r);
}

}  // namespace afx
