// Batched DTW of feature sequences: librosa.sequence.dtw(X, Y, metric, global_constraints, band_rad) at its defaults,
// the step the reference's aligner runs on the MFCC frames this library extracts
// (05_dtw_alignment_experiment/dtw_alignment.py:930-970, :1092-1130).
//
// k_dtw: one wave per pair.  The wave walks the rows in strips of 64, one row per lane, and inside a strip runs the DP as a
// skewed wavefront: at step s lane l owns cell (i0 + l, s - l).  Its three predecessors are
//   (i, j-1)   the lane's own value of step s-1,
//   (i-1, j)   lane l-1's value of step s-1            (DPP wave_shr:1 on both dwords of the double),
//   (i-1, j-1) what the lane received that way at step s-1;
// lane 0 takes row i0-1 from the boundary row the previous strip's lane 63 left in global memory (in place: column j is
// read at step j and overwritten at step j + 63).  The local cost is computed by each lane from its x row (VGPRs) and
// the y column s - l, read with ds_read_b128 from an LDS ring of the last 72 columns; the ring's stride (DIMP + 4 floats,
// an odd number of 16-byte units) puts the 64 skewed reads of a step on distinct banks.  Eight steps form an unrolled
// tile; a tile's y columns and boundary values are loaded into registers two tiles before it runs.
// Steps whose 64 cells all lie outside the band are never executed.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "afx.h"
#include "afx_dtw.h"
#include "afx_dtw_dev.h"

namespace afx {
namespace {

constexpr double kInf = kDtwInf;
typedef dtw_f2 f2;

__device__ __forceinline__ double shr1(double v, double lane0) { return dtw_shr1(v, lane0); }
__device__ __forceinline__ double shl1(double v) { return dtw_shl1(v); }

// frame-major features of stride dim -> stride dimp (zero-padded, so that the DP reads whole 16-byte units without a
// per-element test): one element per thread, coalesced on both sides
__global__ void k_dtw_pack(const float* __restrict__ feats, int dim, int dimp, int64_t n_elems, float* __restrict__ packed) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n_elems) return;
  const int64_t t = e / dimp;
  const int k = (int)(e - t * dimp);
  packed[e] = k < dim ? feats[t * dim + k] : 0.f;
}

// norms[t] = |frame t| in float32, from the packed rows (DIMP / 4 16-byte loads per frame)
template <int DIMP>
__global__ void k_dtw_norms(const float* __restrict__ packed, int64_t n_frames, float* __restrict__ norms) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_frames) return;
  const float4* f = reinterpret_cast<const float4*>(packed + t * DIMP);
  float a = 0.f;
#pragma unroll
  for (int q = 0; q < DIMP / 4; ++q) {
    const float4 v = f[q];
    a = fmaf(v.x, v.x, a); a = fmaf(v.y, v.y, a); a = fmaf(v.z, v.z, a); a = fmaf(v.w, v.w, a);
  }
  norms[t] = sqrtf(a);
}

__global__ void k_dtw_fill_inf(double* __restrict__ p, int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += stride) p[t] = kInf;
}

// METRIC: AFX_DTW_EUCLIDEAN / AFX_DTW_SQEUCLIDEAN / AFX_DTW_COSINE; DIMP: dim rounded up to a multiple of 8
template <int DIMP, int METRIC>
__global__ void __launch_bounds__(64) k_dtw(const float* __restrict__ feats, const float* __restrict__ norms,
                                            const DtwPair* __restrict__ pairs, uint32_t* __restrict__ codes,
                                            double* __restrict__ rows, double* __restrict__ dmat,
                                            double* __restrict__ cost, int32_t* __restrict__ status, int backtrack,
                                            int store_d) {
  constexpr int S = DIMP + 4;             // ring stride in floats; slot S-4 holds the column's norm (cosine)
  constexpr int R = kDtwRing;
  constexpr int E = kDtwTile * DIMP / 64; // y elements a lane stages per tile
  static_assert(DIMP % 8 == 0 && (S / 4) % 2 == 1, "ring stride must be an odd number of 16-byte units");
  __shared__ __attribute__((aligned(16))) float ys[R * S];

  const int l = threadIdx.x;
  const DtwPair P = pairs[blockIdx.x];
  const int N = P.n, M = P.m;

  // ---- NaN / inf anywhere in X or Y, or a zero-norm frame under cosine: librosa raises; the pair is skipped
  if (dtw_pair_nonfinite<DIMP, METRIC>(feats, norms, P, l)) {
    if (l == 0) { cost[blockIdx.x] = __builtin_nan(""); status[blockIdx.x] = AFX_DTW_NONFINITE; }
    return;
  }

  const float* fy = feats + P.y_frame * DIMP;
  double* row = rows + P.row;
  uint32_t* cw = codes + (backtrack ? P.codes : 0);
  double* D = dmat + (store_d ? P.d : 0);
  double fin = kInf;                       // D[N-1, M-1], held by the lane that computes it
  const int nstrips = (N + 63) >> 6;

  for (int strip = 0; strip < nstrips; ++strip) {
    const int i0 = strip << 6, i = i0 + l;
    const bool rowok = i < N;
    const int last = min(N - 1, i0 + 63);
    // steps that touch the band: row i0 starts at j = i0 + lo + 1, row `last` ends at j = last + hi - 1.  The walk starts
    // one column early so that lane 0 receives D[i0-1, i0+lo], the diagonal predecessor of the strip's first cell.
    const int jlo = max(0, i0 + P.lo), jhi = min(M - 1, last + P.hi - 1);
    if (jlo > jhi) continue;
    const int s_begin = jlo & ~(kDtwTile - 1), s_end = jhi + (last - i0);

    f2 xr[DIMP / 2];
    float nx = 0.f;
    {
      const float4* fx = reinterpret_cast<const float4*>(feats + (P.x_frame + min(i, N - 1)) * DIMP);
#pragma unroll
      for (int q = 0; q < DIMP / 4; ++q) {
        const float4 v = fx[q];
        xr[2 * q] = f2{v.x, v.y}; xr[2 * q + 1] = f2{v.z, v.w};
      }
      if (METRIC == AFX_DTW_COSINE) nx = rowok ? norms[P.x_frame + i] : 1.f;
    }

    // staging of one tile: E y elements per lane, plus the boundary value and the norm of column c0 + l for l < 8.  Two
    // stages alternate, so that a tile's loads are issued two tiles before it runs.
    struct Stage {
      float y[E];
      double rb;
      float ny;
    } sa, sb;
    auto fetch = [&](int c0, Stage& st) {
#pragma unroll
      for (int t = 0; t < E; ++t) {
        const int e = l + 64 * t, g = c0 + e / DIMP;
        st.y[t] = g < M ? fy[(int64_t)c0 * DIMP + e] : 0.f;
      }
      const int g = c0 + l;
      st.rb = kInf;
      if (l < kDtwTile && g < M && strip > 0 && g - (i0 - 1) > P.lo && g - (i0 - 1) < P.hi)
        st.rb = __hip_atomic_load(row + g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      st.ny = 1.f;
      if (METRIC == AFX_DTW_COSINE && l < kDtwTile && g < M) st.ny = norms[P.y_frame + g];
    };
    __threadfence_block();                 // the previous strip's boundary row is visible to every lane
    fetch(s_begin, sa);
    if (s_begin + kDtwTile <= s_end) fetch(s_begin + kDtwTile, sb);

    double dlast = kInf, upprev = kInf;
    uint32_t word = 0;
    int slot = (s_begin - l + 2 * R) % R;  // ring slot of column s - l
    auto run_tile = [&](int c0, Stage& cur) {
      const int base = c0 % R;
#pragma unroll
      for (int t = 0; t < E; ++t) {
        const int e = l + 64 * t, col = e / DIMP, k = e % DIMP;
        int sl = base + col;
        sl = sl >= R ? sl - R : sl;
        ys[sl * S + k] = cur.y[t];
      }
      if (METRIC == AFX_DTW_COSINE && l < kDtwTile) {
        int sl = base + l;
        sl = sl >= R ? sl - R : sl;
        ys[sl * S + DIMP] = cur.ny;
      }
      double rb = cur.rb;                  // lane 0 holds the boundary value of step c0 + b after b left shifts
      __syncthreads();
      if (c0 + 2 * kDtwTile <= s_end) fetch(c0 + 2 * kDtwTile, cur);

#pragma unroll
      for (int b = 0; b < kDtwTile; ++b) {
        const int s = c0 + b, j = s - l;
        const float c = dtw_local_cost<DIMP, METRIC>(xr, nx, ys, slot);
        const int dj = j - i;
        const bool valid = rowok && j >= 0 && j < M;
        const bool inband = valid && dj > P.lo && dj < P.hi;
        const double cd = inband ? (double)c : kInf;

        const double up = shr1(dlast, rb);
        rb = shl1(rb);
        const double s0 = upprev + cd, s1 = dlast + cd, s2 = up + cd;
        double best = s0;
        uint32_t code = 0;
        if (s1 < best) { best = s1; code = 1; }
        if (s2 < best) { best = s2; code = 2; }
        if (i == 0 && j == 0) { best = cd; code = 0; }
        const double d = valid ? best : kInf;
        upprev = up;
        dlast = d;
        word |= code << (2 * (s & 15));
        if (store_d && valid) D[(int64_t)i * M + j] = d;
        if (l == 63 && valid) __hip_atomic_store(row + j, d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (i == N - 1 && j == M - 1) fin = d;
        slot = slot + 1 == R ? 0 : slot + 1;
      }
      if (c0 & kDtwTile) {                 // the word of steps 16q .. 16q+15 is complete: every lane stores it
        if (backtrack) cw[((int64_t)strip * P.qn + (c0 >> 4)) * 64 + l] = word;
        word = 0;
      }
      __syncthreads();                     // the ring slots of the next tile are free
    };
    int c0 = s_begin;
    for (; c0 <= s_end; c0 += 2 * kDtwTile) {
      run_tile(c0, sa);
      if (c0 + kDtwTile <= s_end) run_tile(c0 + kDtwTile, sb);
    }
    const int c_last = (s_end - s_begin) / kDtwTile * kDtwTile + s_begin;   // the last tile run
    if (backtrack && (c_last & kDtwTile) == 0) cw[((int64_t)strip * P.qn + (c_last >> 4)) * 64 + l] = word;
  }
  if (l == ((N - 1) & 63)) {
    cost[blockIdx.x] = fin;
    status[blockIdx.x] = isinf(fin) ? AFX_DTW_NO_PATH : AFX_DTW_OK;
  }
}

__global__ void k_dtw_backtrack(const DtwPair* __restrict__ pairs, int n_pairs, const uint32_t* __restrict__ codes,
                                const int32_t* __restrict__ status, int32_t* __restrict__ path, int32_t* __restrict__ len) {
  dtw_backtrack_walk<2>(pairs, n_pairs, codes, status, nullptr, false, path, len, [](uint32_t code, int& i, int& j) {
    i -= code != 1;                        // 0: (1,1), 1: (0,1), 2: (1,0)
    j -= code < 2;
    return true;
  });
}

}  // namespace

int dtw_dimp(int dim) {
  return dtw_with_dimp(dim, [](auto dimp) { return (int)decltype(dimp)::value; });
}

hipError_t launch_dtw_pack(hipStream_t s, const float* feats, int dim, int64_t n_frames, float* packed, float* norms) {
  if (n_frames <= 0) return hipSuccess;
  const int dimp = dtw_dimp(dim);
  const int64_t n_elems = n_frames * dimp;
  k_dtw_pack<<<dim3((unsigned)((n_elems + 255) / 256)), dim3(256), 0, s>>>(feats, dim, dimp, n_elems, packed);
  return dtw_with_dimp(dim, [&](auto dimp_c) {
    k_dtw_norms<decltype(dimp_c)::value><<<dim3((unsigned)((n_frames + 255) / 256)), dim3(256), 0, s>>>(packed, n_frames, norms);
    return hipGetLastError();
  });
}

hipError_t launch_dtw_fill_inf(hipStream_t s, double* p, int64_t n) {
  if (n <= 0) return hipSuccess;
  const int64_t blocks = std::min<int64_t>((n + 255) / 256, 8192);
  k_dtw_fill_inf<<<dim3((unsigned)blocks), dim3(256), 0, s>>>(p, n);
  return hipGetLastError();
}

hipError_t launch_dtw(hipStream_t s, const float* feats, const float* norms, int dim, int metric, const DtwPair* pairs,
                      int n_pairs, uint32_t* codes, double* rows, double* dmat, double* cost, int32_t* status,
                      bool backtrack, bool store_d) {
  if (n_pairs <= 0) return hipSuccess;
  return dtw_dispatch(dim, metric, [&](auto dimp, auto met) {
    k_dtw<decltype(dimp)::value, decltype(met)::value><<<dim3(n_pairs), dim3(64), 0, s>>>(
        feats, norms, pairs, codes, rows, dmat, cost, status, backtrack ? 1 : 0, store_d ? 1 : 0);
    return hipGetLastError();
  });
}

hipError_t launch_dtw_backtrack(hipStream_t s, const DtwPair* pairs, int n_pairs, const uint32_t* codes,
                                const int32_t* status, int32_t* path, int32_t* len) {
  if (n_pairs <= 0) return hipSuccess;
  k_dtw_backtrack<<<dim3((n_pairs + 63) / 64), dim3(64), 0, s>>>(pairs, n_pairs, codes, status, path, len);
  return hipGetLastError();
}

}  // namespace afx
