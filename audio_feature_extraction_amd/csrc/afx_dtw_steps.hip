// Batched DTW with a step list: librosa.sequence.dtw(X, Y, step_sizes_sigma, weights_add, weights_mul, subseq, ...).
// The default call stays on k_dtw (afx_dtw.hip); this is the recurrence for steps that reach up to two rows and two
// columns back, with a weight pair per step and the subsequence seed / end rule.
//
// k_dtw_steps: one wave per pair, the packed features, strips of 64 rows, the skew and the LDS ring of y columns of
// k_dtw: at wavefront step s lane l owns cell (i0 + l, s - l).  The predecessor of step (di, dj) is cell
// (i - di, j - dj), which lane l - di owned at wavefront step s - di - dj.  A lane therefore keeps, as a rotated register
// set (the tile of eight steps is unrolled, so the rotation is renaming):
//   h1, h2          its own values of steps s-1, s-2                          -> (0,1), (0,2)
//   u1, u2, u3      u1 = lane l-1's h1 (DPP wave_shr:1), u2 / u3 the u1 of one / two steps ago
//                                                                             -> (1,0), (1,1), (1,2)
//   v2, v3, v4      v2 = lane l-1's u1 of the step before (wave_shr:1 again, so two lanes in two steps),
//                   v3 / v4 the v2 of one / two steps ago                     -> (2,0), (2,1), (2,2)
// which is two 64-bit lane shifts per step whatever the list holds.  The list is a kernel argument (SGPRs): per entry a
// selector into the eight registers above, the recorded index and the weight pair; each candidate is
// pred + (w_mul * c + w_add), multiply and add unfused, compared with a strict < in list order from the cell's seed
// (C[0, 0] at (0, 0), C[0, j] on row 0 under subseq, +inf elsewhere).
//
// Boundary rows.  Lane 0's u1 is D[i0-1, s] and its v2 is D[i0-2, s]; lane 1's v2 (row i0-1) is lane 0's previous u1, so
// only lane 0 reads global memory.  A pair has two boundary rows: A = D[i0-1, :], written by lane 63 of the previous strip,
// and B = D[i0-2, :], written by its lane 62; both are reused in place.  Timing, in wavefront steps of the reading strip:
// column g of either row is loaded with the staging of the tile that holds step g, i.e. between steps g - 23 and g - 16
// (two tiles ahead), never after step g; the two-column look-back needs no second read because columns g-1 and g-2 are
// the lane's own u2 / u3 (v3 / v4).  Column g is overwritten by lane 63 at step g + 63 (row A) and by lane 62 at step
// g + 62 (row B).  So every read of a column precedes its overwrite by at least 62 + 16 steps, and a write never lands in a
// column whose staging load is still to come: in-place reuse holds for both rows.  Across strips the previous strip has
// run to its end before the first load (one wave, program order, __threadfence_block).  A column the previous strip did
// not visit (outside the band) holds an older strip's value; the load masks it with the band test of its own row.
// The walk of a strip starts two columns before row i0's first cell inside the band, so that v4 = D[i0-2, i0+lo-1], the
// (2,2) predecessor of that cell, has arrived; every other predecessor inside the band lies at a later step.
//
// Step codes are 4 bits (indices 0 .. 7): every lane stores one dword per tile of eight steps, word [strip][s/8][lane].
// Under subseq the lane that owns row N-1 keeps the running first minimum of that row (one lane visits the row's cells
// in increasing j, so the strict < is the first argmin; no reduction across lanes is involved).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "afx.h"
#include "afx_dtw.h"
#include "afx_dtw_dev.h"

namespace afx {
namespace {

__device__ __forceinline__ double weighted(double wm, double c, double wa) {
#pragma clang fp contract(off)
  const double t = wm * c;      // float64 multiply, then float64 add: numpy's order, so integer-valued cases agree bit for bit
  return t + wa;
}

// the lane's x row as dtw_local_cost indexes it: DIMP / 2 register pairs, or (XLDS) the row's address in LDS
struct XRowLds {
  const float* p;
  __device__ __forceinline__ dtw_f2 operator[](int h) const { return *reinterpret_cast<const dtw_f2*>(p + 2 * h); }
};
template <int DIMP, bool XLDS> struct XRow { typedef dtw_f2 type[DIMP / 2]; };
template <int DIMP> struct XRow<DIMP, true> { typedef XRowLds type; };

template <int DIMP, int METRIC>
__global__ void __launch_bounds__(64) k_dtw_steps(const float* __restrict__ feats, const float* __restrict__ norms,
                                                  const DtwPair* __restrict__ pairs, const DtwSteps T,
                                                  uint32_t* __restrict__ codes, double* __restrict__ rows,
                                                  double* __restrict__ dmat, double* __restrict__ cost,
                                                  int32_t* __restrict__ status, int32_t* __restrict__ end, int backtrack,
                                                  int store_d) {
  constexpr int S = DIMP + 4;             // ring stride in floats; slot S-4 holds the column's norm (cosine)
  constexpr int R = kDtwRing;
  constexpr int E = kDtwTile * DIMP / 64; // y elements a lane stages per tile
  // The 128-wide instance keeps the strip's x rows in LDS too (k_dtw's 128 registers of x leave no room for the six
  // carried doubles): lane l reads row l at the ring's stride, so a step's 64 reads fall on distinct banks as well.
  constexpr bool XLDS = DIMP > 64;
  static_assert(DIMP % 8 == 0 && (S / 4) % 2 == 1, "ring stride must be an odd number of 16-byte units");
  static_assert(kDtwTile == 8, "one code word of 4-bit codes per tile");
  __shared__ __attribute__((aligned(16))) float ys[R * S];
  __shared__ __attribute__((aligned(16))) float xs[XLDS ? 64 * S : 4];

  const int l = threadIdx.x;
  const DtwPair P = pairs[blockIdx.x];
  const int N = P.n, M = P.m;
  const bool subseq = T.subseq != 0;

  if (dtw_pair_nonfinite<DIMP, METRIC>(feats, norms, P, l)) {
    if (l == 0) { cost[blockIdx.x] = __builtin_nan(""); status[blockIdx.x] = AFX_DTW_NONFINITE; end[blockIdx.x] = -1; }
    return;
  }

  const float* fy = feats + P.y_frame * DIMP;
  double* rowA = rows + P.row;             // D[i0-1, :]
  double* rowB = rowA + M;                 // D[i0-2, :]
  uint32_t* cw = codes + (backtrack ? P.codes : 0);
  double* D = dmat + (store_d ? P.d : 0);
  double fin = kDtwInf;                    // D[N-1, M-1], or the running first minimum of row N-1, in the lane of that row
  int jend = subseq ? 0 : M - 1;
  const int nstrips = (N + 63) >> 6;

  for (int strip = 0; strip < nstrips; ++strip) {
    const int i0 = strip << 6, i = i0 + l;
    const bool rowok = i < N;
    const int last = min(N - 1, i0 + 63);
    // steps that touch the band: row i0 starts at j = i0 + lo + 1, row `last` ends at j = last + hi - 1; two columns early
    // for the (2,2) predecessor of the strip's first cell (header)
    const int jlo = max(0, i0 + P.lo - 1), jhi = min(M - 1, last + P.hi - 1);
    if (jlo > jhi) continue;
    const int s_begin = jlo & ~(kDtwTile - 1), s_end = jhi + (last - i0);

    typename XRow<DIMP, XLDS>::type xr;
    float nx = 0.f;
    {
      const float4* fx = reinterpret_cast<const float4*>(feats + (P.x_frame + min(i, N - 1)) * DIMP);
      if constexpr (XLDS) {
        xr.p = xs + l * S;                 // each lane writes and reads its own row only: no barrier is needed
#pragma unroll
        for (int q = 0; q < DIMP / 4; ++q) reinterpret_cast<float4*>(xs + l * S)[q] = fx[q];
      } else {
#pragma unroll
        for (int q = 0; q < DIMP / 4; ++q) {
          const float4 v = fx[q];
          xr[2 * q] = dtw_f2{v.x, v.y}; xr[2 * q + 1] = dtw_f2{v.z, v.w};
        }
      }
      if (METRIC == AFX_DTW_COSINE) nx = rowok ? norms[P.x_frame + i] : 1.f;
    }

    // staging of one tile: E y elements per lane, plus the two boundary values and the norm of column c0 + l for l < 8.
    // Two stages alternate, so that a tile's loads are issued two tiles before it runs.
    struct Stage {
      float y[E];
      double ra, rb;
      float ny;
    } sa, sb;
    auto fetch = [&](int c0, Stage& st) {
#pragma unroll
      for (int t = 0; t < E; ++t) {
        const int e = l + 64 * t, g = c0 + e / DIMP;
        st.y[t] = g < M ? fy[(int64_t)c0 * DIMP + e] : 0.f;
      }
      const int g = c0 + l;
      st.ra = kDtwInf;
      st.rb = kDtwInf;
      if (l < kDtwTile && g < M && strip > 0) {
        const int da = g - (i0 - 1), db = g - (i0 - 2);
        if (da > P.lo && da < P.hi) st.ra = __hip_atomic_load(rowA + g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (db > P.lo && db < P.hi) st.rb = __hip_atomic_load(rowB + g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      }
      st.ny = 1.f;
      if (METRIC == AFX_DTW_COSINE && l < kDtwTile && g < M) st.ny = norms[P.y_frame + g];
    };
    __threadfence_block();                 // the previous strip's boundary rows are visible to every lane
    fetch(s_begin, sa);
    if ( s_begin + kDtwTile <= s_end) fetch(s_begin + kDtwTile, sb);

    double h1 = kDtwInf, h2 = kDtwInf, u1 = kDtwInf, u2 = kDtwInf, v2 = kDtwInf, v3 = kDtwInf;   // of the step before
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
      double ra = cur.ra, rb = cur.rb;     // lane 0 holds the boundary values of step c0 + b after b left shifts
      __syncthreads();
      if (c0 + 2 * kDtwTile <= s_end) fetch(c0 + 2 * kDtwTile, cur);

      uint32_t word = 0;
#pragma unroll
      for (int b = 0; b < kDtwTile; ++b) {
        const int s = c0 + b, j = s - l;
        const float c = dtw_local_cost<DIMP, METRIC>(xr, nx, ys, slot);
        const int dj = j - i;
        const bool valid = rowok && j >= 0 && j < M;
        const bool inband = valid && dj > P.lo && dj < P.hi;
        const double cd = inband ? (double)c : kDtwInf;

        const double n1 = dtw_shr1(h1, ra);   // (i-1, j)
        const double m2 = dtw_shr1(u1, rb);   // (i-2, j)
        ra = dtw_shl1(ra);
        rb = dtw_shl1(rb);
        const double u3 = u2, v4 = v3;
        u2 = u1; u1 = n1;
        v3 = v2; v2 = m2;

        double best = (i == 0 && (subseq || j == 0)) ? cd : kDtwInf;
        uint32_t code = 0;
#pragma unroll
        for (int k = 0; k < kDtwMaxSteps; ++k) {
          if (k < T.n) {
            const int sel = T.sel[k];
            const double p = sel == 1 ? h1 : sel == 2 ? h2 : sel == 3 ? u1 : sel == 4 ? u2 : sel == 5 ? u3
                           : sel == 6 ? v2 : sel == 7 ? v3 : v4;
            const double cand = p + weighted(T.w_mul[k], cd, T.w_add[k]);
            if (cand < best) { best = cand; code = (uint32_t)T.idx[k]; }
          }
        }
        const double d = valid ? best : kDtwInf;
        h2 = h1;
        h1 = d;
        word |= code << (4 * b);
        if (store_d && valid) D[(int64_t)i * M + j] = d;
        if (l == 63 && valid) __hip_atomic_store(rowA + j, d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (l == 62 && valid) __hip_atomic_store(rowB + j, d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (i == N - 1 && valid && (subseq ? d < fin : j == M - 1)) { fin = d; jend = j; }
        slot = slot + 1 == R ? 0 : slot + 1;
      }
      if (backtrack) cw[((int64_t)strip * P.qn + (c0 >> 3)) * 64 + l] = word;
      __syncthreads();                     // the ring slots of the next tile are free
    };
    int c0 = s_begin;
    for (; c0 <= s_end; c0 += 2 * kDtwTile) {
      run_tile(c0, sa);
      if (c0 + kDtwTile <= s_end) run_tile(c0 + kDtwTile, sb);
    }
  }
  if (l == ((N - 1) & 63)) {
    cost[blockIdx.x] = fin;
    status[blockIdx.x] = isinf(fin) ? AFX_DTW_NO_PATH : AFX_DTW_OK;
    end[blockIdx.x] = jend;
  }
}

__global__ void k_dtw_steps_backtrack(const DtwPair* __restrict__ pairs, int n_pairs, const DtwSteps T,
                                      const uint32_t* __restrict__ codes, const int32_t* __restrict__ status,
                                      const int32_t* __restrict__ end, int32_t* __restrict__ path, int32_t* __restrict__ len) {
  uint32_t table = 0;                      // selector (di * 3 + dj) by recorded index, 4 bits each
  for (int k = 0; k < T.n; ++k) table |= (uint32_t)T.sel[k] << (4 * T.idx[k]);
  dtw_backtrack_walk<4>(pairs, n_pairs, codes, status, end, T.subseq != 0, path, len, [table](uint32_t code, int& i, int& j) {
    const uint32_t sel = (table >> (4 * (code & 7u))) & 15u;
    i -= (int)(sel / 3u);
    j -= (int)(sel % 3u);
    return sel != 0;                       // 0: an index no step of the list recorded
  });
}

}  // namespace

hipError_t launch_dtw_steps(hipStream_t s, const float* feats, const float* norms, int dim, int metric, const DtwPair* pairs,
                            int n_pairs, const DtwSteps& T, uint32_t* codes, double* rows, double* dmat, double* cost,
                            int32_t* status, int32_t* end, bool backtrack, bool store_d) {
  if (n_pairs <= 0) return hipSuccess;
  return dtw_dispatch(dim, metric, [&](auto dimp, auto met) {
    k_dtw_steps<decltype(dimp)::value, decltype(met)::value><<<dim3(n_pairs), dim3(64), 0, s>>>(
        feats, norms, pairs, T, codes, rows, dmat, cost, status, end, backtrack ? 1 : 0, store_d ? 1 : 0);
    return hipGetLastError();
  });
}

hipError_t launch_dtw_steps_backtrack(hipStream_t s, const DtwPair* pairs, int n_pairs, const DtwSteps& T,
                                      const uint32_t* codes, const int32_t* status, const int32_t* end, int32_t* path,
                                      int32_t* len) {
  if (n_pairs <= 0) return hipSuccess;
  k_dtw_steps_backtrack<<<dim3((n_pairs + 63) / 64), dim3(64), 0, s>>>(pairs, n_pairs, T, codes, status, end, path, len);
  return hipGetLastError();
}

}  // namespace afx
