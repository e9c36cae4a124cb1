// BS.1770 gated loudness for gfx950 (decomposition, records and the shared arithmetic: afx_loudness.h and afx_filt.h; the
// same chain on the CPU: afx_loudness_host.cpp).  Two walks over the samples and no per-sample workspace: the first leaves
// the end state of every 64-sample block, a per-clip scan turns them into entry states, the second walks every block from
// its entry state and leaves two float64 sums of squares.  No atomics: every value is written once, by one lane, from one
// fixed order of float64 operations.  A tile belongs to one clip, and every index into the caller's samples is checked
// against that clip's length: a neighbour in the packed buffer is never read.
//
// One lane walks one block, a wave a tile of kFiltB blocks staged in LDS as float32 rows of kLoudStride (16.6 KiB: nine
// workgroups of one wave per CU).  The tile comes in with the lanes on adjacent samples (coalesced); the walk reads a
// column, lane i on row i, which the odd row stride keeps off shared banks.
#include <cfloat>

#include <hip/hip_runtime.h>

#include "afx.h"
#include "afx_loudness.h"

namespace afx {

// Tables and records every lane reads at one address go through the constant address space: scalar loads, and the
// coefficients reach v_fma_f64 as scalar operands.  (Loads only.)
template <typename T> using ld_const = const __attribute__((address_space(4))) T*;
template <typename T> __device__ __forceinline__ ld_const<T> ld_as_const(const T* p) { return (ld_const<T>)(uintptr_t)p; }

struct LdClip { int64_t in_off, out_off, n; double tg, rate; int first_tile, n_blocks, tab, c; };

// the record whose tile range holds tile g (every record has at least one tile)
__device__ __forceinline__ LdClip ld_find(const LoudClip* clips, int n, int g) {
  const ld_const<LoudClip> cc = ld_as_const(clips);
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (cc[mid].first_tile <= g) lo = mid; else hi = mid - 1;
  }
  LdClip r;
  r.in_off = cc[lo].in_off; r.out_off = cc[lo].out_off; r.n = cc[lo].n; r.tg = cc[lo].tg; r.rate = cc[lo].rate;
  r.first_tile = cc[lo].first_tile; r.n_blocks = cc[lo].n_blocks; r.tab = cc[lo].tab; r.c = lo;
  return r;
}

__device__ __forceinline__ void ld_sections(const FiltTab* tab, FiltSec* sec) {
  const ld_const<FiltTab> t = ld_as_const(tab);
#pragma unroll
  for (int s = 0; s < kLoudS; ++s) { sec[s].b0 = t->sec[s].b0; sec[s].b1 = t->sec[s].b1; sec[s].b2 = t->sec[s].b2; sec[s].a1 = t->sec[s].a1; sec[s].a2 = t->sec[s].a2; }
}

// the tile's samples into LDS, zeros past the clip's end; -> the lane's max |x| and non-finite flag
__device__ __forceinline__ void ld_stage(const void* in, int fmt, const LdClip& cl, int64_t j0, int lane, float* tile, float* mx,
                                         unsigned* bad) {
  float m = 0.0f;
  unsigned b = 0;
  for (int q = 0; q < kFiltB; ++q) {
    const int64_t j = j0 + q * kFiltL + lane;
    const float x = j < cl.n ? loud_raw(in, fmt, cl.in_off + j) : 0.0f;
    const float a = fabsf(x);
    if (!(a <= FLT_MAX)) b = 1;
    m = fmaxf(m, a);
    tile[q * kLoudStride + lane] = x;
  }
  *mx = m; *bad = b;
}

// Blocks past the clip's last one are walked like any other (over zeros): their end states land in the tile-granular
// workspace and are never read.
__global__ void __launch_bounds__(64) k_loud_ends(const void* __restrict__ in, int fmt, const FiltTab* __restrict__ tabs,
                                                  const LoudClip* __restrict__ clips, int n, double* __restrict__ carry,
                                                  float* __restrict__ tile_peak, uint32_t* __restrict__ tile_bad) {
  __shared__ float tile[kFiltB * kLoudStride];
  const LdClip cl = ld_find(clips, n, blockIdx.x);
  const int lane = threadIdx.x;
  const int64_t j0 = (int64_t)(blockIdx.x - cl.first_tile) * kFiltTile;
  float mx;
  unsigned bad;
  ld_stage(in, fmt, cl, j0, lane, tile, &mx, &bad);
  __syncthreads();
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
  const int any_bad = __any((int)bad);
  if (lane == 0) { tile_peak[blockIdx.x] = mx; tile_bad[blockIdx.x] = any_bad ? 1u : 0u; }
  FiltSec sec[kLoudS];
  ld_sections(tabs + cl.tab, sec);
  double z[kLoudZ];
#pragma unroll
  for (int j = 0; j < kLoudZ; ++j) z[j] = 0.0;
  const float* row = tile + lane * kLoudStride;
  for (int m = 0; m < kFiltL; ++m) (void)filt_cascade<kLoudS>(sec, (double)row[m], z);
  double* c = carry + ((int64_t)blockIdx.x * kFiltB + lane) * kLoudZ;
#pragma unroll
  for (int j = 0; j < kLoudZ; ++j) c[j] = z[j];
}

// One wave per clip, its blocks in order: the end state in carry[block] is replaced by the state entering the block.  The
// chain is sequential and one lane runs it, in the host executor's order; the other lanes move the states: 64 blocks a
// round come into LDS with coalesced loads (the next round's are in flight while the lane works) and go back the same way.
__global__ void __launch_bounds__(64) k_loud_scan(const FiltTab* __restrict__ tabs, const LoudClip* __restrict__ clips,
                                                  double* __restrict__ carry) {
  __shared__ double st[64 * kLoudZ];
  const ld_const<LoudClip> cc = ld_as_const(clips);
  const int c = blockIdx.x, lane = threadIdx.x;
  const int64_t nb = (cc[c].n + kFiltL - 1) / kFiltL;
  double* base = carry + (int64_t)cc[c].first_tile * kFiltB * kLoudZ;
  const ld_const<FiltTab> t = ld_as_const(tabs + cc[c].tab);
  double T[kLoudZ][kLoudZ];
#pragma unroll
  for (int i = 0; i < kLoudZ; ++i)
#pragma unroll
    for (int j = 0; j < kLoudZ; ++j) T[i][j] = t->T[i][j];
  double z[kLoudZ], nx[kLoudZ];
#pragma unroll
  for (int j = 0; j < kLoudZ; ++j) { z[j] = 0.0; nx[j] = lane < nb ? base[(int64_t)lane * kLoudZ + j] : 0.0; }
  for (int64_t q0 = 0; q0 < nb; q0 += 64) {
    const int cnt = (int)(nb - q0 < 64 ? nb - q0 : 64);
#pragma unroll
    for (int j = 0; j < kLoudZ; ++j) st[lane * kLoudZ + j] = nx[j];
    __syncthreads();
    if (q0 + 64 + lane < nb) {
#pragma unroll
      for (int j = 0; j < kLoudZ; ++j) nx[j] = base[(q0 + 64 + lane) * kLoudZ + j];
    }
    if (lane == 0) {
      for (int u = 0; u < cnt; ++u) {
        double fin[kLoudZ];
#pragma unroll
        for (int j = 0; j < kLoudZ; ++j) { fin[j] = st[u * kLoudZ + j]; st[u * kLoudZ + j] = z[j]; }
        filt_carry<kLoudS>(T, z, fin);
      }
    }
    __syncthreads();
    if (lane < cnt) {
#pragma unroll
      for (int j = 0; j < kLoudZ; ++j) base[(q0 + lane) * kLoudZ + j] = st[lane * kLoudZ + j];
    }
    __syncthreads();
  }
}

__global__ void __launch_bounds__(64) k_loud_sums(const void* __restrict__ in, int fmt, const FiltTab* __restrict__ tabs,
                                                  const LoudClip* __restrict__ clips, int n, const double* __restrict__ carry,
                                                  double* __restrict__ part) {
  __shared__ float tile[kFiltB * kLoudStride];
  const LdClip cl = ld_find(clips, n, blockIdx.x);
  const int lane = threadIdx.x;
  const int64_t j0 = (int64_t)(blockIdx.x - cl.first_tile) * kFiltTile;
  float mx;
  unsigned bad;
  ld_stage(in, fmt, cl, j0, lane, tile, &mx, &bad);
  __syncthreads();
  const int64_t blk = (int64_t)blockIdx.x * kFiltB + lane;
  int split, stop;
  loud_block_cut(cl.tg, cl.rate, j0 + (int64_t)lane * kFiltL, loud_limit(cl.tg, cl.rate, cl.n, cl.n_blocks), &split, &stop);
  double p[2] = {0.0, 0.0};
  if (stop > 0) {
    FiltSec sec[kLoudS];
    ld_sections(tabs + cl.tab, sec);
    double z[kLoudZ];
#pragma unroll
    for (int j = 0; j < kLoudZ; ++j) z[j] = carry[blk * kLoudZ + j];
    const float* row = tile + lane * kLoudStride;
    loud_block_sums(sec, z, split, stop, [row](int m) { return row[m]; }, p);
  }
  part[2 * blk] = p[0];
  part[2 * blk + 1] = p[1];
}

// v[0] = the halving-tree sum of the 64 lanes' values (the order of loud_sum64_host)
__device__ __forceinline__ double ld_tree(double* v, int lane, double a) {
  __syncthreads();
  v[lane] = a;
  __syncthreads();
  for (int w = 32; w > 0; w >>= 1) {
    if (lane < w) v[lane] += v[lane + w];
    __syncthreads();
  }
  return v[0];
}

// One wave per clip: the tiles' peaks and flags, the segment sums, z_j, both gates in the linear domain.
__global__ void __launch_bounds__(64) k_loud_gate(const LoudClip* __restrict__ clips, const double* __restrict__ part,
                                                  const float* __restrict__ tile_peak, const uint32_t* __restrict__ tile_bad,
                                                  double abs_gate, double* __restrict__ seg, double* __restrict__ z,
                                                  double* __restrict__ rec) {
  __shared__ double v[64];
  const ld_const<LoudClip> cc = ld_as_const(clips);
  const int c = blockIdx.x, lane = threadIdx.x;
  const int64_t n = cc[c].n, seg_off = cc[c].seg_off, z_off = cc[c].z_off;
  const double tg = cc[c].tg, rate = cc[c].rate;
  const int first_tile = cc[c].first_tile, n_tiles = cc[c].n_tiles, nbk = cc[c].n_blocks;
  float mx = 0.0f;
  int bad = 0;
  for (int q = lane; q < n_tiles; q += 64) { mx = fmaxf(mx, tile_peak[first_tile + q]); bad |= (int)tile_bad[first_tile + q]; }
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
  bad = __any(bad);
  const int64_t lim = loud_limit(tg, rate, n, nbk);
  const int64_t nseg = nbk > 0 ? (int64_t)nbk + 3 : 0;
  const double* mypart = part + (int64_t)first_tile * kFiltB * 2;
  double* myseg = seg + seg_off;
  double* myz = z + z_off;
  for (int64_t k = lane; k < nseg; k += 64) myseg[k] = loud_seg_sum(tg, rate, lim, k, mypart);
  __syncthreads();
  const double tg_rate = tg * rate;
  for (int64_t j = lane; j < nbk; j += 64) myz[j] = loud_z(myseg, j, tg_rate);
  __syncthreads();
  double a_all = 0.0, a1 = 0.0;
  int c1 = 0;
  for (int64_t j = lane; j < nbk; j += 64) {
    const double zj = myz[j];
    a_all += zj;
    if (zj >= abs_gate) { a1 += zj; ++c1; }
  }
  const double s_all = ld_tree(v, lane, a_all);
  const double s1 = ld_tree(v, lane, a1);
  for (int o = 32; o > 0; o >>= 1) c1 += __shfl_xor(c1, o);
  const double mean1 = c1 > 0 ? s1 / (double)c1 : 0.0;
  const double rel = mean1 / 10.0;
  double a2 = 0.0;
  int c2 = 0;
  for (int64_t j = lane; j < nbk; j += 64) {
    const double zj = myz[j];
    if (zj > rel && zj > abs_gate) { a2 += zj; ++c2; }
  }
  const double s2 = ld_tree(v, lane, a2);
  for (int o = 32; o > 0; o >>= 1) c2 += __shfl_xor(c2, o);
  if (lane == 0) {
    double* r = rec + (int64_t)c * kLoudRec;
    r[kLdBlocks] = (double)nbk; r[kLdN1] = (double)c1; r[kLdN2] = (double)c2;
    r[kLdMean1] = mean1;
    r[kLdMean2] = c2 > 0 ? s2 / (double)c2 : 0.0;
    r[kLdMeanAll] = nbk > 0 ? s_all / (double)nbk : 0.0;
    r[kLdPeak] = (double)mx;
    r[kLdBad] = bad ? 1.0 : 0.0;
  }
}

__global__ void __launch_bounds__(256) k_loud_gain(const void* __restrict__ in, int fmt, const LoudClip* __restrict__ clips, int n,
                                                   const float* __restrict__ gain, float* __restrict__ out) {
  const LdClip cl = ld_find(clips, n, blockIdx.x);
  const float g = gain[cl.c];
  if (g != g) return;                          // a clip that is not to be written
  const int64_t j0 = (int64_t)(blockIdx.x - cl.first_tile) * kFiltTile;
  for (int e = threadIdx.x; e < kFiltTile; e += 256) {
    const int64_t i = j0 + e;
    if (i >= cl.n) break;
    out[cl.out_off + i] = g * loud_raw(in, fmt, cl.in_off + i);
  }
}

hipError_t launch_loud_ends(hipStream_t s, const void* in, int fmt, const FiltTab* tabs, const LoudClip* clips, int n, int n_tiles,
                            double* carry, float* tile_peak, uint32_t* tile_bad) {
  hipLaunchKernelGGL(k_loud_ends, dim3(n_tiles), dim3(64), 0, s, in, fmt, tabs, clips, n, carry, tile_peak, tile_bad);
  return hipGetLastError();
}

hipError_t launch_loud_scan(hipStream_t s, const FiltTab* tabs, const LoudClip* clips, int n, double* carry) {
  hipLaunchKernelGGL(k_loud_scan, dim3(n), dim3(64), 0, s, tabs, clips, carry);
  return hipGetLastError();
}

hipError_t launch_loud_sums(hipStream_t s, const void* in, int fmt, const FiltTab* tabs, const LoudClip* clips, int n, int n_tiles,
                            const double* carry, double* part) {
  hipLaunchKernelGGL(k_loud_sums, dim3(n_tiles), dim3(64), 0, s, in, fmt, tabs, clips, n, carry, part);
  return hipGetLastError();
}

hipError_t launch_loud_gate(hipStream_t s, const LoudClip* clips, int n, const double* part, const float* tile_peak,
                            const uint32_t* tile_bad, double abs_gate, double* seg, double* z, double* rec) {
  hipLaunchKernelGGL(k_loud_gate, dim3(n), dim3(64), 0, s, clips, part, tile_peak, tile_bad, abs_gate, seg, z, rec);
  return hipGetLastError();
}

hipError_t launch_loud_gain(hipStream_t s, const void* in, int fmt, const LoudClip* clips, int n, int n_tiles, const float* gain,
                            float* out) {
  hipLaunchKernelGGL(k_loud_gain, dim3(n_tiles), dim3(256), 0, s, in, fmt, clips, n, gain, out);
  return hipGetLastError();
}

}  // namespace afx
