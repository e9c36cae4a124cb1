// Beat tracking: the dynamic programme of librosa.beat.beat_track on the onset envelope and the tempo the rhythm kernels
// leave on the device (tests/beat_ref.py is the spec, afx_beat_host.cpp the same definition on the CPU).  Float64 throughout.
//   k_beat_stage    envelope mode only, one workgroup per clip: the caller's envelope into the envelope buffer, NaN / inf found
//   k_beat_score    one workgroup per clip: mean and std (ddof 1) as 256 strided partial sums and a tree, x = env / (std +
//                   DBL_MIN), the Gaussian window of 2 fpb + 1 taps in LDS, the local score of a frame per thread (taps in
//                   ascending order), its maximum by the same tree
//   k_beat_dp       one wave per clip, sequential in time: the penalty of every distance in LDS, the last 2048 cumulative
//                   scores in an LDS ring; the lanes stride over a frame's candidates in 64s, the wave takes the maximum and,
//                   of equal scores, the nearest predecessor; cumscore and backlink leave in rows of 64 frames
//   k_beat_finish   one wave per clip: the local maxima of cumscore as order-preserving integer keys, their median by
//                   bisecting the key (64 counting passes, any count), the last beat, then one lane walks the chain: the trim's
//                   threshold, the kept range, the flags
// No float atomics, no inline assembly; nothing depends on the order in which waves run.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <climits>
#include <cstdint>

#include "afx_beat.h"
#include "afx_wave.h"

namespace afx {

// ---- reductions ------------------------------------------------------------------------------------------------------
struct BtAdd { __device__ double operator()(double a, double b) const { return a + b; } };
struct BtMax { __device__ double operator()(double a, double b) const { return b > a ? b : a; } };

// the tree afx_beat_host.cpp's strided_tree walks: red[t] = op(red[t], red[t + s]), s = 128 .. 1
template <typename Op>
__device__ __forceinline__ double bt_block_reduce(double v, double* red, Op op) {
  red[threadIdx.x] = v;
  __syncthreads();
#pragma unroll
  for (int s = kBeatThreads / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] = op(red[threadIdx.x], red[threadIdx.x + s]);
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}

#define AFX_DPP_D(v, ctrl) \
  __hiloint2double(AFX_DPP_I(__double2hiint(v), ctrl, false), AFX_DPP_I(__double2loint(v), ctrl, false))
__device__ __forceinline__ double bt_readlane_d(double v, int l) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}
__device__ __forceinline__ double bt_max2(double a, double b) { return b > a ? b : a; }
// the wave's largest value (NaN never wins), uniform
__device__ __forceinline__ double bt_wave_max(double v) {
  v = bt_max2(v, AFX_DPP_D(v, 0xB1));
  v = bt_max2(v, AFX_DPP_D(v, 0x4E));
  v = bt_max2(v, AFX_DPP_D(v, 0x141));
  v = bt_max2(v, AFX_DPP_D(v, 0x140));
  return bt_max2(bt_max2(bt_readlane_d(v, 0), bt_readlane_d(v, 16)), bt_max2(bt_readlane_d(v, 32), bt_readlane_d(v, 48)));
}
__device__ __forceinline__ int bt_wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ int bt_wave_max_i(int v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = max(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ unsigned long long bt_wave_min_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const unsigned long long w = __shfl_xor(v, o);
    v = w < v ? w : v;
  }
  return v;
}

// order-preserving uint64 image of a double and back
__device__ __forceinline__ unsigned long long bt_key(double d) {
  const unsigned long long u = (unsigned long long)__double_as_longlong(d);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double bt_unkey(unsigned long long k) {
  const unsigned long long u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  return __longlong_as_double((long long)u);
}

// ---- envelope mode: the caller's envelopes ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_beat_stage(const float* __restrict__ in, const HpssClip* __restrict__ clips,
                                                    float* __restrict__ env, uint32_t* __restrict__ bad) {
  const HpssClip c = clips[blockIdx.x];
  const float* src = in + c.in_off;
  int nf = 0;
  for (int t = threadIdx.x; t < c.T; t += 256) nf |= !isfinite(src[t]);
  nf = __syncthreads_or(nf);
  float* dst = env + c.frame_base;
  for (int t = threadIdx.x; t < c.T; t += 256) dst[t] = nf ? 0.f : src[t];
  if (threadIdx.x == 0) bad[blockIdx.x] = nf ? 1u : 0u;
}

// ---- the record and the local score -----------------------------------------------------------------------------------
__global__ __launch_bounds__(kBeatThreads) void k_beat_score(const float* __restrict__ env, const HpssClip* __restrict__ clips,
                                                             const uint32_t* __restrict__ bad, const double* __restrict__ res,
                                                             const double* __restrict__ bpm_in, double fps,
                                                             double* __restrict__ x, double* __restrict__ localscore,
                                                             BeatRec* __restrict__ rec) {
#pragma clang fp contract(off)
  __shared__ double red[kBeatThreads];
  __shared__ double w[kBeatTaps];
  const int tid = threadIdx.x, b = blockIdx.x;
  const HpssClip c = clips[b];
  const int T = c.T;
  const float* e = env + c.frame_base;
  double tempo = res[4 * (int64_t)b];
  if (bpm_in && bpm_in[b] > 0.0) tempo = bpm_in[b];
  if (bad[b]) tempo = 0.0;
  int fpb = 0;
  if (tempo > 0.0) {
    const double q = fps * 60.0;
    const double r = rint(q / tempo);
    fpb = (r >= 1.0 && r <= (double)kBeatMaxFpb) ? (int)r : 0;   // the host refuses a tempo outside; the decided one is inside
  }
  int nz = 0;
  double s = 0.0;
  for (int t = tid; t < T; t += kBeatThreads) { s += (double)e[t]; nz |= e[t] != 0.f; }
  nz = __syncthreads_or(nz);
  const bool active = T >= 2 && nz && fpb > 0;
  const int lo = (int)rint((double)fpb / 2.0);
  if (!active) {
    if (tid == 0) rec[b] = BeatRec{tempo, 0.0, 0.0, fpb, lo, 0, 0};
    return;
  }
  const double mean = bt_block_reduce(s, red, BtAdd()) / (double)T;
  double v = 0.0;
  for (int t = tid; t < T; t += kBeatThreads) { const double d = (double)e[t] - mean; const double d2 = d * d; v += d2; }
  const double var = bt_block_reduce(v, red, BtAdd()) / (double)(T - 1);
  const double denom = sqrt(var) + DBL_MIN;
  double* xs = x + c.frame_base;
  for (int t = tid; t < T; t += kBeatThreads) xs[t] = (double)e[t] / denom;
  for (int k = tid; k <= 2 * fpb; k += kBeatThreads) {
    const double a = (double)(k - fpb) * 32.0 / (double)fpb;
    const double a2 = a * a;
    w[k] = exp(-0.5 * a2);
  }
  __syncthreads();                                       // x (this workgroup's own stores) and w are visible
  double* ls = localscore + c.frame_base;
  double m = -INFINITY;
  for (int i = tid; i < T; i += kBeatThreads) {
    const int k0 = max(0, i + fpb - (T - 1)), k1 = min(2 * fpb, i + fpb);
    double acc = 0.0;
    for (int k = k0; k <= k1; ++k) {                      // x index i + fpb - k stays in [0, T - 1]
      const double p = w[k] * xs[i + fpb - k];
      acc += p;
    }
    ls[i] = acc;
    m = acc > m ? acc : m;
  }
  m = bt_block_reduce(m, red, BtMax());
  if (tid == 0) rec[b] = BeatRec{tempo, denom, m, fpb, lo, 1, 0};
}

// ---- the dynamic programme ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_beat_dp(const HpssClip* __restrict__ clips, const BeatRec* __restrict__ rec,
                                                const double* __restrict__ localscore, double tightness,
                                                double* __restrict__ cumscore, int32_t* __restrict__ backlink) {
#pragma clang fp contract(off)
  __shared__ double pen[kBeatTaps];
  __shared__ double ring[kBeatRing];
  const int lane = threadIdx.x, b = blockIdx.x;
  const BeatRec r = rec[b];
  if (!r.active) return;
  const HpssClip c = clips[b];
  const int T = c.T, fpb = r.fpb, dmin = max(r.lo, 1);     // distance 0 (fpb 1) scores -inf and never wins
  const double logf = log((double)fpb);
  for (int d = dmin + lane; d <= 2 * fpb; d += 64) {
    const double g = log((double)d) - logf;
    const double g2 = g * g;
    pen[d] = -(tightness * g2);
  }
  __syncthreads();
  const double thresh = 0.01 * r.maxls;
  const double* ls = localscore + c.frame_base;
  double* cum = cumscore + c.frame_base;
  int32_t* bl = backlink + c.frame_base;
  bool first = true;
  for (int i0 = 0; i0 < T; i0 += 64) {
    const int rows = min(64, T - i0);
    const double lsv = lane < rows ? ls[i0 + lane] : 0.0;  // the row's local scores; its results gather in the lanes
    double cumv = 0.0;
    int blv = -1;
    for (int j = 0; j < rows; ++j) {
      const int i = i0 + j, dmax = min(2 * fpb, i);
      double best = -INFINITY;
      int bd = INT_MAX;
      for (int d = dmin + lane; d <= dmax; d += 64) {      // ascending d and a strict comparison: the lane's nearest maximum
        const double sc = ring[(i - d) & (kBeatRing - 1)] + pen[d];
        if (sc > best) { best = sc; bd = d; }
      }
      const double top = bt_wave_max(best);
      unsigned long long tie = __ballot(bd != INT_MAX && best == top);
      int d = INT_MAX;
      while (tie) {                                        // of equal scores the smallest distance (uniform loop)
        const int l = __ffsll((long long)tie) - 1;
        d = min(d, __builtin_amdgcn_readlane(bd, l));
        tie &= tie - 1;
      }
      const double lsi = bt_readlane_d(lsv, j);
      const double cv = d != INT_MAX ? lsi + top : lsi;
      int link = -1;
      if (!(first && lsi < thresh)) { link = d != INT_MAX ? i - d : -1; first = false; }
      if (lane == j) { cumv = cv; blv = link; }
      if (lane == 0) ring[i & (kBeatRing - 1)] = cv;
      __syncthreads();
    }
    if (lane < rows) { cum[i0 + lane] = cumv; bl[i0 + lane] = blv; }
  }
}

// ---- the last beat, the backtrack, the trim -------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_beat_finish(const HpssClip* __restrict__ clips, const double* __restrict__ localscore,
                                                    const double* __restrict__ cumscore, const int32_t* __restrict__ backlink,
                                                    int trim, unsigned long long* __restrict__ keys,
                                                    uint8_t* __restrict__ beats, BeatRec* __restrict__ rec) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x, b = blockIdx.x;
  if (!rec[b].active) return;
  const HpssClip c = clips[b];
  const int T = c.T;
  const double* ls = localscore + c.frame_base;
  const double* cum = cumscore + c.frame_base;
  const int32_t* bl = backlink + c.frame_base;
  unsigned long long* key = keys + c.frame_base;
  // a lane writes and later reads only the frames lane, lane + 64, ...: its own stores.  Not a local maximum: the largest key
  // (a NaN is never a maximum, so no score maps there)
  int n = 0;
  for (int i = lane; i < T; i += 64) {
    const double v = cum[i];
    const bool mx = v > cum[max(i - 1, 0)] && v >= cum[min(i + 1, T - 1)];
    key[i] = mx ? bt_key(v) : ~0ull;
    n += mx;
  }
  n = bt_wave_sum_i(n);
  if (n == 0) return;
  // the (n - 1) / 2-th smallest key: the smallest K with count(key <= K) > (n - 1) / 2, found bit by bit from the top
  const int k = (n - 1) / 2;
  unsigned long long K = 0;
  for (int bit = 63; bit >= 0; --bit) {
    const unsigned long long probe = K | ((1ull << bit) - 1);   // the largest key with this prefix and the bit clear
    int cnt = 0;
    for (int i = lane; i < T; i += 64) cnt += key[i] <= probe;
    if (bt_wave_sum_i(cnt) <= k) K |= 1ull << bit;
  }
  double med = bt_unkey(K);
  if ((n & 1) == 0) {                                      // the next one up: K again when it repeats, else the smallest above
    int cnt = 0;
    unsigned long long up = ~0ull;
    for (int i = lane; i < T; i += 64) {
      const unsigned long long q = key[i];
      cnt += q <= K;
      if (q > K && q < up) up = q;
    }
    cnt = bt_wave_sum_i(cnt);
    up = bt_wave_min_u64(up);
    const double hi = cnt >= k + 2 ? med : bt_unkey(up);
    med = (med + hi) * 0.5;
  }
  const double half = 0.5 * med;
  int tail = -1;
  for (int i = lane; i < T; i += 64)
    if (key[i] != ~0ull && cum[i] >= half) tail = i;
  tail = bt_wave_max_i(tail);
  if (tail < 0 || lane != 0) return;
  // one lane walks the chain from the last beat back, as afx_beat_track_host does
  int keep_lo = 0, keep_hi = tail;
  if (trim) {
    double sum = 0.0, later = 0.0;
    int nb = 0;
    for (int f = tail; f >= 0; f = bl[f]) {
      const int p = bl[f];
      const double here = ls[f], earlier = p >= 0 ? ls[p] : 0.0;
      const double sm = (0.5 * earlier + here) + 0.5 * later;
      const double sm2 = sm * sm;
      sum += sm2;
      later = here;
      ++nb;
    }
    const double th = 0.5 * sqrt(sum / (double)nb);
    keep_lo = keep_hi = -1;
    later = 0.0;
    for (int f = tail; f >= 0; f = bl[f]) {
      const int p = bl[f];
      const double here = ls[f], earlier = p >= 0 ? ls[p] : 0.0;
      const double sm = (0.5 * earlier + here) + 0.5 * later;
      if (sm > th) { if (keep_hi < 0) keep_hi = f; keep_lo = f; }
      later = here;
    }
    if (keep_hi < 0) return;
  }
  uint8_t* o = beats + c.frame_base;
  int nb = 0;
  for (int f = tail; f >= 0; f = bl[f])
    if (f >= keep_lo && f <= keep_hi) { o[f] = 1; ++nb; }
  rec[b].n_beats = nb;
}

// ---------------------------------------------------------------------------------------------------------------------
hipError_t launch_beat_stage(hipStream_t s, const float* in, const HpssClip* clips, int n, float* env, uint32_t* bad) {
  hipLaunchKernelGGL(k_beat_stage, dim3(n), dim3(256), 0, s, in, clips, env, bad);
  return hipGetLastError();
}

hipError_t launch_beat_score(hipStream_t s, const float* env, const HpssClip* clips, const uint32_t* bad, int n,
                             const double* res, const double* bpm_in, double fps, double* x, double* localscore, BeatRec* rec) {
  hipLaunchKernelGGL(k_beat_score, dim3(n), dim3(kBeatThreads), 0, s, env, clips, bad, res, bpm_in, fps, x, localscore, rec);
  return hipGetLastError();
}

hipError_t launch_beat_dp(hipStream_t s, const HpssClip* clips, int n, const BeatRec* rec, const double* localscore,
                          double tightness, double* cumscore, int32_t* backlink) {
  hipLaunchKernelGGL(k_beat_dp, dim3(n), dim3(64), 0, s, clips, rec, localscore, tightness, cumscore, backlink);
  return hipGetLastError();
}

hipError_t launch_beat_finish(hipStream_t s, const HpssClip* clips, int n, const double* localscore, const double* cumscore,
                              const int32_t* backlink, int trim, uint64_t* keys, uint8_t* beats, BeatRec* rec) {
  hipLaunchKernelGGL(k_beat_finish, dim3(n), dim3(64), 0, s, clips, localscore, cumscore, backlink, trim,
                     (unsigned long long*)keys, beats, rec);
  return hipGetLastError();
}

}  // namespace afx
