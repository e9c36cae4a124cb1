// ITU-R BS.1770-4 gated (integrated) loudness of mono clips and the gain that normalises them: geometry, the clip record,
// and the arithmetic the kernels of afx_loudness.hip and the host executor of afx_loudness_host.cpp share.  Internal to
// libafx.so; include/afx.h (afx_loudness_batch, afx_loudness_host, afx_kweight_sos, afx_loudness_geometry,
// afx_loudness_blocks, afx_loudness_cost) is the ABI.
//
// K-weighting is a causal cascade of two sections from zero state (scipy.signal.lfilter without zi), run with the block
// decomposition of afx_filt.h (S = 2): a clip is cut into blocks of kFiltL samples,
//   1. every block alone, from zero state: only its end state fin (nothing per sample is stored);
//   2. per clip: zin[k + 1] = T zin[k] + fin[k], zin[0] = 0;
//   3. every block again from its true entry state zin[k] -- in the per-section state basis that IS the sequential
//      recurrence, so there is no correction term --, squaring and summing its outputs in float64.
// The gating blocks of BS.1770 (length T_g, 75 % overlap) are four consecutive SEGMENTS with boundaries
// b_k = int(T_g * (k * 0.25) * rate), evaluated left to right in float64 (pyloudnorm's slice bounds; j * 0.25 + 1 ==
// (j + 4) * 0.25 exactly).  Rates whose shortest segment is under kFiltL samples are refused, so a block of the filter
// straddles at most one segment boundary and owns two partial sums: the part in the segment of its first sample, the rest.
// Every sum has one writer and one fixed order; there are no atomics.
#pragma once
#include "afx_filt.h"

namespace afx {

constexpr int kLoudS = 2;                      // sections of the K-weighting cascade
constexpr int kLoudZ = 2 * kLoudS;             // state slots of a block
constexpr int kLoudStride = kFiltL + 1;        // LDS row stride in float32: lane i on row i reads bank (i + m) % 64
constexpr int kLoudMinRate = 4000;             // the shelf's corner (1500 Hz) must lie well below Nyquist
constexpr int kLoudMaxRate = 192000;
constexpr int kLoudMaxRates = 16;              // distinct rates of one afx_loudness_batch call (one FiltTab each)
constexpr int kLoudRec = 8;                    // doubles a clip's gate leaves on the device (LoudDev)
constexpr int kLoudModeMeasure = 0, kLoudModeLoudness = 1, kLoudModePeak = 2;

// one clip of a chunk as the kernels see it
struct LoudClip {
  int64_t in_off, out_off, n;                  // sample offsets in the (staged or caller's) buffers
  int64_t seg_off, z_off;                      // first segment sum / first z_j of the clip in the chunk's workspace
  double tg, rate;                             // T_g (seconds) and the rate as doubles: the operands of b_k
  int32_t first_tile, n_tiles;
  int32_t n_blocks;                            // gating blocks (0: the clip is only scaled, peak mode)
  int32_t tab;                                 // which FiltTab
};
static_assert(sizeof(LoudClip) == 72, "LoudClip layout");

// what the gate leaves per clip (kLoudRec doubles)
enum { kLdBlocks = 0, kLdN1 = 1, kLdN2 = 2, kLdMean1 = 3, kLdMean2 = 4, kLdMeanAll = 5, kLdPeak = 6, kLdBad = 7 };

AFX_HD inline float loud_raw(const void* in, int fmt, int64_t i) {
  if (fmt == 1) return (float)((const int16_t*)in)[i] * (1.0f / 32768.0f);
  return ((const float*)in)[i];
}

// b_k: two rounded products, no sum to contract
AFX_HD inline int64_t loud_bound(double tg, double rate, int64_t k) { return (int64_t)(tg * ((double)k * 0.25) * rate); }

// the segment that holds sample s >= 0: the largest k with b_k <= s (an estimate, then exact steps)
AFX_HD inline int64_t loud_seg_of(double tg, double rate, int64_t s) {
  int64_t k = (int64_t)((double)s / (tg * 0.25 * rate));
  while (k > 0 && loud_bound(tg, rate, k) > s) --k;
  while (loud_bound(tg, rate, k + 1) <= s) ++k;
  return k;
}

// the samples the gating blocks cover: [0, min(n, b_{n_blocks + 3}))
AFX_HD inline int64_t loud_limit(double tg, double rate, int64_t n, int32_t n_blocks) {
  if (n_blocks <= 0) return 0;
  const int64_t e = loud_bound(tg, rate, (int64_t)n_blocks + 3);
  return e < n ? e : n;
}

// One block of the filter from its entry state z over samples x[0 .. kFiltL) (zeros past the clip): p[0] = the sum of y^2
// over steps m < split, p[1] over split <= m < stop; steps from stop on only advance the state.  get(m): sample m.
template <typename Get>
AFX_HD inline void loud_block_sums(const FiltSec* sec, double* z, int split, int stop, Get get, double* p) {
  double a0 = 0.0, a1 = 0.0;
  for (int m = 0; m < kFiltL; ++m) {
    const double y = filt_cascade<kLoudS>(sec, (double)get(m), z);
    if (m < split) a0 = fma(y, y, a0);
    else if (m < stop) a1 = fma(y, y, a1);
  }
  p[0] = a0; p[1] = a1;
}

// where a block that starts at sample s splits: (split, stop) of loud_block_sums
AFX_HD inline void loud_block_cut(double tg, double rate, int64_t s, int64_t lim, int* split, int* stop) {
  if (s >= lim) { *split = 0; *stop = 0; return; }
  const int64_t left = lim - s;
  const int st = left < kFiltL ? (int)left : kFiltL;
  const int64_t nb = loud_bound(tg, rate, loud_seg_of(tg, rate, s) + 1) - s;     // >= 1
  *stop = st;
  *split = nb < st ? (int)nb : st;
}

// the sum of segment k from the blocks' partial sums part[block][2], ascending: the second part of the block b_k falls
// into (its first part when b_k is a block's first sample), then the first parts of the blocks that start inside it
template <typename P>
AFX_HD inline double loud_seg_sum(double tg, double rate, int64_t lim, int64_t k, P part) {
  const int64_t b0 = loud_bound(tg, rate, k);
  int64_t b1 = loud_bound(tg, rate, k + 1);
  if (b1 > lim) b1 = lim;
  if (b0 >= b1) return 0.0;
  const int64_t q0 = b0 / kFiltL, q1 = (b1 - 1) / kFiltL;
  double a = part[2 * q0 + (b0 % kFiltL ? 1 : 0)];
  for (int64_t q = q0 + 1; q <= q1; ++q) a += part[2 * q];
  return a;
}

// z_j of gating block j from the segment sums
template <typename P>
AFX_HD inline double loud_z(P seg, int64_t j, double tg_rate) {
  return (((seg[j] + seg[j + 1]) + seg[j + 2]) + seg[j + 3]) / tg_rate;
}

// The order of the gate's sums: lane l of 64 adds its own terms j = l, l + 64, .. ascending, then a halving tree
// (v[l] += v[l + w], w = 32 .. 1).  Host form: f(j) -> the term (0 for a block outside the set).
template <typename F>
inline double loud_sum64_host(int64_t count, F f) {
  double v[64];
  for (int l = 0; l < 64; ++l) {
    double a = 0.0;
    for (int64_t j = l; j < count; j += 64) a += f(j);
    v[l] = a;
  }
  for (int w = 32; w > 0; w >>= 1)
    for (int l = 0; l < w; ++l) v[l] += v[l + w];
  return v[0];
}

// afx_loudness_host.cpp (host-only)
struct StftCost;
// nullptr, or why (rate, block_size) is refused; *code: AFX_ERR_INVALID / AFX_ERR_UNSUPPORTED
const char* loud_refusal(int rate, double block_size, int* code);
// gating blocks of a clip of n samples (pyloudnorm's numBlocks; 0 when n < block_size * rate)
int64_t loud_n_blocks(int64_t n, int rate, double block_size);
// the two sections and their tables
void loud_build_tab(int rate, FiltTab& t);
// the absolute gate in the linear domain: 10^((-70 + 0.691) / 10)
double loud_abs_gate();
// dev[kLoudRec] -> rec[AFX_LOUD_N] and the float32 gain (1 when nothing is to be scaled): host double arithmetic
float loud_finish(const double* dev, int mode, double target, double* rec);
void loud_cost(int sample_fmt, int mem_kind, int out_mem_kind, int mode, StftCost& cost);

}  // namespace afx

#if defined(__HIP_PLATFORM_AMD__) && !defined(AFX_FILT_HOST_ONLY)
namespace afx {
// afx_loudness.hip.  tabs, clips and every workspace: device memory; n: clip records; n_tiles: tiles of all records
// carry[block][kLoudZ] = the blocks' end states from zero state; tile_peak / tile_bad[tile] = max |x| and the non-finite flag
hipError_t launch_loud_ends(hipStream_t s, const void* in, int fmt, const FiltTab* tabs, const LoudClip* clips, int n, int n_tiles,
                            double* carry, float* tile_peak, uint32_t* tile_bad);
// carry[block] <- the state entering the block (the clip's first block: zero)
hipError_t launch_loud_scan(hipStream_t s, const FiltTab* tabs, const LoudClip* clips, int n, double* carry);
// part[block][2] = the block's partial sums of y^2
hipError_t launch_loud_sums(hipStream_t s, const void* in, int fmt, const FiltTab* tabs, const LoudClip* clips, int n, int n_tiles,
                            const double* carry, double* part);
// seg, z: the clips' segment sums and z_j; rec[clip][kLoudRec]
hipError_t launch_loud_gate(hipStream_t s, const LoudClip* clips, int n, const double* part, const float* tile_peak,
                            const uint32_t* tile_bad, double abs_gate, double* seg, double* z, double* rec);
// out = gain[clip] * x, one rounded float32 product per sample; a clip whose gain is NaN is not written
hipError_t launch_loud_gain(hipStream_t s, const void* in, int fmt, const LoudClip* clips, int n, int n_tiles, const float* gain,
                            float* out);
}  // namespace afx
#endif
