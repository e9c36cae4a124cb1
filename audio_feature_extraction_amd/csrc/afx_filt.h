// Zero-phase IIR filtering (scipy.signal.filtfilt semantics, cascaded second-order sections) and the experiment extractor's
// preprocess_audio around it: geometry, tables, the clip record, and the arithmetic the kernels of afx_filt.hip and the host
// executor of afx_filt_host.cpp share.  Internal to libafx.so; include/afx.h (afx_sosfiltfilt_batch, afx_sosfiltfilt_host,
// afx_butter_sos, afx_filtfilt_geometry) is the ABI.
//
// A clip x[0 .. n) becomes the extended signal e[0 .. N), N = n + 2 padlen (odd extension, in the samples' own float32 as
// scipy computes it for a float32 array).  e is cut into blocks of kFiltL samples.  A pass over e is
//   1. every block alone, from zero state (the pass's first block from the pass's true initial state): outputs and the
//      block's end state fin;
//   2. per clip, over its blocks in pass order: zin[k + 1] = T zin[k] + fin[k], zin[first] = 0   (T: kFiltL zero-input steps);
//   3. out[m] += R[m] . zin[block]                                    (R[m]: output of zero-input step m per unit state).
// The state is the per-section transposed-direct-form-II pair of every section, in float64: in that basis the blocked result
// is the sequential one to rounding at every rate (the companion basis of a (b, a) recursion is not: DESIGN.md).  R and T
// are built by running the section recurrences over kFiltL zero samples from unit states, never by matrix powers.
// The backward pass runs over the same blocks from the end: its first block is the clip's last, possibly partial, one, and
// starts from the true state (steady state times the forward pass's last output), so T is only ever applied to full blocks.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define AFX_HD __host__ __device__
#else
#define AFX_HD
#endif

namespace afx {

constexpr int kFiltL = 64;                     // samples of a block (one lane walks one block)
constexpr int kFiltB = 64;                     // blocks of a tile (one wave walks one tile)
constexpr int kFiltTile = kFiltL * kFiltB;     // extended samples of a tile
constexpr int kFiltStride = kFiltL + 1;        // LDS row stride in float64: 64 lanes on 64 rows read 32 distinct bank pairs per half-wave
constexpr int kFiltMaxS = 4;                   // sections (orders 1 .. 8)
constexpr int kFiltZ = 2 * kFiltMaxS;          // state slots of a block's carry record (2 S used)
constexpr int kFiltMaxPad = kFiltTile;         // padlen bound
constexpr int kFiltModePlain = 0, kFiltModeExperiment = 1;

struct FiltSec { double b0, b1, b2, a1, a2; };

struct FiltTab {
  FiltSec sec[kFiltMaxS];
  double zi[kFiltZ];                           // steady state of the cascade for a unit step (scipy.signal.sosfilt_zi)
  double R[kFiltL][kFiltZ];
  double T[kFiltZ][kFiltZ];                    // T[i][j]: state i after kFiltL zero-input steps from unit state j
};

// one clip of a chunk as the kernels see it (clips with n <= padlen never get a record)
struct FiltClip {
  int64_t in_off, out_off, n;                  // sample offsets in the (staged or caller's) buffers
  int32_t first_tile, n_tiles;
};
static_assert(sizeof(FiltClip) == 32, "FiltClip layout");

struct FiltState {
  double peak_out;                             // max |y| of the filter output, float64
  float peak_in;                               // max |x|
  uint32_t bad;                                // 1: a NaN / inf sample
};
static_assert(sizeof(FiltState) == 16, "FiltState layout");

// what turns the stored samples into the filter's input
struct FiltIn {
  const void* in;
  int64_t off, n;
  int fmt;                                     // AFX_FMT_*
  int mode;
  float peak, coef;                            // experiment mode: divide by peak when norm, then y[i] + coef * y[i - 1]
  int norm;
  int32_t padlen;
};

// float32 operations rounded one by one (never contracted into a fused multiply-add): librosa's pre-emphasis is
// scipy.signal.lfilter on float32, one rounded product and one rounded sum per sample.  HIP's __fmul_rn / __fadd_rn are plain
// * and + and would fuse: the pragma takes the licence away from these operations, wherever they are inlined.  (A compiler
// that does not know the pragma builds host code only, for a target without a fused instruction; volatile keeps it honest.)
#if defined(__clang__)
#define AFX_FILT_NO_CONTRACT _Pragma("clang fp contract(off)")
#define AFX_FILT_ROUNDED const float
#else
#define AFX_FILT_NO_CONTRACT
#define AFX_FILT_ROUNDED volatile float
#endif
// y + coef * prev
AFX_HD inline float filt_pre(float y, float prev, float coef) {
  AFX_FILT_NO_CONTRACT
  AFX_FILT_ROUNDED p = coef * prev;
  return y + p;
}
// 2 a - b (the product is exact)
AFX_HD inline float filt_odd(float a, float b) {
  AFX_FILT_NO_CONTRACT
  AFX_FILT_ROUNDED t = 2.0f * a;
  return t - b;
}

AFX_HD inline float filt_raw(const FiltIn& f, int64_t i) {
  if (f.fmt == 1) return (float)((const int16_t*)f.in)[f.off + i] * (1.0f / 32768.0f);
  return ((const float*)f.in)[f.off + i];
}
// librosa.util.normalize in float32: y / max|y| (a correctly rounded division), unchanged below tiny(float32)
AFX_HD inline float filt_scaled(const FiltIn& f, int64_t i) {
  const float x = filt_raw(f, i);
  return f.norm ? x / f.peak : x;
}
// the filter's input u[i], 0 <= i < n.  Experiment mode: librosa.effects.preemphasis in float32 with its initial state
// zi = 2 y[0] - y[1]  (u[0] = y[0] + zi)
AFX_HD inline float filt_u(const FiltIn& f, int64_t i) {
  const float y = filt_scaled(f, i);
  if (f.mode == kFiltModePlain) return y;
  if (i == 0) {
    AFX_FILT_NO_CONTRACT
    AFX_FILT_ROUNDED zi = f.n > 1 ? filt_odd(y, filt_scaled(f, 1)) : y;
    return y + zi;
  }
  return filt_pre(y, filt_scaled(f, i - 1), f.coef);
}
// the extended signal e[j], 0 <= j < n + 2 padlen (scipy.signal._arraytools.odd_ext on a float32 array: float32 arithmetic)
AFX_HD inline double filt_e(const FiltIn& f, int64_t j) {
  const int64_t p = f.padlen;
  if (j < p) return (double)filt_odd(filt_u(f, 0), filt_u(f, p - j));
  if (j < p + f.n) return (double)filt_u(f, j - p);
  return (double)filt_odd(filt_u(f, f.n - 1), filt_u(f, f.n - 2 - (j - p - f.n)));
}

// one sample through one section (transposed direct form II, the recurrence of scipy's sosfilt), every product fused into
// the sum it feeds: the host executor and the kernels round alike
AFX_HD inline double filt_step(const FiltSec& c, double x, double& z0, double& z1) {
  const double y = fma(c.b0, x, z0);
  z0 = fma(c.b1, x, fma(-c.a1, y, z1));
  z1 = fma(c.b2, x, -c.a2 * y);
  return y;
}

template <int S>
AFX_HD inline double filt_cascade(const FiltSec* sec, double x, double* z) {
#pragma unroll
  for (int s = 0; s < S; ++s) x = filt_step(sec[s], x, z[2 * s], z[2 * s + 1]);
  return x;
}

// out[m] += R[m] . zin: fixed order, fused
template <int S, typename RP, typename ZP>
AFX_HD inline double filt_correct(double v, RP Rm, ZP zin) {
#pragma unroll
  for (int j = 0; j < 2 * S; ++j) v = fma(Rm[j], zin[j], v);
  return v;
}

// z <- T z + fin
template <int S, typename TP>
AFX_HD inline void filt_carry(TP T, double* z, const double* fin) {
  double nz[2 * S];
#pragma unroll
  for (int i = 0; i < 2 * S; ++i) {
    double a = fin[i];
#pragma unroll
    for (int j = 0; j < 2 * S; ++j) a = fma(T[i][j], z[j], a);
    nz[i] = a;
  }
#pragma unroll
  for (int i = 0; i < 2 * S; ++i) z[i] = nz[i];
}

// afx_filt_host.cpp (host-only)
// checks the sections (finite, a0 == 1) and builds zi, R and T; false with the reason
bool filt_build_tab(const double* sos, int n_sections, FiltTab& t, const char** why);

}  // namespace afx

#if defined(__HIP_PLATFORM_AMD__) && !defined(AFX_FILT_HOST_ONLY)
#include <hip/hip_runtime_api.h>
namespace afx {
// afx_filt.hip.  tab, clips, st: device memory; n: clip records; n_tiles: tiles of all records; S: sections
// st[c] = max |x| and the non-finite flag of every clip
hipError_t launch_filt_peak(hipStream_t s, const void* in, int fmt, const FiltClip* clips, int n, FiltState* st);
// forward blocks: W[tile * kFiltTile ..) = the zero-state outputs, carry[block][kFiltZ] = the blocks' end states
hipError_t launch_filt_forward(hipStream_t s, const void* in, int fmt, int mode, float coef, int padlen, int S,
                               const FiltTab* tab, const FiltClip* clips, int n, int n_tiles, const FiltState* st, double* W,
                               double* carry);
// carry[block] <- the state correction entering the block; backward: blocks taken from the clip's last
hipError_t launch_filt_scan(hipStream_t s, int padlen, int S, const FiltTab* tab, const FiltClip* clips, int n,
                            const FiltState* st, double* carry, bool backward);
// forward correction, backward blocks and their end states, in place
hipError_t launch_filt_backward(hipStream_t s, int padlen, int S, const FiltTab* tab, const FiltClip* clips, int n, int n_tiles,
                                const FiltState* st, double* W, double* carry);
// backward correction and the per-tile max |y| over the clip's own samples; plain mode (out != nullptr): the float32 result
hipError_t launch_filt_final(hipStream_t s, int padlen, int S, const FiltTab* tab, const FiltClip* clips, int n, int n_tiles,
                             const FiltState* st, double* W, const double* carry, double* tile_max, float* out);
// st[c].peak_out = the largest of the clip's tile maxima
hipError_t launch_filt_clipmax(hipStream_t s, const FiltClip* clips, int n, const double* tile_max, FiltState* st);
// experiment mode: out = float32(y / peak_out), unchanged below tiny(float64)
hipError_t launch_filt_scale(hipStream_t s, int padlen, const FiltClip* clips, int n, int n_tiles, const FiltState* st,
                             const double* W, float* out);
}  // namespace afx
#endif
