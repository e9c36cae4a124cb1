// Spectral-gating noise reduction (afx_gate.hip): noisereduce's reduce_noise, stationary and non-stationary, on scipy's
// STFT grid at n_fft 1024 / hop 256 or 2048 / 512 (04_feature_extraction_experiment/process_audio.py:82-98).  The grid
// records, the derived parameters, the cost record and the launchers.  Internal to libafx.so.
#pragma once
#include <cstdint>

#include <hip/hip_runtime_api.h>

#include "afx.h"
#include "afx_hpss.h"

namespace afx {

constexpr int kGateMaxNf = 128;            // most bins / frames on one side of the smoothing filter
constexpr int kGateMaxNt = 64;
constexpr int kGateMaxPad = 1 << 20;       // samples of zero padding on each side of a clip
constexpr int kGateMaxChunk = 1 << 24;     // longest clip the entry point can be asked to take (chunk_size)

__host__ __device__ constexpr int gate_bins(int n_fft) { return n_fft / 2 + 1; }
// float32 per frame row of a magnitude / mask plane (513 -> 528, 1025 -> 1040: 64-byte aligned rows)
__host__ __device__ constexpr int gate_pitch(int n_fft) { return (n_fft / 2 + 1 + 15) / 16 * 16; }
// uint32 per frame row of the hard-mask bit plane: bit (b & 31) of word b >> 5
__host__ __device__ constexpr int gate_words(int n_fft) { return (n_fft / 2 + 1 + 31) / 32; }

// One STFT grid of one clip (host-built): the signal grid over padding + clip + padding, or the noise grid over the noise
// clip alone.  Frame t covers the samples [t hop - n_fft / 2 - shift, .. + n_fft) of the clip; only the frames ta .. ta + na - 1
// reach a sample of it ("active"), every other frame of the grid is zero.
struct GateGrid {
  int64_t y_off;        // sample 0 in the chunk's float32 signal buffer
  int64_t out_off;      // signal grid: sample 0 in the output the overlap-add writes
  int64_t len;          // samples
  int64_t row_base;     // row of frame 0 in the grid's planes
  int64_t unit_base;    // first unit of the clip in a frame launch (a unit is one wave: one frame at 2048, two at 1024)
  int64_t arow_base;    // signal grid: row of frame ta in the time-domain rows the overlap-add reads
  int32_t T;            // frames
  int32_t ta, na;       // the active frames
  int32_t shift;        // the padding in front of the clip (0 on the noise grid)
  int32_t clip;         // the clip's place in the chunk (its flags are bad[clip] and bad[n + clip])
  int32_t pad_;
};

// What the options derive to (gate_derive; afx_gate_params hands it to a caller without a device)
struct GateDerived {
  int n_f, n_t;         // noisereduce's n_grad_freq, n_grad_time
  bool smooth;          // false when both are 1
  double beta;          // the non-stationary recurrence's coefficient
  double vf[2 * kGateMaxNf + 1], vt[2 * kGateMaxNt + 1];   // the taps of each axis, each normalised to sum 1
};
// AFX_OK, or AFX_ERR_INVALID / AFX_ERR_UNSUPPORTED with `why` set (afx_gate_host.cpp; no device)
int gate_derive(const afx_gate_opts& o, GateDerived& d, const char** why);
inline int64_t gate_frames(int64_t len, int hop, int pad) { return 1 + (len + 2 * (int64_t)pad) / hop; }
// the active frames of the signal grid of a clip of len >= 1 samples
inline void gate_active(int64_t len, int n_fft, int hop, int pad, int64_t T, int32_t* ta, int32_t* na) {
  // frame t holds the chunk samples [t hop - n_fft / 2, t hop + n_fft / 2); the clip is [pad, pad + len)
  int64_t lo = pad - n_fft / 2 < 0 ? 0 : (pad - n_fft / 2) / hop + 1;            // first t with t hop + n_fft / 2 > pad
  int64_t hi = (pad + len + n_fft / 2 - 1) / hop;                               // last t with t hop - n_fft / 2 < pad + len
  if (hi > T - 1) hi = T - 1;
  if (lo > hi) { *ta = 0; *na = 0; return; }
  *ta = (int32_t)lo; *na = (int32_t)(hi - lo + 1);
}
// What a clip costs a chunk of afx_gate_batch, in cut_stft_chunk's units (frames of hop 512)
void gate_cost(int n_fft, int stationary, int padding, int sample_fmt, int mem_kind, int out_mem_kind, int with_noise, StftCost& cost);

struct GateTabs {
  const float* window;  // periodic Hann of n_fft floats
  const float* w1024;   // exp(-2 pi i k / 1024), k < 1024, float2
  const float* w2048;   // exp(-2 pi i k / 2048), k < 1024, float2 (n_fft 2048 only)
  const double* vf;     // 2 n_f + 1 taps
  const double* vt;     // 2 n_t + 1 taps
};

// |X| of every active frame of the grids into plane rows (row_base + t) of gate_pitch floats; the plane is zeroed first
hipError_t launch_gate_mag(hipStream_t s, int n_fft, const float* y, const GateGrid* grids, const uint32_t* bad, int n,
                           int64_t n_units, GateTabs tb, float* plane);
// stationary, per (clip, bin), float64 in a fixed order: the noise rows' maximum, mean and std in dB -> thr (dB) and the
// amplitude the signal grid is compared with (-1 where the signal row's floor passes every frame)
hipError_t launch_gate_stats(hipStream_t s, int n_fft, const GateGrid* sig, const GateGrid* noise, int n, const float* mag,
                             const float* nmag, double n_std, double* thr, double* amp);
// the hard mask of every frame of the signal grids as bit rows of gate_words words
hipError_t launch_gate_hard(hipStream_t s, int n_fft, const GateGrid* sig, int n, int64_t n_rows, const float* mag,
                            const double* amp, uint32_t* bits);
// non-stationary, per (clip, bin): filtfilt([beta], [1, beta - 1]) along time in float64 (fwd holds the forward pass), the
// sigmoid mask over |X| in place
hipError_t launch_gate_recur(hipStream_t s, int n_fft, const GateGrid* sig, int n, double beta, double n_mult, double slope,
                             float* mag, double* fwd);
// the smoothed mask: +- n_t frames, then +- n_f bins, zero beyond the array's four edges; bits != nullptr: of
// bit p + (1 - p); else of the plane, and p out + (1 - p) behind it
hipError_t launch_gate_smooth(hipStream_t s, int n_fft, const GateGrid* sig, int n, int64_t n_rows, const uint32_t* bits,
                              const float* plane, int n_f, int n_t, double p, GateTabs tb, float* mask);
// every active frame again: FFT, x mask, inverse FFT, x window, as rows of n_fft floats at arow_base + t - ta
hipError_t launch_gate_apply(hipStream_t s, int n_fft, const float* y, const GateGrid* sig, const uint32_t* bad, int n,
                             int64_t n_units, GateTabs tb, const float* mask, float* rows);
// overlap-add as a gather in increasing frame order, / the overlap-added window^2 where that exceeds 1e-10, cut to the clip
hipError_t launch_gate_ola(hipStream_t s, int n_fft, const float* rows, const GateGrid* sig, const uint32_t* bad, int n,
                           int64_t max_len, GateTabs tb, float* out);

}  // namespace afx
