// The whole-clip DFT of any length and the spectral term of the PESQ-like score (afx_cfft.hip, afx_cfft_host.cpp):
// audio_quality_assessment.py:150-201, spec_dist = mean(| |fft(ref)| - |fft(deg)| | / (|fft(ref)| + 1e-10)).  Job records,
// geometry, the cost record and the launchers.  Internal to libafx.so; include/afx.h (afx_specdist_batch,
// afx_clip_fft_batch) is the ABI.
//
// Bluestein.  X[k] = w_k sum_j (x_j w_j) conj(w_{k-j}) with the chirp w_k = exp(-i pi k^2 / N): a circular convolution of
// a_j = x_j w_j (zeros from N on) with b_j = conj(w_j) wrapped to the power of two M >= 2 N - 1, done as
// IFFT_M(FFT_M(a) FFT_M(b)).  The phase is reduced in integers (k^2 mod 2 N in 64 bits, then one sincospi), so it is
// as good at k = 2^21 as at k = 1.  FFT_M(b) depends on N alone: one per distinct N of a chunk.
//
// The power-of-two transform.  A workgroup of 256 lanes transforms a tile of 4096 complex128 points held in LDS (64 KB)
// by radix-2 butterflies: decimation in frequency forwards (natural order in, bit-reversed out), decimation in time
// backwards (bit-reversed in, natural out).  A convolution needs no reordering in between: both spectra are in the same
// permuted order.  M <= 4096 is one kernel for the whole chain.  A larger M = M1 M2 (M1 = 2^floor(log2 M / 2) <= M2 <= 2048)
// is the four-step form in three passes over the M points, element e = n1 M2 + n2 throughout:
//   columns forwards   chirp product on load, transforms of length M1 over n1 for 4096 / M1 adjacent n2 per workgroup
//   rows               twiddle exp(-2 pi i n2 k1 / M), transforms of length M2 over n2 for 4096 / M2 rows per workgroup
//                      (4096 adjacent points), filter product, the same transforms backwards, conjugate twiddle
//   columns backwards  transforms of length M1, chirp product and 1 / M on store, the N points kept
// Stage twiddles come from one float64 table exp(-2 pi i j / 4096), j < 2048, built on the host and kept in the context.
#pragma once
#include <cstdint>

#include "afx.h"
#include "afx_hpss.h"

namespace afx {

constexpr int kCfLanes = 256;                 // lanes of a workgroup of the transform kernels
constexpr int kCfTailLanes = 1024;            // ... of the tail: one workgroup per pair, so a wide one
constexpr int kCfTileLog = 12;
constexpr int kCfTile = 1 << kCfTileLog;      // complex128 points of a workgroup's tile: 64 KB of LDS
constexpr int64_t kCfMaxN = AFX_CFFT_MAX_N;   // M <= 2^22: M1 = M2 = 2048
constexpr int kCfBad = 1, kCfDiffers = 2;     // what a lane saw while loading: a NaN / inf sample; r_j != d_j

// one transform as the kernels see it: a pair (z = r + i d), a clip (d_off < 0: no imaginary part) or a filter (n only)
struct CfJob {
  int64_t r_off, d_off; // element offsets of the two sides in the buffers the kernels read
  int64_t n;            // N >= 1
  int64_t work_off;     // complex offset of the job's M points in the work buffer (a filter job: in the filter buffer)
  int64_t filt_off;     // complex offset of the spectrum of the filter of this N
  int64_t blk_base;     // first workgroup of the job in the passes of the four-step form
  int32_t logM, logM1;  // M = 2^logM; logM1 = 0 for M <= kCfTile
};
static_assert(sizeof(CfJob) == 56, "CfJob layout");

// smallest power of two M >= 2 n - 1 (n >= 1), as its logarithm; M < 4 n
inline int cf_log_m(int64_t n) {
  int l = 0;
  while (((int64_t)1 << l) < 2 * n - 1) ++l;
  return l;
}
inline int cf_log_m1(int logM) { return logM <= kCfTileLog ? 0 : logM / 2; }
// workgroups of one pass over a job
inline int64_t cf_tiles(int logM) { return logM <= kCfTileLog ? 1 : (int64_t)1 << (logM - kCfTileLog); }

// What a pair (or clip) costs a chunk (afx_cfft_host.cpp; no device): 16 M bytes of work and, counted for every pair though
// pairs of one N share it, 16 M of filter spectrum; M < 4 n, so 128 bytes a sample, plus the uploads.
void specdist_cost(int sample_fmt, int mem_kind, StftCost& cost);

// exp(-2 pi i j / 4096), j < 2048, as (re, im) pairs: 4096 doubles
void cf_twiddle_table(double* out);

}  // namespace afx

#ifdef __HIP_PLATFORM_AMD__
#include <hip/hip_runtime_api.h>
namespace afx {
// afx_cfft.hip.  jobs (device): n_small jobs of M <= kCfTile, then n_large of the four-step form whose passes take
// large_blocks workgroups.  The filter launch leaves FFT_M(b) at filt + work_off of each job; the signal launch reads
// filt + filt_off and leaves the N points of the DFT at work + work_off.  flags (two words per job, zeroed by the caller):
// flags[2 q] = 1 for a job with a NaN / inf sample, flags[2 q + 1] = 1 for a pair whose two sides are not the same samples.
hipError_t launch_cfft_filters(hipStream_t s, const CfJob* jobs, int n_small, int n_large, int large_blocks,
                               const double* tw, double* filt);
hipError_t launch_cfft(hipStream_t s, const void* ref, const void* deg, int sample_fmt, const CfJob* jobs, int n_small,
                       int n_large, int large_blocks, const double* tw, const double* filt, double* work, int32_t* flags);
// rec: AFX_SPECDIST_N doubles per job (NaN for a bad one), from the spectra launch_cfft left
hipError_t launch_specdist_tail(hipStream_t s, const CfJob* jobs, int n_jobs, const double* work, const int32_t* flags,
                                double* rec);
}  // namespace afx
#endif
