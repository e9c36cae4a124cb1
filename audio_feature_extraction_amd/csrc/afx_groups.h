// The fused pass over the spectral, harmonic, timbre and rhythm groups (afx_groups.hip, afx_groups_batch in
// afx_features.cpp): one STFT of y per chunk, every group reading the same rows.  The kernels of afx_hpss.hip,
// afx_chroma.hip, afx_rhythm.hip and afx_filt.hip are called as they are; what is new here works on the rows they leave:
//   k_groups_square   |X|^2 of the complex rows as launch_hpss_stft_power's rows (same expression, same bits)
//   k_spec_rows       one wave per stored power row: centroid (, bandwidth, roll-off, the 14 contrast band extremes)
//   k_spec_stats      per clip, float64: the eight spectral statistics with power_to_db's clip-global clamp
//   k_mfcc_rows       one wave per four frames of k_rhythm_mel's dB rows: clamp, DCT-II 128 -> 13, the frame's two sums
//   k_mfcc_stats      per clip, float64: mean and std of the 13 x T MFCC matrix
//   k_groups_record   per clip: the 24 doubles of afx_groups_batch, the tuning slot and the lag
// Geometry, the cost record and the launchers.  Internal to libafx.so.
#pragma once
#include <cstdint>

#include <hip/hip_runtime_api.h>

#include "afx_filt.h"
#include "afx_frames3.h"
#include "afx_hpss.h"
#include "afx_rhythm.h"

namespace afx {

constexpr int kGroupsStats = 24;           // doubles per clip of afx_groups_batch's out_stats
constexpr int kGroupsMfcc = 13;            // librosa.feature.mfcc's n_mfcc as the experiment extractor calls it
constexpr int kGroupsAll = 15;             // AFX_GROUP_SPECTRAL | _HARMONIC | _TIMBRE | _RHYTHM
constexpr int kGroupsPadlen = 18;          // scipy's default padlen of the experiment's 5th-order filter
constexpr int kGroupsMfccFrames = 4;       // frames a wave of k_mfcc_rows walks with the table in registers

// The StftCost of a chunk (afx_host.cpp; no device): the union of the buffers the asked groups keep, at the largest table
// sizes any plan has (768 lags, 1023 piptrack bins, 128 mel bands, float32 host samples), so that it needs no plan.
void groups_cost(int groups, bool preprocess, StftCost& cost);
// rows k < 13 of the orthonormal DCT-II of n_mels points, float64 rounded once, as [13][128] (columns past n_mels zero)
void groups_dct_table(int n_mels, float* out);

// what k_groups_record gathers; a null pointer is a group that was not asked for (its fields are NaN)
struct GroupsSrc {
  const double* spec;      // [n][8]   k_spec_stats
  const double* harm;      // [n][4]   k_hpss_stats
  const double* chroma;    // [n][4]   k_chroma_stats
  const double* mfcc;      // [n][2]   k_mfcc_stats
  const double* rhythm;    // [n][4]   k_rhythm_reduce: tempo, mean, std, lag
  const double* acmean;    // [n][win]
  const int32_t* slot;     // [n]      k_chroma_tuning
  const FiltState* filt;   // [n]      the preprocess (peaks, bad)
  int32_t win;
};

#if defined(__HIP_PLATFORM_AMD__)
// S rows (kHpssPowPitch floats, the pad zeroed) = |X|^2 of the complex rows X (kHpssPitch float2)
hipError_t launch_groups_square(hipStream_t s, const float2* X, int64_t n_frames, float* S);
// full: the 17 floats of afx_spectral_batch's layout per row of S at desc[17 g]; else the centroid alone, at desc[17 g]
hipError_t launch_spec_rows(hipStream_t s, const float* S, int64_t n_frames, const SpecBands& sb, bool full, float* desc);
// stats[8 c ..] = mean, std of centroid, bandwidth, roll-off, contrast of clip c's rows desc[17 (frame_base + t)]
hipError_t launch_spec_stats(hipStream_t s, const float* desc, const HpssClip* clips, int n, double* stats);
// parts[2 g ..] = sum and sum of squares of frame g's 13 coefficients (db: launch_rhythm_mel's rows and clip maxima)
hipError_t launch_mfcc_rows(hipStream_t s, const float* db, const uint32_t* clip_max, const HpssClip* clips, int n,
                            int64_t n_frames, int n_mels, const float* dct, double* parts);
hipError_t launch_mfcc_stats(hipStream_t s, const double* parts, const HpssClip* clips, int n, double* stats);
// bad[c] |= the preprocess's non-finite flag of clip c
hipError_t launch_groups_mark_bad(hipStream_t s, const FiltState* st, int n, uint32_t* bad);
// rec[24 c ..], ints[2 c ..] = tuning slot, lag; a clip with bad[c] set has an all-NaN record
hipError_t launch_groups_record(hipStream_t s, const GroupsSrc& src, const HpssClip* clips, const uint32_t* bad, int n,
                                double* rec, int32_t* ints);
#endif

}  // namespace afx
