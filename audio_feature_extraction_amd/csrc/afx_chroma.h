// Chroma, tuning estimate and mel power (afx_chroma.hip): librosa.feature.chroma_stft / estimate_tuning / melspectrogram at
// librosa's defaults on the 2048 / 512 Hann power spectrum that launch_hpss_stft_power leaves on the device
// (tests/chroma_ref.py is the spec).  Table geometry and the launchers.  Internal to libafx.so.
//
// The clip records are afx_hpss.h's HpssClip (the front end is HPSS's prep + STFT); here tile_base counts the clip's
// 16-frame tiles (k_chroma_apply) and spec_off is unused.
#pragma once
#include <cstdint>

#include <hip/hip_runtime_api.h>

#include "afx_hpss.h"

namespace afx {

constexpr int kChromaSteps = kHpssPowPitch / 16;      // 65 steps of 16 bins cover a row
constexpr int kChromaImg = kChromaSteps * 4 * 64;     // floats of one filterbank as MFMA A images (66 560 B)
constexpr int kChromaGrid = 100;                      // tunings -0.5 + 0.01 k: the per-plan table holds all of them
constexpr int kChromaMelGroups = 8;                   // 16 mel filters per group: n_mels <= 128
constexpr int kChromaHist = 102;                      // per clip: peaks, kept, counts[100]

// A image of step s, sub-step c (k_dct16's convention: lane (f, q) holds bins 16 s + 4 q + {0..3} of frame f in one
// 16-byte load): img[(4 s + c) * 64 + l] = W[l & 15][16 s + 4 (l >> 4) + c], zero for rows / bins that do not exist
struct ChromaMel {
  const float* img;                                   // group g's images of steps s0[g] .. s1[g] - 1 start at off[g] * 256 floats
  int32_t n_groups, n_mels;
  int32_t s0[kChromaMelGroups], s1[kChromaMelGroups], off[kChromaMelGroups];
};

// piptrack's band: bins kmin .. kmin + nr - 1 (150 Hz <= f < min(4000 Hz, sr / 2), inside 1 .. 1023)
struct ChromaBand {
  int32_t kmin, nr;
  float hz_per_bin;
};

// per (frame, band bin): the interpolated magnitude of a pitch peak (0: no peak) and the histogram bin 0 .. 99 of its
// tuning residual (255: no peak), dense at (frame_base + t) * nr + (k - kmin)
hipError_t launch_chroma_peaks(hipStream_t s, const float* S, int64_t n_frames, ChromaBand band, float* mag, uint8_t* bin);
// per clip: the median of the peak magnitudes (exact, radix select), the 100-bin count of the peaks at or above it, the first
// maximum -> slot[c] (50 when the clip has no peak); hist[c * kChromaHist ..]
hipError_t launch_chroma_tuning(hipStream_t s, const HpssClip* clips, int n, ChromaBand band, const float* mag,
                                const uint8_t* bin, int32_t* slot, int32_t* hist);
// filterbank slot[c] (< 100: grid, else extra + (slot - 100) images) x S, every frame divided by its maximum; the mel
// contraction of the same rows when mel_out or parts is given.  chroma at 12 frame_base + row T + t, mel at n_mels
// frame_base + row T + t, parts[4 (frame_base + t)] = sum, sum of squares of the frame's chroma and mel values
hipError_t launch_chroma_apply(hipStream_t s, const float* S, const HpssClip* clips, int n, int n_tiles, const int32_t* slot,
                               const float* grid, const float* extra, ChromaMel mel, bool want_mel, float* chroma_out,
                               float* mel_out, double* parts);
// per clip, float64 in a fixed order: mean and std of the mel matrix, mean and std of the chroma matrix
hipError_t launch_chroma_stats(hipStream_t s, const HpssClip* clips, int n, int n_mels, const double* parts, double* stats);

}  // namespace afx
