// Onset strength, tempogram and tempo (afx_rhythm.hip): librosa.onset.onset_strength, librosa.feature.tempogram at the
// window beat_track gives it (int(8 sr) // 512 frames) and librosa.feature.tempo's decision, at librosa's defaults, on the
// 2048 / 512 Hann power spectrum that launch_hpss_stft_power leaves on the device (tests/rhythm_ref.py is the spec).
// Geometry and the launchers.  Internal to libafx.so.
//
// The clip records are afx_hpss.h's HpssClip (the front end is HPSS's prep + STFT); tile_base counts the clip's 16-frame
// tiles, as in afx_chroma.h, and spec_off is unused.  The mel bank is afx_chroma.h's ChromaMel.
#pragma once
#include <cstdint>

#include <hip/hip_runtime_api.h>

#include "afx_chroma.h"
#include "afx_hpss.h"

namespace afx {

constexpr int kRhMels = 16 * kChromaMelGroups;        // floats per frame row of the dB workspace (bands past n_mels unused)
constexpr int kRhMaxWin = 768;                        // tempogram window (lags) the kernels hold: sr <= 49215 at hop 512
constexpr int kRhTile = 16;                           // frames per k_rhythm_tempogram workgroup: 4 waves x 4 frames
constexpr int kRhOnsetLag = 3;                        // zeros in front of the envelope: lag 1 + n_fft / (2 hop)

// the plan's table: bpm[win], logprior[win] (afx_tempo_table), then window[win] (periodic Hann, float32)
struct RhythmTab {
  const float* window;
  const double* bpm;
  const double* logprior;
  int32_t win;                                        // lags = frames of the autocorrelation window
};

// mel contraction of the power rows: db[(frame_base + t) * kRhMels + m] = 10 log10(max(1e-10, mel[m, t])) (float32, not
// yet clamped) and clip_max[c] = the bits of the clip's largest mel power (integer atomic max; zeroed by the caller)
hipError_t launch_rhythm_mel(hipStream_t s, const float* S, const HpssClip* clips, int n, int n_tiles, ChromaMel mel,
                             float* db, uint32_t* clip_max);
// env[frame_base + t]: 0 for t < 3, else the mean over the bands of max(0, dB[m, t - 2] - dB[m, t - 3]) with dB clamped
// at the clip's maximum - 80
hipError_t launch_rhythm_env(hipStream_t s, const float* db, const uint32_t* clip_max, const HpssClip* clips, int n,
                             int64_t n_frames, int n_mels, float* env);
// per frame: the windowed autocorrelation of the padded envelope divided by its largest magnitude; parts[tile * win + k] =
// the float64 sum of lag k over the tile's frames in a fixed order; tg != nullptr: the tempogram itself, win x T row-major
// per clip at win * frame_base
hipError_t launch_rhythm_tempogram(hipStream_t s, const float* env, const HpssClip* clips, int n, int n_tiles, RhythmTab tab,
                                   double* parts, float* tg);
// per clip, float64 in a fixed order: acmean[c * win + k]; res[4 c ..] = tempo, mean(env), std(env), lag (first maximum of
// log1p(1e6 acmean) + logprior; lag 0 and tempo 0 when the envelope is all zero)
hipError_t launch_rhythm_reduce(hipStream_t s, const float* env, const HpssClip* clips, int n, RhythmTab tab,
                                const double* parts, double* acmean, double* res);

}  // namespace afx
