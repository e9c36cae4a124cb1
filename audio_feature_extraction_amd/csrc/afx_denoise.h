// STFT-domain noise reduction (afx_denoise.hip): spectral subtraction and the Wiener filter of
// 00_audio_data_collection_experiment/noise_reduction.py:15-92 and the aligner's preprocess of
// 05_dtw_alignment_experiment/process_audio.py:9-54, on the 2048 / 512 Hann STFT of afx_hpss.h.  The cost record, the
// per-clip results and the launchers.  Internal to libafx.so.
#pragma once
#include <cstdint>

#include <hip/hip_runtime_api.h>

#include "afx_hpss.h"

namespace afx {

constexpr int kDnProfPitch = 1040;         // float32 per clip row of the noise profile (1025 bins; 4160 B, 64-byte aligned rows)
constexpr int kDnMaxNoiseFrames = 64;
constexpr int kDnInfo = 4;                 // doubles per clip: gain, VAD threshold, speech frames, VAD frames

// the energy VAD's framing: librosa.feature.rms(frame_length=fl, hop_length=hop, center=True) over the L' kept samples
struct DnVad {
  int fl, hop;          // int(0.025 sr), int(0.010 sr); fl == 0: no VAD
};
// VAD frames of a clip whose denoised signal has Lp samples (0 when there is none)
__host__ __device__ inline int64_t dn_vad_frames(int64_t Lp, int fl, int hop) { return Lp < 512 ? 0 : 1 + (Lp + 2 * (int64_t)(fl / 2) - fl) / hop; }

// What a clip costs a chunk of afx_denoise_batch (afx_host.cpp; no device): one row buffer per frame; y, the output and
// the upload per sample, with the VAD one float more (a clip of L samples has at most L + 1 VAD frames: hop >= 1); the
// profile row, the record and the info per clip.
void denoise_cost(int flags, int sample_fmt, int mem_kind, StftCost& cost);

// info[c] = {gain, NaN, 0, 0}: gain = fl32(0.1 / (sqrt(sum y^2 / len) + 1e-6)) with the sum in float64 in a fixed order
// (rms_gain), else 1
hipError_t launch_dn_gain(hipStream_t s, const float* y, const HpssClip* clips, int n, bool rms_gain, double* info);
// prof[c] = mean over the first min(T, noise_frames) frames of |X| (power: |X|^2) of fl32(y gain), summed in increasing t
hipError_t launch_dn_profile(hipStream_t s, const float* y, const HpssClip* clips, const uint32_t* bad, int n, int noise_frames,
                             bool power, const double* info, HpssTabs tb, float* prof);
// every frame: STFT of fl32(y gain), the gain of its clip's profile row, irfft x window as rows of kHpssPitch float2 (what
// launch_hpss_ola reads); zeros for a bad clip
hipError_t launch_dn_frames(hipStream_t s, const float* y, const HpssClip* clips, const uint32_t* bad, int n, int64_t n_frames,
                            bool wiener, float beta, const double* info, const float* prof, HpssTabs tb, float2* rows);
// e[y_off + c + i] = RMS of VAD frame i of d[0, L'); then info[c][1..3] = threshold fl32(0.5 mean e), frames above it, frames
hipError_t launch_dn_vad(hipStream_t s, const float* d, const HpssClip* clips, const uint32_t* bad, int n, int64_t max_len,
                         DnVad vad, float* e, double* info);
// in place: d[j] = 0 for j >= L' and for a bad clip; with the VAD also outside the uncentred windows of the speech frames
hipError_t launch_dn_finish(hipStream_t s, float* d, const HpssClip* clips, const uint32_t* bad, int n, int64_t max_len,
                            DnVad vad, const float* e, const double* info);

}  // namespace afx
