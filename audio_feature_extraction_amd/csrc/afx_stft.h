// librosa-style stft / istft at n_fft 1024 and 2048 (afx_stft.hip): any hop in [1, n_fft], any window table, center on or
// off, constant or reflect padding, istft's length rule.  Both frame lengths ride the 1024-point complex FFT of
// afx_hpss_dev.h: 2048 as one real frame per transform, 1024 as two.  The clip records, the frame arithmetic the host and
// the entry points share, the cost records and the launchers.  Internal to libafx.so.
#pragma once
#include <cstdint>

#include <hip/hip_runtime_api.h>

#include "afx.h"
#include "afx_hpss.h"

namespace afx {

__host__ __device__ constexpr int stft_bins(int n_fft) { return n_fft / 2 + 1; }

// One clip of a chunk of afx_stft_batch (host-built).  A unit is one wave: one frame at 2048, two at 1024.
struct StftClip {
  int64_t y_off;        // sample 0 in the chunk's float32 signal
  int64_t len;          // samples
  int64_t out_off;      // row 0 in the output, in output elements (complex64, or float32 for the magnitude kinds)
  int64_t unit_base;    // first unit of the clip in the frame launch
  int32_t T;            // frames
  int32_t clip;         // the clip's place in the chunk (its flag is bad[clip])
};

// One clip of a chunk of afx_istft_batch (host-built)
struct IstftClip {
  int64_t spec_off;     // row 0 of the spectrum, in complex64 elements
  int64_t row_base;     // first of the clip's time rows in the workspace
  int64_t unit_base;
  int64_t out_off;      // sample 0 in the output
  int64_t n_out;        // samples written
  int32_t n_frames;     // frames kept (istft's length rule)
  int32_t pad_;
};

struct StftTabs {
  const float* window;  // the caller's window, n_fft floats
  const float* w1024;   // exp(-2 pi i k / 1024), k < 1024, float2
  const float* w2048;   // exp(-2 pi i k / 2048), k < 1024, float2 (n_fft 2048 only)
};

// AFX_OK, or AFX_ERR_INVALID / AFX_ERR_UNSUPPORTED with `why` set (afx_stft_host.cpp; no device)
int stft_check_opts(const afx_stft_opts& o, const char** why);
// frames of a clip of `length` >= 0 samples and its status (T = 0 unless AFX_CLIP_OK)
void stft_frames(const afx_stft_opts& o, int64_t length, int64_t* T, int32_t* status);
// frames kept and samples written by istft of T >= 1 frames; length < 0: none given
void istft_samples(const afx_stft_opts& o, int64_t T, int64_t length, int64_t* n_frames, int64_t* n_out);
// what cut_stft_chunk is handed as a clip's length by afx_istft_batch: n_frames + ceil(n_out / hop)
inline int64_t istft_weight(const afx_stft_opts& o, int64_t n_frames, int64_t n_out) { return n_frames + (n_out + o.hop - 1) / o.hop; }
// What a clip costs a chunk, in bytes per unit of the length cut_stft_chunk sees: samples (forward), istft_weight (inverse)
void stft_cost(const afx_stft_opts& o, int sample_fmt, int mem_kind, int out_mem_kind, int inverse, StftCost& cost);

// rfft(frame x window) of every frame of the clips: complex64 rows of n_fft / 2 + 1 (AFX_STFT_COMPLEX), or |D| / |D|^2 as
// float32 rows of the same count; zeros for a clip whose flag is set
hipError_t launch_stft_frames(hipStream_t s, const afx_stft_opts& o, const float* y, const StftClip* clips, const uint32_t* bad,
                              int n, int64_t n_units, StftTabs tb, void* out);
// window x irfft of the kept rows of every clip, as rows of n_fft floats at row_base + t; a row with a NaN / inf bin gives a
// row of NaN and touches no other
hipError_t launch_istft_frames(hipStream_t s, int n_fft, const float2* spec, const IstftClip* clips, int n, int64_t n_units,
                               StftTabs tb, float* rows);
// overlap-add as a gather in increasing frame order with the overlap-added window^2 beside it, librosa's tiny rule, zeros
// beyond the last frame
hipError_t launch_istft_ola(hipStream_t s, const afx_stft_opts& o, const float* rows, const IstftClip* clips, int n,
                            int64_t max_out, StftTabs tb, float* out);

}  // namespace afx
