// Harmonic-percussive separation (afx_hpss.hip): librosa.effects.hpss at librosa 0.11's defaults on a 2048 / 512 Hann
// STFT.  Workspace geometry, the per-clip record and the launchers.  Internal to libafx.so.
#pragma once
#include <cstdint>
#include <vector>

#include <hip/hip_runtime_api.h>

namespace afx {

constexpr int kHpssBins = 1025;            // n_fft / 2 + 1
constexpr int kHpssPitch = 1032;           // complex64 per frame row of the spectrum workspace (8256 B, 64-byte aligned rows)
constexpr int kHpssPowPitch = 1040;        // float32 per frame row of the power spectrum (launch_hpss_stft_power): 65 x 16 bins, 4160 B
constexpr int kHpssTile = 64;              // k_hpss_mask: 64 frames x 64 bins per workgroup
constexpr int kHpssBinTiles = 17;          // ceil(1025 / 64)
constexpr int kHpssHalo = 15;              // kernel_size 31

// One per clip of a chunk (host-built).  Clips of length 0 are not in the list.
struct HpssClip {
  int64_t in_off;       // element offset of sample 0 in the input the kernels read (the chunk's upload, or the caller's buffer)
  int64_t y_off;        // offset of sample 0 in the chunk's float32 signal buffers (y, h, p)
  int64_t len;          // samples
  int64_t frame_base;   // first row of the clip in the spectrum workspace
  int64_t spec_off;     // AFX_HPSS_STORE_SPEC: float offset of S, Hm, Pm (3 x 1025 x T) in the chunk's debug buffer
  int32_t T;            // 1 + len / 512
  int32_t tile_base;    // first 64-frame tile of the clip (k_hpss_mask)
};

// What a clip costs the chunk of an STFT-based group (afx_hpss_batch, afx_chroma_batch, afx_rhythm_batch), in bytes of
// device workspace: T per_frame + ceil(T / tile) per_tile + len per_sample + per_clip, T = 1 + len / 512
struct StftCost {
  int64_t per_frame, per_tile, per_sample, per_clip;
  int64_t tile;         // frames per tile
  int64_t tile_cap;     // most tiles a chunk may hold
  int64_t spec_floats;  // floats of spec_off per frame (0 except for AFX_HPSS_STORE_SPEC)
};

// One chunk of a batch: the records of its clips (in_off is the caller's offset) and what they add up to
struct StftChunk {
  std::vector<HpssClip> recs;
  std::vector<int> idx;               // recs[q] is clip idx[q] of the batch
  int64_t frames, samples, spec_floats;
  int64_t lo, hi, max_len;            // the chunk's clips lie in [lo, hi) of the caller's samples
  int tiles;
  int next;                           // the first clip of the batch the chunk does not hold
};

constexpr int kStftChunkClips = 32768;

// The chunk that starts at clip `first` (afx_host.cpp; no device): zero-length clips are skipped and cost nothing, a chunk
// holds at least one clip, and it ends before the clip that would take its bytes past the budget or its tiles past the
// cap, or at kStftChunkClips records.  afx_stft_chunks hands the same rule to a caller without a device.
void cut_stft_chunk(const int64_t* offsets, const int64_t* lengths, int n_clips, int first, int64_t budget,
                    const StftCost& cost, StftChunk& ck);

struct HpssTabs {
  const float* window;  // periodic Hann, 2048 floats
  const float* w1024;   // exp(-2 pi i k / 1024), k < 1024, float2
  const float* w2048;   // exp(-2 pi i k / 2048), k < 1024, float2
};

#ifdef __HIPCC__
// clip of a row / tile index: the last record whose base is <= g (wave-uniform binary search)
template <typename F>
__device__ __forceinline__ int hp_find(int n, int64_t g, F base) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (base(mid) <= g) lo = mid; else hi = mid - 1;
  }
  return lo;
}
#endif

// y[y_off + i] = sample i (pre-emphasised when flags has AFX_FLAG_PREEMPH); bad[c] = 1 when clip c holds a NaN / inf
hipError_t launch_hpss_prep(hipStream_t s, const void* in, int fmt, int flags, float preemph_b1, const HpssClip* clips,
                            int n, int64_t max_len, float* y, uint32_t* bad);
// the complex spectrum of every frame into rows of X (zeros for a bad clip)
hipError_t launch_hpss_stft(hipStream_t s, const float* y, const HpssClip* clips, const uint32_t* bad, int n,
                            int64_t n_frames, HpssTabs tb, float2* X);
// |X|^2 of every frame as float32 rows of kHpssPowPitch, entries 1025 .. 1039 zero (zeros for a bad clip)
hipError_t launch_hpss_stft_power(hipStream_t s, const float* y, const HpssClip* clips, const uint32_t* bad, int n,
                                  int64_t n_frames, HpssTabs tb, float* S);
// both medians of |X|, the soft masks, Yh = X mh and (Yp != nullptr) Yp = X mp; spec != nullptr: S, Hm, Pm as well
hipError_t launch_hpss_mask(hipStream_t s, const float2* X, const HpssClip* clips, int n, int n_tiles, float2* Yh,
                            float2* Yp, float* spec);
// irfft x window of every row of Yh (and Yp), in place: row r then holds 2048 float samples
hipError_t launch_hpss_irfft(hipStream_t s, float2* Yh, float2* Yp, int64_t n_frames, HpssTabs tb);
// overlap-add as a gather, window-sum-square normalisation, cut to length: h (and p) at y_off
hipError_t launch_hpss_ola(hipStream_t s, const float2* Yh, const float2* Yp, const HpssClip* clips, int n, int64_t max_len,
                           HpssTabs tb, float* h, float* p);
// per clip, in float64 and in a fixed order: sum h^2, sum y^2, mean and std of the centroid frames desc[desc_off[c] + 17 t]
hipError_t launch_hpss_stats(hipStream_t s, const float* y, const float* h, const HpssClip* clips, int n,
                             const float* desc, const int64_t* desc_off, double* stats);

}  // namespace afx
