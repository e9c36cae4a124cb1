// Beat tracking (afx_beat.hip, afx_beat_host.cpp): librosa.beat.beat_track's dynamic programme on the onset envelope and the
// tempo that launch_rhythm_reduce leaves on the device (tests/beat_ref.py is the spec).  The per-clip record, the order of the
// reductions both executors share, and the launchers.  Internal to libafx.so.
//
// The clip records are afx_hpss.h's HpssClip, as for afx_rhythm.h.
#pragma once
#include <cstdint>

#include <hip/hip_runtime_api.h>

#include "afx_hpss.h"

namespace afx {

constexpr int kBeatMaxFpb = 768;                      // frames per beat: the tempogram window's bound (afx_rhythm.h)
constexpr int kBeatTaps = 2 * kBeatMaxFpb + 1;        // most taps of the local score's window, most distances of the penalty
constexpr int kBeatRing = 2048;                       // k_beat_dp's ring of cumulative scores: a power of two above 2 x 768
constexpr int kBeatThreads = 256;                     // k_beat_score: the strided partial sums both executors form, then a tree

// One per clip of a chunk, written by k_beat_score, completed by k_beat_finish
struct BeatRec {
  double tempo;         // the tempo the clip is tracked at: the caller's, else the one launch_rhythm_reduce decided
  double denom;         // std(env, ddof 1) + DBL_MIN
  double maxls;         // the largest local score
  int32_t fpb;          // round(fps 60 / tempo), half to even; 0 for tempo 0
  int32_t lo;           // round(fpb / 2), half to even
  int32_t active;       // T >= 2, a non-zero envelope, tempo > 0: the dynamic programme runs
  int32_t n_beats;
};

// frames per beat of a tempo > 0, round(fps 60 / bpm) half to even; false when it is outside [1, 768] (afx_beat_host.cpp)
bool beat_fpb(double fps, double bpm, int32_t* fpb);

// res = launch_rhythm_reduce's records; bpm_in: NULL, or per clip the caller's tempo (0: the decided one).  Per clip: the
// record, x = env / denom in float64 and the local score (both at frame_base; written for an active clip only)
hipError_t launch_beat_score(hipStream_t s, const float* env, const HpssClip* clips, const uint32_t* bad, int n,
                             const double* res, const double* bpm_in, double fps, double* x, double* localscore, BeatRec* rec);
// cumscore and backlink of every active clip (at frame_base)
hipError_t launch_beat_dp(hipStream_t s, const HpssClip* clips, int n, const BeatRec* rec, const double* localscore,
                          double tightness, double* cumscore, int32_t* backlink);
// the last beat, the backtrack, the trim: beats[frame_base + t] = 1 for a beat (the caller zeroes beats), rec[c].n_beats;
// keys: a uint64 per frame of workspace (x's space is free by now)
hipError_t launch_beat_finish(hipStream_t s, const HpssClip* clips, int n, const double* localscore, const double* cumscore,
                              const int32_t* backlink, int trim, uint64_t* keys, uint8_t* beats, BeatRec* rec);
// envelope mode: env[frame_base + t] = in[in_off + t] for the T frames of a clip, zeros and bad[c] = 1 when one is NaN / inf
hipError_t launch_beat_stage(hipStream_t s, const float* in, const HpssClip* clips, int n, float* env, uint32_t* bad);

}  // namespace afx
