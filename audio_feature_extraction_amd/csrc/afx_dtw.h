// Batched DTW (librosa.sequence.dtw: its defaults, and custom step sizes / weights / subseq): pair records and kernel launchers.  Internal to libafx.so;
// include/afx.h (afx_dtw_batch) is the ABI.
#pragma once
#include <cstdint>

#include <hip/hip_runtime_api.h>

namespace afx {

constexpr int kDtwMaxDim = 128;
constexpr int kDtwTile = 8;                     // steps per unrolled tile; y columns staged per tile
constexpr int kDtwRing = 64 + kDtwTile;         // y columns held in LDS: the 64-lane skew plus one tile

// One pair, host-built.  The band is lo < j - i < hi (librosa's fill_off_diagonal; unconstrained: +-2^30).
struct DtwPair {
  int64_t x_frame, y_frame;   // first frame of X / Y in the packed features
  int64_t codes;              // first step-code word of the pair in the code workspace (-1: not kept)
  int64_t d;                  // first double of the pair's N x M matrix in the D workspace (-1: not kept)
  int64_t path;               // first (i, j) pair of the pair's path in the path workspace
  int64_t row;                // first double of the pair's boundary row (M doubles; the general-step kernel: two rows, 2 M)
  int32_t n, m, lo, hi;
  int32_t qn;                 // code words per strip and lane: steps 16q .. 16q+15 per word (general-step kernel: 8q .. 8q+7)
  int32_t pad_;
};
static_assert(sizeof(DtwPair) == 72, "DtwPair layout");

// words of step codes one pair needs: ceil(n / 64) strips x qn x 64 lanes
inline int32_t dtw_qn(int m) { return (m + 62) / 16 + 1; }
inline int64_t dtw_code_words(int n, int m) { return (int64_t)((n + 63) / 64) * dtw_qn(m) * 64; }

// The step list of the general-step kernel, uniform per launch (a kernel argument, so it lives in SGPRs).  Entry k
// reaches back (di, dj) = (sel / 3, sel % 3) and is recorded as step index idx (librosa's: 0-2 the default steps, 3 + k
// the caller's).  The three defaults behind a custom list carry inf weights and never win; they are not listed here.
constexpr int kDtwMaxSteps = 5;
struct DtwSteps {
  int32_t n;
  int32_t sel[kDtwMaxSteps];
  int32_t idx[kDtwMaxSteps];
  int32_t subseq;
  double w_add[kDtwMaxSteps], w_mul[kDtwMaxSteps];
};
// its step codes are 4 bits: one word per lane and tile of 8 steps
inline int32_t dtw_steps_qn(int m) { return (m + 62) / 8 + 1; }
inline int64_t dtw_steps_code_words(int n, int m) { return (int64_t)((n + 63) / 64) * dtw_steps_qn(m) * 64; }

// the row stride of the packed features the DP reads: dim rounded up to one of the compiled widths (8 .. 128)
int dtw_dimp(int dim);
// feats (stride dim) -> packed (stride dtw_dimp(dim), zero-padded); norms[t] = |feats[t, :]| in float32
hipError_t launch_dtw_pack(hipStream_t s, const float* feats, int dim, int64_t n_frames, float* packed, float* norms);
// fills n doubles with +inf (the cells of D a banded DP never visits)
hipError_t launch_dtw_fill_inf(hipStream_t s, double* p, int64_t n);
// the DP over the packed features: one wave per pair; writes cost[p], status[p] (afx_dtw_status), the step codes (backtrack) and D (store_d)
hipError_t launch_dtw(hipStream_t s, const float* feats, const float* norms, int dim, int metric, const DtwPair* pairs,
                      int n_pairs, uint32_t* codes, double* rows, double* dmat, double* cost, int32_t* status,
                      bool backtrack, bool store_d);
// the walk from (N-1, M-1) to (0, 0), one lane per pair: path[2k], path[2k+1] = i, j; len[p] = L (0 for a failed pair)
hipError_t launch_dtw_backtrack(hipStream_t s, const DtwPair* pairs, int n_pairs, const uint32_t* codes,
                                const int32_t* status, int32_t* path, int32_t* len);

// the same with a step list (k_dtw_steps): rows holds two boundary rows per pair, end[p] = the path's first column j*
// (m - 1 unless steps.subseq)
hipError_t launch_dtw_steps(hipStream_t s, const float* feats, const float* norms, int dim, int metric, const DtwPair* pairs,
                            int n_pairs, const DtwSteps& steps, uint32_t* codes, double* rows, double* dmat, double* cost,
                            int32_t* status, int32_t* end, bool backtrack, bool store_d);
// the walk from (N-1, end[p]) along the recorded steps to (0, 0), or to the first cell of row 0 under subseq
hipError_t launch_dtw_steps_backtrack(hipStream_t s, const DtwPair* pairs, int n_pairs, const DtwSteps& steps,
                                      const uint32_t* codes, const int32_t* status, const int32_t* end, int32_t* path,
                                      int32_t* len);

}  // namespace afx
