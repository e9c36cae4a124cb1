// Batched polyphase resampler (wavio.resample: Kaiser-windowed sinc through scipy.signal.resample_poly): filter design,
// the grouped tap table and the kernel launchers.  Internal to libafx.so; include/afx.h (afx_resample_design,
// afx_resample_batch) is the ABI.
//
//   out[m] = float32( sum_i x[i] * (up * h[m * down + half - i * up]) )          float64 products and sum
//
// Work layout.  Outputs are taken in "super-periods" of opp = pl * up consecutive outputs (pl = 1 when up >= 8, else
// ceil(8 / up)): output m = sp * opp + o reads x[sp * rw + t] (rw = pl * down) with the tap h[o * down + half - t * up],
// which does not depend on sp.  A wave therefore gives each lane one super-period and walks t for a GROUP of eight
// adjacent o together: every step is one x sample from LDS per lane and eight v_fma_f64 whose tap operands are the same
// for all lanes -- they sit in scalar registers, loaded from the group table G[group][step][8] (taps times `up`, zero
// where a group member's filter has ended).  The x tile of a workgroup is held in LDS as float32 (S16 / 32768 is exact
// in float32) in rows of rw samples padded to an odd stride, so lanes rw samples apart fall on different banks.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

namespace afx {

constexpr int kRsGroup = 8;                    // outputs a lane accumulates together
constexpr int kRsMaxUp = 2048;                 // bounds of the supported rate pairs (AFX_ERR_UNSUPPORTED beyond):
constexpr int kRsMaxRow = 2048;                //   up, pl * down and the number of taps
constexpr int kRsMaxTaps = 1 << 21;
constexpr int kRsLdsBytes = 160 * 1024;        // LDS of a CU: a workgroup may use all of it
constexpr int kRsCopyChunk = 4096;             // samples per workgroup of the sr_in == sr_out conversion

struct RsDesign {
  int up = 1, down = 1, n_taps = 0, half = 0;
  std::vector<double> h;                       // unity DC gain (scipy.signal.firwin), n_taps entries
};

// what the kernel needs to know about one rate pair
struct RsParams {
  int32_t up, down, opp, rw, stride;           // stride: rw | 1
  int32_t n_groups, n_steps;                   // groups of kRsGroup outputs per super-period; steps (x samples) per group
  int32_t lanes, tc, tile_sp;                  // super-periods per wave pass (<= 64), passes per tile, lanes * tc
  int32_t r_back, rows;                        // rows of history in front of the tile; rows held in LDS
  int32_t n_waves;
};

struct RsTables {
  RsParams p{};
  std::vector<double> G;                       // [n_groups][n_steps][kRsGroup]
  std::vector<int32_t> tstart;                 // [n_groups] first t of the group's walk
};

// one clip as the kernels see it
struct RsClip {
  int64_t in_off, in_len, out_off, out_len;
  int32_t first_block, pad_;
};
static_assert(sizeof(RsClip) == 40, "RsClip layout");

// afx_resample_tables.cpp (host-only)
// kaiserord(125 dB) / Kaiser window / firwin exactly as wavio._resample_filter; taps only when want_taps.
// Returns AFX_OK, AFX_ERR_INVALID (rates) or AFX_ERR_UNSUPPORTED (beyond the bounds above).
int resample_design(int sr_in, int sr_out, RsDesign& d, bool want_taps, std::string& why);
// the group table and the tile geometry for taps h[n_taps] (odd); AFX_ERR_UNSUPPORTED when no tile fits the LDS
int resample_tables(int up, int down, const double* h, int n_taps, RsTables& t, std::string& why);
int64_t resample_out_len(int64_t n, int up, int down);       // ceil(n * up / down)

}  // namespace afx

#ifdef __HIP_PLATFORM_AMD__
#include <hip/hip_runtime_api.h>
namespace afx {
// afx_resample.hip
hipError_t launch_resample(hipStream_t s, const void* in, int fmt, float* out, const RsClip* clips, int n_clips,
                           int n_blocks, const double* G, const int32_t* tstart, const RsParams& p);
// sr_in == sr_out: out = float32(in) per clip (first_block counts kRsCopyChunk-sample blocks)
hipError_t launch_resample_copy(hipStream_t s, const void* in, int fmt, float* out, const RsClip* clips, int n_clips,
                                int n_blocks);
}  // namespace afx
#endif
