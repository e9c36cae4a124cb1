// Developer switches of libafx.so, read ONCE per process when the first caller asks (never on the per-call path:
// getenv is not safe against a host program that writes os.environ from other threads, and a batch must not pay for it).
// They exist for same-box A/B runs (tools/ab_env.sh) and for tests that exercise the multi-chunk paths with small
// batches; none of them is part of the ABI.  Internal to libafx.so.  (Round 1's 4-wave 1024 / 256 frame kernel and
// the switch that chose between it and k_frames<1024> were removed: see git log.)
#pragma once
#include <cstdint>

namespace afx {

struct DevEnv {
  int debug_skip = 0, f0_debug = 0;
  bool stamps = false, f3_debug = false, no_spec = false, no_tickets = false;
  bool no_frames3 = false, no_frames3s = false, no_frames3d = false;   // fall back to round 1's kernels (A/B)
  bool f3_generic_mel = false;        // the generic mel walk instead of the compiled-in schedule (A/B)
  bool no_dct16l = false;             // k_dct16<2|3> instead of k_dct16l (A/B)
  bool host_blocks = false;           // build the speculative block list on the host and upload it (A/B of k_build_blocks3)
  bool no_fused_tail = false;         // k_dct16* + k_stats instead of the fused per-clip DCT + statistics kernel (A/B)
  int tail_mode = 0;                  // k_tail: 1 registers, 2 / 3 / 4 LDS-DMA ring of 4 waves x 4 tiles / 8 x 2 / 4 x 2 with two workgroups per CU,
                                      // 5 / 6 one slot per wave + register-held images with four workgroups per CU, default / nt DMA (A/B)
  int tail_skip = 0;                  // libafx_dbg.so only: timing ablations of k_tail's one-slot form (1 no arithmetic, 2 no DMA, 4 no epilogue)
  int f3_xchg2 = 0;                   // AFX_F3_XCHG2: k_frames3 / k_frames3s hand the butterfly-ja half of FFT exchange 2 over through LDS (1, "lds":
                                      // the form before the lane swaps) or by lane swaps (2, "swap"); 0 unset: the per-shape default (A/B, tests)
  int f3_waves = 0;                   // 12 / 16: force the workgroup size of the wave-level frame kernels
  int f3_spare_cus = -1;              // AFX_F3_SPARE_CUS: workgroups taken off the speculative frame launch of a submitted batch, whatever its
                                      // size (>= 0; -1 unset: the per-shape default on full grids only; -2 a negative value was given)
  int chunk_clips = 32768;
  int64_t f0_chunk_frames = 1280 * 1024;
  int64_t dtw_budget = (int64_t)2 << 30;   // device workspace bytes of one afx_dtw_batch chunk
  int64_t hpss_budget = (int64_t)2 << 30;  // device workspace bytes of one afx_hpss_batch chunk
  int64_t chroma_budget = (int64_t)2 << 30; // device workspace bytes of one afx_chroma_batch chunk
  int64_t rhythm_budget = (int64_t)2 << 30; // device workspace bytes of one afx_rhythm_batch chunk
  int64_t groups_budget = (int64_t)2 << 30; // device workspace bytes of one afx_groups_batch chunk
  int64_t filt_budget = (int64_t)2 << 30;  // device workspace bytes of one afx_sosfiltfilt_batch chunk
  int64_t assess_budget = (int64_t)2 << 30; // device workspace bytes of one afx_assess_batch / afx_compare_batch chunk
  int64_t specdist_budget = (int64_t)2 << 30; // device workspace bytes of one afx_specdist_batch / afx_clip_fft_batch chunk
  int64_t smooth_budget = (int64_t)2 << 30; // device workspace bytes of one afx_medfilt_batch / afx_savgol_batch / afx_energy_zcr_batch chunk
  int64_t loud_budget = (int64_t)2 << 30;   // device workspace bytes of one afx_loudness_batch chunk
  int64_t gate_budget = (int64_t)2 << 30;   // device workspace bytes of one afx_gate_batch chunk
  int64_t stft_budget = (int64_t)2 << 30;   // device workspace bytes of one afx_stft_batch / afx_istft_batch chunk
  const char* f0_dump = nullptr;
  DevEnv();
};
const DevEnv& dev_env();             // afx_api.cpp

}  // namespace afx
