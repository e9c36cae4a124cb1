// The state behind the opaque handles of include/afx.h (afx_ctx, afx_plan) and the front end every batch entry point
// shares: argument checks, sample staging, the preprocessing chain, per-frame output ranges.  Internal to libafx.so:
// included by afx_api.cpp (which defines the plan's helpers), afx_features.cpp and afx_ctx_ops.cpp (which defines the context's).
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include <hip/hip_runtime.h>

#include "afx_assess.h"
#include "afx_beat.h"
#include "afx_cfft.h"
#include "afx_chroma.h"
#include "afx_decode.h"
#include "afx_device.h"
#include "afx_f0.h"
#include "afx_filt.h"
#include "afx_frames3.h"
#include "afx_groups.h"
#include "afx_internal.h"
#include "afx_gate.h"
#include "afx_loudness.h"
#include "afx_resample.h"
#include "afx_rhythm.h"
#include "afx_smooth.h"
#include "afx_stft.h"
#include "afx_pvoc.h"

namespace afx {

struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
};

}  // namespace afx

using namespace afx;

struct afx_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  DevBuf dtw_raw, dtw_feats, dtw_norms, dtw_pairs, dtw_codes, dtw_rows, dtw_d, dtw_path, dtw_cost, dtw_status, dtw_len, dtw_end;   // afx_dtw_batch, afx_dtw_steps_batch
  // Staging of host batches, shared by every entry point below: the packed input image (stage_in) and the packed result
  // (out_buffer).  A chunk stages its input once and obtains its output buffer once, before its first launch, and nothing
  // calls ensure on either again until the chunk's synchronise: ensure frees the old buffer when it grows.
  DevBuf wave_in, wave_out;
  // afx_resample_batch: the tables of the last rate pair (or caller-supplied filter) used
  struct {
    bool valid = false, custom = false;
    int up = 0, down = 0;
    std::vector<double> taps;        // the caller's filter the tables were built from (custom only)
    RsTables t;
  } rs;
  DevBuf rs_g, rs_tstart, rs_clips;
  DevBuf dc_clips;                     // afx_decode_batch: clip records
  // afx_sosfiltfilt_batch: tables and, filled by run_filtfilt_chain, a chunk's clip records and states, the float64
  // workspace, the blocks' carries, the tile maxima
  DevBuf ft_tab, ft_clips, ft_st, ft_w, ft_carry, ft_tmax;
  // afx_assess_batch / afx_compare_batch: a chunk's records, the pieces (the spans' sums of a pair), the span records, the
  // results and flags
  DevBuf as_clips, as_pieces, as_spans, as_rec, as_bad;
  // afx_specdist_batch / afx_clip_fft_batch: the stage twiddle table (built at first use), a chunk's job records, the
  // transforms' points, the filter spectra, the results and flags
  DevBuf cf_tw, cf_jobs, cf_work, cf_filt, cf_rec, cf_bad;
  bool cf_tw_ready = false;
  // afx_medfilt_batch / afx_savgol_batch: the Savitzky-Golay tables, a chunk's clip records and non-finite flags.
  // afx_energy_zcr_batch (with these and the filter workspace above): the frame records, the preprocessed,
  // median-filtered and smoothed signals, the sign plane, the smoothed peaks, the frame rows of both groups, the records
  DevBuf sm_tab, sm_clips, sm_bad;
  DevBuf ez_clips, ez_y, ez_m, ez_s, ez_neg, ez_peak, ez_energy, ez_rate, ez_rec;
  // afx_loudness_batch: one table per distinct rate, a chunk's clip records, the blocks' states and partial sums, the tiles'
  // peaks and flags, the segment sums, z_j, the clips' scalars, the gains
  DevBuf ld_tab, ld_clips, ld_carry, ld_part, ld_tpeak, ld_tbad, ld_seg, ld_z, ld_rec, ld_gain;
  // afx_gate_batch: the window / twiddles / taps, a chunk's grid records, its float32 signal, the non-finite flags, the
  // magnitude planes of both grids, the mask plane, the forward pass, the bit plane, thr and its amplitude, the time rows
  DevBuf gt_tab, gt_grids, gt_y, gt_bad, gt_mag, gt_nmag, gt_mask, gt_fwd, gt_bits, gt_thr, gt_amp, gt_rows;
  // afx_stft_batch / afx_istft_batch: the window and twiddles, a chunk's clip records, its float32 signal and non-finite
  // flags (forward), the time rows the overlap-add reads (inverse)
  DevBuf st_tab, st_recs, st_y, st_bad, st_rows;
  // afx_pvoc_batch / afx_time_stretch_batch: a chunk's clip records and non-finite flags, the angle and magnitude planes,
  // the tile sums; the stretch's spectrum and its vocoded rows (it takes the window, y and the time rows from the st_ set)
  DevBuf pv_recs, pv_bad, pv_ang, pv_mag, pv_sum, pv_spec, pv_out;
};

struct afx_plan {
  afx_ctx* ctx = nullptr;
  int device = 0;             // copy: the plan may be destroyed after its context by a garbage-collected binding
  afx_params p{};
  KParams kp{};
  HostTables ht;
  DevTables dt{};
  F3Tables f3{};              // k_frames3 (n_fft 1024 / hop 256): mel schedule + twiddle source
  bool use_f3 = false;
  std::vector<void*> table_allocs;
  DevBuf samples, clips, info, blocks, bsum, logmel, rms, mfcc, frames, frame_offs, stamps;     // statistics go straight to h_pin
  DevBuf blocks_spec, blockmax, items, n_items;      // speculative pipeline (k_frames3 before the trim decision)
  std::vector<BlockDesc> h_blocks;     // AFX_HOST_BLOCKS (A/B) only: the block list is built by k_build_blocks3
  // pinned staging of the clip records: the upload is a true asynchronous copy, and the event tells when the
  // staging may be rewritten (no stream synchronisation on a batch whose clip lengths are new)
  ClipDesc* h_clips_pin = nullptr;
  size_t h_clips_pin_cap = 0;
  hipEvent_t clips_ev = nullptr;
  bool clips_ev_pending = false;
  // extract_f0 (pYIN): tables for the last (fmin, fmax) used and the stage's workspace
  bool f0_ready = false;
  double f0_fmin = 0.0, f0_fmax = 0.0;
  HostF0Tables f0_ht;
  F0Tables f0_dt{};
  std::vector<void*> f0_allocs;
  DevBuf f0_in, f0_ysig, f0_energy, f0_cnt, f0_vp, f0_bin, f0_prob, f0_lprob, f0_lu, f0_ptr, f0_best, f0_states, f0_stats, f0_out, f0_offs;
  DevBuf hp_clips, hp_y, hp_h, hp_p, hp_x, hp_yh, hp_yp, hp_bad, hp_stats, hp_spec;   // afx_hpss_batch
  // afx_chroma_batch (with hp_clips, hp_y, hp_bad, hp_stats): the 100-tuning filterbank and the mel bank as MFMA images
  // (built at first use), a chunk's off-grid filterbanks, the power rows, the peak records and the results
  DevBuf ch_grid, ch_extra, ch_mel, ch_s, ch_mag, ch_bin, ch_slot, ch_hist, ch_chroma, ch_melout, ch_parts;
  ChromaMel ch_melrec{};
  // afx_rhythm_batch (with hp_clips, hp_y, hp_bad, ch_s, ch_mel): the window / bpm / logprior table (built at first use),
  // the dB rows, the clip maxima, the envelope, the per-tile lag sums, the tempogram (when asked for) and the results
  DevBuf rh_tab, rh_db, rh_max, rh_env, rh_parts, rh_tg, rh_acmean, rh_res;
  RhythmTab rh_tabrec{};
  // afx_beat_batch (with the buffers of afx_rhythm_batch): x = env / std (later the keys of the local maxima), the local and
  // cumulative scores, the backlinks, the flags, the records, the caller's tempi
  DevBuf bt_x, bt_ls, bt_cum, bt_bl, bt_beats, bt_rec, bt_bpm;
  // afx_groups_batch (with the buffers of the three entry points above and the filter workspace of the context): the clip
  // records with 64-frame tiles (k_hpss_mask), the preprocess's upload and output, the descriptor rows of y and the centroid
  // rows of h, the per-group statistics, the MFCC table (built at first use) and per-frame sums, the records
  DevBuf gp_clips64, gp_in, gp_filt, gp_desc, gp_hdesc, gp_doff, gp_sstats, gp_cstats, gp_mparts, gp_mstats, gp_dct, gp_rec, gp_ints;
  // afx_denoise_batch (with hp_clips, hp_y, hp_bad, the rows in hp_yh and the signal in hp_h): the profile rows, the per-clip
  // info, the VAD energies
  DevBuf dn_prof, dn_info, dn_e;
  std::vector<float> gp_rows;   // AFX_GROUPS_STORE_DESC: the 17-float rows of the last call, clip after clip (afx_groups_debug_rows)
  // cached per-batch descriptors
  std::vector<int64_t> c_off, c_len;
  std::vector<ClipDesc> h_clips;
  std::vector<int64_t> h_rebased;   // per-frame output offsets of the pending chunk (source of an asynchronous upload: lives until collect)
  int nblocks = 0, max_tblocks = 0, max_tmax = 0;
  int64_t total_tpad = 0, total_tblk = 0;
  // pinned staging for the small per-call results (a device-to-pageable copy is staged and synchronous)
  void* h_pin = nullptr;
  void* h_pin_dev = nullptr;       // the same block as the device addresses it
  size_t h_pin_cap = 0;
  int info_clean_n = 0;            // leading clip records (and the counters) known to be zero on the stream
  // a submitted, not yet collected chunk (afx_extract_submit / afx_extract_collect; afx_extract_batch = both, per chunk)
  struct Pending {
    bool active = false;
    bool listed = false;             // in the list of submitted batches (afx_api.cpp) under `stream`
    hipStream_t stream = nullptr;
    int n = 0;
    size_t stats_bytes = 0;
    float* out_stats = nullptr; int32_t* out_status = nullptr; int64_t* out_trim = nullptr; int32_t* out_nframes = nullptr;
  } pend;
  hipEvent_t done = nullptr;       // recorded behind the chunk's last copy: collect waits for this chunk, not for the stream
  volatile unsigned* flag = nullptr;   // host word the device stores the chunk's sequence number to (behind the same copy)
  unsigned* flag_dev = nullptr;
  unsigned seq = 0;
  // timing
  bool timing = false;
  bool timing_frames_only = false;   // afx_plan_set_timing(plan, 2): events around the frame kernel only
  hipEvent_t ev[AFX_K_COUNT][2] = {};
  bool ev_ready = false;
  double ms_sum[AFX_K_COUNT] = {};
  int32_t launches[AFX_K_COUNT] = {};
  std::vector<std::pair<double, double>> spans[AFX_K_COUNT];   // (start, end) ms on the device's common clock, newest kMaxSpans
  int n_cu = 256;
};

// everything below is internal to libafx.so: none of it is exported
#pragma GCC visibility push(hidden)

#define HIP_TRY(expr)                                                                  \
  do {                                                                                 \
    hipError_t e__ = (expr);                                                           \
    if (e__ != hipSuccess) {                                                           \
      set_error(std::string(#expr) + ": " + hipGetErrorString(e__));                   \
      return AFX_ERR_HIP;                                                              \
    }                                                                                  \
  } while (0)

inline int ensure(DevBuf& b, size_t bytes) {
  if (bytes <= b.cap && b.p) return AFX_OK;
  if (b.p) { (void)hipFree(b.p); b.p = nullptr; b.cap = 0; }
  size_t want = std::max<size_t>(bytes + bytes / 8, 256);
  hipError_t e = hipMalloc(&b.p, want);
  if (e != hipSuccess) {
    set_error(std::string("hipMalloc(") + std::to_string(want) + "): " + hipGetErrorString(e));
    b.p = nullptr;
    return e == hipErrorOutOfMemory ? AFX_ERR_NOMEM : AFX_ERR_HIP;
  }
  b.cap = want;
  return AFX_OK;
}

inline void release(DevBuf& b) {
  if (b.p) (void)hipFree(b.p);
  b.p = nullptr; b.cap = 0;
}

// ---- the front end of the batch entry points (afx_api.cpp).  who: the entry point's name, in front of every error text ----
int null_arg(const char* who);       // sets "who: null/invalid argument", returns AFX_ERR_INVALID
int check_sample_format(const char* who, int sample_fmt, int mem_kind);
// plan, clip arrays and sample format of a plan-based entry point (its own output pointers are the caller's to check);
// empty_ok: a batch of no clips may come with null arrays
int check_batch_args(const char* who, afx_plan* pl, const void* samples, int sample_fmt, int mem_kind,
                     const int64_t* offsets, const int64_t* lengths, int n_clips, bool empty_ok = false);
// offsets (and out_offsets, when given) in [0, max_off], lengths in [0, 2^31]
int check_clip_ranges(const char* who, const int64_t* offsets, const int64_t* lengths, const int64_t* out_offsets, int n_clips,
                      int64_t max_off);
// clears a stale HIP error, selects the plan's device, refuses a plan whose submitted batch has not been collected
int begin_plan_call(const char* who, afx_plan* pl);
// *d_samples: the caller's buffer if it is device memory, else a copy of [0, highest sample of the batch) in buf
int stage_samples(afx_plan* pl, DevBuf& buf, const void* samples, int sample_fmt, int mem_kind, const int64_t* offsets,
                  const int64_t* lengths, int n, const void** d_samples);
int prepare_descriptors(afx_plan* pl, const int64_t* offsets, const int64_t* lengths, int n);
// the clips prepare_descriptors saw last: cleared clip records, k_trim_blocks, k_trim_decide and, with f0_prep, the
// preprocessed signal in pl->f0_ysig
int run_preprocess(afx_plan* pl, const void* d_samples, int n, const KParams& kp, bool f0_prep);
// Per-frame output: the chunk's clips occupy [*lo, *hi) of the caller's buffer (per_frame elements per frame).  The device
// copy holds exactly that range (rebased = offs - *lo), so that a later chunk never touches -- or copies stale device
// memory over -- an earlier one's rows.  what names the offsets in the error text.
int rebase_offsets(const afx_plan* pl, const char* what, const int64_t* offs, int n, int64_t per_frame,
                   std::vector<int64_t>& rebased, int64_t* lo, int64_t* hi);
// uploads n rebased offsets to d_offs and fills bytes of out with the byte fill
int upload_frame_range(afx_plan* pl, const int64_t* rebased, int n, DevBuf& d_offs, DevBuf& out, size_t bytes, int fill);
// k_frames3s<DESC> over a device signal: kSpecFloats per frame into pl->frames (count floats) at the n host offsets
int run_spectral(afx_plan* pl, const void* d_signal, int n, const KParams& kp, const int64_t* h_offsets, size_t count,
                 const SpecBands& sb);
// downloads the clip records (synchronises the stream): AFX_CLIP_NONFINITE or AFX_CLIP_OK per clip
int statuses_from_info(afx_plan* pl, int n, int32_t* out_status);

// ---- what the context entry points share (afx_ctx_ops.cpp), all on ctx->stream; see the rule at afx_ctx::wave_in ----
// the pieces packed into image (total_bytes, zero between them; pack_pieces), uploaded to ctx->wave_in: *d_in
int stage_in(afx_ctx* ctx, std::vector<char>& image, int64_t total_bytes, const std::vector<HostPiece>& pieces, const void** d_in);
// where a chunk's kernels write: the caller's out if it is device memory, else ctx->wave_out grown to total floats
int out_buffer(afx_ctx* ctx, float* out, int out_mem_kind, int64_t total, float** d_out);
// one copy of total floats at d_out into host, not waited for; scatter_pieces hands them on after the caller's synchronise
int fetch_out(afx_ctx* ctx, const float* d_out, int64_t total, std::vector<float>& host);
// scipy's sosfiltfilt over the tiles of recs, from d_in (sample_fmt) to d_out: its workspace in the context's ft_*
// buffers, the records uploaded, then k_filt_peak, forward, scan, backward, scan, final and clipmax.  AFX_FILT_PLAIN:
// k_filt_final writes d_out; AFX_FILT_EXPERIMENT (pre-emphasis preemph): k_filt_scale does.  The clips' FiltState records
// are left in ctx->ft_st, one per record.
int run_filtfilt_chain(afx_ctx* ctx, const void* d_in, int sample_fmt, int mode, float preemph, int padlen, int n_sections,
                       const std::vector<FiltClip>& recs, int64_t tiles, const FiltTab* d_tab, float* d_out);

#pragma GCC visibility pop
