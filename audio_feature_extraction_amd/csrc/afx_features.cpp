// The plan-based feature entry points of libafx.so beside the MFCC / RMS pipeline (afx_api.cpp): pYIN f0, zero-crossing
// rate, the spectral descriptors, preprocess_audio, and the three STFT-based groups -- harmonic-percussive separation,
// chroma / tuning / mel power, onset strength / tempogram / tempo -- which run in chunks on one front end of their own
// (check_stft_plan .. end_stft_chunk below), and afx_groups_batch, the pass that runs all of them on one STFT.  Each reads:
// check -> begin -> stage -> its own work -> finish, on the front end of afx_plan.h.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include <hip/hip_runtime.h>

#include "afx_denoise.h"
#include "afx_device.h"
#include "afx_devenv.h"
#include "afx_f0.h"
#include "afx_frames3.h"
#include "afx_groups.h"
#include "afx_hpss.h"
#include "afx_internal.h"
#include "afx_plan.h"

// ---- extract_f0 ---------------------------------------------------------------------------------
static int f0_setup(afx_plan* pl, double fmin, double fmax) {
  if (pl->f0_ready && pl->f0_fmin == fmin && pl->f0_fmax == fmax) return AFX_OK;
  std::string why;
  HostF0Tables ht;
  F0Dispatch disp;
  // a refusal leaves the tables of the last accepted range installed (f0_ready, f0_fmin / f0_fmax untouched)
  if (!f0_plan(pl->p.sr, pl->p.n_fft, pl->p.hop, fmin, fmax, ht, disp, why)) {
    set_error("afx_f0_batch: " + why);
    return AFX_ERR_UNSUPPORTED;
  }
  for (void* q : pl->f0_allocs) (void)hipFree(q);
  pl->f0_allocs.clear();
  pl->f0_ready = false;
  auto up = [&](const std::vector<double>& v, const double** dst) -> int {
    void* d = nullptr;
    HIP_TRY(hipMalloc(&d, v.size() * sizeof(double)));
    pl->f0_allocs.push_back(d);
    HIP_TRY(hipMemcpy(d, v.data(), v.size() * sizeof(double), hipMemcpyHostToDevice));
    *dst = (const double*)d;
    return AFX_OK;
  };
  int rc;
  if ((rc = up(ht.thr, &pl->f0_dt.thr)) != AFX_OK || (rc = up(ht.beta, &pl->f0_dt.beta)) != AFX_OK ||
      (rc = up(ht.cumbeta, &pl->f0_dt.cumbeta)) != AFX_OK || (rc = up(ht.bfact, &pl->f0_dt.bfact)) != AFX_OK ||
      (rc = up(ht.bexp, &pl->f0_dt.bexp)) != AFX_OK || (rc = up(ht.lt, &pl->f0_dt.lt)) != AFX_OK || (rc = up(ht.ltw, &pl->f0_dt.ltw)) != AFX_OK ||
      (rc = up(ht.freqs, &pl->f0_dt.freqs)) != AFX_OK)
    return rc;
  if (dev_env().f0_debug) ht.p.debug = dev_env().f0_debug;
  pl->f0_ht = ht;
  pl->f0_fmin = fmin; pl->f0_fmax = fmax;
  pl->f0_ready = true;
  return AFX_OK;
}

static int f0_chunk(afx_plan* pl, const void* d_samples, int fmt, const int64_t* offsets, const int64_t* lengths,
                    int n, int flags, double* out_stats, int32_t* out_status, double* out_f0,
                    const int64_t* f0_offsets) {
  hipStream_t s = pl->ctx->stream;
  const F0Params& fp = pl->f0_ht.p;
  int rc;
  if ((rc = prepare_descriptors(pl, offsets, lengths, n)) != AFX_OK) return rc;
  const int64_t frames = std::max<int64_t>(pl->total_tpad, 1);
  if ((rc = ensure(pl->f0_energy, (size_t)frames * fp.n_tau_pad * sizeof(float))) != AFX_OK) return rc;
  if ((rc = ensure(pl->f0_cnt, (size_t)frames * sizeof(int32_t))) != AFX_OK) return rc;
  if ((rc = ensure(pl->f0_vp, (size_t)frames * sizeof(double))) != AFX_OK) return rc;
  if ((rc = ensure(pl->f0_bin, f0_cand_bins_bytes(fp, frames))) != AFX_OK) return rc;
  const bool dump_obs = dev_env().f0_dump != nullptr;        // the linear probabilities are kept for the diagnostic dump only
  if (dump_obs && (rc = ensure(pl->f0_prob, f0_cand_prob_bytes(fp, frames))) != AFX_OK) return rc;
  if ((rc = ensure(pl->f0_ptr, f0_vrows_bytes(fp, frames))) != AFX_OK) return rc;
  if ((rc = ensure(pl->f0_best, (size_t)frames * sizeof(VitBest))) != AFX_OK) return rc;
  if ((rc = ensure(pl->f0_lprob, f0_cand_prob_bytes(fp, frames))) != AFX_OK) return rc;
  if ((rc = ensure(pl->f0_lu, (size_t)frames * sizeof(double))) != AFX_OK) return rc;
  if ((rc = ensure(pl->f0_states, (size_t)frames * sizeof(uint16_t))) != AFX_OK) return rc;
  if ((rc = ensure(pl->f0_stats, (size_t)n * 4 * sizeof(double))) != AFX_OK) return rc;
  // per-frame f0 of this chunk: [o_lo, o_hi) of the caller's buffer, device copy rebased to it (rebase_offsets)
  double* d_f0 = nullptr;
  int64_t o_lo = 0, o_hi = 0;
  std::vector<int64_t> rebased;
  if (out_f0) {
    if (!f0_offsets) { set_error("out_f0 given without f0_offsets"); return AFX_ERR_INVALID; }
    if ((rc = rebase_offsets(pl, "f0", f0_offsets, n, 1, rebased, &o_lo, &o_hi)) != AFX_OK) return rc;
    // 0xff: NaN wherever no clip writes
    if ((rc = upload_frame_range(pl, rebased.data(), n, pl->f0_offs, pl->f0_out, (size_t)(o_hi - o_lo) * sizeof(double), 0xff)) != AFX_OK) return rc;
    d_f0 = (double*)pl->f0_out.p;
  }
  KParams kp = pl->kp;
  kp.flags = flags; kp.fmt = fmt;
  const ClipDesc* d_clips = (const ClipDesc*)pl->clips.p;
  if ((rc = run_preprocess(pl, d_samples, n, kp, true)) != AFX_OK) return rc;
  ClipInfo* d_info = (ClipInfo*)pl->info.p;
  HIP_TRY(launch_f0_energy(s, (const float*)pl->f0_ysig.p, d_clips, d_info, (float*)pl->f0_energy.p, n, pl->max_tmax, fp));
  HIP_TRY(launch_f0_yin(s, (const float*)pl->f0_ysig.p, d_clips, d_info, (const float*)pl->f0_energy.p, pl->f0_dt, fp,
                        (int32_t*)pl->f0_cnt.p, (double*)pl->f0_vp.p, (int16_t*)pl->f0_bin.p,
                        dump_obs ? (double*)pl->f0_prob.p : nullptr, (double*)pl->f0_lprob.p, (double*)pl->f0_lu.p, n, pl->max_tmax));
  HIP_TRY(launch_f0_viterbi(s, d_clips, d_info, pl->f0_dt, fp, (const int32_t*)pl->f0_cnt.p,
                            (const int16_t*)pl->f0_bin.p, (const double*)pl->f0_lprob.p,
                            (const double*)pl->f0_lu.p, (double*)pl->f0_ptr.p, (VitBest*)pl->f0_best.p,
                            (uint16_t*)pl->f0_states.p, (double*)pl->f0_stats.p, d_f0, (const int64_t*)pl->f0_offs.p, n));
  HIP_TRY(hipMemcpyAsync(out_stats, pl->f0_stats.p, (size_t)n * 4 * sizeof(double), hipMemcpyDeviceToHost, s));
  if (out_f0 && o_hi > o_lo) HIP_TRY(hipMemcpyAsync(out_f0 + o_lo, d_f0, (size_t)(o_hi - o_lo) * sizeof(double), hipMemcpyDeviceToHost, s));
  if ((rc = statuses_from_info(pl, n, out_status)) != AFX_OK) return rc;
  if (const char* dump = dev_env().f0_dump) {                       // diagnostics: the sparse observation columns
    std::vector<int32_t> cnt(frames); std::vector<double> vp(frames), pr((size_t)frames * fp.cap);
    std::vector<int16_t> bn((size_t)frames * fp.cap);
    HIP_TRY(hipMemcpy(cnt.data(), pl->f0_cnt.p, frames * sizeof(int32_t), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(vp.data(), pl->f0_vp.p, frames * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(pr.data(), pl->f0_prob.p, pr.size() * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(bn.data(), pl->f0_bin.p, bn.size() * sizeof(int16_t), hipMemcpyDeviceToHost));
    if (FILE* f = fopen(dump, "wb")) {
      const int64_t hdr[2] = {frames, fp.cap};
      fwrite(hdr, sizeof(hdr), 1, f);
      fwrite(cnt.data(), sizeof(int32_t), cnt.size(), f); fwrite(vp.data(), sizeof(double), vp.size(), f);
      fwrite(bn.data(), sizeof(int16_t), bn.size(), f); fwrite(pr.data(), sizeof(double), pr.size(), f);
      fclose(f);
    }
  }
  return AFX_OK;
}

extern "C" int afx_f0_batch(afx_plan* pl, const void* samples, int sample_fmt, int mem_kind,
                            const int64_t* offsets, const int64_t* lengths, int n_clips, int flags,
                            double fmin, double fmax, double* out_f0stats, int32_t* out_status,
                            double* out_f0, const int64_t* f0_offsets) {
  if (!out_f0stats || !out_status) return null_arg("afx_f0_batch");
  int rc = check_batch_args("afx_f0_batch", pl, samples, sample_fmt, mem_kind, offsets, lengths, n_clips);
  if (rc != AFX_OK) return rc;
  if (n_clips == 0) return AFX_OK;
  if ((rc = begin_plan_call("afx_f0_batch", pl)) != AFX_OK) return rc;
  if ((rc = f0_setup(pl, fmin, fmax)) != AFX_OK) return rc;
  const void* d_samples = nullptr;
  if ((rc = stage_samples(pl, pl->f0_in, samples, sample_fmt, mem_kind, offsets, lengths, n_clips, &d_samples)) != AFX_OK) return rc;
  // the stage keeps ~14 KB of workspace per frame (Viterbi value columns 9.6 KB, candidates and their logs, energies): bound it
  // per chunk (18 GB; a chunk should still hold several clips per CU so that every CU runs two Viterbi workgroups)
  const int64_t kMaxFrames = dev_env().f0_chunk_frames;
  int c0 = 0;
  while (c0 < n_clips) {
    int n = 0;
    int64_t fr = 0;
    while (c0 + n < n_clips && n < dev_env().chunk_clips) {
      const int64_t t = 1 + lengths[c0 + n] / pl->p.hop + kFramesPerBlock;
      if (n > 0 && fr + t > kMaxFrames) break;
      fr += t; ++n;
    }
    rc = f0_chunk(pl, d_samples, sample_fmt, offsets + c0, lengths + c0, n, flags, out_f0stats + (size_t)c0 * 4,
                  out_status + c0, out_f0, f0_offsets ? f0_offsets + c0 : nullptr);
    if (rc != AFX_OK) return rc;
    c0 += n;
  }
  return AFX_OK;
}

// ---- zero-crossing rate per frame (the sibling feature the reference's experiment scripts store) ---------
extern "C" int afx_zcr_batch(afx_plan* pl, const void* samples, int sample_fmt, int mem_kind,
                             const int64_t* offsets, const int64_t* lengths, int n_clips, int flags,
                             double* out_zcr, const int64_t* zcr_offsets, int32_t* out_status) {
  if (!out_zcr || !zcr_offsets || !out_status) return null_arg("afx_zcr_batch");
  int rc = check_batch_args("afx_zcr_batch", pl, samples, sample_fmt, mem_kind, offsets, lengths, n_clips);
  if (rc != AFX_OK) return rc;
  if (n_clips == 0) return AFX_OK;
  if (n_clips > 32768) { set_error("afx_zcr_batch: at most 32768 clips per call"); return AFX_ERR_INVALID; }
  if ((rc = begin_plan_call("afx_zcr_batch", pl)) != AFX_OK) return rc;
  hipStream_t s = pl->ctx->stream;
  const int n = n_clips;
  const void* d_samples = nullptr;
  if ((rc = stage_samples(pl, pl->f0_in, samples, sample_fmt, mem_kind, offsets, lengths, n, &d_samples)) != AFX_OK) return rc;
  if ((rc = prepare_descriptors(pl, offsets, lengths, n)) != AFX_OK) return rc;
  size_t count = 0;
  for (int i = 0; i < n; ++i) count = std::max<size_t>(count, (size_t)zcr_offsets[i] + (size_t)pl->h_clips[i].tmax);
  if ((rc = upload_frame_range(pl, zcr_offsets, n, pl->f0_offs, pl->f0_out, std::max<size_t>(count, 1) * sizeof(double), 0)) != AFX_OK) return rc;
  KParams kp = pl->kp;
  kp.flags = flags; kp.fmt = sample_fmt;
  if ((rc = run_preprocess(pl, d_samples, n, kp, true)) != AFX_OK) return rc;
  HIP_TRY(launch_zcr(s, (const float*)pl->f0_ysig.p, (const ClipDesc*)pl->clips.p, (const ClipInfo*)pl->info.p, pl->p.n_fft, pl->p.hop,
                     (double*)pl->f0_out.p, (const int64_t*)pl->f0_offs.p, n, pl->max_tmax));
  HIP_TRY(hipMemcpyAsync(out_zcr, pl->f0_out.p, count * sizeof(double), hipMemcpyDeviceToHost, s));
  return statuses_from_info(pl, n, out_status);
}

// octave bands of librosa.feature.spectral_contrast(fmin=200, n_bands=6, quantile=0.02) as bin ranges (n_fft 2048)
static bool spectral_bands(int sr_hz, SpecBands& sb) {
  sb = SpecBands{};
  const int NB = 1025;
  const double sr = (double)sr_hz, df = sr / 2048.0;
  double octa[8];
  octa[0] = 0.0;
  for (int i = 1; i < 8; ++i) octa[i] = 200.0 * std::pow(2.0, (double)(i - 1));
  for (int i = 0; i < 7; ++i)
    if (octa[i] >= 0.5 * sr) { set_error("spectral_contrast: frequency band exceeds Nyquist (sr too low for 6 octave bands from 200 Hz)"); return false; }
  for (int k = 0; k < 7; ++k) {
    int b0 = -1, b1 = -1;
    for (int b = 0; b < NB; ++b) { const double f = (double)b * df; if (f >= octa[k] && f <= octa[k + 1]) { if (b0 < 0) b0 = b; b1 = b; } }
    if (b0 < 0) { set_error("spectral_contrast: empty band"); return false; }
    if (k > 0) b0 -= 1;
    if (k == 6) b1 = NB - 1;
    const int n_cur = b1 - b0 + 1;
    sb.cnt[k] = std::max(1, (int)std::nearbyint(0.02 * (double)n_cur));
    sb.lo[k] = b0; sb.hi[k] = (k < 6) ? b1 - 1 : b1;
  }
  sb.hz_per_bin = (float)df; sb.roll_percent = 0.85f;
  return true;
}

// ---- spectral descriptors (librosa.feature.spectral_centroid / _bandwidth / _rolloff / _contrast at their defaults) ------
extern "C" int afx_spectral_batch(afx_plan* pl, const void* samples, int sample_fmt, int mem_kind,
                                  const int64_t* offsets, const int64_t* lengths, int n_clips, int flags,
                                  float* out_desc, const int64_t* desc_offsets, int32_t* out_status) {
  if (!out_desc || !desc_offsets || !out_status) return null_arg("afx_spectral_batch");
  int rc = check_batch_args("afx_spectral_batch", pl, samples, sample_fmt, mem_kind, offsets, lengths, n_clips);
  if (rc != AFX_OK) return rc;
  if (pl->p.n_fft != 2048 || pl->p.hop != 512 || !pl->use_f3) {
    set_error("afx_spectral_batch: the plan must have frame_length 2048 and hop_length 512 (librosa's defaults for these features)");
    return AFX_ERR_UNSUPPORTED;
  }
  if (flags & AFX_FLAG_TRIM) { set_error("afx_spectral_batch: trim is not applied here; pass the preprocessed signal"); return AFX_ERR_UNSUPPORTED; }
  if (n_clips == 0) return AFX_OK;
  if (n_clips > 32768) { set_error("afx_spectral_batch: at most 32768 clips per call"); return AFX_ERR_INVALID; }
  SpecBands sb{};
  if (!spectral_bands(pl->p.sr, sb)) return AFX_ERR_UNSUPPORTED;
  if ((rc = begin_plan_call("afx_spectral_batch", pl)) != AFX_OK) return rc;
  hipStream_t s = pl->ctx->stream;
  const int n = n_clips;
  const void* d_samples = nullptr;
  if ((rc = stage_samples(pl, pl->samples, samples, sample_fmt, mem_kind, offsets, lengths, n, &d_samples)) != AFX_OK) return rc;
  if ((rc = prepare_descriptors(pl, offsets, lengths, n)) != AFX_OK) return rc;
  int64_t d_lo = 0, d_hi = 0;
  std::vector<int64_t> rebased;
  if ((rc = rebase_offsets(pl, "descriptor", desc_offsets, n, kSpecFloats, rebased, &d_lo, &d_hi)) != AFX_OK) return rc;
  KParams kp = pl->kp;
  kp.flags = flags; kp.fmt = sample_fmt;
  if ((rc = run_spectral(pl, d_samples, n, kp, rebased.data(), (size_t)(d_hi - d_lo), sb)) != AFX_OK) return rc;
  HIP_TRY(hipMemcpyAsync(out_desc + d_lo, pl->frames.p, (size_t)(d_hi - d_lo) * sizeof(float), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  for (int i = 0; i < n; ++i) out_status[i] = lengths[i] < 2 ? AFX_CLIP_TOO_SHORT : AFX_CLIP_OK;
  return AFX_OK;
}

extern "C" int afx_preprocess(afx_plan* pl, const float* y, int64_t n, float* out_y,
                              int64_t* start, int64_t* end, int32_t* status) {
  if (!pl || !y || !out_y || !start || !end || !status || n < 0) return null_arg("afx_preprocess");
  int rc = begin_plan_call("afx_preprocess", pl);
  if (rc != AFX_OK) return rc;
  hipStream_t s = pl->ctx->stream;
  const int64_t off = 0;
  if ((rc = prepare_descriptors(pl, &off, &n, 1)) != AFX_OK) return rc;
  if ((rc = ensure(pl->samples, (size_t)n * 4 + 16)) != AFX_OK) return rc;
  if ((rc = ensure(pl->logmel, (size_t)std::max<int64_t>(n, 1) * sizeof(float))) != AFX_OK) return rc;   // y_pre scratch
  if (n > 0) HIP_TRY(hipMemcpyAsync(pl->samples.p, y, (size_t)n * 4, hipMemcpyHostToDevice, s));
  KParams kp = pl->kp;
  kp.flags = AFX_FLAG_PREEMPH | AFX_FLAG_TRIM; kp.fmt = AFX_FMT_F32;
  if ((rc = run_preprocess(pl, pl->samples.p, 1, kp, false)) != AFX_OK) return rc;
  if (n > 0) {
    HIP_TRY(launch_preemph(s, (const float*)pl->samples.p, (float*)pl->logmel.p, n, kp.preemph_b1));
    HIP_TRY(hipMemcpyAsync(out_y, pl->logmel.p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
  }
  ClipInfo ci{};
  HIP_TRY(hipMemcpyAsync(&ci, pl->info.p, sizeof(ClipInfo), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  // T is about the MFCC stage; preprocess_audio itself only fails on < 2 samples / non-finite input
  *start = ci.start; *end = ci.end;
  *status = (n < 2) ? AFX_CLIP_TOO_SHORT : (ci.nonfinite ? AFX_CLIP_NONFINITE : AFX_CLIP_OK);
  return AFX_OK;
}

// ---- the chunked front end of the STFT-based groups: afx_hpss_batch, afx_chroma_batch, afx_rhythm_batch ----
// what the three refuse of a plan and of flags; called before begin_plan_call, so that a refusal touches no device
static int check_stft_plan(const char* who, const afx_plan* pl, int flags, int allowed, bool need_mel) {
  const std::string w(who);
  if (pl->p.n_fft != 2048 || pl->p.hop != 512 || pl->p.window != AFX_WINDOW_HANN || !pl->use_f3) {
    set_error(w + ": the plan must have frame_length 2048, hop_length 512 and the Hann window (librosa's defaults)");
    return AFX_ERR_UNSUPPORTED;
  }
  if (need_mel && pl->p.n_mels > 16 * kChromaMelGroups) { set_error(w + ": at most 128 mel bands"); return AFX_ERR_UNSUPPORTED; }
  if (flags & AFX_FLAG_TRIM) { set_error(w + ": trim is not applied here; pass the preprocessed signal"); return AFX_ERR_UNSUPPORTED; }
  if (flags & ~allowed) { set_error(w + ": unknown flag"); return AFX_ERR_INVALID; }
  return AFX_OK;
}

// bytes per sample a chunk's copy of host input takes in pl->samples (device input is read where it lies)
static int64_t upload_sample_bytes(int sample_fmt, int mem_kind) {
  return mem_kind != AFX_MEM_HOST ? 0 : sample_fmt == AFX_FMT_S16 ? 2 : 4;
}

// A cut chunk on the device: [lo, hi) of a host batch in pl->samples with in_off rebased to it, the records in hp_clips,
// hp_bad cleared and k_hpss_prep's float32 signal in hp_y
static int stage_stft_chunk(afx_plan* pl, const void* samples, int sample_fmt, int mem_kind, int flags, StftChunk& ck) {
  hipStream_t s = pl->ctx->stream;
  const int n = (int)ck.recs.size();
  int rc;
  const void* d_in = samples;
  if (mem_kind == AFX_MEM_HOST) {
    const size_t esz = (size_t)upload_sample_bytes(sample_fmt, mem_kind);
    if ((rc = ensure(pl->samples, (size_t)(ck.hi - ck.lo) * esz + 16)) != AFX_OK) return rc;
    HIP_TRY(hipMemcpyAsync(pl->samples.p, (const char*)samples + (size_t)ck.lo * esz, (size_t)(ck.hi - ck.lo) * esz, hipMemcpyHostToDevice, s));
    for (HpssClip& r : ck.recs) r.in_off -= ck.lo;
    d_in = pl->samples.p;
  }
  if ((rc = ensure(pl->hp_clips, n * sizeof(HpssClip))) != AFX_OK) return rc;
  if ((rc = ensure(pl->hp_bad, n * sizeof(uint32_t))) != AFX_OK) return rc;
  if ((rc = ensure(pl->hp_y, (size_t)ck.samples * sizeof(float) + 64)) != AFX_OK) return rc;
  HIP_TRY(hipMemcpyAsync(pl->hp_clips.p, ck.recs.data(), n * sizeof(HpssClip), hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemsetAsync(pl->hp_bad.p, 0, n * sizeof(uint32_t), s));
  HIP_TRY(launch_hpss_prep(s, d_in, sample_fmt, flags & AFX_FLAG_PREEMPH, pl->kp.preemph_b1, (const HpssClip*)pl->hp_clips.p, n,
                           ck.max_len, (float*)pl->hp_y.p, (uint32_t*)pl->hp_bad.p));
  return AFX_OK;
}

// Rows of a chunk to the caller's dst + off[clip]: `per` floats for every frame (by_frames) or every sample of a clip, as
// they lie in src.  One copy when the caller's layout is the chunk's (packed clips in order), else one per clip.
static int copy_rows_out(hipStream_t s, const StftChunk& ck, float* dst, const int64_t* off, const float* src, int64_t per,
                         bool by_frames) {
  const int n = (int)ck.recs.size();
  auto base = [&](int q) { return per * (by_frames ? ck.recs[q].frame_base : ck.recs[q].y_off); };
  bool packed = true;
  for (int q = 0; q < n && packed; ++q) packed = off[ck.idx[q]] - off[ck.idx[0]] == base(q);
  if (packed) {
    HIP_TRY(hipMemcpyAsync(dst + off[ck.idx[0]], src, (size_t)(per * (by_frames ? ck.frames : ck.samples)) * sizeof(float), hipMemcpyDeviceToHost, s));
    return AFX_OK;
  }
  for (int q = 0; q < n; ++q) {
    const int64_t count = per * (by_frames ? (int64_t)ck.recs[q].T : ck.recs[q].len);
    HIP_TRY(hipMemcpyAsync(dst + off[ck.idx[q]], src + base(q), (size_t)count * sizeof(float), hipMemcpyDeviceToHost, s));
  }
  return AFX_OK;
}

// the end of a chunk: hp_bad of its n clips on the host, the stream drained (every copy of the chunk has landed)
static int end_stft_chunk(afx_plan* pl, int n, std::vector<uint32_t>& h_bad) {
  hipStream_t s = pl->ctx->stream;
  h_bad.resize(n);
  HIP_TRY(hipMemcpyAsync(h_bad.data(), pl->hp_bad.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return AFX_OK;
}

// ---- harmonic-percussive separation (librosa.effects.hpss / harmonic) and the harmonic features -----------------------
extern "C" int afx_hpss_batch(afx_plan* pl, const void* samples, int sample_fmt, int mem_kind,
                              const int64_t* offsets, const int64_t* lengths, int n_clips, int flags,
                              float* out_harm, float* out_perc, double* out_stats,
                              float* out_spec, const int64_t* spec_off, int32_t* out_status) {
  const bool sd = (flags & AFX_HPSS_STORE_SPEC) != 0;
  if (n_clips > 0 && !out_status) return null_arg("afx_hpss_batch");
  int rc = check_batch_args("afx_hpss_batch", pl, samples, sample_fmt, mem_kind, offsets, lengths, n_clips, true);
  if (rc != AFX_OK) return rc;
  if ((rc = check_stft_plan("afx_hpss_batch", pl, flags, AFX_FLAG_PREEMPH | AFX_HPSS_STORE_SPEC, false)) != AFX_OK) return rc;
  if (sd && n_clips > 0 && (!out_spec || !spec_off)) { set_error("afx_hpss_batch: AFX_HPSS_STORE_SPEC needs out_spec and spec_off"); return AFX_ERR_INVALID; }
  if ((rc = check_clip_ranges("afx_hpss_batch", offsets, lengths, sd ? spec_off : nullptr, n_clips, INT64_MAX / 4)) != AFX_OK) return rc;
  const double nan = std::nan("");
  for (int i = 0; i < n_clips; ++i) {
    out_status[i] = lengths[i] == 0 ? AFX_CLIP_TOO_SHORT : AFX_CLIP_OK;
    if (out_stats) for (int k = 0; k < 4; ++k) out_stats[4 * i + k] = nan;
  }
  if (n_clips == 0) return AFX_OK;
  // the centroid runs k_frames3s<DESC>, which also forms the contrast bands; below 12.8 kHz they do not exist and are
  // replaced by a harmless single bin (only the centroid is read here)
  SpecBands sb{};
  if (out_stats && !spectral_bands(pl->p.sr, sb)) {
    sb = SpecBands{};
    for (int k = 0; k < 8; ++k) { sb.lo[k] = 0; sb.hi[k] = 0; sb.cnt[k] = 1; }
    sb.hz_per_bin = (float)((double)pl->p.sr / 2048.0); sb.roll_percent = 0.85f;
  }
  if ((rc = begin_plan_call("afx_hpss_batch", pl)) != AFX_OK) return rc;
  hipStream_t s = pl->ctx->stream;
  const bool want_p = out_perc != nullptr;
  const int nsig = want_p ? 3 : 2;                  // y, h (, p) and X, Yh (, Yp)
  StftCost cost{};
  cost.per_frame = kHpssPitch * 8 * nsig + kSpecFloats * 4 + (sd ? 3 * kHpssBins * 4 : 0);
  cost.per_sample = 4 * nsig + upload_sample_bytes(sample_fmt, mem_kind);
  cost.per_clip = 128;
  cost.tile = kHpssTile; cost.tile_cap = 65535; cost.spec_floats = sd ? 3 * kHpssBins : 0;
  const HpssTabs tb{pl->f3.window, pl->f3.w1024, pl->f3.w2048};
  StftChunk ck;
  std::vector<int64_t> h_off, h_len, d_off;
  std::vector<uint32_t> h_bad;
  std::vector<double> h_stats;
  for (int c0 = 0; c0 < n_clips; c0 = ck.next) {
    cut_stft_chunk(offsets, lengths, n_clips, c0, dev_env().hpss_budget, cost, ck);
    const int n = (int)ck.recs.size(), tiles = ck.tiles;
    const int64_t frames = ck.frames, max_len = ck.max_len;
    const std::vector<HpssClip>& recs = ck.recs;
    if (n == 0) continue;
    const size_t spec_bytes = (size_t)frames * kHpssPitch * sizeof(float2), sig_bytes = (size_t)ck.samples * sizeof(float) + 64;
    if ((rc = ensure(pl->hp_h, sig_bytes)) != AFX_OK) return rc;
    if ((rc = ensure(pl->hp_x, spec_bytes)) != AFX_OK) return rc;
    if ((rc = ensure(pl->hp_yh, spec_bytes)) != AFX_OK) return rc;
    if (want_p) {
      if ((rc = ensure(pl->hp_p, sig_bytes)) != AFX_OK) return rc;
      if ((rc = ensure(pl->hp_yp, spec_bytes)) != AFX_OK) return rc;
    }
    if (sd && (rc = ensure(pl->hp_spec, (size_t)ck.spec_floats * sizeof(float))) != AFX_OK) return rc;
    if (out_stats && (rc = ensure(pl->hp_stats, (size_t)n * 4 * sizeof(double))) != AFX_OK) return rc;
    if ((rc = stage_stft_chunk(pl, samples, sample_fmt, mem_kind, flags, ck)) != AFX_OK) return rc;
    const HpssClip* d_clips = (const HpssClip*)pl->hp_clips.p;
    const uint32_t* d_bad = (const uint32_t*)pl->hp_bad.p;
    const float* d_y = (const float*)pl->hp_y.p;
    float* d_h = (float*)pl->hp_h.p;
    float* d_p = want_p ? (float*)pl->hp_p.p : nullptr;
    float2* d_yp = want_p ? (float2*)pl->hp_yp.p : nullptr;
    HIP_TRY(launch_hpss_stft(s, d_y, d_clips, d_bad, n, frames, tb, (float2*)pl->hp_x.p));
    HIP_TRY(launch_hpss_mask(s, (const float2*)pl->hp_x.p, d_clips, n, tiles, (float2*)pl->hp_yh.p, d_yp,
                             sd ? (float*)pl->hp_spec.p : nullptr));
    HIP_TRY(launch_hpss_irfft(s, (float2*)pl->hp_yh.p, d_yp, frames, tb));
    HIP_TRY(launch_hpss_ola(s, (const float2*)pl->hp_yh.p, d_yp, d_clips, n, max_len, tb, d_h, d_p));
    if (out_stats) {
      // spectral_centroid(y=h): k_frames3s<DESC> over the device-resident h, then the per-clip reduction
      h_off.resize(n); h_len.resize(n); d_off.resize(n);
      for (int q = 0; q < n; ++q) { h_off[q] = recs[q].y_off; h_len[q] = recs[q].len; d_off[q] = kSpecFloats * recs[q].frame_base; }
      if ((rc = prepare_descriptors(pl, h_off.data(), h_len.data(), n)) != AFX_OK) return rc;
      KParams kp = pl->kp;
      kp.flags = 0; kp.fmt = AFX_FMT_F32;
      if ((rc = run_spectral(pl, d_h, n, kp, d_off.data(), (size_t)frames * kSpecFloats, sb)) != AFX_OK) return rc;
      HIP_TRY(launch_hpss_stats(s, d_y, d_h, d_clips, n, (const float*)pl->frames.p, (const int64_t*)pl->frame_offs.p,
                                (double*)pl->hp_stats.p));
      h_stats.resize((size_t)n * 4);
      HIP_TRY(hipMemcpyAsync(h_stats.data(), pl->hp_stats.p, (size_t)n * 4 * sizeof(double), hipMemcpyDeviceToHost, s));
    }
    if (out_harm && (rc = copy_rows_out(s, ck, out_harm, offsets, d_h, 1, false)) != AFX_OK) return rc;
    if (out_perc && (rc = copy_rows_out(s, ck, out_perc, offsets, d_p, 1, false)) != AFX_OK) return rc;
    if (sd && (rc = copy_rows_out(s, ck, out_spec, spec_off, (const float*)pl->hp_spec.p, 3 * kHpssBins, true)) != AFX_OK) return rc;
    if ((rc = end_stft_chunk(pl, n, h_bad)) != AFX_OK) return rc;
    for (int q = 0; q < n; ++q) {
      const int i = ck.idx[q];
      out_status[i] = h_bad[q] ? AFX_CLIP_NONFINITE : AFX_CLIP_OK;
      if (out_stats && !h_bad[q]) {
        for (int k = 0; k < 4; ++k) out_stats[4 * i + k] = h_stats[4 * (size_t)q + k];
        if (recs[q].len < 2) out_stats[4 * i + 2] = out_stats[4 * i + 3] = nan;   // k_frames3s skips clips of one sample
      }
    }
  }
  return AFX_OK;
}

// ---- STFT-domain noise reduction and the aligner's preprocess (noise_reduction.py:15-92, process_audio.py:9-54) ----------
// Per chunk: the gain, the profile rows, the fused frame kernel into hp_yh, HPSS's overlap-add into hp_h, the VAD's energies
// and threshold, the finishing gather in place.  hp_y, hp_yh and hp_h are this call's for its duration.
extern "C" int afx_denoise_batch(afx_plan* pl, const void* samples, int sample_fmt, int mem_kind,
                                 const int64_t* offsets, const int64_t* lengths, int n_clips,
                                 int flags, int mode, double beta, int noise_frames,
                                 float* out, double* out_info, int32_t* out_status) {
  const char* who = "afx_denoise_batch";
  if (n_clips > 0 && (!out || !out_status)) return null_arg(who);
  int rc = check_batch_args(who, pl, samples, sample_fmt, mem_kind, offsets, lengths, n_clips, true);
  if (rc != AFX_OK) return rc;
  if ((rc = check_stft_plan(who, pl, flags, AFX_FLAG_PREEMPH | AFX_DENOISE_RMS_GAIN | AFX_DENOISE_VAD, false)) != AFX_OK) return rc;
  if (mode != AFX_DENOISE_SPECSUB && mode != AFX_DENOISE_WIENER) { set_error(std::string(who) + ": unknown mode"); return AFX_ERR_INVALID; }
  if (!std::isfinite(beta) || beta < 0.0) { set_error(std::string(who) + ": beta must be finite and >= 0"); return AFX_ERR_INVALID; }
  if (noise_frames < 1 || noise_frames > kDnMaxNoiseFrames) { set_error(std::string(who) + ": noise_frames must be in [1, 64]"); return AFX_ERR_INVALID; }
  const bool rms = (flags & AFX_DENOISE_RMS_GAIN) != 0, want_vad = (flags & AFX_DENOISE_VAD) != 0;
  DnVad vad{0, 0};
  if (want_vad) {
    vad.fl = (int)(0.025 * (double)pl->p.sr); vad.hop = (int)(0.010 * (double)pl->p.sr);
    if (vad.hop < 1) { set_error(std::string(who) + ": the VAD needs a sample rate of at least 100 Hz"); return AFX_ERR_INVALID; }
  }
  if ((rc = check_clip_ranges(who, offsets, lengths, nullptr, n_clips, INT64_MAX / 4)) != AFX_OK) return rc;
  const double nan = std::nan("");
  for (int i = 0; i < n_clips; ++i) {
    out_status[i] = lengths[i] == 0 ? AFX_CLIP_TOO_SHORT : AFX_CLIP_OK;
    if (out_info) for (int k = 0; k < kDnInfo; ++k) out_info[kDnInfo * i + k] = nan;
  }
  if (n_clips == 0) return AFX_OK;
  if ((rc = begin_plan_call(who, pl)) != AFX_OK) return rc;
  hipStream_t s = pl->ctx->stream;
  StftCost cost;
  denoise_cost(flags, sample_fmt, mem_kind, cost);
  const HpssTabs tb{pl->f3.window, pl->f3.w1024, pl->f3.w2048};
  StftChunk ck;
  std::vector<uint32_t> h_bad;
  std::vector<double> h_info;
  for (int c0 = 0; c0 < n_clips; c0 = ck.next) {
    cut_stft_chunk(offsets, lengths, n_clips, c0, dev_env().hpss_budget, cost, ck);
    const int n = (int)ck.recs.size();
    if (n == 0) continue;
    if ((rc = ensure(pl->hp_h, (size_t)ck.samples * sizeof(float) + 64)) != AFX_OK) return rc;
    if ((rc = ensure(pl->hp_yh, (size_t)ck.frames * kHpssPitch * sizeof(float2))) != AFX_OK) return rc;
    if ((rc = ensure(pl->dn_prof, (size_t)n * kDnProfPitch * sizeof(float))) != AFX_OK) return rc;
    if ((rc = ensure(pl->dn_info, (size_t)n * kDnInfo * sizeof(double))) != AFX_OK) return rc;
    if (want_vad && (rc = ensure(pl->dn_e, (size_t)(ck.samples + n) * sizeof(float) + 64)) != AFX_OK) return rc;
    if ((rc = stage_stft_chunk(pl, samples, sample_fmt, mem_kind, flags, ck)) != AFX_OK) return rc;
    const HpssClip* d_clips = (const HpssClip*)pl->hp_clips.p;
    const uint32_t* d_bad = (const uint32_t*)pl->hp_bad.p;
    const float* d_y = (const float*)pl->hp_y.p;
    float* d_d = (float*)pl->hp_h.p;
    float* d_e = want_vad ? (float*)pl->dn_e.p : nullptr;
    double* d_info = (double*)pl->dn_info.p;
    HIP_TRY(launch_dn_gain(s, d_y, d_clips, n, rms, d_info));
    HIP_TRY(launch_dn_profile(s, d_y, d_clips, d_bad, n, noise_frames, mode == AFX_DENOISE_WIENER, d_info, tb, (float*)pl->dn_prof.p));
    HIP_TRY(launch_dn_frames(s, d_y, d_clips, d_bad, n, ck.frames, mode == AFX_DENOISE_WIENER, (float)beta, d_info,
                             (const float*)pl->dn_prof.p, tb, (float2*)pl->hp_yh.p));
    HIP_TRY(launch_hpss_ola(s, (const float2*)pl->hp_yh.p, nullptr, d_clips, n, ck.max_len, tb, d_d, nullptr));
    if (want_vad) HIP_TRY(launch_dn_vad(s, d_d, d_clips, d_bad, n, ck.max_len, vad, d_e, d_info));
    HIP_TRY(launch_dn_finish(s, d_d, d_clips, d_bad, n, ck.max_len, vad, d_e, d_info));
    h_info.resize((size_t)n * kDnInfo);
    HIP_TRY(hipMemcpyAsync(h_info.data(), d_info, (size_t)n * kDnInfo * sizeof(double), hipMemcpyDeviceToHost, s));
    if ((rc = copy_rows_out(s, ck, out, offsets, d_d, 1, false)) != AFX_OK) return rc;
    if ((rc = end_stft_chunk(pl, n, h_bad)) != AFX_OK) return rc;
    for (int q = 0; q < n; ++q) {
      const int i = ck.idx[q];
      out_status[i] = h_bad[q] ? AFX_CLIP_NONFINITE : (want_vad && ck.recs[q].len < 512) ? AFX_CLIP_TOO_SHORT : AFX_CLIP_OK;
      if (out_info && out_status[i] == AFX_CLIP_OK)
        for (int k = 0; k < kDnInfo; ++k) out_info[kDnInfo * i + k] = h_info[kDnInfo * (size_t)q + k];
    }
  }
  return AFX_OK;
}

// ---- chroma_stft / estimate_tuning / melspectrogram (04_feature_extraction_experiment/feature_extractor.py:558-590) ------
// a 12 x 1025 filterbank (afx_chroma_filters) as the A images k_chroma_apply reads (afx_chroma.h)
static void chroma_images(const float* w, int rows, const float* dense, int row0, int s0, int s1, float* img) {
  for (int s = s0; s < s1; ++s)
    for (int c = 0; c < 4; ++c)
      for (int l = 0; l < 64; ++l) {
        const int r = row0 + (l & 15), b = 16 * s + 4 * (l >> 4) + c;
        img[((size_t)(s - s0) * 4 + c) * 64 + l] = (r < rows && b < kHpssBins) ? (w ? w : dense)[(size_t)r * kHpssBins + b] : 0.f;
      }
}

// the mel bank cut to the steps each group of 16 filters touches, at first use (afx_chroma_batch and afx_rhythm_batch)
static int mel_images_setup(afx_plan* pl, const char* who) {
  if (pl->ch_melrec.img) return AFX_OK;
  const int M = pl->p.n_mels;
  if (pl->ht.mel_dense.size() != (size_t)M * kHpssBins) { set_error(std::string(who) + ": the plan has no mel table"); return AFX_ERR_INVALID; }
  int rc;
  ChromaMel mr{};
  mr.n_mels = M; mr.n_groups = (M + 15) / 16;
  std::vector<float> mimg;
  for (int g = 0; g < mr.n_groups; ++g) {
    int lo = kHpssBins, hi = -1;
    for (int r = 16 * g; r < std::min(M, 16 * g + 16); ++r)
      for (int b = 0; b < kHpssBins; ++b)
        if (pl->ht.mel_dense[(size_t)r * kHpssBins + b] != 0.f) { lo = std::min(lo, b); hi = std::max(hi, b); }
    mr.s0[g] = hi < 0 ? 0 : lo / 16; mr.s1[g] = hi < 0 ? 0 : hi / 16 + 1; mr.off[g] = (int32_t)(mimg.size() / 256);
    mimg.resize(mimg.size() + (size_t)(mr.s1[g] - mr.s0[g]) * 256);
    chroma_images(nullptr, M, pl->ht.mel_dense.data(), 16 * g, mr.s0[g], mr.s1[g], mimg.data() + (size_t)mr.off[g] * 256);
  }
  if ((rc = ensure(pl->ch_mel, std::max<size_t>(mimg.size(), 1) * sizeof(float))) != AFX_OK) return rc;
  if (!mimg.empty()) HIP_TRY(hipMemcpy(pl->ch_mel.p, mimg.data(), mimg.size() * sizeof(float), hipMemcpyHostToDevice));
  mr.img = (const float*)pl->ch_mel.p;
  pl->ch_melrec = mr;                                  // set last: its image pointer marks the bank as ready
  return AFX_OK;
}

// the plan's tables, at first use: every tuning of estimate_tuning's grid, and the mel bank
static int chroma_setup(afx_plan* pl) {
  if (pl->ch_grid.p) return AFX_OK;
  int rc;
  if ((rc = mel_images_setup(pl, "afx_chroma_batch")) != AFX_OK) return rc;
  std::vector<float> w(12 * kHpssBins), img((size_t)kChromaGrid * kChromaImg);
  for (int k = 0; k < kChromaGrid; ++k) {
    if ((rc = afx_chroma_filters(pl->p.sr, (double)k * 0.01 + -0.5, w.data())) != AFX_OK) return rc;
    chroma_images(w.data(), 12, nullptr, 0, 0, kChromaSteps, img.data() + (size_t)k * kChromaImg);
  }
  DevBuf gbuf;
  if ((rc = ensure(gbuf, img.size() * sizeof(float))) != AFX_OK) return rc;
  hipError_t e = hipMemcpy(gbuf.p, img.data(), img.size() * sizeof(float), hipMemcpyHostToDevice);
  if (e != hipSuccess) { release(gbuf); set_error(std::string("afx_chroma_batch: table upload: ") + hipGetErrorString(e)); return AFX_ERR_HIP; }
  pl->ch_grid = gbuf;                                  // set last: its presence marks the tables as ready
  return AFX_OK;
}

// piptrack's band, with the spec's own comparisons: 150 <= k sr / 2048 < min(4000, sr / 2), inside bins 1 .. 1023
static ChromaBand piptrack_band(int sr) {
  ChromaBand band{1, 0, (float)((double)sr / 2048.0)};
  const double df = (double)sr / 2048.0, fmax = std::min(4000.0, 0.5 * sr);
  int k0 = -1, k1 = -1;
  for (int k = 1; k < 1024; ++k)
    if ((double)k * df >= 150.0 && (double)k * df < fmax) { if (k0 < 0) k0 = k; k1 = k; }
  if (k0 > 0) { band.kmin = k0; band.nr = k1 - k0 + 1; }
  return band;
}

extern "C" int afx_chroma_batch(afx_plan* pl, const void* samples, int sample_fmt, int mem_kind,
                                const int64_t* offsets, const int64_t* lengths, int n_clips, int flags,
                                const double* tuning_in, float* out_chroma, const int64_t* chroma_off,
                                float* out_mel, const int64_t* mel_off, double* out_tuning, double* out_stats,
                                int32_t* out_hist, int32_t* out_status) {
  const char* who = "afx_chroma_batch";
  const bool sh = (flags & AFX_CHROMA_STORE_HIST) != 0;
  if (n_clips > 0 && !out_status) return null_arg(who);
  int rc = check_batch_args(who, pl, samples, sample_fmt, mem_kind, offsets, lengths, n_clips, true);
  if (rc != AFX_OK) return rc;
  if ((rc = check_stft_plan(who, pl, flags, AFX_FLAG_PREEMPH | AFX_CHROMA_STORE_HIST, true)) != AFX_OK) return rc;
  if (n_clips > 0 && ((out_chroma && !chroma_off) || (out_mel && !mel_off) || (sh && !out_hist))) {
    set_error("afx_chroma_batch: out_chroma needs chroma_off, out_mel needs mel_off, AFX_CHROMA_STORE_HIST needs out_hist");
    return AFX_ERR_INVALID;
  }
  if ((rc = check_clip_ranges(who, offsets, lengths, out_chroma ? chroma_off : nullptr, n_clips, INT64_MAX / 4)) != AFX_OK) return rc;
  if ((rc = check_clip_ranges(who, offsets, lengths, out_mel ? mel_off : nullptr, n_clips, INT64_MAX / 4)) != AFX_OK) return rc;
  const int M = pl->p.n_mels;
  const double nan = std::nan("");
  for (int i = 0; i < n_clips; ++i) {
    if (tuning_in && !std::isfinite(tuning_in[i])) { set_error("afx_chroma_batch: tuning_in must be finite"); return AFX_ERR_INVALID; }
    out_status[i] = lengths[i] == 0 ? AFX_CLIP_TOO_SHORT : AFX_CLIP_OK;
    if (out_stats) for (int k = 0; k < 4; ++k) out_stats[4 * i + k] = nan;
    if (out_tuning) out_tuning[i] = tuning_in ? tuning_in[i] : 0.0;
    if (sh) std::fill(out_hist + (size_t)kChromaHist * i, out_hist + (size_t)kChromaHist * (i + 1), 0);
    if (lengths[i] == 0) {                              // one all-zero frame
      if (out_chroma) std::fill(out_chroma + chroma_off[i], out_chroma + chroma_off[i] + 12, 0.f);
      if (out_mel) std::fill(out_mel + mel_off[i], out_mel + mel_off[i] + M, 0.f);
    }
  }
  if (n_clips == 0) return AFX_OK;
  if ((rc = begin_plan_call(who, pl)) != AFX_OK) return rc;
  if ((rc = chroma_setup(pl)) != AFX_OK) return rc;
  hipStream_t s = pl->ctx->stream;
  const ChromaBand band = piptrack_band(pl->p.sr);
  const bool est = tuning_in == nullptr, want_mel = out_mel || out_stats;
  const HpssTabs tb{pl->f3.window, pl->f3.w1024, pl->f3.w2048};
  StftCost cost{};
  cost.per_frame = kHpssPowPitch * 4 + (est ? band.nr * 5 : 0) + 12 * 4 + (want_mel ? M * 4 : 0) + 32;
  cost.per_sample = 4 + upload_sample_bytes(sample_fmt, mem_kind);
  cost.per_clip = kChromaHist * 4 + 128;
  cost.tile = 16; cost.tile_cap = INT32_MAX / 2;
  StftChunk ck;
  std::vector<uint32_t> h_bad;
  std::vector<int32_t> h_slot, h_hist;
  std::vector<double> h_stats, extra_t;
  std::vector<float> w(12 * kHpssBins), eimg;
  for (int c0 = 0; c0 < n_clips; c0 = ck.next) {
    cut_stft_chunk(offsets, lengths, n_clips, c0, dev_env().chroma_budget, cost, ck);
    const int n = (int)ck.recs.size(), tiles = ck.tiles;
    const int64_t frames = ck.frames;
    const std::vector<int>& idx = ck.idx;
    if (n == 0) continue;
    if ((rc = ensure(pl->ch_s, (size_t)frames * kHpssPowPitch * sizeof(float))) != AFX_OK) return rc;
    if ((rc = ensure(pl->ch_slot, n * sizeof(int32_t))) != AFX_OK) return rc;
    if ((rc = ensure(pl->ch_hist, (size_t)n * kChromaHist * sizeof(int32_t))) != AFX_OK) return rc;
    if ((rc = ensure(pl->ch_chroma, (size_t)frames * 12 * sizeof(float))) != AFX_OK) return rc;
    if (est && band.nr > 0) {
      if ((rc = ensure(pl->ch_mag, (size_t)frames * band.nr * sizeof(float))) != AFX_OK) return rc;
      if ((rc = ensure(pl->ch_bin, (size_t)frames * band.nr)) != AFX_OK) return rc;
    }
    if (out_mel && (rc = ensure(pl->ch_melout, (size_t)frames * M * sizeof(float))) != AFX_OK) return rc;
    if (out_stats) {
      if ((rc = ensure(pl->ch_parts, (size_t)frames * 4 * sizeof(double))) != AFX_OK) return rc;
      if ((rc = ensure(pl->hp_stats, (size_t)n * 4 * sizeof(double))) != AFX_OK) return rc;
    }
    if ((rc = stage_stft_chunk(pl, samples, sample_fmt, mem_kind, flags, ck)) != AFX_OK) return rc;
    const HpssClip* d_clips = (const HpssClip*)pl->hp_clips.p;
    const uint32_t* d_bad = (const uint32_t*)pl->hp_bad.p;
    const float* d_y = (const float*)pl->hp_y.p;
    float* d_S = (float*)pl->ch_s.p;
    int32_t* d_slot = (int32_t*)pl->ch_slot.p;
    float* d_mel = out_mel ? (float*)pl->ch_melout.p : nullptr;
    double* d_parts = out_stats ? (double*)pl->ch_parts.p : nullptr;
    HIP_TRY(launch_hpss_stft_power(s, d_y, d_clips, d_bad, n, frames, tb, d_S));
    if (est) {
      if (band.nr > 0) HIP_TRY(launch_chroma_peaks(s, d_S, frames, band, (float*)pl->ch_mag.p, (uint8_t*)pl->ch_bin.p));
      HIP_TRY(launch_chroma_tuning(s, d_clips, n, band, (const float*)pl->ch_mag.p, (const uint8_t*)pl->ch_bin.p, d_slot,
                                   (int32_t*)pl->ch_hist.p));
    } else {
      // a tuning on estimate_tuning's grid reads the plan's table; every other distinct value gets images of its own
      h_slot.resize(n); extra_t.clear();
      for (int q = 0; q < n; ++q) {
        const double t = tuning_in[idx[q]];
        const long k = std::lround((t + 0.5) * 100.0);
        if (k >= 0 && k < kChromaGrid && (double)k * 0.01 + -0.5 == t) { h_slot[q] = (int32_t)k; continue; }
        size_t j = std::find(extra_t.begin(), extra_t.end(), t) - extra_t.begin();
        if (j == extra_t.size()) extra_t.push_back(t);
        h_slot[q] = kChromaGrid + (int32_t)j;
      }
      if (!extra_t.empty()) {
        eimg.resize(extra_t.size() * kChromaImg);
        for (size_t j = 0; j < extra_t.size(); ++j) {
          if ((rc = afx_chroma_filters(pl->p.sr, extra_t[j], w.data())) != AFX_OK) return rc;
          chroma_images(w.data(), 12, nullptr, 0, 0, kChromaSteps, eimg.data() + j * kChromaImg);
        }
        if ((rc = ensure(pl->ch_extra, eimg.size() * sizeof(float))) != AFX_OK) return rc;
        HIP_TRY(hipMemcpyAsync(pl->ch_extra.p, eimg.data(), eimg.size() * sizeof(float), hipMemcpyHostToDevice, s));
      }
      HIP_TRY(hipMemcpyAsync(d_slot, h_slot.data(), n * sizeof(int32_t), hipMemcpyHostToDevice, s));
    }
    HIP_TRY(launch_chroma_apply(s, d_S, d_clips, n, tiles, d_slot, (const float*)pl->ch_grid.p, (const float*)pl->ch_extra.p,
                                pl->ch_melrec, want_mel, (float*)pl->ch_chroma.p, d_mel, d_parts));
    if (out_stats) {
      HIP_TRY(launch_chroma_stats(s, d_clips, n, M, d_parts, (double*)pl->hp_stats.p));
      h_stats.resize((size_t)n * 4);
      HIP_TRY(hipMemcpyAsync(h_stats.data(), pl->hp_stats.p, (size_t)n * 4 * sizeof(double), hipMemcpyDeviceToHost, s));
    }
    if (out_chroma && (rc = copy_rows_out(s, ck, out_chroma, chroma_off, (const float*)pl->ch_chroma.p, 12, true)) != AFX_OK) return rc;
    if (out_mel && (rc = copy_rows_out(s, ck, out_mel, mel_off, d_mel, M, true)) != AFX_OK) return rc;
    if (est) {
      h_slot.resize(n);
      HIP_TRY(hipMemcpyAsync(h_slot.data(), d_slot, n * sizeof(int32_t), hipMemcpyDeviceToHost, s));
      if (sh) {
        h_hist.resize((size_t)n * kChromaHist);
        HIP_TRY(hipMemcpyAsync(h_hist.data(), pl->ch_hist.p, h_hist.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
      }
    }
    if ((rc = end_stft_chunk(pl, n, h_bad)) != AFX_OK) return rc;
    for (int q = 0; q < n; ++q) {
      const int i = idx[q];
      out_status[i] = h_bad[q] ? AFX_CLIP_NONFINITE : AFX_CLIP_OK;
      if (est && out_tuning) out_tuning[i] = (double)h_slot[q] * 0.01 + -0.5;
      if (est && sh) std::copy(h_hist.begin() + (size_t)q * kChromaHist, h_hist.begin() + (size_t)(q + 1) * kChromaHist, out_hist + (size_t)kChromaHist * i);
      if (out_stats && !h_bad[q])
        for (int k = 0; k < 4; ++k) out_stats[4 * i + k] = h_stats[4 * (size_t)q + k];
    }
  }
  return AFX_OK;
}

// ---- onset_strength / tempogram / tempo (04_feature_extraction_experiment/feature_extractor.py:592-622) -----------------
// the plan's table, at first use: bpm and logprior (afx_tempo_table), then the periodic Hann window of win lags as float32
static int rhythm_setup(afx_plan* pl) {
  if (pl->rh_tabrec.window) return AFX_OK;
  int32_t win = 0, kmin = 0;
  int rc = afx_tempo_table(pl->p.sr, &win, &kmin, nullptr, nullptr);
  if (rc != AFX_OK) { set_error("afx_rhythm_batch: the 8 s tempogram window must hold 2 .. 768 frames (128 <= sr <= 49215)"); return rc; }
  if ((rc = mel_images_setup(pl, "afx_rhythm_batch")) != AFX_OK) return rc;
  std::vector<double> tab((size_t)2 * win);            // bpm, logprior; the window as float32 behind them
  if ((rc = afx_tempo_table(pl->p.sr, &win, &kmin, tab.data(), tab.data() + win)) != AFX_OK) return rc;
  std::vector<float> hw(win);
  for (int i = 0; i < win; ++i) hw[i] = (float)(0.5 - 0.5 * std::cos(2.0 * M_PI * (double)i / (double)win));
  const size_t tab_bytes = tab.size() * sizeof(double);
  if ((rc = ensure(pl->rh_tab, tab_bytes + hw.size() * sizeof(float))) != AFX_OK) return rc;
  HIP_TRY(hipMemcpy(pl->rh_tab.p, tab.data(), tab_bytes, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy((char*)pl->rh_tab.p + tab_bytes, hw.data(), hw.size() * sizeof(float), hipMemcpyHostToDevice));
  RhythmTab t{};
  t.bpm = (const double*)pl->rh_tab.p; t.logprior = t.bpm + win; t.win = win;
  t.window = (const float*)((const char*)pl->rh_tab.p + tab_bytes);
  pl->rh_tabrec = t;                                   // set last: its window pointer marks the table as ready
  return AFX_OK;
}

extern "C" int afx_rhythm_batch(afx_plan* pl, const void* samples, int sample_fmt, int mem_kind,
                                const int64_t* offsets, const int64_t* lengths, int n_clips, int flags,
                                float* out_env, const int64_t* env_off, float* out_tempogram, const int64_t* tg_off,
                                double* out_acmean, double* out_tempo, int32_t* out_lag, double* out_stats,
                                int32_t* out_status) {
  const char* who = "afx_rhythm_batch";
  if (n_clips > 0 && (!out_status || !out_tempo || !out_lag)) return null_arg(who);
  int rc = check_batch_args(who, pl, samples, sample_fmt, mem_kind, offsets, lengths, n_clips, true);
  if (rc != AFX_OK) return rc;
  if ((rc = check_stft_plan(who, pl, flags, AFX_FLAG_PREEMPH, true)) != AFX_OK) return rc;
  int32_t win = 0;
  if (afx_tempo_table(pl->p.sr, &win, nullptr, nullptr, nullptr) != AFX_OK) {
    set_error("afx_rhythm_batch: the 8 s tempogram window must hold 2 .. 768 frames (128 <= sr <= 49215)");
    return AFX_ERR_UNSUPPORTED;
  }
  if (n_clips > 0 && ((out_env && !env_off) || (out_tempogram && !tg_off))) {
    set_error("afx_rhythm_batch: out_env needs env_off, out_tempogram needs tg_off");
    return AFX_ERR_INVALID;
  }
  if ((rc = check_clip_ranges(who, offsets, lengths, out_env ? env_off : nullptr, n_clips, INT64_MAX / 4)) != AFX_OK) return rc;
  if ((rc = check_clip_ranges(who, offsets, lengths, out_tempogram ? tg_off : nullptr, n_clips, INT64_MAX / 4)) != AFX_OK) return rc;
  const int M = pl->p.n_mels;
  const double nan = std::nan("");
  for (int i = 0; i < n_clips; ++i) {
    out_status[i] = lengths[i] == 0 ? AFX_CLIP_TOO_SHORT : AFX_CLIP_OK;
    out_tempo[i] = nan; out_lag[i] = 0;
    if (out_stats) out_stats[2 * i] = out_stats[2 * i + 1] = nan;
    if (out_acmean) std::fill(out_acmean + (size_t)win * i, out_acmean + (size_t)win * (i + 1), 0.0);
    if (lengths[i] == 0) {                              // one all-zero frame
      if (out_env) out_env[env_off[i]] = 0.f;
      if (out_tempogram) std::fill(out_tempogram + tg_off[i], out_tempogram + tg_off[i] + win, 0.f);
    }
  }
  if (n_clips == 0) return AFX_OK;
  if ((rc = begin_plan_call(who, pl)) != AFX_OK) return rc;
  if ((rc = rhythm_setup(pl)) != AFX_OK) return rc;
  hipStream_t s = pl->ctx->stream;
  const RhythmTab tab = pl->rh_tabrec;
  const bool want_tg = out_tempogram != nullptr;
  const HpssTabs tb{pl->f3.window, pl->f3.w1024, pl->f3.w2048};
  StftCost cost{};
  cost.per_frame = kHpssPowPitch * 4 + kRhMels * 4 + 4 + (want_tg ? win * 4 : 0);
  cost.per_tile = win * 8;
  cost.per_sample = 4 + upload_sample_bytes(sample_fmt, mem_kind);
  cost.per_clip = win * 8 + 128;
  cost.tile = kRhTile; cost.tile_cap = INT32_MAX / 2;
  StftChunk ck;
  std::vector<uint32_t> h_bad;
  std::vector<double> h_res;
  for (int c0 = 0; c0 < n_clips; c0 = ck.next) {
    cut_stft_chunk(offsets, lengths, n_clips, c0, dev_env().rhythm_budget, cost, ck);
    const int n = (int)ck.recs.size(), tiles = ck.tiles;
    const int64_t frames = ck.frames;
    if (n == 0) continue;
    if ((rc = ensure(pl->ch_s, (size_t)frames * kHpssPowPitch * sizeof(float))) != AFX_OK) return rc;
    if ((rc = ensure(pl->rh_db, (size_t)frames * kRhMels * sizeof(float))) != AFX_OK) return rc;
    if ((rc = ensure(pl->rh_max, n * sizeof(uint32_t))) != AFX_OK) return rc;
    if ((rc = ensure(pl->rh_env, (size_t)frames * sizeof(float))) != AFX_OK) return rc;
    if ((rc = ensure(pl->rh_parts, (size_t)tiles * win * sizeof(double))) != AFX_OK) return rc;
    if (want_tg && (rc = ensure(pl->rh_tg, (size_t)frames * win * sizeof(float))) != AFX_OK) return rc;
    if ((rc = ensure(pl->rh_acmean, (size_t)n * win * sizeof(double))) != AFX_OK) return rc;
    if ((rc = ensure(pl->rh_res, (size_t)n * 4 * sizeof(double))) != AFX_OK) return rc;
    if ((rc = stage_stft_chunk(pl, samples, sample_fmt, mem_kind, flags, ck)) != AFX_OK) return rc;
    const HpssClip* d_clips = (const HpssClip*)pl->hp_clips.p;
    const uint32_t* d_bad = (const uint32_t*)pl->hp_bad.p;
    const float* d_y = (const float*)pl->hp_y.p;
    float* d_S = (float*)pl->ch_s.p;
    float* d_env = (float*)pl->rh_env.p;
    float* d_tg = want_tg ? (float*)pl->rh_tg.p : nullptr;
    HIP_TRY(hipMemsetAsync(pl->rh_max.p, 0, n * sizeof(uint32_t), s));
    HIP_TRY(launch_hpss_stft_power(s, d_y, d_clips, d_bad, n, frames, tb, d_S));
    HIP_TRY(launch_rhythm_mel(s, d_S, d_clips, n, tiles, pl->ch_melrec, (float*)pl->rh_db.p, (uint32_t*)pl->rh_max.p));
    HIP_TRY(launch_rhythm_env(s, (const float*)pl->rh_db.p, (const uint32_t*)pl->rh_max.p, d_clips, n, frames, M, d_env));
    HIP_TRY(launch_rhythm_tempogram(s, d_env, d_clips, n, tiles, tab, (double*)pl->rh_parts.p, d_tg));
    HIP_TRY(launch_rhythm_reduce(s, d_env, d_clips, n, tab, (const double*)pl->rh_parts.p, (double*)pl->rh_acmean.p,
                                 (double*)pl->rh_res.p));
    h_res.resize((size_t)n * 4);
    HIP_TRY(hipMemcpyAsync(h_res.data(), pl->rh_res.p, (size_t)n * 4 * sizeof(double), hipMemcpyDeviceToHost, s));
    if (out_env && (rc = copy_rows_out(s, ck, out_env, env_off, d_env, 1, true)) != AFX_OK) return rc;
    if (out_tempogram && (rc = copy_rows_out(s, ck, out_tempogram, tg_off, d_tg, win, true)) != AFX_OK) return rc;
    if (out_acmean) {
      bool dense = ck.idx[n - 1] - ck.idx[0] == n - 1;  // no zero-length clip inside the chunk: the rows are the caller's
      if (dense) {
        HIP_TRY(hipMemcpyAsync(out_acmean + (size_t)win * ck.idx[0], pl->rh_acmean.p, (size_t)n * win * sizeof(double), hipMemcpyDeviceToHost, s));
      } else {
        for (int q = 0; q < n; ++q)
          HIP_TRY(hipMemcpyAsync(out_acmean + (size_t)win * ck.idx[q], (const double*)pl->rh_acmean.p + (size_t)win * q, (size_t)win * sizeof(double), hipMemcpyDeviceToHost, s));
      }
    }
    if ((rc = end_stft_chunk(pl, n, h_bad)) != AFX_OK) return rc;
    for (int q = 0; q < n; ++q) {
      const int i = ck.idx[q];
      out_status[i] = h_bad[q] ? AFX_CLIP_NONFINITE : AFX_CLIP_OK;
      if (h_bad[q]) continue;                            // its rows are zero: so are the envelope, the tempogram and acmean
      out_tempo[i] = h_res[4 * (size_t)q]; out_lag[i] = (int32_t)h_res[4 * (size_t)q + 3];
      if (out_stats) { out_stats[2 * i] = h_res[4 * (size_t)q + 1]; out_stats[2 * i + 1] = h_res[4 * (size_t)q + 2]; }
    }
  }
  return AFX_OK;
}

// ---- beat positions (librosa.beat.beat_track, 04_feature_extraction_experiment/feature_extractor.py:604-607) ----
// T values of `esz` bytes per frame of a chunk to the caller's dst + esz off[clip], as they lie in src: one copy when the
// caller's layout is the chunk's, else one per clip
static int copy_frames_out(hipStream_t s, const StftChunk& ck, void* dst, const int64_t* off, const void* src, size_t esz) {
  const int n = (int)ck.recs.size();
  bool packed = true;
  for (int q = 0; q < n && packed; ++q) packed = off[ck.idx[q]] - off[ck.idx[0]] == ck.recs[q].frame_base;
  if (packed) {
    HIP_TRY(hipMemcpyAsync((char*)dst + esz * (size_t)off[ck.idx[0]], src, esz * (size_t)ck.frames, hipMemcpyDeviceToHost, s));
    return AFX_OK;
  }
  for (int q = 0; q < n; ++q)
    HIP_TRY(hipMemcpyAsync((char*)dst + esz * (size_t)off[ck.idx[q]], (const char*)src + esz * (size_t)ck.recs[q].frame_base,
                           esz * (size_t)ck.recs[q].T, hipMemcpyDeviceToHost, s));
  return AFX_OK;
}

extern "C" int afx_beat_batch(afx_plan* pl, const void* samples, int sample_fmt, int mem_kind,
                              const int64_t* offsets, const int64_t* lengths, int n_clips, int flags,
                              const double* in_bpm, double tightness, int trim,
                              uint8_t* out_beats, const int64_t* frame_off,
                              int32_t* out_n_beats, double* out_tempo, int32_t* out_fpb,
                              float* out_env, double* out_localscore, double* out_cumscore, int32_t* out_backlink,
                              int32_t* out_status) {
  const char* who = "afx_beat_batch";
  const bool envm = (flags & AFX_BEAT_INPUT_ENVELOPE) != 0;
  if (n_clips > 0 && (!out_status || !out_tempo || !out_fpb || !out_n_beats || !out_beats || !frame_off)) return null_arg(who);
  int rc = check_batch_args(who, pl, samples, sample_fmt, mem_kind, offsets, lengths, n_clips, true);
  if (rc != AFX_OK) return rc;
  if ((rc = check_stft_plan(who, pl, flags, AFX_FLAG_PREEMPH | AFX_BEAT_INPUT_ENVELOPE, true)) != AFX_OK) return rc;
  if (envm && (flags & AFX_FLAG_PREEMPH)) { set_error("afx_beat_batch: AFX_FLAG_PREEMPH does not apply to envelopes"); return AFX_ERR_INVALID; }
  if (envm && sample_fmt != AFX_FMT_F32) { set_error("afx_beat_batch: envelopes are float32"); return AFX_ERR_INVALID; }
  if (!std::isfinite(tightness) || tightness <= 0.0) { set_error("afx_beat_batch: tightness must be finite and > 0"); return AFX_ERR_INVALID; }
  int32_t win = 0;
  if (afx_tempo_table(pl->p.sr, &win, nullptr, nullptr, nullptr) != AFX_OK) {
    set_error("afx_beat_batch: the 8 s tempogram window must hold 2 .. 768 frames (128 <= sr <= 49215)");
    return AFX_ERR_UNSUPPORTED;
  }
  if ((rc = check_clip_ranges(who, offsets, lengths, frame_off, n_clips, INT64_MAX / 8)) != AFX_OK) return rc;
  const double fps = (double)pl->p.sr / 512.0;
  for (int i = 0; i < n_clips; ++i) {
    if (envm && lengths[i] > ((int64_t)1 << 22)) {
      set_error("afx_beat_batch: clip " + std::to_string(i) + ": more than 2^22 frames is not supported");
      return AFX_ERR_UNSUPPORTED;
    }
    int32_t f = 0;
    if (in_bpm && (!std::isfinite(in_bpm[i]) || in_bpm[i] < 0.0 || (in_bpm[i] > 0.0 && !beat_fpb(fps, in_bpm[i], &f)))) {
      set_error("afx_beat_batch: clip " + std::to_string(i) + ": the tempo must be finite, >= 0 and give 1 .. 768 frames per beat");
      return AFX_ERR_INVALID;
    }
  }
  // envelope mode cuts with sample counts that give the clips' frame counts: T frames = 1 + ((T - 1) 512 + 1) / 512
  std::vector<int64_t> cut_len;
  if (envm) {
    cut_len.resize(n_clips);
    for (int i = 0; i < n_clips; ++i) cut_len[i] = lengths[i] > 0 ? (lengths[i] - 1) * 512 + 1 : 0;
  }
  const int64_t* clens = envm ? cut_len.data() : lengths;
  const double nan = std::nan("");
  for (int i = 0; i < n_clips; ++i) {
    out_status[i] = (!envm && lengths[i] == 0) ? AFX_CLIP_TOO_SHORT : AFX_CLIP_OK;
    out_tempo[i] = (envm && lengths[i] == 0) ? 0.0 : nan;
    out_fpb[i] = 0; out_n_beats[i] = 0;
    if (!envm && lengths[i] == 0) {                        // one all-zero frame
      const int64_t o = frame_off[i];
      out_beats[o] = 0;
      if (out_env) out_env[o] = 0.f;
      if (out_localscore) out_localscore[o] = 0.0;
      if (out_cumscore) out_cumscore[o] = 0.0;
      if (out_backlink) out_backlink[o] = -1;
    }
  }
  if (n_clips == 0) return AFX_OK;
  if ((rc = begin_plan_call(who, pl)) != AFX_OK) return rc;
  if ((rc = rhythm_setup(pl)) != AFX_OK) return rc;
  hipStream_t s = pl->ctx->stream;
  const RhythmTab tab = pl->rh_tabrec;
  const HpssTabs tb{pl->f3.window, pl->f3.w1024, pl->f3.w2048};
  const int M = pl->p.n_mels;
  // afx_rhythm_batch's record (an envelope costs its upload instead of the STFT's rows) and, per frame, x, the two scores, the
  // backlink and the flag
  StftCost cost{};
  cost.per_frame = (envm ? 4 + 4 : kHpssPowPitch * 4 + kRhMels * 4 + 4) + 3 * 8 + 4 + 1;
  cost.per_tile = win * 8;
  cost.per_sample = envm ? 0 : 4 + upload_sample_bytes(sample_fmt, mem_kind);
  cost.per_clip = win * 8 + 128 + (int64_t)sizeof(BeatRec) + 8;
  cost.tile = kRhTile; cost.tile_cap = INT32_MAX / 2;
  StftChunk ck;
  std::vector<uint32_t> h_bad;
  std::vector<BeatRec> h_rec;
  std::vector<double> h_bpm;
  for (int c0 = 0; c0 < n_clips; c0 = ck.next) {
    cut_stft_chunk(offsets, clens, n_clips, c0, dev_env().rhythm_budget, cost, ck);
    const int n = (int)ck.recs.size(), tiles = ck.tiles;
    const int64_t frames = ck.frames;
    if (n == 0) continue;
    if ((rc = ensure(pl->rh_env, (size_t)frames * sizeof(float))) != AFX_OK) return rc;
    if ((rc = ensure(pl->rh_parts, (size_t)tiles * win * sizeof(double))) != AFX_OK) return rc;
    if ((rc = ensure(pl->rh_acmean, (size_t)n * win * sizeof(double))) != AFX_OK) return rc;
    if ((rc = ensure(pl->rh_res, (size_t)n * 4 * sizeof(double))) != AFX_OK) return rc;
    if ((rc = ensure(pl->bt_x, (size_t)frames * sizeof(double))) != AFX_OK) return rc;
    if ((rc = ensure(pl->bt_ls, (size_t)frames * sizeof(double))) != AFX_OK) return rc;
    if ((rc = ensure(pl->bt_cum, (size_t)frames * sizeof(double))) != AFX_OK) return rc;
    if ((rc = ensure(pl->bt_bl, (size_t)frames * sizeof(int32_t))) != AFX_OK) return rc;
    if ((rc = ensure(pl->bt_beats, (size_t)frames)) != AFX_OK) return rc;
    if ((rc = ensure(pl->bt_rec, (size_t)n * sizeof(BeatRec))) != AFX_OK) return rc;
    float* d_env = (float*)pl->rh_env.p;
    const HpssClip* d_clips = (const HpssClip*)pl->hp_clips.p;
    const uint32_t* d_bad = (const uint32_t*)pl->hp_bad.p;
    if (envm) {
      // the chunk's envelopes, [lo, hi) of the caller's buffer
      int64_t lo = INT64_MAX, hi = 0;
      for (int q = 0; q < n; ++q) { lo = std::min(lo, offsets[ck.idx[q]]); hi = std::max(hi, offsets[ck.idx[q]] + lengths[ck.idx[q]]); }
      const float* d_in = (const float*)samples;
      for (HpssClip& r : ck.recs) r.len = r.T;
      if (mem_kind == AFX_MEM_HOST) {
        if ((rc = ensure(pl->samples, (size_t)(hi - lo) * sizeof(float) + 16)) != AFX_OK) return rc;
        HIP_TRY(hipMemcpyAsync(pl->samples.p, (const float*)samples + lo, (size_t)(hi - lo) * sizeof(float), hipMemcpyHostToDevice, s));
        for (HpssClip& r : ck.recs) r.in_off -= lo;
        d_in = (const float*)pl->samples.p;
      }
      if ((rc = ensure(pl->hp_clips, n * sizeof(HpssClip))) != AFX_OK) return rc;
      if ((rc = ensure(pl->hp_bad, n * sizeof(uint32_t))) != AFX_OK) return rc;
      d_clips = (const HpssClip*)pl->hp_clips.p; d_bad = (const uint32_t*)pl->hp_bad.p;
      HIP_TRY(hipMemcpyAsync(pl->hp_clips.p, ck.recs.data(), n * sizeof(HpssClip), hipMemcpyHostToDevice, s));
      HIP_TRY(launch_beat_stage(s, d_in, d_clips, n, d_env, (uint32_t*)pl->hp_bad.p));
    } else {
      if ((rc = ensure(pl->ch_s, (size_t)frames * kHpssPowPitch * sizeof(float))) != AFX_OK) return rc;
      if ((rc = ensure(pl->rh_db, (size_t)frames * kRhMels * sizeof(float))) != AFX_OK) return rc;
      if ((rc = ensure(pl->rh_max, n * sizeof(uint32_t))) != AFX_OK) return rc;
      if ((rc = stage_stft_chunk(pl, samples, sample_fmt, mem_kind, flags & AFX_FLAG_PREEMPH, ck)) != AFX_OK) return rc;
      d_clips = (const HpssClip*)pl->hp_clips.p; d_bad = (const uint32_t*)pl->hp_bad.p;
      float* d_S = (float*)pl->ch_s.p;
      HIP_TRY(hipMemsetAsync(pl->rh_max.p, 0, n * sizeof(uint32_t), s));
      HIP_TRY(launch_hpss_stft_power(s, (const float*)pl->hp_y.p, d_clips, d_bad, n, frames, tb, d_S));
      HIP_TRY(launch_rhythm_mel(s, d_S, d_clips, n, tiles, pl->ch_melrec, (float*)pl->rh_db.p, (uint32_t*)pl->rh_max.p));
      HIP_TRY(launch_rhythm_env(s, (const float*)pl->rh_db.p, (const uint32_t*)pl->rh_max.p, d_clips, n, frames, M, d_env));
    }
    HIP_TRY(launch_rhythm_tempogram(s, d_env, d_clips, n, tiles, tab, (double*)pl->rh_parts.p, nullptr));
    HIP_TRY(launch_rhythm_reduce(s, d_env, d_clips, n, tab, (const double*)pl->rh_parts.p, (double*)pl->rh_acmean.p,
                                 (double*)pl->rh_res.p));
    const double* d_bpm = nullptr;
    if (in_bpm) {
      h_bpm.resize(n);
      for (int q = 0; q < n; ++q) h_bpm[q] = in_bpm[ck.idx[q]];
      if ((rc = ensure(pl->bt_bpm, (size_t)n * sizeof(double))) != AFX_OK) return rc;
      HIP_TRY(hipMemcpyAsync(pl->bt_bpm.p, h_bpm.data(), (size_t)n * sizeof(double), hipMemcpyHostToDevice, s));
      d_bpm = (const double*)pl->bt_bpm.p;
    }
    // a clip the dynamic programme does not run for keeps these: scores 0, backlinks -1, no flags
    HIP_TRY(hipMemsetAsync(pl->bt_ls.p, 0, (size_t)frames * sizeof(double), s));
    HIP_TRY(hipMemsetAsync(pl->bt_cum.p, 0, (size_t)frames * sizeof(double), s));
    HIP_TRY(hipMemsetAsync(pl->bt_bl.p, 0xff, (size_t)frames * sizeof(int32_t), s));
    HIP_TRY(hipMemsetAsync(pl->bt_beats.p, 0, (size_t)frames, s));
    BeatRec* d_rec = (BeatRec*)pl->bt_rec.p;
    HIP_TRY(launch_beat_score(s, d_env, d_clips, d_bad, n, (const double*)pl->rh_res.p, d_bpm, fps, (double*)pl->bt_x.p,
                              (double*)pl->bt_ls.p, d_rec));
    HIP_TRY(launch_beat_dp(s, d_clips, n, d_rec, (const double*)pl->bt_ls.p, tightness, (double*)pl->bt_cum.p, (int32_t*)pl->bt_bl.p));
    HIP_TRY(launch_beat_finish(s, d_clips, n, (const double*)pl->bt_ls.p, (const double*)pl->bt_cum.p, (const int32_t*)pl->bt_bl.p,
                               trim != 0, (uint64_t*)pl->bt_x.p, (uint8_t*)pl->bt_beats.p, d_rec));
    h_rec.resize(n);
    HIP_TRY(hipMemcpyAsync(h_rec.data(), d_rec, (size_t)n * sizeof(BeatRec), hipMemcpyDeviceToHost, s));
    if ((rc = copy_frames_out(s, ck, out_beats, frame_off, pl->bt_beats.p, 1)) != AFX_OK) return rc;
    if (out_env && (rc = copy_frames_out(s, ck, out_env, frame_off, d_env, sizeof(float))) != AFX_OK) return rc;
    if (out_localscore && (rc = copy_frames_out(s, ck, out_localscore, frame_off, pl->bt_ls.p, sizeof(double))) != AFX_OK) return rc;
    if (out_cumscore && (rc = copy_frames_out(s, ck, out_cumscore, frame_off, pl->bt_cum.p, sizeof(double))) != AFX_OK) return rc;
    if (out_backlink && (rc = copy_frames_out(s, ck, out_backlink, frame_off, pl->bt_bl.p, sizeof(int32_t))) != AFX_OK) return rc;
    if ((rc = end_stft_chunk(pl, n, h_bad)) != AFX_OK) return rc;
    for (int q = 0; q < n; ++q) {
      const int i = ck.idx[q];
      out_status[i] = h_bad[q] ? AFX_CLIP_NONFINITE : AFX_CLIP_OK;
      if (h_bad[q]) continue;                              // tempo NaN, no beats; its envelope and scores are zero
      out_tempo[i] = h_rec[q].tempo; out_fpb[i] = h_rec[q].fpb; out_n_beats[i] = h_rec[q].n_beats;
    }
  }
  return AFX_OK;
}

// ---- the spectral, harmonic, timbre and rhythm groups on one STFT (04_feature_extraction_experiment/feature_extractor.py:624-687;
// DESIGN.md 18) ------------------------------------------------------------------------------------------------------------
// the MFCC table, at first use
static int groups_setup(afx_plan* pl) {
  if (pl->gp_dct.p) return AFX_OK;
  std::vector<float> t((size_t)kGroupsMfcc * kRhMels);
  groups_dct_table(pl->p.n_mels, t.data());
  DevBuf b;
  int rc;
  if ((rc = ensure(b, t.size() * sizeof(float))) != AFX_OK) return rc;
  hipError_t e = hipMemcpy(b.p, t.data(), t.size() * sizeof(float), hipMemcpyHostToDevice);
  if (e != hipSuccess) { release(b); set_error(std::string("afx_groups_batch: table upload: ") + hipGetErrorString(e)); return AFX_ERR_HIP; }
  pl->gp_dct = b;                                      // set last: its presence marks the table as ready
  return AFX_OK;
}

// The experiment preprocess of a cut chunk (run_filtfilt_chain, as afx_sosfiltfilt_batch's): the clips of ck
// (in_off: the caller's offsets) from the caller's device buffer or a copy of [lo, hi) in gp_in to gp_filt at y_off; the
// records then name gp_filt as their input.  The states stay in the context's ft_st, one per record.
static int groups_preprocess_chunk(afx_plan* pl, const void* samples, int sample_fmt, int mem_kind, int n_sections,
                                   StftChunk& ck, std::vector<FiltClip>& frecs) {
  afx_ctx* ctx = pl->ctx;
  hipStream_t s = ctx->stream;
  const int n = (int)ck.recs.size();
  int rc;
  const void* d_in = samples;
  const bool h_in = mem_kind == AFX_MEM_HOST;
  if (h_in) {
    const size_t esz = (size_t)upload_sample_bytes(sample_fmt, mem_kind);
    if ((rc = ensure(pl->gp_in, (size_t)(ck.hi - ck.lo) * esz + 16)) != AFX_OK) return rc;
    HIP_TRY(hipMemcpyAsync(pl->gp_in.p, (const char*)samples + (size_t)ck.lo * esz, (size_t)(ck.hi - ck.lo) * esz, hipMemcpyHostToDevice, s));
    d_in = pl->gp_in.p;
  }
  frecs.resize(n);
  int64_t tiles = 0;
  for (int q = 0; q < n; ++q) {
    const HpssClip& r = ck.recs[q];
    const int64_t nt = (r.len + 2 * (int64_t)kGroupsPadlen + kFiltTile - 1) / kFiltTile;
    frecs[q] = FiltClip{h_in ? r.in_off - ck.lo : r.in_off, r.y_off, r.len, (int32_t)tiles, (int32_t)nt};
    tiles += nt;
    if (tiles > (1 << 24)) { set_error("afx_groups_batch: clip too large for one launch"); return AFX_ERR_UNSUPPORTED; }
  }
  if ((rc = ensure(pl->gp_filt, (size_t)ck.samples * sizeof(float) + 64)) != AFX_OK) return rc;
  if ((rc = run_filtfilt_chain(ctx, d_in, sample_fmt, AFX_FILT_EXPERIMENT, 0.98f, kGroupsPadlen, n_sections, frecs, tiles,
                               (const FiltTab*)ctx->ft_tab.p, (float*)pl->gp_filt.p)) != AFX_OK) return rc;
  for (HpssClip& r : ck.recs) r.in_off = r.y_off;
  return AFX_OK;
}

extern "C" int afx_groups_batch(afx_plan* pl, const void* samples, int sample_fmt, int mem_kind,
                                const int64_t* offsets, const int64_t* lengths, int n_clips, int flags, int groups,
                                double* out_stats, double* out_tuning, int32_t* out_lag, int32_t* out_status) {
  const char* who = "afx_groups_batch";
  if (n_clips > 0 && (!out_stats || !out_status)) return null_arg(who);
  int rc = check_batch_args(who, pl, samples, sample_fmt, mem_kind, offsets, lengths, n_clips, true);
  if (rc != AFX_OK) return rc;
  if (groups <= 0 || (groups & ~kGroupsAll)) { set_error("afx_groups_batch: groups must be a non-empty set of AFX_GROUP_* bits"); return AFX_ERR_INVALID; }
  const bool sp = groups & AFX_GROUP_SPECTRAL, ha = groups & AFX_GROUP_HARMONIC, ti = groups & AFX_GROUP_TIMBRE, rh = groups & AFX_GROUP_RHYTHM;
  const bool pre = (flags & AFX_GROUPS_PREPROCESS) != 0, keep = sp && (flags & AFX_GROUPS_STORE_DESC) != 0;
  if ((rc = check_stft_plan(who, pl, flags, AFX_FLAG_PREEMPH | AFX_GROUPS_PREPROCESS | AFX_GROUPS_STORE_DESC, ti || rh)) != AFX_OK) return rc;
  if (pre && (flags & AFX_FLAG_PREEMPH)) { set_error("afx_groups_batch: AFX_GROUPS_PREPROCESS has a pre-emphasis of its own; AFX_FLAG_PREEMPH cannot be added"); return AFX_ERR_INVALID; }
  // only the centroid of h reads the bands of a plan that has none (sr <= 12.8 kHz): its bin width is all it needs
  SpecBands sb{};
  sb.hz_per_bin = (float)((double)pl->p.sr / 2048.0); sb.roll_percent = 0.85f;
  if (sp && !spectral_bands(pl->p.sr, sb)) return AFX_ERR_UNSUPPORTED;
  int32_t win = 0;
  if (rh && afx_tempo_table(pl->p.sr, &win, nullptr, nullptr, nullptr) != AFX_OK) {
    set_error("afx_groups_batch: the 8 s tempogram window must hold 2 .. 768 frames (128 <= sr <= 49215)");
    return AFX_ERR_UNSUPPORTED;
  }
  FiltTab ftab;
  int n_sections = 0;
  if (pre) {
    double sos[kFiltMaxS * 6];
    n_sections = 3;
    if ((rc = afx_butter_sos(5, 200.0 / ((double)pl->p.sr / 2.0), 1, sos)) != AFX_OK) return rc;
    const char* why = "";
    if (!filt_build_tab(sos, n_sections, ftab, &why)) { set_error(std::string(who) + ": " + why); return AFX_ERR_INVALID; }
  }
  if ((rc = check_clip_ranges(who, offsets, lengths, nullptr, n_clips, INT64_MAX / 4)) != AFX_OK) return rc;
  const double nan = std::nan("");
  // a clip the preprocess refuses (scipy's filtfilt needs more than padlen samples) is in no chunk, like an empty one
  std::vector<int64_t> eff((size_t)n_clips);
  for (int i = 0; i < n_clips; ++i) {
    eff[i] = pre && lengths[i] <= kGroupsPadlen ? 0 : lengths[i];
    out_status[i] = eff[i] == 0 ? AFX_CLIP_TOO_SHORT : AFX_CLIP_OK;
    std::fill(out_stats + (size_t)kGroupsStats * i, out_stats + (size_t)kGroupsStats * (i + 1), nan);
    if (out_tuning) out_tuning[i] = 0.0;
    if (out_lag) out_lag[i] = 0;
  }
  if (n_clips == 0) return AFX_OK;
  if ((rc = begin_plan_call(who, pl)) != AFX_OK) return rc;
  if (ti && (rc = chroma_setup(pl)) != AFX_OK) return rc;
  if (ti && (rc = groups_setup(pl)) != AFX_OK) return rc;
  if (rh && (rc = rhythm_setup(pl)) != AFX_OK) return rc;
  hipStream_t s = pl->ctx->stream;
  if (pre) {
    if ((rc = ensure(pl->ctx->ft_tab, sizeof(FiltTab))) != AFX_OK) return rc;
    HIP_TRY(hipMemcpyAsync(pl->ctx->ft_tab.p, &ftab, sizeof(FiltTab), hipMemcpyHostToDevice, s));
  }
  pl->gp_rows.clear();
  const ChromaBand band = piptrack_band(pl->p.sr);
  const RhythmTab tab = pl->rh_tabrec;
  const HpssTabs tb{pl->f3.window, pl->f3.w1024, pl->f3.w2048};
  const int M = pl->p.n_mels;
  const bool need_s = sp || ti || rh;
  StftCost cost{};
  groups_cost(groups, pre, cost);
  StftChunk ck;
  std::vector<FiltClip> frecs;
  std::vector<HpssClip> recs64;
  std::vector<int64_t> d_off;
  std::vector<uint32_t> h_bad;
  std::vector<double> h_rec;
  std::vector<int32_t> h_ints;
  for (int c0 = 0; c0 < n_clips; c0 = ck.next) {
    cut_stft_chunk(offsets, eff.data(), n_clips, c0, dev_env().groups_budget, cost, ck);
    const int n = (int)ck.recs.size(), tiles = ck.tiles;
    const int64_t frames = ck.frames;
    if (n == 0) continue;
    const size_t spec_bytes = (size_t)frames * kHpssPitch * sizeof(float2), sig_bytes = (size_t)ck.samples * sizeof(float) + 64;
    const size_t desc_bytes = (size_t)frames * kSpecFloats * sizeof(float);
    if (need_s && (rc = ensure(pl->ch_s, (size_t)frames * kHpssPowPitch * sizeof(float))) != AFX_OK) return rc;
    if (sp) {
      if ((rc = ensure(pl->gp_desc, desc_bytes)) != AFX_OK) return rc;
      if ((rc = ensure(pl->gp_sstats, (size_t)n * 8 * sizeof(double))) != AFX_OK) return rc;
    }
    if (ha) {
      if ((rc = ensure(pl->hp_h, sig_bytes)) != AFX_OK) return rc;
      if ((rc = ensure(pl->hp_x, spec_bytes)) != AFX_OK) return rc;
      if ((rc = ensure(pl->hp_yh, spec_bytes)) != AFX_OK) return rc;
      if ((rc = ensure(pl->gp_clips64, n * sizeof(HpssClip))) != AFX_OK) return rc;
      if ((rc = ensure(pl->gp_hdesc, desc_bytes)) != AFX_OK) return rc;
      if ((rc = ensure(pl->gp_doff, n * sizeof(int64_t))) != AFX_OK) return rc;
      if ((rc = ensure(pl->hp_stats, (size_t)n * 4 * sizeof(double))) != AFX_OK) return rc;
    }
    if (ti) {
      if ((rc = ensure(pl->ch_slot, n * sizeof(int32_t))) != AFX_OK) return rc;
      if ((rc = ensure(pl->ch_hist, (size_t)n * kChromaHist * sizeof(int32_t))) != AFX_OK) return rc;
      if (band.nr > 0) {
        if ((rc = ensure(pl->ch_mag, (size_t)frames * band.nr * sizeof(float))) != AFX_OK) return rc;
        if ((rc = ensure(pl->ch_bin, (size_t)frames * band.nr)) != AFX_OK) return rc;
      }
      if ((rc = ensure(pl->ch_parts, (size_t)frames * 4 * sizeof(double))) != AFX_OK) return rc;
      if ((rc = ensure(pl->gp_cstats, (size_t)n * 4 * sizeof(double))) != AFX_OK) return rc;
      if ((rc = ensure(pl->gp_mparts, (size_t)frames * 2 * sizeof(double))) != AFX_OK) return rc;
      if ((rc = ensure(pl->gp_mstats, (size_t)n * 2 * sizeof(double))) != AFX_OK) return rc;
    }
    if (ti || rh) {
      if ((rc = ensure(pl->rh_db, (size_t)frames * kRhMels * sizeof(float))) != AFX_OK) return rc;
      if ((rc = ensure(pl->rh_max, n * sizeof(uint32_t))) != AFX_OK) return rc;
    }
    if (rh) {
      if ((rc = ensure(pl->rh_env, (size_t)frames * sizeof(float))) != AFX_OK) return rc;
      if ((rc = ensure(pl->rh_parts, (size_t)tiles * win * sizeof(double))) != AFX_OK) return rc;
      if ((rc = ensure(pl->rh_acmean, (size_t)n * win * sizeof(double))) != AFX_OK) return rc;
      if ((rc = ensure(pl->rh_res, (size_t)n * 4 * sizeof(double))) != AFX_OK) return rc;
    }
    if ((rc = ensure(pl->gp_rec, (size_t)n * kGroupsStats * sizeof(double))) != AFX_OK) return rc;
    if ((rc = ensure(pl->gp_ints, (size_t)n * 2 * sizeof(int32_t))) != AFX_OK) return rc;
    // the chunk's signal: the caller's samples, or the preprocess's output, through the front end's prep either way
    if (pre) {
      if ((rc = groups_preprocess_chunk(pl, samples, sample_fmt, mem_kind, n_sections, ck, frecs)) != AFX_OK) return rc;
      if ((rc = stage_stft_chunk(pl, pl->gp_filt.p, AFX_FMT_F32, AFX_MEM_DEVICE, 0, ck)) != AFX_OK) return rc;
      HIP_TRY(launch_groups_mark_bad(s, (const FiltState*)pl->ctx->ft_st.p, n, (uint32_t*)pl->hp_bad.p));
    } else if ((rc = stage_stft_chunk(pl, samples, sample_fmt, mem_kind, flags, ck)) != AFX_OK) {
      return rc;
    }
    const HpssClip* d_clips = (const HpssClip*)pl->hp_clips.p;
    const uint32_t* d_bad = (const uint32_t*)pl->hp_bad.p;
    const float* d_y = (const float*)pl->hp_y.p;
    float* d_S = need_s ? (float*)pl->ch_s.p : nullptr;
    // one STFT of y: the complex rows when HPSS wants them (the power rows are then their squares), else the power rows
    if (ha) {
      HIP_TRY(launch_hpss_stft(s, d_y, d_clips, d_bad, n, frames, tb, (float2*)pl->hp_x.p));
      if (need_s) HIP_TRY(launch_groups_square(s, (const float2*)pl->hp_x.p, frames, d_S));
    } else {
      HIP_TRY(launch_hpss_stft_power(s, d_y, d_clips, d_bad, n, frames, tb, d_S));
    }
    if (sp) {
      HIP_TRY(launch_spec_rows(s, d_S, frames, sb, true, (float*)pl->gp_desc.p));
      HIP_TRY(launch_spec_stats(s, (const float*)pl->gp_desc.p, d_clips, n, (double*)pl->gp_sstats.p));
    }
    if (ti) {
      int32_t* d_slot = (int32_t*)pl->ch_slot.p;
      if (band.nr > 0) HIP_TRY(launch_chroma_peaks(s, d_S, frames, band, (float*)pl->ch_mag.p, (uint8_t*)pl->ch_bin.p));
      HIP_TRY(launch_chroma_tuning(s, d_clips, n, band, (const float*)pl->ch_mag.p, (const uint8_t*)pl->ch_bin.p, d_slot,
                                   (int32_t*)pl->ch_hist.p));
      HIP_TRY(launch_chroma_apply(s, d_S, d_clips, n, tiles, d_slot, (const float*)pl->ch_grid.p, (const float*)pl->ch_extra.p,
                                  pl->ch_melrec, true, nullptr, nullptr, (double*)pl->ch_parts.p));
      HIP_TRY(launch_chroma_stats(s, d_clips, n, M, (const double*)pl->ch_parts.p, (double*)pl->gp_cstats.p));
    }
    if (ti || rh) {
      // the mel dB rows are k_rhythm_mel's output, whichever of the two groups reads them
      HIP_TRY(hipMemsetAsync(pl->rh_max.p, 0, n * sizeof(uint32_t), s));
      HIP_TRY(launch_rhythm_mel(s, d_S, d_clips, n, tiles, pl->ch_melrec, (float*)pl->rh_db.p, (uint32_t*)pl->rh_max.p));
    }
    if (ti) {
      HIP_TRY(launch_mfcc_rows(s, (const float*)pl->rh_db.p, (const uint32_t*)pl->rh_max.p, d_clips, n, frames, M,
                               (const float*)pl->gp_dct.p, (double*)pl->gp_mparts.p));
      HIP_TRY(launch_mfcc_stats(s, (const double*)pl->gp_mparts.p, d_clips, n, (double*)pl->gp_mstats.p));
    }
    if (rh) {
      float* d_env = (float*)pl->rh_env.p;
      HIP_TRY(launch_rhythm_env(s, (const float*)pl->rh_db.p, (const uint32_t*)pl->rh_max.p, d_clips, n, frames, M, d_env));
      HIP_TRY(launch_rhythm_tempogram(s, d_env, d_clips, n, tiles, tab, (double*)pl->rh_parts.p, nullptr));
      HIP_TRY(launch_rhythm_reduce(s, d_env, d_clips, n, tab, (const double*)pl->rh_parts.p, (double*)pl->rh_acmean.p,
                                   (double*)pl->rh_res.p));
    }
    if (ha) {
      // k_hpss_mask's tiles hold 64 frames, the chunk's 16: the same records with tile_base counted in its tiles
      recs64 = ck.recs;
      int tiles64 = 0;
      for (HpssClip& r : recs64) { r.tile_base = tiles64; tiles64 += (r.T + kHpssTile - 1) / kHpssTile; }
      HIP_TRY(hipMemcpyAsync(pl->gp_clips64.p, recs64.data(), n * sizeof(HpssClip), hipMemcpyHostToDevice, s));
      float* d_h = (float*)pl->hp_h.p;
      HIP_TRY(launch_hpss_mask(s, (const float2*)pl->hp_x.p, (const HpssClip*)pl->gp_clips64.p, n, tiles64, (float2*)pl->hp_yh.p,
                               nullptr, nullptr));
      HIP_TRY(launch_hpss_irfft(s, (float2*)pl->hp_yh.p, nullptr, frames, tb));
      HIP_TRY(launch_hpss_ola(s, (const float2*)pl->hp_yh.p, nullptr, d_clips, n, ck.max_len, tb, d_h, nullptr));
      // spectral_centroid(y=h): X is dead behind the mask, so its space takes the power rows of h
      float* d_Sh = (float*)pl->hp_x.p;
      HIP_TRY(launch_hpss_stft_power(s, d_h, d_clips, d_bad, n, frames, tb, d_Sh));
      HIP_TRY(launch_spec_rows(s, d_Sh, frames, sb, false, (float*)pl->gp_hdesc.p));
      d_off.resize(n);
      for (int q = 0; q < n; ++q) d_off[q] = kSpecFloats * ck.recs[q].frame_base;
      HIP_TRY(hipMemcpyAsync(pl->gp_doff.p, d_off.data(), n * sizeof(int64_t), hipMemcpyHostToDevice, s));
      HIP_TRY(launch_hpss_stats(s, d_y, d_h, d_clips, n, (const float*)pl->gp_hdesc.p, (const int64_t*)pl->gp_doff.p,
                                (double*)pl->hp_stats.p));
    }
    GroupsSrc src{};
    src.spec = sp ? (const double*)pl->gp_sstats.p : nullptr;
    src.harm = ha ? (const double*)pl->hp_stats.p : nullptr;
    src.chroma = ti ? (const double*)pl->gp_cstats.p : nullptr;
    src.mfcc = ti ? (const double*)pl->gp_mstats.p : nullptr;
    src.slot = ti ? (const int32_t*)pl->ch_slot.p : nullptr;
    src.rhythm = rh ? (const double*)pl->rh_res.p : nullptr;
    src.acmean = rh ? (const double*)pl->rh_acmean.p : nullptr;
    src.filt = pre ? (const FiltState*)pl->ctx->ft_st.p : nullptr;
    src.win = win;
    HIP_TRY(launch_groups_record(s, src, d_clips, d_bad, n, (double*)pl->gp_rec.p, (int32_t*)pl->gp_ints.p));
    h_rec.resize((size_t)n * kGroupsStats); h_ints.resize((size_t)n * 2);
    HIP_TRY(hipMemcpyAsync(h_rec.data(), pl->gp_rec.p, h_rec.size() * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(h_ints.data(), pl->gp_ints.p, h_ints.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    if (keep) {
      const size_t at = pl->gp_rows.size();
      pl->gp_rows.resize(at + (size_t)frames * kSpecFloats);
      HIP_TRY(hipMemcpyAsync(pl->gp_rows.data() + at, pl->gp_desc.p, desc_bytes, hipMemcpyDeviceToHost, s));
    }
    if ((rc = end_stft_chunk(pl, n, h_bad)) != AFX_OK) return rc;
    for (int q = 0; q < n; ++q) {
      const int i = ck.idx[q];
      out_status[i] = h_bad[q] ? AFX_CLIP_NONFINITE : AFX_CLIP_OK;
      if (h_bad[q]) continue;
      std::copy(h_rec.begin() + (size_t)q * kGroupsStats, h_rec.begin() + (size_t)(q + 1) * kGroupsStats, out_stats + (size_t)kGroupsStats * i);
      if (out_tuning && ti) out_tuning[i] = (double)h_ints[2 * (size_t)q] * 0.01 + -0.5;
      if (out_lag) out_lag[i] = h_ints[2 * (size_t)q + 1];
    }
  }
  return AFX_OK;
}

extern "C" int afx_groups_debug_rows(afx_plan* pl, float* out, int64_t n_floats, int64_t* count) {
  if (!pl || !count || n_floats < 0 || (n_floats > 0 && !out)) return null_arg("afx_groups_debug_rows");
  const int64_t have = (int64_t)pl->gp_rows.size();
  if (n_floats > 0) std::copy(pl->gp_rows.begin(), pl->gp_rows.begin() + std::min(have, n_floats), out);
  *count = have;
  return AFX_OK;
}
