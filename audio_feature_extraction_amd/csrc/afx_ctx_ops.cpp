// The entry points of libafx.so that work on a context, not a plan: batched DTW, polyphase resampling, the conversion /
// mix-down of raw WAVE data, zero-phase IIR filtering, the recording screen and the compare sums, the whole-clip DFT and
// the spectral distance, the median and Savitzky-Golay filters with the energy and ZCR groups, BS.1770 loudness,
// spectral gating, librosa-style stft / istft, the phase vocoder and time stretching -- and what they share: the staging of a host batch and the launches of the zero-phase filter.
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <string>
#include <vector>

#include <hip/hip_runtime.h>

#include "afx_decode.h"
#include "afx_devenv.h"
#include "afx_dtw.h"
#include "afx_internal.h"
#include "afx_plan.h"
#include "afx_resample.h"

// ---- what the entry points share (declared in afx_plan.h; the rule of the two buffers is at afx_ctx::wave_in) ----------
int stage_in(afx_ctx* ctx, std::vector<char>& image, int64_t total_bytes, const std::vector<HostPiece>& pieces, const void** d_in) {
  pack_pieces(image, total_bytes, pieces);
  if (int rc = ensure(ctx->wave_in, std::max<size_t>(image.size(), 1))) return rc;
  HIP_TRY(hipMemcpyAsync(ctx->wave_in.p, image.data(), image.size(), hipMemcpyHostToDevice, ctx->stream));
  *d_in = ctx->wave_in.p;
  return AFX_OK;
}

int out_buffer(afx_ctx* ctx, float* out, int out_mem_kind, int64_t total, float** d_out) {
  *d_out = out;
  if (out_mem_kind != AFX_MEM_HOST) return AFX_OK;
  if (int rc = ensure(ctx->wave_out, (size_t)total * sizeof(float))) return rc;
  *d_out = (float*)ctx->wave_out.p;
  return AFX_OK;
}

int fetch_out(afx_ctx* ctx, const float* d_out, int64_t total, std::vector<float>& host) {
  host.resize((size_t)total);
  HIP_TRY(hipMemcpyAsync(host.data(), d_out, (size_t)total * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  return AFX_OK;
}

int run_filtfilt_chain(afx_ctx* ctx, const void* d_in, int sample_fmt, int mode, float preemph, int padlen, int n_sections,
                       const std::vector<FiltClip>& recs, int64_t tiles, const FiltTab* d_tab, float* d_out) {
  hipStream_t s = ctx->stream;
  const int n = (int)recs.size(), nt = (int)tiles, S = n_sections;
  int rc;
  if ((rc = ensure(ctx->ft_clips, n * sizeof(FiltClip))) != AFX_OK) return rc;
  if ((rc = ensure(ctx->ft_st, n * sizeof(FiltState))) != AFX_OK) return rc;
  if ((rc = ensure(ctx->ft_w, (size_t)nt * kFiltTile * sizeof(double))) != AFX_OK) return rc;
  if ((rc = ensure(ctx->ft_carry, (size_t)nt * kFiltB * kFiltZ * sizeof(double))) != AFX_OK) return rc;
  if ((rc = ensure(ctx->ft_tmax, (size_t)nt * sizeof(double))) != AFX_OK) return rc;
  HIP_TRY(hipMemcpyAsync(ctx->ft_clips.p, recs.data(), n * sizeof(FiltClip), hipMemcpyHostToDevice, s));
  const FiltClip* d_clips = (const FiltClip*)ctx->ft_clips.p;
  FiltState* d_st = (FiltState*)ctx->ft_st.p;
  double *W = (double*)ctx->ft_w.p, *carry = (double*)ctx->ft_carry.p, *tmax = (double*)ctx->ft_tmax.p;
  const bool plain = mode == AFX_FILT_PLAIN;
  HIP_TRY(launch_filt_peak(s, d_in, sample_fmt, d_clips, n, d_st));
  HIP_TRY(launch_filt_forward(s, d_in, sample_fmt, mode, -preemph, padlen, S, d_tab, d_clips, n, nt, d_st, W, carry));
  HIP_TRY(launch_filt_scan(s, padlen, S, d_tab, d_clips, n, d_st, carry, false));
  HIP_TRY(launch_filt_backward(s, padlen, S, d_tab, d_clips, n, nt, d_st, W, carry));
  HIP_TRY(launch_filt_scan(s, padlen, S, d_tab, d_clips, n, d_st, carry, true));
  HIP_TRY(launch_filt_final(s, padlen, S, d_tab, d_clips, n, nt, d_st, W, carry, tmax, plain ? d_out : nullptr));
  HIP_TRY(launch_filt_clipmax(s, d_clips, n, tmax, d_st));
  if (!plain) HIP_TRY(launch_filt_scale(s, padlen, d_clips, n, nt, d_st, W, d_out));
  return AFX_OK;
}

// The argument checks of an entry point that reads clips of samples: the context and the arrays (own_ok: its own required
// arrays are there), the sample format where the samples lie and -- out_mem_kind >= 0: it writes samples too -- where the
// result goes, the clip ranges.
static int clip_batch_args(const char* who, afx_ctx* ctx, int sample_fmt, int mem_kind, const int64_t* offsets, const int64_t* lengths,
                           int n_clips, int out_mem_kind, const int64_t* out_offsets, const int32_t* out_status, bool own_ok = true) {
  const bool writes = out_mem_kind >= 0;
  if (!ctx || n_clips < 0 || (n_clips > 0 && (!offsets || !lengths || (writes && !out_offsets) || !out_status || !own_ok))) return null_arg(who);
  int rc;
  if ((rc = check_sample_format(who, sample_fmt, mem_kind)) != AFX_OK) return rc;
  if (writes && (rc = check_sample_format(who, sample_fmt, out_mem_kind)) != AFX_OK) return rc;
  return check_clip_ranges(who, offsets, lengths, out_offsets, n_clips, INT64_MAX / 8);
}

// n samples of esz bytes from element src_off of a host buffer, to element dst_off of the packed image
static HostPiece clip_piece(const void* src, int64_t src_off, int64_t dst_off, int64_t n, size_t esz) {
  return {(const char*)src + (size_t)src_off * esz, dst_off * (int64_t)esz, n * (int64_t)esz};
}

// row i of a table of n-double records, before anything is known of clip i
static void nan_row(double* rec, int n, int i) { std::fill(rec + (size_t)n * i, rec + (size_t)n * (i + 1), std::nan("")); }

// ---- batched DTW (librosa.sequence.dtw): the alignment step the reference runs on the extracted MFCC frames ----------
// The body of afx_dtw_batch (T == nullptr: k_dtw, the default steps) and afx_dtw_steps_batch (T: k_dtw_steps).
static int dtw_run(const std::string& who, afx_ctx* ctx, const float* feats, int dim,
                   const int64_t* x_off, const int64_t* x_len, const int64_t* y_off, const int64_t* y_len,
                   const int32_t* band_r, int n_pairs, int metric, int flags, const DtwSteps* T,
                   double* out_cost, int32_t* out_status,
                   int32_t* out_path, const int64_t* path_off, int32_t* out_path_len,
                   double* out_D, const int64_t* d_off, int32_t* out_end) {
  const bool bt = (flags & AFX_DTW_BACKTRACK) != 0, sd = (flags & AFX_DTW_STORE_D) != 0;
  if (!ctx || n_pairs < 0 || (n_pairs > 0 && (!feats || !x_off || !x_len || !y_off || !y_len || !out_cost || !out_status))) {
    set_error(who + ": null/invalid argument");
    return AFX_ERR_INVALID;
  }
  if (flags & ~(AFX_DTW_BACKTRACK | AFX_DTW_STORE_D | (T ? AFX_DTW_SUBSEQ : 0))) { set_error(who + ": unknown flag"); return AFX_ERR_INVALID; }
  if (metric != AFX_DTW_EUCLIDEAN && metric != AFX_DTW_SQEUCLIDEAN && metric != AFX_DTW_COSINE) {
    set_error(who + ": unknown metric");
    return AFX_ERR_INVALID;
  }
  if (n_pairs > 0 && bt && (!out_path || !path_off || !out_path_len)) {
    set_error(who + ": AFX_DTW_BACKTRACK needs out_path, path_off and out_path_len");
    return AFX_ERR_INVALID;
  }
  if (n_pairs > 0 && sd && (!out_D || !d_off)) { set_error(who + ": AFX_DTW_STORE_D needs out_D and d_off"); return AFX_ERR_INVALID; }
  if (dim < 1) { set_error(who + ": dim must be >= 1"); return AFX_ERR_INVALID; }
  if (dim > kDtwMaxDim) { set_error(who + ": dim > 128 is not supported by the DTW kernel"); return AFX_ERR_UNSUPPORTED; }
  int64_t n_frames = 0;
  for (int p = 0; p < n_pairs; ++p) {
    if (x_off[p] < 0 || y_off[p] < 0 || x_len[p] < 1 || y_len[p] < 1 || x_off[p] > INT64_MAX / 2 || y_off[p] > INT64_MAX / 2 ||
        x_len[p] > INT32_MAX || y_len[p] > INT32_MAX) {
      set_error(who + ": pair " + std::to_string(p) + ": offsets must be >= 0 and lengths >= 1");
      return AFX_ERR_INVALID;
    }
    if (x_len[p] * y_len[p] > ((int64_t)1 << 31) || x_len[p] > (1 << 30) || y_len[p] > (1 << 30)) {
      set_error(who + ": pair " + std::to_string(p) + ": N * M > 2^31 cells is not supported");
      return AFX_ERR_UNSUPPORTED;
    }
    if ((bt && path_off[p] < 0) || (sd && d_off[p] < 0)) {
      set_error(who + ": pair " + std::to_string(p) + ": negative output offset");
      return AFX_ERR_INVALID;
    }
    n_frames = std::max(n_frames, std::max(x_off[p] + x_len[p], y_off[p] + y_len[p]));
  }
  if (n_pairs == 0) return AFX_OK;
  if (n_frames > INT64_MAX / 4 / dim) { set_error(who + ": feature buffer too large"); return AFX_ERR_INVALID; }

  (void)hipGetLastError();
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  int rc;
  // the caller's frames are uploaded once and re-strided on the device to the padded width the DP kernel reads
  const size_t feat_bytes = (size_t)n_frames * dim * sizeof(float);
  if ((rc = ensure(ctx->dtw_raw, feat_bytes)) != AFX_OK) return rc;
  if ((rc = ensure(ctx->dtw_feats, (size_t)n_frames * dtw_dimp(dim) * sizeof(float))) != AFX_OK) return rc;
  if ((rc = ensure(ctx->dtw_norms, (size_t)n_frames * sizeof(float))) != AFX_OK) return rc;
  HIP_TRY(hipMemcpyAsync(ctx->dtw_raw.p, feats, feat_bytes, hipMemcpyHostToDevice, s));
  HIP_TRY(launch_dtw_pack(s, (const float*)ctx->dtw_raw.p, dim, n_frames, (float*)ctx->dtw_feats.p, (float*)ctx->dtw_norms.p));
  const float* d_norms = (const float*)ctx->dtw_norms.p;

  const int64_t budget = dev_env().dtw_budget;
  std::vector<DtwPair> recs;
  std::vector<int32_t> h_path, h_len;
  for (int c0 = 0; c0 < n_pairs;) {
    // one chunk: as many pairs as the workspace budget holds (at least one)
    recs.clear();
    int64_t codes = 0, dcells = 0, paths = 0, rows = 0, bytes = 0;
    int c1 = c0;
    while (c1 < n_pairs) {
      const int n = (int)x_len[c1], m = (int)y_len[c1];
      const int64_t pc = !bt ? 0 : T ? dtw_steps_code_words(n, m) : dtw_code_words(n, m), pr = T ? 2 * (int64_t)m : m, pd = sd ? (int64_t)n * m : 0, pp = bt ? (int64_t)n + m - 1 : 0;
      const int64_t pb = pc * 4 + pd * 8 + pp * 8 + pr * 8 + (int64_t)sizeof(DtwPair) + 16;
      if (c1 > c0 && bytes + pb > budget) break;
      DtwPair r{};
      r.x_frame = x_off[c1]; r.y_frame = y_off[c1];
      r.codes = bt ? codes : -1; r.d = sd ? dcells : -1; r.path = paths; r.row = rows;
      r.n = n; r.m = m; r.qn = T ? dtw_steps_qn(m) : dtw_qn(m);
      const int64_t rad = band_r ? band_r[c1] : -1;
      if (rad < 0) {
        r.lo = -(1 << 30); r.hi = 1 << 30;
      } else {
        const int64_t rr = std::min<int64_t>(rad, (int64_t)n + m), off = std::abs(n - m);
        r.lo = (int32_t)(-rr - (n >= m ? off : 0));
        r.hi = (int32_t)(rr + (n < m ? off : 0));
      }
      recs.push_back(r);
      codes += pc; dcells += pd; paths += pp; rows += pr; bytes += pb;
      ++c1;
    }
    const int n = c1 - c0;
    if ((rc = ensure(ctx->dtw_pairs, n * sizeof(DtwPair))) != AFX_OK) return rc;
    if ((rc = ensure(ctx->dtw_rows, (size_t)rows * sizeof(double))) != AFX_OK) return rc;
    if ((rc = ensure(ctx->dtw_cost, n * sizeof(double))) != AFX_OK) return rc;
    if ((rc = ensure(ctx->dtw_status, n * sizeof(int32_t))) != AFX_OK) return rc;
    if (T && (rc = ensure(ctx->dtw_end, n * sizeof(int32_t))) != AFX_OK) return rc;
    if (bt) {
      if ((rc = ensure(ctx->dtw_codes, (size_t)codes * sizeof(uint32_t))) != AFX_OK) return rc;
      if ((rc = ensure(ctx->dtw_path, (size_t)paths * 2 * sizeof(int32_t))) != AFX_OK) return rc;
      if ((rc = ensure(ctx->dtw_len, n * sizeof(int32_t))) != AFX_OK) return rc;
    }
    if (sd) {
      if ((rc = ensure(ctx->dtw_d, (size_t)dcells * sizeof(double))) != AFX_OK) return rc;
      HIP_TRY(launch_dtw_fill_inf(s, (double*)ctx->dtw_d.p, dcells));
    }
    HIP_TRY(hipMemcpyAsync(ctx->dtw_pairs.p, recs.data(), n * sizeof(DtwPair), hipMemcpyHostToDevice, s));
    const DtwPair* d_pairs = (const DtwPair*)ctx->dtw_pairs.p;
    if (T) {
      HIP_TRY(launch_dtw_steps(s, (const float*)ctx->dtw_feats.p, d_norms, dim, metric, d_pairs, n, *T,
                               (uint32_t*)ctx->dtw_codes.p, (double*)ctx->dtw_rows.p, (double*)ctx->dtw_d.p,
                               (double*)ctx->dtw_cost.p, (int32_t*)ctx->dtw_status.p, (int32_t*)ctx->dtw_end.p, bt, sd));
      if (bt)
        HIP_TRY(launch_dtw_steps_backtrack(s, d_pairs, n, *T, (const uint32_t*)ctx->dtw_codes.p,
                                           (const int32_t*)ctx->dtw_status.p, (const int32_t*)ctx->dtw_end.p,
                                           (int32_t*)ctx->dtw_path.p, (int32_t*)ctx->dtw_len.p));
      if (out_end) HIP_TRY(hipMemcpyAsync(out_end + c0, ctx->dtw_end.p, n * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    } else {
      HIP_TRY(launch_dtw(s, (const float*)ctx->dtw_feats.p, d_norms, dim, metric, d_pairs, n, (uint32_t*)ctx->dtw_codes.p,
                         (double*)ctx->dtw_rows.p, (double*)ctx->dtw_d.p, (double*)ctx->dtw_cost.p,
                         (int32_t*)ctx->dtw_status.p, bt, sd));
      if (bt)
        HIP_TRY(launch_dtw_backtrack(s, d_pairs, n, (const uint32_t*)ctx->dtw_codes.p, (const int32_t*)ctx->dtw_status.p,
                                     (int32_t*)ctx->dtw_path.p, (int32_t*)ctx->dtw_len.p));
    }
    HIP_TRY(hipMemcpyAsync(out_cost + c0, ctx->dtw_cost.p, n * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(out_status + c0, ctx->dtw_status.p, n * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    if (bt) {
      h_path.resize((size_t)paths * 2);
      h_len.resize(n);
      HIP_TRY(hipMemcpyAsync(h_path.data(), ctx->dtw_path.p, (size_t)paths * 2 * sizeof(int32_t), hipMemcpyDeviceToHost, s));
      HIP_TRY(hipMemcpyAsync(h_len.data(), ctx->dtw_len.p, n * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    }
    if (sd)
      for (int q = 0; q < n; ++q)
        HIP_TRY(hipMemcpyAsync(out_D + d_off[c0 + q], (const double*)ctx->dtw_d.p + recs[q].d,
                               (size_t)recs[q].n * recs[q].m * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (bt)
      for (int q = 0; q < n; ++q) {
        out_path_len[c0 + q] = h_len[q];
        std::memcpy(out_path + 2 * path_off[c0 + q], h_path.data() + 2 * recs[q].path, (size_t)h_len[q] * 2 * sizeof(int32_t));
      }
    c0 = c1;
  }
  return AFX_OK;
}

extern "C" int afx_dtw_batch(afx_ctx* ctx, const float* feats, int dim,
                             const int64_t* x_off, const int64_t* x_len, const int64_t* y_off, const int64_t* y_len,
                             const int32_t* band_r, int n_pairs, int metric, int flags,
                             double* out_cost, int32_t* out_status,
                             int32_t* out_path, const int64_t* path_off, int32_t* out_path_len,
                             double* out_D, const int64_t* d_off) {
  return dtw_run("afx_dtw_batch", ctx, feats, dim, x_off, x_len, y_off, y_len, band_r, n_pairs, metric, flags, nullptr,
                 out_cost, out_status, out_path, path_off, out_path_len, out_D, d_off, nullptr);
}

// the step list of afx_dtw_steps_batch as the kernel takes it; false (and the error set) when the caller's is refused
static bool dtw_step_list(const int32_t* steps, int n_steps, const double* w_add, const double* w_mul, bool subseq,
                          DtwSteps& T, int& rc) {
  const std::string who = "afx_dtw_steps_batch: ";
  auto fail = [&](int code, const std::string& what) { set_error(who + what); rc = code; return false; };
  T = DtwSteps{};
  T.subseq = subseq ? 1 : 0;
  if (!steps) {                                      // the default steps (1,1), (0,1), (1,0), weights optional
    static const int32_t def_sel[3] = {4, 1, 3};
    T.n = 3;
    for (int k = 0; k < 3; ++k) { T.sel[k] = def_sel[k]; T.idx[k] = k; }
  } else {
    if (n_steps < 1) return fail(AFX_ERR_INVALID, "n_steps must be >= 1");
    if (n_steps > kDtwMaxSteps) return fail(AFX_ERR_UNSUPPORTED, "more than 5 custom steps are not supported");
    for (int k = 0; k < n_steps; ++k) {
      const int32_t di = steps[2 * k], dj = steps[2 * k + 1];
      if (di < 0 || dj < 0) return fail(AFX_ERR_INVALID, "step " + std::to_string(k) + " has a negative component");
      if (di == 0 && dj == 0) return fail(AFX_ERR_INVALID, "step " + std::to_string(k) + " is (0, 0)");
      if (di > 2 || dj > 2) return fail(AFX_ERR_UNSUPPORTED, "step " + std::to_string(k) + ": components above 2 are not supported");
      T.sel[k] = di * 3 + dj;
      T.idx[k] = 3 + k;                              // behind librosa's three defaults, whose inf weights never win
    }
    T.n = n_steps;
  }
  for (int k = 0; k < T.n; ++k) {
    T.w_add[k] = w_add ? w_add[k] : 0.0;
    T.w_mul[k] = w_mul ? w_mul[k] : 1.0;
    if (!(T.w_add[k] >= 0.0) || !(T.w_mul[k] >= 0.0) || std::isinf(T.w_add[k]) || std::isinf(T.w_mul[k]))
      return fail(AFX_ERR_INVALID, "weight " + std::to_string(k) + " is negative or not finite");
  }
  return true;
}

extern "C" int afx_dtw_steps_batch(afx_ctx* ctx, const float* feats, int dim,
                                   const int64_t* x_off, const int64_t* x_len, const int64_t* y_off, const int64_t* y_len,
                                   const int32_t* band_r, int n_pairs, int metric, int flags,
                                   const int32_t* steps, int n_steps, const double* w_add, const double* w_mul,
                                   double* out_cost, int32_t* out_status,
                                   int32_t* out_path, const int64_t* path_off, int32_t* out_path_len,
                                   double* out_D, const int64_t* d_off, int32_t* out_end) {
  DtwSteps T;
  int rc = AFX_OK;
  if (!dtw_step_list(steps, n_steps, w_add, w_mul, (flags & AFX_DTW_SUBSEQ) != 0, T, rc)) return rc;
  if (T.n == 1 && T.sel[0] == 4 && x_len && y_len)   // (1,1) alone cannot shorten a sequence (librosa raises)
    for (int p = 0; p < n_pairs; ++p)
      if (x_len[p] > y_len[p]) {
        set_error("afx_dtw_steps_batch: pair " + std::to_string(p) + ": the step list [(1,1)] needs N <= M");
        return AFX_ERR_INVALID;
      }
  return dtw_run("afx_dtw_steps_batch", ctx, feats, dim, x_off, x_len, y_off, y_len, band_r, n_pairs, metric, flags, &T,
                 out_cost, out_status, out_path, path_off, out_path_len, out_D, d_off, out_end);
}

// ---- batched polyphase resampling (wavio.resample: the resampling half of librosa.load(path, sr=...)) -------------------
extern "C" int afx_resample_batch(afx_ctx* ctx, const void* samples, int sample_fmt, int mem_kind,
                                  const int64_t* offsets, const int64_t* lengths, int n_clips, int sr_in, int sr_out,
                                  const double* taps, int n_taps, float* out, int out_mem_kind,
                                  const int64_t* out_offsets, int64_t* out_lengths) {
  if (!ctx || n_clips < 0 || (n_clips > 0 && (!offsets || !lengths || !out_offsets))) {
    set_error("afx_resample_batch: null/invalid argument");
    return AFX_ERR_INVALID;
  }
  int rc;
  if ((rc = check_sample_format("afx_resample_batch", sample_fmt, mem_kind)) != AFX_OK) return rc;
  if ((rc = check_sample_format("afx_resample_batch", sample_fmt, out_mem_kind)) != AFX_OK) return rc;
  if (sr_in <= 0 || sr_out <= 0) { set_error("afx_resample_batch: sample rates must be positive"); return AFX_ERR_INVALID; }
  if (taps && (n_taps < 1 || !(n_taps & 1))) { set_error("afx_resample_batch: a caller-supplied filter needs an odd number of taps"); return AFX_ERR_INVALID; }
  if ((rc = check_clip_ranges("afx_resample_batch", offsets, lengths, out_offsets, n_clips, INT64_MAX / 8)) != AFX_OK) return rc;
  int64_t total_in = 0, total_out = 0;
  for (int i = 0; i < n_clips; ++i) total_in += lengths[i];
  const int g = std::gcd(sr_in, sr_out);
  const int up = sr_out / g, down = sr_in / g;
  const bool copy = up == down;
  if (!copy) {
    auto& rs = ctx->rs;
    const bool same = rs.valid && rs.up == up && rs.down == down && rs.custom == (taps != nullptr) &&
                      (!taps || ((int)rs.taps.size() == n_taps && std::memcmp(rs.taps.data(), taps, sizeof(double) * n_taps) == 0));
    if (!same) {
      std::string why;
      RsDesign d;
      if (!taps) {
        if ((rc = resample_design(sr_in, sr_out, d, true, why)) != AFX_OK) { set_error("afx_resample_batch: " + why); return rc; }
      }
      rs.valid = false;
      if ((rc = resample_tables(up, down, taps ? taps : d.h.data(), taps ? n_taps : d.n_taps, rs.t, why)) != AFX_OK) {
        set_error("afx_resample_batch: " + why);
        return rc;
      }
      rs.up = up; rs.down = down; rs.custom = taps != nullptr;
      rs.taps.assign(taps ? taps : nullptr, taps ? taps + n_taps : nullptr);
    }
  }
  if (n_clips > 0 && !out) {
    bool any = false;
    for (int i = 0; i < n_clips; ++i) any = any || lengths[i] > 0;
    if (any) { set_error("afx_resample_batch: null out"); return AFX_ERR_INVALID; }
  }
  if (n_clips > 0 && total_in > 0 && !samples) { set_error("afx_resample_batch: null samples"); return AFX_ERR_INVALID; }
  // clip records; a host batch is staged packed (4-element alignment), so only the clips themselves cross the link
  const RsParams& P = ctx->rs.t.p;
  const int64_t per_block = copy ? kRsCopyChunk : (int64_t)P.tile_sp * P.opp;
  std::vector<RsClip> recs((size_t)n_clips);
  int64_t n_blocks = 0, in_pos = 0;
  for (int i = 0; i < n_clips; ++i) {
    RsClip& r = recs[i];
    r.in_len = lengths[i];
    r.out_len = copy ? lengths[i] : resample_out_len(lengths[i], up, down);
    if (out_lengths) out_lengths[i] = r.out_len;
    r.in_off = mem_kind == AFX_MEM_HOST ? in_pos : offsets[i];
    r.out_off = out_mem_kind == AFX_MEM_HOST ? total_out : out_offsets[i];
    r.first_block = (int32_t)n_blocks; r.pad_ = 0;
    in_pos += (lengths[i] + 3) / 4 * 4;
    total_out += r.out_len;
    n_blocks += (r.out_len + per_block - 1) / per_block;
    if (n_blocks > INT32_MAX / 2) { set_error("afx_resample_batch: batch too large for one launch"); return AFX_ERR_UNSUPPORTED; }
  }
  if (n_clips == 0 || total_out == 0) return AFX_OK;
  (void)hipGetLastError();
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  if (!copy && !ctx->rs.valid) {
    const RsTables& t = ctx->rs.t;
    if ((rc = ensure(ctx->rs_g, t.G.size() * sizeof(double))) != AFX_OK) return rc;
    if ((rc = ensure(ctx->rs_tstart, t.tstart.size() * sizeof(int32_t))) != AFX_OK) return rc;
    HIP_TRY(hipMemcpyAsync(ctx->rs_g.p, t.G.data(), t.G.size() * sizeof(double), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(ctx->rs_tstart.p, t.tstart.data(), t.tstart.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));
    ctx->rs.valid = true;
  }
  const size_t esz = sample_fmt == AFX_FMT_S16 ? 2 : 4;
  const void* d_in = samples;
  std::vector<char> h_in;
  std::vector<HostPiece> pieces;
  if (mem_kind == AFX_MEM_HOST) {
    for (int i = 0; i < n_clips; ++i)
      pieces.push_back(clip_piece(samples, offsets[i], recs[i].in_off, lengths[i], esz));
    if ((rc = stage_in(ctx, h_in, in_pos * (int64_t)esz + 16, pieces, &d_in)) != AFX_OK) return rc;    // 16 zero bytes behind the last slot
  }
  float* d_out;
  if ((rc = out_buffer(ctx, out, out_mem_kind, total_out, &d_out)) != AFX_OK) return rc;
  if ((rc = ensure(ctx->rs_clips, recs.size() * sizeof(RsClip))) != AFX_OK) return rc;
  HIP_TRY(hipMemcpyAsync(ctx->rs_clips.p, recs.data(), recs.size() * sizeof(RsClip), hipMemcpyHostToDevice, s));
  const RsClip* d_clips = (const RsClip*)ctx->rs_clips.p;
  if (copy) HIP_TRY(launch_resample_copy(s, d_in, sample_fmt, d_out, d_clips, n_clips, (int)n_blocks));
  else HIP_TRY(launch_resample(s, d_in, sample_fmt, d_out, d_clips, n_clips, (int)n_blocks, (const double*)ctx->rs_g.p,
                               (const int32_t*)ctx->rs_tstart.p, P));
  if (out_mem_kind == AFX_MEM_HOST) {
    std::vector<float> h_out;
    if ((rc = fetch_out(ctx, d_out, total_out, h_out)) != AFX_OK) return rc;
    HIP_TRY(hipStreamSynchronize(s));
    pieces.clear();
    for (int i = 0; i < n_clips; ++i) pieces.push_back({h_out.data() + recs[i].out_off, out_offsets[i] * 4, recs[i].out_len * 4});
    scatter_pieces(out, pieces);
  } else {
    HIP_TRY(hipStreamSynchronize(s));
  }
  return AFX_OK;
}

// ---- raw WAVE data -> mono float32 (wavio.to_float32 + wavio.to_mono: the decode half of librosa.load) -------------------
extern "C" int afx_decode_batch(afx_ctx* ctx, const void* raw, int mem_kind, const int64_t* byte_offsets, const int64_t* frames,
                                const int32_t* kinds, const int32_t* channels, int n_clips,
                                float* out, int out_mem_kind, const int64_t* out_offsets) {
  const std::string who = "afx_decode_batch";
  if (!ctx || n_clips < 0 || (n_clips > 0 && (!byte_offsets || !frames || !kinds || !channels || !out_offsets))) {
    set_error(who + ": null/invalid argument");
    return AFX_ERR_INVALID;
  }
  int rc;
  if ((rc = check_sample_format(who.c_str(), AFX_FMT_F32, mem_kind)) != AFX_OK) return rc;
  if ((rc = check_sample_format(who.c_str(), AFX_FMT_F32, out_mem_kind)) != AFX_OK) return rc;
  // clip records; host batches are staged packed (16-byte / 4-element alignment), so only the clips themselves cross the link
  std::vector<DcClip> recs((size_t)n_clips);
  std::vector<int> order;
  int64_t n_blocks = 0, in_pos = 0, out_pos = 0;
  for (int i = 0; i < n_clips; ++i) {
    const auto clip = [&]() { return who + ": clip " + std::to_string(i); };      // error paths only
    if (byte_offsets[i] < 0 || out_offsets[i] < 0 || frames[i] < 0 || byte_offsets[i] > INT64_MAX / 8 || out_offsets[i] > INT64_MAX / 8) {
      set_error(clip() + ": offsets and frame counts must be >= 0");
      return AFX_ERR_INVALID;
    }
    if (frames[i] > ((int64_t)1 << 31)) { set_error(clip() + ": more than 2^31 sample frames is not supported"); return AFX_ERR_UNSUPPORTED; }
    const int sb = decode_sample_bytes(kinds[i]);
    if (!sb) { set_error(clip() + ": unknown sample kind"); return AFX_ERR_INVALID; }
    if (channels[i] < 1) { set_error(clip() + ": fewer than one channel"); return AFX_ERR_INVALID; }
    if (channels[i] > kDcMaxChannels) { set_error(clip() + ": more than 7 channels is not supported"); return AFX_ERR_UNSUPPORTED; }
    if ((byte_offsets[i] & 15) || (out_offsets[i] & 3)) {
      set_error(clip() + ": byte_offsets must be multiples of 16 and out_offsets multiples of 4");
      return AFX_ERR_INVALID;
    }
    DcClip& r = recs[i];
    r.frames = frames[i]; r.kind = kinds[i]; r.channels = channels[i];
    r.in_off = mem_kind == AFX_MEM_HOST ? in_pos : byte_offsets[i];
    r.out_off = out_mem_kind == AFX_MEM_HOST ? out_pos : out_offsets[i];
    r.first_block = (int32_t)n_blocks; r.pad_ = 0;
    in_pos += (frames[i] * sb * channels[i] + 15) / 16 * 16;
    out_pos += (frames[i] + 3) / 4 * 4;
    n_blocks += (frames[i] + kDcFrames - 1) / kDcFrames;
    if (n_blocks > INT32_MAX / 2) { set_error(who + ": batch too large for one launch"); return AFX_ERR_UNSUPPORTED; }
    if (frames[i] > 0) order.push_back(i);
  }
  // every output element has one writer: the slots (4-element padding included) must not overlap
  std::sort(order.begin(), order.end(), [&](int a, int b) { return out_offsets[a] < out_offsets[b]; });
  for (size_t k = 1; k < order.size(); ++k) {
    const int a = order[k - 1], b = order[k];
    if (out_offsets[a] + (frames[a] + 3) / 4 * 4 > out_offsets[b]) {
      set_error(who + ": the output slots of clips " + std::to_string(a) + " and " + std::to_string(b) + " overlap");
      return AFX_ERR_INVALID;
    }
  }
  if (order.empty()) return AFX_OK;
  if (!raw || !out) { set_error(who + ": null raw / out"); return AFX_ERR_INVALID; }
  (void)hipGetLastError();
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const void* d_in = raw;
  std::vector<char> h_in;
  std::vector<HostPiece> pieces;
  if (mem_kind == AFX_MEM_HOST) {
    for (int i : order)
      pieces.push_back({(const char*)raw + byte_offsets[i], recs[i].in_off, frames[i] * decode_sample_bytes(kinds[i]) * channels[i]});
    if ((rc = stage_in(ctx, h_in, in_pos, pieces, &d_in)) != AFX_OK) return rc;
  }
  float* d_out;
  if ((rc = out_buffer(ctx, out, out_mem_kind, out_pos, &d_out)) != AFX_OK) return rc;
  if ((rc = ensure(ctx->dc_clips, recs.size() * sizeof(DcClip))) != AFX_OK) return rc;
  HIP_TRY(hipMemcpyAsync(ctx->dc_clips.p, recs.data(), recs.size() * sizeof(DcClip), hipMemcpyHostToDevice, s));
  HIP_TRY(launch_decode(s, d_in, d_out, (const DcClip*)ctx->dc_clips.p, n_clips, (int)n_blocks));
  if (out_mem_kind == AFX_MEM_HOST) {
    std::vector<float> h_out;
    if ((rc = fetch_out(ctx, d_out, out_pos, h_out)) != AFX_OK) return rc;
    HIP_TRY(hipStreamSynchronize(s));
    pieces.clear();
    for (int i : order) pieces.push_back({h_out.data() + recs[i].out_off, out_offsets[i] * 4, (frames[i] + 3) / 4 * 4 * 4});
    scatter_pieces(out, pieces);
  } else {
    HIP_TRY(hipStreamSynchronize(s));
  }
  return AFX_OK;
}

// ---- zero-phase IIR filtering (scipy.signal.sosfiltfilt) and the experiment extractor's preprocess_audio around it -------
extern "C" int afx_sosfiltfilt_batch(afx_ctx* ctx, const void* samples, int sample_fmt, int mem_kind,
                                     const int64_t* offsets, const int64_t* lengths, int n_clips,
                                     const double* sos, int n_sections, int padlen, int mode, float preemph,
                                     float* out, int out_mem_kind, const int64_t* out_offsets,
                                     double* out_peak, int32_t* out_status) {
  const char* who = "afx_sosfiltfilt_batch";
  if (!ctx || !sos || n_clips < 0 || (n_clips > 0 && (!offsets || !lengths || !out_offsets || !out_status))) return null_arg(who);
  int rc;
  if ((rc = check_sample_format(who, sample_fmt, mem_kind)) != AFX_OK) return rc;
  if ((rc = check_sample_format(who, sample_fmt, out_mem_kind)) != AFX_OK) return rc;
  if (mode != AFX_FILT_PLAIN && mode != AFX_FILT_EXPERIMENT) { set_error(std::string(who) + ": unknown mode"); return AFX_ERR_INVALID; }
  if (n_sections < 1 || padlen < 0) { set_error(std::string(who) + ": n_sections must be >= 1 and padlen >= 0"); return AFX_ERR_INVALID; }
  if (n_sections > kFiltMaxS || padlen > kFiltMaxPad) {
    set_error(std::string(who) + ": more than 4 sections or padlen > 4096 is not supported");
    return AFX_ERR_UNSUPPORTED;
  }
  if ((rc = check_clip_ranges(who, offsets, lengths, out_offsets, n_clips, INT64_MAX / 8)) != AFX_OK) return rc;
  FiltTab tab;
  const char* why = "";
  if (!filt_build_tab(sos, n_sections, tab, &why)) { set_error(std::string(who) + ": " + why); return AFX_ERR_INVALID; }
  bool any = false;
  for (int i = 0; i < n_clips; ++i) {
    const bool live = lengths[i] > padlen;
    out_status[i] = live ? AFX_CLIP_OK : AFX_CLIP_TOO_SHORT;
    if (out_peak) out_peak[2 * i] = out_peak[2 * i + 1] = 0.0;
    any = any || live;
  }
  if (!any) return AFX_OK;
  if (!samples || !out) { set_error(std::string(who) + ": null samples / out"); return AFX_ERR_INVALID; }

  (void)hipGetLastError();
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  if ((rc = ensure(ctx->ft_tab, sizeof(FiltTab))) != AFX_OK) return rc;
  HIP_TRY(hipMemcpyAsync(ctx->ft_tab.p, &tab, sizeof(FiltTab), hipMemcpyHostToDevice, s));
  const FiltTab* d_tab = (const FiltTab*)ctx->ft_tab.p;
  const size_t esz = sample_fmt == AFX_FMT_S16 ? 2 : 4;
  const bool h_in = mem_kind == AFX_MEM_HOST, h_out = out_mem_kind == AFX_MEM_HOST;
  const int64_t budget = dev_env().filt_budget;
  // bytes of one tile: the float64 workspace, the carries of its blocks, its maximum
  constexpr int64_t kTileBytes = (int64_t)kFiltTile * 8 + (int64_t)kFiltB * kFiltZ * 8 + 8;
  std::vector<FiltClip> recs;
  std::vector<int> idx;
  std::vector<FiltState> h_st;
  std::vector<HostPiece> pieces;
  std::vector<char> image;
  std::vector<float> stage_out;
  for (int c0 = 0; c0 < n_clips;) {
    // one chunk: as many clips as the workspace budget holds (at least one); clips too short to filter cost nothing
    recs.clear(); idx.clear();
    int64_t bytes = 0, tiles = 0, in_pos = 0, out_pos = 0;
    int c1 = c0;
    for (; c1 < n_clips; ++c1) {
      const int64_t n = lengths[c1];
      if (n <= padlen) continue;
      const int64_t nt = (n + 2 * (int64_t)padlen + kFiltTile - 1) / kFiltTile;
      const int64_t cb = nt * kTileBytes + (h_in ? n * (int64_t)esz : 0) + (h_out ? n * 4 : 0) + (int64_t)sizeof(FiltClip) + sizeof(FiltState);
      if (!recs.empty() && (bytes + cb > budget || tiles + nt > (1 << 24) || recs.size() >= 32768)) break;
      FiltClip r{};
      r.n = n;
      r.in_off = h_in ? in_pos : offsets[c1];
      r.out_off = h_out ? out_pos : out_offsets[c1];
      r.first_tile = (int32_t)tiles; r.n_tiles = (int32_t)nt;
      recs.push_back(r); idx.push_back(c1);
      bytes += cb; tiles += nt;
      in_pos += (n + 3) / 4 * 4; out_pos += (n + 3) / 4 * 4;
    }
    c0 = c1;
    if (recs.empty()) break;
    if (tiles > (1 << 24)) { set_error(std::string(who) + ": clip too large for one launch"); return AFX_ERR_UNSUPPORTED; }
    const int n = (int)recs.size();
    const void* d_in = samples;
    if (h_in) {
      pieces.clear();
      for (int q = 0; q < n; ++q)
        pieces.push_back(clip_piece(samples, offsets[idx[q]], recs[q].in_off, recs[q].n, esz));
      if ((rc = stage_in(ctx, image, in_pos * (int64_t)esz, pieces, &d_in)) != AFX_OK) return rc;
    }
    float* d_out;
    if ((rc = out_buffer(ctx, out, out_mem_kind, out_pos, &d_out)) != AFX_OK) return rc;
    if ((rc = run_filtfilt_chain(ctx, d_in, sample_fmt, mode, preemph, padlen, n_sections, recs, tiles, d_tab, d_out)) != AFX_OK) return rc;
    h_st.resize(n);
    HIP_TRY(hipMemcpyAsync(h_st.data(), ctx->ft_st.p, n * sizeof(FiltState), hipMemcpyDeviceToHost, s));
    if (h_out && (rc = fetch_out(ctx, d_out, out_pos, stage_out)) != AFX_OK) return rc;
    HIP_TRY(hipStreamSynchronize(s));
    pieces.clear();
    for (int q = 0; q < n; ++q) {
      const int i = idx[q];
      if (h_st[q].bad) { out_status[i] = AFX_CLIP_NONFINITE; continue; }     // its output range stays as the caller left it
      if (out_peak) { out_peak[2 * i] = (double)h_st[q].peak_in; out_peak[2 * i + 1] = h_st[q].peak_out; }
      if (h_out) pieces.push_back({stage_out.data() + recs[q].out_off, out_offsets[i] * 4, recs[q].n * 4});
    }
    scatter_pieces(out, pieces);
  }
  return AFX_OK;
}

// ---- the recording screen and the compare sums (audio_format_assessment.py:143-300, audio_quality_assessment.py:150-280) ----
// A chunk of either entry point: its clips' samples staged packed (8-element alignment: 16-byte loads) when they are the
// host's, the records uploaded, two launches, the results and flags downloaded.
extern "C" int afx_assess_batch(afx_ctx* ctx, const void* samples, int sample_fmt, int mem_kind,
                                const int64_t* offsets, const int64_t* lengths, const int32_t* frame_short, const int32_t* frame_long,
                                int n_clips, double threshold_db, int64_t noise_cap, double* out_rec, int32_t* out_status) {
  const char* who = "afx_assess_batch";
  int rc = clip_batch_args(who, ctx, sample_fmt, mem_kind, offsets, lengths, n_clips, -1, nullptr, out_status, frame_short && frame_long && out_rec);
  if (rc != AFX_OK) return rc;
  if (const char* why = assess_refusal(0, 1, 1, threshold_db, noise_cap)) { set_error(std::string(who) + ": " + why); return AFX_ERR_INVALID; }
  bool any = false;
  for (int i = 0; i < n_clips; ++i) {
    if (const char* why = assess_refusal(lengths[i], frame_short[i], frame_long[i], threshold_db, noise_cap)) {
      set_error(std::string(who) + ": clip " + std::to_string(i) + ": " + why);
      return AFX_ERR_INVALID;
    }
    any = any || lengths[i] > 0;
  }
  for (int i = 0; i < n_clips; ++i) {
    out_status[i] = lengths[i] == 0 ? AFX_CLIP_TOO_SHORT : AFX_CLIP_OK;
    nan_row(out_rec, AFX_ASSESS_N, i);
  }
  if (!any) return AFX_OK;
  if (!samples) { set_error(std::string(who) + ": null samples"); return AFX_ERR_INVALID; }
  (void)hipGetLastError();
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const double thr_ratio = threshold_db > -80.0 ? std::pow(10.0, threshold_db / 10.0) : -1.0;
  const size_t esz = sample_fmt == AFX_FMT_S16 ? 2 : 4;
  const bool h_in = mem_kind == AFX_MEM_HOST;
  StftCost cost;
  assess_cost(AFX_COST_ASSESS, sample_fmt, mem_kind, cost);
  StftChunk ck;
  std::vector<AsClip> recs;
  std::vector<HostPiece> pieces;
  std::vector<char> stage;
  std::vector<double> h_rec;
  std::vector<int32_t> h_bad;
  for (int c0 = 0; c0 < n_clips; c0 = ck.next) {
    cut_stft_chunk(offsets, lengths, n_clips, c0, dev_env().assess_budget, cost, ck);
    const int n = (int)ck.idx.size();
    if (n == 0) continue;
    recs.assign((size_t)n, AsClip{});
    int64_t slots = 0, spans = 0, in_pos = 0;
    for (int q = 0; q < n; ++q) {
      const int i = ck.idx[q];
      AsClip& r = recs[q];
      r.len = lengths[i];
      r.in_off = h_in ? in_pos : offsets[i];
      r.nw = std::min<int64_t>((int64_t)(0.1 * (double)r.len), noise_cap);
      r.fs = frame_short[i]; r.fl = frame_long[i];
      r.ps_off = slots; slots += as_slots(r.len, r.fs);
      r.pl_off = slots; slots += as_slots(r.len, r.fl);
      r.span_base = spans; spans += as_spans(r.len);
      in_pos += (r.len + 7) / 8 * 8;
    }
    if (spans > INT32_MAX / 2) { set_error(std::string(who) + ": chunk too large for one launch"); return AFX_ERR_UNSUPPORTED; }
    if ((rc = ensure(ctx->as_clips, (size_t)n * sizeof(AsClip))) != AFX_OK) return rc;
    if ((rc = ensure(ctx->as_pieces, (size_t)slots * sizeof(double))) != AFX_OK) return rc;
    if ((rc = ensure(ctx->as_spans, (size_t)spans * sizeof(AsSpan))) != AFX_OK) return rc;
    if ((rc = ensure(ctx->as_rec, (size_t)n * AFX_ASSESS_N * sizeof(double))) != AFX_OK) return rc;
    if ((rc = ensure(ctx->as_bad, (size_t)n * sizeof(int32_t))) != AFX_OK) return rc;
    const void* d_in = samples;
    if (h_in) {
      pieces.clear();
      for (int q = 0; q < n; ++q)
        pieces.push_back(clip_piece(samples, offsets[ck.idx[q]], recs[q].in_off, recs[q].len, esz));
      if ((rc = stage_in(ctx, stage, in_pos * (int64_t)esz, pieces, &d_in)) != AFX_OK) return rc;
    }
    HIP_TRY(hipMemcpyAsync(ctx->as_clips.p, recs.data(), (size_t)n * sizeof(AsClip), hipMemcpyHostToDevice, s));
    HIP_TRY(launch_assess(s, d_in, sample_fmt, (const AsClip*)ctx->as_clips.p, n, (int)spans, thr_ratio, (double*)ctx->as_pieces.p,
                          (AsSpan*)ctx->as_spans.p, (double*)ctx->as_rec.p, (int32_t*)ctx->as_bad.p));
    h_rec.resize((size_t)n * AFX_ASSESS_N); h_bad.resize((size_t)n);
    HIP_TRY(hipMemcpyAsync(h_rec.data(), ctx->as_rec.p, h_rec.size() * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(h_bad.data(), ctx->as_bad.p, h_bad.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (int q = 0; q < n; ++q) {
      const int i = ck.idx[q];
      if (h_bad[q]) { out_status[i] = AFX_CLIP_NONFINITE; continue; }
      std::memcpy(out_rec + (size_t)AFX_ASSESS_N * i, h_rec.data() + (size_t)AFX_ASSESS_N * q, AFX_ASSESS_N * sizeof(double));
    }
  }
  return AFX_OK;
}

extern "C" int afx_compare_batch(afx_ctx* ctx, const void* ref, const void* deg, int sample_fmt, int mem_kind,
                                 const int64_t* ref_offsets, const int64_t* ref_lengths, const int64_t* deg_offsets,
                                 const int64_t* deg_lengths, int n_pairs, double* out_rec, int32_t* out_status) {
  const char* who = "afx_compare_batch";
  int rc = clip_batch_args(who, ctx, sample_fmt, mem_kind, ref_offsets, ref_lengths, n_pairs, -1, nullptr, out_status, deg_offsets && deg_lengths && out_rec);
  if (rc != AFX_OK) return rc;
  if ((rc = check_clip_ranges(who, deg_offsets, deg_lengths, nullptr, n_pairs, INT64_MAX / 8)) != AFX_OK) return rc;
  std::vector<int64_t> lens((size_t)n_pairs);
  bool any = false;
  for (int i = 0; i < n_pairs; ++i) {
    lens[i] = std::min(ref_lengths[i], deg_lengths[i]);
    out_status[i] = lens[i] == 0 ? AFX_CLIP_TOO_SHORT : AFX_CLIP_OK;
    nan_row(out_rec, AFX_COMPARE_N, i);
    any = any || lens[i] > 0;
  }
  if (!any) return AFX_OK;
  if (!ref || !deg) { set_error(std::string(who) + ": null samples"); return AFX_ERR_INVALID; }
  (void)hipGetLastError();
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const size_t esz = sample_fmt == AFX_FMT_S16 ? 2 : 4;
  const bool h_in = mem_kind == AFX_MEM_HOST;
  StftCost cost;
  assess_cost(AFX_COST_COMPARE, sample_fmt, mem_kind, cost);
  StftChunk ck;
  std::vector<CmpPair> recs;
  std::vector<HostPiece> pieces;
  std::vector<char> stage;
  std::vector<double> h_rec;
  std::vector<int32_t> h_bad;
  for (int c0 = 0; c0 < n_pairs; c0 = ck.next) {
    cut_stft_chunk(ref_offsets, lens.data(), n_pairs, c0, dev_env().assess_budget, cost, ck);
    const int n = (int)ck.idx.size();
    if (n == 0) continue;
    recs.assign((size_t)n, CmpPair{});
    int64_t spans = 0, in_pos = 0;
    for (int q = 0; q < n; ++q) {
      const int i = ck.idx[q];
      CmpPair& r = recs[q];
      r.n = lens[i];
      const int64_t slot = (r.n + 7) / 8 * 8;
      r.r_off = h_in ? in_pos : ref_offsets[i];
      r.d_off = h_in ? in_pos + slot : deg_offsets[i];
      r.span_base = spans; spans += as_spans(r.n);
      in_pos += 2 * slot;
    }
    if (spans > INT32_MAX / 2) { set_error(std::string(who) + ": chunk too large for one launch"); return AFX_ERR_UNSUPPORTED; }
    if ((rc = ensure(ctx->as_clips, (size_t)n * sizeof(CmpPair))) != AFX_OK) return rc;
    if ((rc = ensure(ctx->as_pieces, (size_t)spans * kCmpSpanDoubles * sizeof(double))) != AFX_OK) return rc;
    if ((rc = ensure(ctx->as_rec, (size_t)n * AFX_COMPARE_N * sizeof(double))) != AFX_OK) return rc;
    if ((rc = ensure(ctx->as_bad, (size_t)n * sizeof(int32_t))) != AFX_OK) return rc;
    const void *d_ref = ref, *d_deg = deg;
    if (h_in) {
      pieces.clear();
      for (int q = 0; q < n; ++q) {
        const int i = ck.idx[q];
        pieces.push_back(clip_piece(ref, ref_offsets[i], recs[q].r_off, recs[q].n, esz));
        pieces.push_back(clip_piece(deg, deg_offsets[i], recs[q].d_off, recs[q].n, esz));
      }
      if ((rc = stage_in(ctx, stage, in_pos * (int64_t)esz, pieces, &d_ref)) != AFX_OK) return rc;
      d_deg = d_ref;
    }
    HIP_TRY(hipMemcpyAsync(ctx->as_clips.p, recs.data(), (size_t)n * sizeof(CmpPair), hipMemcpyHostToDevice, s));
    HIP_TRY(launch_compare(s, d_ref, d_deg, sample_fmt, (const CmpPair*)ctx->as_clips.p, n, (int)spans, (double*)ctx->as_pieces.p,
                           (double*)ctx->as_rec.p, (int32_t*)ctx->as_bad.p));
    h_rec.resize((size_t)n * AFX_COMPARE_N); h_bad.resize((size_t)n);
    HIP_TRY(hipMemcpyAsync(h_rec.data(), ctx->as_rec.p, h_rec.size() * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(h_bad.data(), ctx->as_bad.p, h_bad.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (int q = 0; q < n; ++q) {
      const int i = ck.idx[q];
      if (h_bad[q]) { out_status[i] = AFX_CLIP_NONFINITE; continue; }
      std::memcpy(out_rec + (size_t)AFX_COMPARE_N * i, h_rec.data() + (size_t)AFX_COMPARE_N * q, AFX_COMPARE_N * sizeof(double));
    }
  }
  return AFX_OK;
}

// ---- the whole-clip DFT and the spectral term of the PESQ-like score (audio_quality_assessment.py:150-201) ----
// The body of afx_specdist_batch (deg given: z = r + i d, out_rec) and afx_clip_fft_batch (deg == nullptr: out_bins at
// out_offsets).  A chunk: its samples staged packed when they are the host's, one filter job per distinct length and one
// signal job per pair -- those of M <= 4096 first --, the filter launches, the signal launches, the tail or the copies.
static int cfft_run(const char* who, afx_ctx* ctx, const void* ref, const void* deg, int sample_fmt, int mem_kind,
                    const int64_t* ref_offsets, const int64_t* deg_offsets, const int64_t* lens, int n_pairs,
                    double* out_rec, double* out_bins, const int64_t* out_offsets, int32_t* out_status) {
  (void)hipGetLastError();
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  int rc;
  if (!ctx->cf_tw_ready) {
    std::vector<double> tw((size_t)kCfTile);
    cf_twiddle_table(tw.data());
    if ((rc = ensure(ctx->cf_tw, tw.size() * sizeof(double))) != AFX_OK) return rc;
    HIP_TRY(hipMemcpyAsync(ctx->cf_tw.p, tw.data(), tw.size() * sizeof(double), hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));                                  // tw dies with this scope
    ctx->cf_tw_ready = true;
  }
  const size_t esz = sample_fmt == AFX_FMT_S16 ? 2 : 4;
  const bool h_in = mem_kind == AFX_MEM_HOST, pair = deg != nullptr;
  StftCost cost;
  specdist_cost(sample_fmt, mem_kind, cost);
  StftChunk ck;
  std::vector<CfJob> jobs, filt_jobs;
  std::vector<int> order, slot_of;
  std::vector<int64_t> distinct, in_r, in_d;
  std::vector<HostPiece> pieces;
  std::vector<char> stage;
  std::vector<double> h_rec;
  std::vector<int32_t> h_bad;
  const double nan = std::nan("");
  for (int c0 = 0; c0 < n_pairs; c0 = ck.next) {
    cut_stft_chunk(ref_offsets, lens, n_pairs, c0, dev_env().specdist_budget, cost, ck);
    const int n = (int)ck.idx.size();
    if (n == 0) continue;
    // the staging's layout, in the chunk's order
    in_r.assign((size_t)n, 0); in_d.assign((size_t)n, -1);
    int64_t in_pos = 0;
    for (int q = 0; q < n; ++q) {
      const int i = ck.idx[q];
      const int64_t slot = (lens[i] + 7) / 8 * 8;
      in_r[q] = h_in ? in_pos : ref_offsets[i];
      if (pair) in_d[q] = h_in ? in_pos + slot : deg_offsets[i];
      in_pos += (pair ? 2 : 1) * slot;
    }
    // the distinct lengths, ascending: their filters, then the jobs -- either list with its M <= kCfTile first
    distinct.clear();
    for (int q = 0; q < n; ++q) distinct.push_back(lens[ck.idx[q]]);
    std::sort(distinct.begin(), distinct.end());
    distinct.erase(std::unique(distinct.begin(), distinct.end()), distinct.end());
    filt_jobs.assign(distinct.size(), CfJob{});
    int64_t filt_pts = 0, f_blocks = 0;
    int f_small = 0;
    for (size_t k = 0; k < distinct.size(); ++k) {                     // ascending n: ascending M, the small ones first
      CfJob& f = filt_jobs[k];
      f.n = distinct[k]; f.r_off = 0; f.d_off = -1;
      f.logM = cf_log_m(f.n); f.logM1 = cf_log_m1(f.logM);
      f.work_off = f.filt_off = filt_pts; filt_pts += (int64_t)1 << f.logM;
      if (f.logM <= kCfTileLog) { ++f_small; f.blk_base = 0; }
      else { f.blk_base = f_blocks; f_blocks += cf_tiles(f.logM); }
    }
    order.resize((size_t)n);
    std::iota(order.begin(), order.end(), 0);
    std::stable_partition(order.begin(), order.end(), [&](int q) { return cf_log_m(lens[ck.idx[q]]) <= kCfTileLog; });
    jobs.assign((size_t)n, CfJob{});
    int64_t work_pts = 0, j_blocks = 0;
    int j_small = 0;
    for (int p = 0; p < n; ++p) {
      const int q = order[p];
      CfJob& j = jobs[p];
      j.n = lens[ck.idx[q]]; j.r_off = in_r[q]; j.d_off = in_d[q];
      j.logM = cf_log_m(j.n); j.logM1 = cf_log_m1(j.logM);
      j.work_off = work_pts; work_pts += (int64_t)1 << j.logM;
      j.filt_off = filt_jobs[(size_t)(std::lower_bound(distinct.begin(), distinct.end(), j.n) - distinct.begin())].filt_off;
      if (j.logM <= kCfTileLog) { ++j_small; j.blk_base = 0; }
      else { j.blk_base = j_blocks; j_blocks += cf_tiles(j.logM); }
    }
    if (j_blocks > INT32_MAX / 2 || f_blocks > INT32_MAX / 2) { set_error(std::string(who) + ": chunk too large for one launch"); return AFX_ERR_UNSUPPORTED; }
    const size_t nf = filt_jobs.size();
    if ((rc = ensure(ctx->cf_jobs, (nf + (size_t)n) * sizeof(CfJob))) != AFX_OK) return rc;
    if ((rc = ensure(ctx->cf_filt, (size_t)filt_pts * 16)) != AFX_OK) return rc;
    if ((rc = ensure(ctx->cf_work, (size_t)work_pts * 16)) != AFX_OK) return rc;
    if ((rc = ensure(ctx->cf_rec, (size_t)n * AFX_SPECDIST_N * sizeof(double))) != AFX_OK) return rc;
    if ((rc = ensure(ctx->cf_bad, (size_t)n * 2 * sizeof(int32_t))) != AFX_OK) return rc;
    const void *d_ref = ref, *d_deg = deg;
    if (h_in) {
      pieces.clear();
      for (int q = 0; q < n; ++q) {
        const int i = ck.idx[q];
        pieces.push_back(clip_piece(ref, ref_offsets[i], in_r[q], lens[i], esz));
        if (pair) pieces.push_back(clip_piece(deg, deg_offsets[i], in_d[q], lens[i], esz));
      }
      if ((rc = stage_in(ctx, stage, std::max<int64_t>(in_pos, 1) * (int64_t)esz, pieces, &d_ref)) != AFX_OK) return rc;
      d_deg = pair ? d_ref : nullptr;
    }
    CfJob* d_fjobs = (CfJob*)ctx->cf_jobs.p;
    CfJob* d_jobs = d_fjobs + nf;
    HIP_TRY(hipMemcpyAsync(d_fjobs, filt_jobs.data(), nf * sizeof(CfJob), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_jobs, jobs.data(), (size_t)n * sizeof(CfJob), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(ctx->cf_bad.p, 0, (size_t)n * 2 * sizeof(int32_t), s));
    const double* tw = (const double*)ctx->cf_tw.p;
    HIP_TRY(launch_cfft_filters(s, d_fjobs, f_small, (int)nf - f_small, (int)f_blocks, tw, (double*)ctx->cf_filt.p));
    HIP_TRY(launch_cfft(s, d_ref, d_deg, sample_fmt, d_jobs, j_small, n - j_small, (int)j_blocks, tw, (const double*)ctx->cf_filt.p,
                        (double*)ctx->cf_work.p, (int32_t*)ctx->cf_bad.p));
    h_bad.resize((size_t)n * 2);
    if (pair) {
      HIP_TRY(launch_specdist_tail(s, d_jobs, n, (const double*)ctx->cf_work.p, (const int32_t*)ctx->cf_bad.p, (double*)ctx->cf_rec.p));
      h_rec.resize((size_t)n * AFX_SPECDIST_N);
      HIP_TRY(hipMemcpyAsync(h_rec.data(), ctx->cf_rec.p, h_rec.size() * sizeof(double), hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(hipMemcpyAsync(h_bad.data(), ctx->cf_bad.p, h_bad.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (int p = 0; p < n; ++p) {
      const int i = ck.idx[order[p]];
      const bool isbad = h_bad[2 * p] != 0;
      if (isbad) out_status[i] = AFX_CLIP_NONFINITE;
      if (pair) {
        if (!isbad) std::memcpy(out_rec + (size_t)AFX_SPECDIST_N * i, h_rec.data() + (size_t)AFX_SPECDIST_N * p, AFX_SPECDIST_N * sizeof(double));
        continue;
      }
      double* dst = out_bins + 2 * out_offsets[i];
      const size_t bins = (size_t)(lens[i] / 2 + 1);
      if (isbad) { std::fill(dst, dst + 2 * bins, nan); continue; }
      HIP_TRY(hipMemcpyAsync(dst, (const char*)ctx->cf_work.p + (size_t)jobs[p].work_off * 16, bins * 16, hipMemcpyDeviceToHost, s));
    }
    if (!pair) HIP_TRY(hipStreamSynchronize(s));
  }
  return AFX_OK;
}

extern "C" int afx_specdist_batch(afx_ctx* ctx, const void* ref, const void* deg, int sample_fmt, int mem_kind,
                                  const int64_t* ref_offsets, const int64_t* ref_lengths, const int64_t* deg_offsets,
                                  const int64_t* deg_lengths, int n_pairs, double* out_rec, int32_t* out_status) {
  const char* who = "afx_specdist_batch";
  int rc = clip_batch_args(who, ctx, sample_fmt, mem_kind, ref_offsets, ref_lengths, n_pairs, -1, nullptr, out_status, deg_offsets && deg_lengths && out_rec);
  if (rc != AFX_OK) return rc;
  if ((rc = check_clip_ranges(who, deg_offsets, deg_lengths, nullptr, n_pairs, INT64_MAX / 8)) != AFX_OK) return rc;
  std::vector<int64_t> lens((size_t)n_pairs);
  bool any = false;
  for (int i = 0; i < n_pairs; ++i) {
    lens[i] = std::min(ref_lengths[i], deg_lengths[i]);
    if (lens[i] > kCfMaxN) {
      set_error(std::string(who) + ": pair " + std::to_string(i) + ": more than 2^21 samples are not supported");
      return AFX_ERR_UNSUPPORTED;
    }
    any = any || lens[i] > 0;
  }
  for (int i = 0; i < n_pairs; ++i) {
    out_status[i] = lens[i] == 0 ? AFX_CLIP_TOO_SHORT : AFX_CLIP_OK;
    nan_row(out_rec, AFX_SPECDIST_N, i);
  }
  if (!any) return AFX_OK;
  if (!ref || !deg) { set_error(std::string(who) + ": null samples"); return AFX_ERR_INVALID; }
  return cfft_run(who, ctx, ref, deg, sample_fmt, mem_kind, ref_offsets, deg_offsets, lens.data(), n_pairs, out_rec, nullptr, nullptr,
                  out_status);
}

extern "C" int afx_clip_fft_batch(afx_ctx* ctx, const void* samples, int sample_fmt, int mem_kind, const int64_t* offsets,
                                  const int64_t* lengths, int n_clips, double* out, const int64_t* out_offsets,
                                  int32_t* out_status) {
  const char* who = "afx_clip_fft_batch";
  if (!ctx || n_clips < 0 || (n_clips > 0 && (!offsets || !lengths || !out_offsets || !out_status))) return null_arg(who);
  int rc;
  if ((rc = check_sample_format(who, sample_fmt, mem_kind)) != AFX_OK) return rc;
  if ((rc = check_clip_ranges(who, offsets, lengths, out_offsets, n_clips, INT64_MAX / 32)) != AFX_OK) return rc;
  bool any = false;
  for (int i = 0; i < n_clips; ++i) {
    if (lengths[i] > kCfMaxN) {
      set_error(std::string(who) + ": clip " + std::to_string(i) + ": more than 2^21 samples are not supported");
      return AFX_ERR_UNSUPPORTED;
    }
    any = any || lengths[i] > 0;
  }
  for (int i = 0; i < n_clips; ++i) out_status[i] = lengths[i] == 0 ? AFX_CLIP_TOO_SHORT : AFX_CLIP_OK;
  if (!any) return AFX_OK;
  if (!samples || !out) { set_error(std::string(who) + ": null samples or output"); return AFX_ERR_INVALID; }
  return cfft_run(who, ctx, samples, nullptr, sample_fmt, mem_kind, offsets, nullptr, lengths, n_clips, nullptr, out, out_offsets,
                  out_status);
}

// ---- scipy.signal.medfilt / savgol_filter on samples, and the experiment extractor's energy and ZCR groups ----------------
// What a clip of n samples costs a chunk of the three entry points below, in device bytes (the chunk rule of
// afx_sosfiltfilt_batch: as many clips as the budget holds, at least one).
struct SmoothCost {
  int64_t per_sample = 0;        // staging of host samples and of a host result, the workspace signals
  int64_t per_frame = 0;         // the frame rows of the groups
  int64_t per_filt_tile = 0;     // the preprocess's workspace
  int64_t per_clip = 0;          // records, flags, results
  int64_t of(int64_t n, int64_t frames, int64_t filt_tiles) const {
    return per_sample * ((n + 3) / 4 * 4) + per_frame * frames + per_filt_tile * filt_tiles + per_clip;
  }
};
constexpr int kSmoothMaxClips = 1 << 20;       // records of a chunk
constexpr int64_t kSmoothMaxTiles = 1 << 24;   // workgroups of a launch

// The body of afx_medfilt_batch (tab == nullptr: the median of K) and afx_savgol_batch (tab: its tables): clips of min_n
// samples or more, chunk by chunk -- the samples staged packed when they are the host's, the records uploaded, the
// non-finite check and the filter launched, the result copied back when it is the host's.
static int smooth_run(const char* who, afx_ctx* ctx, const void* samples, int sample_fmt, int mem_kind, const int64_t* offsets,
                      const int64_t* lengths, int n_clips, int K, const SgTab* tab, int64_t min_n, float* out, int out_mem_kind,
                      const int64_t* out_offsets, int32_t* out_status) {
  int rc;
  bool any = false;
  for (int i = 0; i < n_clips; ++i) {
    const bool live = lengths[i] >= min_n;
    out_status[i] = live ? AFX_CLIP_OK : AFX_CLIP_TOO_SHORT;
    any = any || live;
  }
  if (!any) return AFX_OK;
  if (!samples || !out) { set_error(std::string(who) + ": null samples / out"); return AFX_ERR_INVALID; }
  (void)hipGetLastError();
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  if (tab) {
    if ((rc = ensure(ctx->sm_tab, sizeof(SgTab))) != AFX_OK) return rc;
    HIP_TRY(hipMemcpyAsync(ctx->sm_tab.p, tab, sizeof(SgTab), hipMemcpyHostToDevice, s));
  }
  const size_t esz = sample_fmt == AFX_FMT_S16 ? 2 : 4;
  const bool h_in = mem_kind == AFX_MEM_HOST, h_out = out_mem_kind == AFX_MEM_HOST;
  SmoothCost cost;
  cost.per_sample = (h_in ? (int64_t)esz : 0) + (h_out ? 4 : 0);
  cost.per_clip = (int64_t)sizeof(SmClip) + 4;
  const int64_t budget = dev_env().smooth_budget;
  std::vector<SmClip> recs;
  std::vector<int> idx;
  std::vector<uint32_t> h_bad;
  std::vector<HostPiece> pieces;
  std::vector<char> image;
  std::vector<float> stage_out;
  for (int c0 = 0; c0 < n_clips;) {
    recs.clear(); idx.clear();
    int64_t bytes = 0, tiles = 0, in_pos = 0, out_pos = 0;
    int c1 = c0;
    for (; c1 < n_clips; ++c1) {
      const int64_t n = lengths[c1];
      if (n < min_n) continue;
      const int64_t nt = (n + kSmTile - 1) / kSmTile, cb = cost.of(n, 0, 0);
      if (!recs.empty() && (bytes + cb > budget || tiles + nt > kSmoothMaxTiles || (int)recs.size() >= kSmoothMaxClips)) break;
      SmClip r{};
      r.n = n;
      r.in_off = h_in ? in_pos : offsets[c1];
      r.out_off = h_out ? out_pos : out_offsets[c1];
      r.first_tile = (int32_t)tiles; r.n_tiles = (int32_t)nt;
      recs.push_back(r); idx.push_back(c1);
      bytes += cb; tiles += nt;
      in_pos += (n + 3) / 4 * 4; out_pos += (n + 3) / 4 * 4;
    }
    c0 = c1;
    if (recs.empty()) break;
    if (tiles > kSmoothMaxTiles) { set_error(std::string(who) + ": clip too large for one launch"); return AFX_ERR_UNSUPPORTED; }
    const int n = (int)recs.size(), nt = (int)tiles;
    if ((rc = ensure(ctx->sm_clips, n * sizeof(SmClip))) != AFX_OK) return rc;
    if ((rc = ensure(ctx->sm_bad, n * sizeof(uint32_t))) != AFX_OK) return rc;
    const void* d_in = samples;
    if (h_in) {
      pieces.clear();
      for (int q = 0; q < n; ++q)
        pieces.push_back(clip_piece(samples, offsets[idx[q]], recs[q].in_off, recs[q].n, esz));
      if ((rc = stage_in(ctx, image, in_pos * (int64_t)esz, pieces, &d_in)) != AFX_OK) return rc;
    }
    float* d_out;
    if ((rc = out_buffer(ctx, out, out_mem_kind, out_pos, &d_out)) != AFX_OK) return rc;
    HIP_TRY(hipMemcpyAsync(ctx->sm_clips.p, recs.data(), n * sizeof(SmClip), hipMemcpyHostToDevice, s));
    const SmClip* d_clips = (const SmClip*)ctx->sm_clips.p;
    uint32_t* d_bad = (uint32_t*)ctx->sm_bad.p;
    HIP_TRY(launch_sm_check(s, d_in, sample_fmt, d_clips, n, d_bad));
    if (tab) HIP_TRY(launch_savgol(s, d_in, sample_fmt, (const SgTab*)ctx->sm_tab.p, 0, d_clips, n, nt, d_bad, 1, d_out));
    else HIP_TRY(launch_medfilt(s, d_in, sample_fmt, K, d_clips, n, nt, d_bad, 1, d_out));
    h_bad.resize(n);
    HIP_TRY(hipMemcpyAsync(h_bad.data(), d_bad, n * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    if (h_out && (rc = fetch_out(ctx, d_out, out_pos, stage_out)) != AFX_OK) return rc;
    HIP_TRY(hipStreamSynchronize(s));
    pieces.clear();
    for (int q = 0; q < n; ++q) {
      const int i = idx[q];
      if (h_bad[q]) { out_status[i] = AFX_CLIP_NONFINITE; continue; }       // its output range stays as the caller left it
      if (h_out) pieces.push_back({stage_out.data() + recs[q].out_off, out_offsets[i] * 4, recs[q].n * 4});
    }
    scatter_pieces(out, pieces);
  }
  return AFX_OK;
}

extern "C" int afx_medfilt_batch(afx_ctx* ctx, const void* samples, int sample_fmt, int mem_kind,
                                 const int64_t* offsets, const int64_t* lengths, int n_clips, int kernel_size,
                                 float* out, int out_mem_kind, const int64_t* out_offsets, int32_t* out_status) {
  const char* who = "afx_medfilt_batch";
  int code;
  if (const char* why = medfilt_refusal(kernel_size, &code)) { set_error(std::string(who) + ": " + why); return code; }
  if (int rc = clip_batch_args(who, ctx, sample_fmt, mem_kind, offsets, lengths, n_clips, out_mem_kind, out_offsets, out_status)) return rc;
  return smooth_run(who, ctx, samples, sample_fmt, mem_kind, offsets, lengths, n_clips, kernel_size, nullptr, 1, out, out_mem_kind,
                    out_offsets, out_status);
}

extern "C" int afx_savgol_batch(afx_ctx* ctx, const void* samples, int sample_fmt, int mem_kind,
                                const int64_t* offsets, const int64_t* lengths, int n_clips,
                                int window_length, int polyorder, int deriv, double delta,
                                float* out, int out_mem_kind, const int64_t* out_offsets, int32_t* out_status) {
  const char* who = "afx_savgol_batch";
  int code;
  if (const char* why = savgol_refusal(window_length, polyorder, deriv, delta, &code)) { set_error(std::string(who) + ": " + why); return code; }
  if (int rc = clip_batch_args(who, ctx, sample_fmt, mem_kind, offsets, lengths, n_clips, out_mem_kind, out_offsets, out_status)) return rc;
  SgTab tab;
  savgol_build_tab(window_length, polyorder, deriv, delta, tab);
  return smooth_run(who, ctx, samples, sample_fmt, mem_kind, offsets, lengths, n_clips, 0, &tab, window_length, out, out_mem_kind,
                    out_offsets, out_status);
}

// One upload, the preprocess (run_filtfilt_chain, as afx_sosfiltfilt_batch's), the ZCR chain with the launchers
// of the two entry points above, the frame rows of both groups in one launch, the statistics; only the records come back.
extern "C" int afx_energy_zcr_batch(afx_ctx* ctx, const void* samples, int sample_fmt, int mem_kind,
                                    const int64_t* offsets, const int64_t* lengths, int n_clips,
                                    int sr, int frame_length, int hop_length, int flags, double* out_rec, int32_t* out_status) {
  const char* who = "afx_energy_zcr_batch";
  if (!ctx || n_clips < 0 || (n_clips > 0 && (!offsets || !lengths || !out_rec || !out_status))) return null_arg(who);
  int rc, code;
  if ((rc = check_sample_format(who, sample_fmt, mem_kind)) != AFX_OK) return rc;
  if (const char* why = ez_refusal(sr, frame_length, hop_length, flags, &code)) { set_error(std::string(who) + ": " + why); return code; }
  if ((rc = check_clip_ranges(who, offsets, lengths, nullptr, n_clips, INT64_MAX / 8)) != AFX_OK) return rc;
  const bool pre = flags & AFX_EZ_PREPROCESS, en = flags & AFX_EZ_ENERGY, zc = flags & AFX_EZ_ZCR;
  constexpr int kPadlen = 18;                  // scipy's default for the experiment's 5th-order filter
  const int64_t min_n = pre ? kPadlen + 1 : 1;
  bool any = false;
  for (int i = 0; i < n_clips; ++i) {
    out_status[i] = lengths[i] >= min_n ? AFX_CLIP_OK : AFX_CLIP_TOO_SHORT;
    nan_row(out_rec, AFX_EZ_N, i);
    any = any || lengths[i] >= min_n;
  }
  if (!any) return AFX_OK;
  if (!samples) { set_error(std::string(who) + ": null samples"); return AFX_ERR_INVALID; }
  (void)hipGetLastError();
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  constexpr int kSections = 3;
  if (pre) {
    double sos[kSections * 6];
    FiltTab ftab;
    const char* why = "";
    if ((rc = afx_butter_sos(5, 200.0 / ((double)sr / 2.0), 1, sos)) != AFX_OK) return rc;
    if (!filt_build_tab(sos, kSections, ftab, &why)) { set_error(std::string(who) + ": " + why); return AFX_ERR_INVALID; }
    if ((rc = ensure(ctx->ft_tab, sizeof(FiltTab))) != AFX_OK) return rc;
    HIP_TRY(hipMemcpyAsync(ctx->ft_tab.p, &ftab, sizeof(FiltTab), hipMemcpyHostToDevice, s));
  }
  if (zc) {
    SgTab tab;
    savgol_build_tab(11, 3, 0, 1.0, tab);
    if ((rc = ensure(ctx->sm_tab, sizeof(SgTab))) != AFX_OK) return rc;
    HIP_TRY(hipMemcpyAsync(ctx->sm_tab.p, &tab, sizeof(SgTab), hipMemcpyHostToDevice, s));
  }
  const size_t esz = sample_fmt == AFX_FMT_S16 ? 2 : 4;
  const bool h_in = mem_kind == AFX_MEM_HOST;
  SmoothCost cost;
  cost.per_sample = (h_in ? (int64_t)esz : 0) + (pre ? 4 : 0) + (zc ? 4 + 4 + 1 : 0);
  cost.per_frame = (en ? 8 : 0) + (zc ? 8 : 0);
  cost.per_filt_tile = pre ? (int64_t)kFiltTile * 8 + (int64_t)kFiltB * kFiltZ * 8 + 8 : 0;
  cost.per_clip = (int64_t)sizeof(FiltClip) + sizeof(FiltState) + 2 * sizeof(SmClip) + sizeof(EzClip) + 4 + 4 + AFX_EZ_N * 8;
  const int64_t budget = dev_env().smooth_budget;
  std::vector<FiltClip> frecs;
  std::vector<SmClip> srecs;
  std::vector<EzClip> erecs;
  std::vector<int> idx;
  std::vector<FiltState> h_st;
  std::vector<uint32_t> h_bad;
  std::vector<float> h_peak;
  std::vector<double> h_rec;
  std::vector<HostPiece> pieces;
  std::vector<char> image;
  for (int c0 = 0; c0 < n_clips;) {
    frecs.clear(); erecs.clear(); idx.clear();
    int64_t bytes = 0, ftiles = 0, stiles = 0, frames = 0, in_pos = 0, pos = 0;
    int c1 = c0;
    for (; c1 < n_clips; ++c1) {
      const int64_t n = lengths[c1];
      if (n < min_n) continue;
      const EzFrame fr = ez_framing(n, frame_length, hop_length);
      const int64_t nft = pre ? (n + 2 * (int64_t)kPadlen + kFiltTile - 1) / kFiltTile : 0, nst = (n + kSmTile - 1) / kSmTile;
      const int64_t cb = cost.of(n, fr.T, nft);
      if (!erecs.empty() && (bytes + cb > budget || ftiles + nft > kSmoothMaxTiles || stiles + nst > kSmoothMaxTiles ||
                             frames + fr.T > ((int64_t)1 << 30) || (int)erecs.size() >= kSmoothMaxClips)) break;
      const int64_t src_off = h_in ? in_pos : offsets[c1];
      frecs.push_back(FiltClip{src_off, pos, n, (int32_t)ftiles, (int32_t)nft});
      EzClip e{};
      e.y_off = pre ? pos : src_off; e.off = pos; e.n = n; e.T = fr.T; e.first_frame = frames; e.fl = fr.fl; e.hop = fr.hop;
      erecs.push_back(e); idx.push_back(c1);
      bytes += cb; ftiles += nft; stiles += nst; frames += fr.T;
      in_pos += (n + 3) / 4 * 4; pos += (n + 3) / 4 * 4;
    }
    c0 = c1;
    if (erecs.empty()) break;
    if (ftiles > kSmoothMaxTiles || stiles > kSmoothMaxTiles || frames > ((int64_t)1 << 30)) {
      set_error(std::string(who) + ": clip too large for one launch");
      return AFX_ERR_UNSUPPORTED;
    }
    const int n = (int)erecs.size(), nst = (int)stiles;
    // the ZCR chain's tile records: [0, n) from the groups' input into the workspace (the median), [n, 2 n) within it
    srecs.resize((size_t)2 * n);
    for (int q = 0, t = 0; q < n; ++q) {
      const int32_t k = (int32_t)((erecs[q].n + kSmTile - 1) / kSmTile);
      srecs[q] = SmClip{erecs[q].y_off, erecs[q].off, erecs[q].n, t, k};
      srecs[n + q] = SmClip{erecs[q].off, erecs[q].off, erecs[q].n, t, k};
      t += k;
    }
    const void* d_in = samples;
    if (h_in) {
      pieces.clear();
      for (int q = 0; q < n; ++q)
        pieces.push_back(clip_piece(samples, offsets[idx[q]], frecs[q].in_off, frecs[q].n, esz));
      if ((rc = stage_in(ctx, image, in_pos * (int64_t)esz, pieces, &d_in)) != AFX_OK) return rc;
    }
    if ((rc = ensure(ctx->ez_clips, n * sizeof(EzClip))) != AFX_OK) return rc;
    if ((rc = ensure(ctx->sm_clips, 2 * n * sizeof(SmClip))) != AFX_OK) return rc;
    if ((rc = ensure(ctx->ez_rec, (size_t)n * AFX_EZ_N * sizeof(double))) != AFX_OK) return rc;
    HIP_TRY(hipMemcpyAsync(ctx->ez_clips.p, erecs.data(), n * sizeof(EzClip), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(ctx->sm_clips.p, srecs.data(), 2 * n * sizeof(SmClip), hipMemcpyHostToDevice, s));
    const EzClip* d_eclips = (const EzClip*)ctx->ez_clips.p;
    const SmClip* d_sclips = (const SmClip*)ctx->sm_clips.p;
    const void* d_y = d_in;                    // the groups' input
    int y_fmt = sample_fmt;
    const uint32_t* d_bad;
    int bad_stride;
    if (pre) {
      if ((rc = ensure(ctx->ez_y, (size_t)pos * sizeof(float))) != AFX_OK) return rc;
      if ((rc = run_filtfilt_chain(ctx, d_in, sample_fmt, AFX_FILT_EXPERIMENT, 0.98f, kPadlen, kSections, frecs, ftiles,
                                   (const FiltTab*)ctx->ft_tab.p, (float*)ctx->ez_y.p)) != AFX_OK) return rc;
      d_y = ctx->ez_y.p; y_fmt = AFX_FMT_F32;
      static_assert(offsetof(FiltState, bad) == 12 && sizeof(FiltState) == 16, "the flag of record c is word 4 c + 3");
      d_bad = (const uint32_t*)ctx->ft_st.p + 3; bad_stride = 4;
    } else {
      if ((rc = ensure(ctx->sm_bad, n * sizeof(uint32_t))) != AFX_OK) return rc;
      HIP_TRY(launch_sm_check(s, d_in, sample_fmt, d_sclips, n, (uint32_t*)ctx->sm_bad.p));
      d_bad = (const uint32_t*)ctx->sm_bad.p; bad_stride = 1;
    }
    if (zc) {
      if ((rc = ensure(ctx->ez_m, (size_t)pos * sizeof(float))) != AFX_OK) return rc;
      if ((rc = ensure(ctx->ez_s, (size_t)pos * sizeof(float))) != AFX_OK) return rc;
      if ((rc = ensure(ctx->ez_neg, (size_t)pos)) != AFX_OK) return rc;
      if ((rc = ensure(ctx->ez_peak, n * sizeof(float))) != AFX_OK) return rc;
      if ((rc = ensure(ctx->ez_rate, (size_t)frames * sizeof(double))) != AFX_OK) return rc;
      HIP_TRY(launch_medfilt(s, d_y, y_fmt, 3, d_sclips, n, nst, d_bad, bad_stride, (float*)ctx->ez_m.p));
      // the reference's guard: savgol_filter(11, 3) only when len(y) > 11; shorter clips pass through
      HIP_TRY(launch_savgol(s, ctx->ez_m.p, AFX_FMT_F32, (const SgTab*)ctx->sm_tab.p, 12, d_sclips + n, n, nst, d_bad, bad_stride, (float*)ctx->ez_s.p));
      HIP_TRY(launch_ez_peak(s, (const float*)ctx->ez_s.p, d_eclips, n, d_bad, bad_stride, (float*)ctx->ez_peak.p));
      HIP_TRY(launch_ez_sign(s, (const float*)ctx->ez_s.p, d_sclips + n, n, nst, d_bad, bad_stride, (const float*)ctx->ez_peak.p, (uint8_t*)ctx->ez_neg.p));
    }
    if (en && (rc = ensure(ctx->ez_energy, (size_t)frames * sizeof(double))) != AFX_OK) return rc;
    if (en || zc) {
      HIP_TRY(launch_ez_frames(s, en ? d_y : nullptr, y_fmt, zc ? (const uint8_t*)ctx->ez_neg.p : nullptr, d_eclips, n, frames, d_bad,
                               bad_stride, (double*)ctx->ez_energy.p, (double*)ctx->ez_rate.p));
      HIP_TRY(launch_ez_stats(s, d_eclips, n, d_bad, bad_stride, flags, (const double*)ctx->ez_energy.p, (const double*)ctx->ez_rate.p,
                              (double*)ctx->ez_rec.p));
      h_rec.resize((size_t)n * AFX_EZ_N);
      HIP_TRY(hipMemcpyAsync(h_rec.data(), ctx->ez_rec.p, h_rec.size() * sizeof(double), hipMemcpyDeviceToHost, s));
    }
    if (zc) {
      h_peak.resize(n);
      HIP_TRY(hipMemcpyAsync(h_peak.data(), ctx->ez_peak.p, n * sizeof(float), hipMemcpyDeviceToHost, s));
    }
    if (pre) {
      h_st.resize(n);
      HIP_TRY(hipMemcpyAsync(h_st.data(), ctx->ft_st.p, n * sizeof(FiltState), hipMemcpyDeviceToHost, s));
    } else {
      h_bad.resize(n);
      HIP_TRY(hipMemcpyAsync(h_bad.data(), ctx->sm_bad.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(hipStreamSynchronize(s));
    for (int q = 0; q < n; ++q) {
      const int i = idx[q];
      if (pre ? h_st[q].bad : h_bad[q]) { out_status[i] = AFX_CLIP_NONFINITE; continue; }
      double* r = out_rec + (size_t)AFX_EZ_N * i;
      const double* g = h_rec.data() + (size_t)AFX_EZ_N * q;
      r[AFX_EZ_T] = (double)erecs[q].T; r[AFX_EZ_FL] = erecs[q].fl; r[AFX_EZ_HOP] = erecs[q].hop;
      if (en) { r[AFX_EZ_ENERGY_MEAN] = g[AFX_EZ_ENERGY_MEAN]; r[AFX_EZ_ENERGY_STD] = g[AFX_EZ_ENERGY_STD]; r[AFX_EZ_ENERGY_P10] = g[AFX_EZ_ENERGY_P10]; }
      if (zc) {
        r[AFX_EZ_ZCR_MEAN] = g[AFX_EZ_ZCR_MEAN]; r[AFX_EZ_ZCR_STD] = g[AFX_EZ_ZCR_STD]; r[AFX_EZ_ZCR_LOCAL] = g[AFX_EZ_ZCR_LOCAL];
        r[AFX_EZ_PEAK_SMOOTH] = (double)h_peak[q];
      }
      if (pre) { r[AFX_EZ_PEAK_IN] = (double)h_st[q].peak_in; r[AFX_EZ_PEAK_FILT] = h_st[q].peak_out; }
    }
  }
  return AFX_OK;
}

// ---- BS.1770 integrated loudness and loudness / peak normalisation (pyloudnorm's Meter and normalize) ----------------------
// A chunk (cut_stft_chunk with the record of loud_cost): the samples staged packed when they are the host's, the records
// uploaded, the two walks around the scan, the gate; the clips' eight scalars come back, log10 and the gain are taken here
// (loud_finish, the host executor's code), and in a normalising mode the gains go up again for one more launch.
extern "C" int afx_loudness_batch(afx_ctx* ctx, const void* samples, int sample_fmt, int mem_kind,
                                  const int64_t* offsets, const int64_t* lengths, const int32_t* rates, int n_clips,
                                  double block_size, int mode, double target,
                                  double* out_rec, double* out_blocks, const int64_t* out_block_offsets,
                                  float* out, int out_mem_kind, const int64_t* out_offsets, int32_t* out_status) {
  const char* who = "afx_loudness_batch";
  if (!ctx || n_clips < 0 || (n_clips > 0 && (!offsets || !lengths || !rates || !out_rec || !out_status))) return null_arg(who);
  if (mode != AFX_LOUD_MEASURE && mode != AFX_LOUD_NORM_LOUDNESS && mode != AFX_LOUD_NORM_PEAK) { set_error(std::string(who) + ": unknown mode"); return AFX_ERR_INVALID; }
  const bool norm = mode != AFX_LOUD_MEASURE;
  int rc;
  if ((rc = check_sample_format(who, sample_fmt, mem_kind)) != AFX_OK) return rc;
  if (norm) {
    if (n_clips > 0 && !out_offsets) return null_arg(who);
    if ((rc = check_sample_format(who, sample_fmt, out_mem_kind)) != AFX_OK) return rc;
    if (!std::isfinite(target)) { set_error(std::string(who) + ": the target must be finite"); return AFX_ERR_INVALID; }
  }
  if ((rc = check_clip_ranges(who, offsets, lengths, norm ? out_offsets : nullptr, n_clips, INT64_MAX / 8)) != AFX_OK) return rc;
  if (out_blocks && out_block_offsets)
    for (int i = 0; i < n_clips; ++i)
      if (out_block_offsets[i] < 0 || out_block_offsets[i] > INT64_MAX / 16) { set_error(std::string(who) + ": out_block_offsets out of range"); return AFX_ERR_INVALID; }
  std::vector<int> rate_list;
  std::vector<int32_t> tab_of((size_t)n_clips), nbk((size_t)n_clips);
  std::vector<int64_t> zoff((size_t)n_clips);
  bool any = false;
  int64_t zpos = 0;
  for (int i = 0; i < n_clips; ++i) {
    int code;
    if (const char* why = loud_refusal(rates[i], block_size, &code)) {
      set_error(std::string(who) + ": clip " + std::to_string(i) + ": " + why);
      return code;
    }
    auto it = std::find(rate_list.begin(), rate_list.end(), (int)rates[i]);
    if (it == rate_list.end()) {
      if ((int)rate_list.size() == kLoudMaxRates) { set_error(std::string(who) + ": more than 16 distinct rates in one call is not supported"); return AFX_ERR_UNSUPPORTED; }
      rate_list.push_back(rates[i]);
      it = rate_list.end() - 1;
    }
    tab_of[i] = (int32_t)(it - rate_list.begin());
    nbk[i] = (int32_t)loud_n_blocks(lengths[i], rates[i], block_size);
    zoff[i] = out_block_offsets ? out_block_offsets[i] : zpos;
    zpos += nbk[i];
  }
  for (int i = 0; i < n_clips; ++i) {
    const bool live = mode == AFX_LOUD_NORM_PEAK ? lengths[i] > 0 : nbk[i] > 0;
    out_status[i] = live ? AFX_CLIP_OK : AFX_CLIP_TOO_SHORT;
    nan_row(out_rec, AFX_LOUD_N, i);
    any = any || live;
  }
  if (!any) return AFX_OK;
  if (!samples || (norm && !out)) { set_error(std::string(who) + ": null samples / out"); return AFX_ERR_INVALID; }

  (void)hipGetLastError();
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  {
    std::vector<FiltTab> tabs(rate_list.size());
    for (size_t r = 0; r < rate_list.size(); ++r) loud_build_tab(rate_list[r], tabs[r]);
    if ((rc = ensure(ctx->ld_tab, tabs.size() * sizeof(FiltTab))) != AFX_OK) return rc;
    HIP_TRY(hipMemcpyAsync(ctx->ld_tab.p, tabs.data(), tabs.size() * sizeof(FiltTab), hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));                  // tabs dies here
  }
  const FiltTab* d_tabs = (const FiltTab*)ctx->ld_tab.p;
  const size_t esz = sample_fmt == AFX_FMT_S16 ? 2 : 4;
  const bool h_in = mem_kind == AFX_MEM_HOST, h_out = norm && out_mem_kind == AFX_MEM_HOST;
  const double gate = loud_abs_gate();
  StftCost cost;
  loud_cost(sample_fmt, mem_kind, out_mem_kind, mode, cost);
  StftChunk ck;
  std::vector<LoudClip> recs;
  std::vector<int> idx;
  std::vector<HostPiece> pieces;
  std::vector<char> image;
  std::vector<float> stage_out, h_gain;
  std::vector<double> h_dev, h_z;
  for (int c0 = 0; c0 < n_clips; c0 = ck.next) {
    cut_stft_chunk(offsets, lengths, n_clips, c0, dev_env().loud_budget, cost, ck);
    recs.clear(); idx.clear();
    int64_t tiles = 0, segs = 0, zs = 0, in_pos = 0, out_pos = 0;
    for (int i : ck.idx) {
      if (out_status[i] != AFX_CLIP_OK) continue;
      LoudClip r{};
      r.n = lengths[i];
      r.in_off = h_in ? in_pos : offsets[i];
      r.out_off = !norm ? 0 : h_out ? out_pos : out_offsets[i];
      r.seg_off = segs; r.z_off = zs;
      r.tg = block_size; r.rate = (double)rates[i];
      r.first_tile = (int32_t)tiles; r.n_tiles = (int32_t)((r.n + kFiltTile - 1) / kFiltTile);
      r.n_blocks = nbk[i]; r.tab = tab_of[i];
      recs.push_back(r); idx.push_back(i);
      tiles += r.n_tiles; segs += nbk[i] > 0 ? (int64_t)nbk[i] + 3 : 0; zs += nbk[i];
      in_pos += (r.n + 3) / 4 * 4; out_pos += (r.n + 3) / 4 * 4;
    }
    const int n = (int)recs.size(), nt = (int)tiles;
    if (n == 0) continue;
    if (tiles > cost.tile_cap) { set_error(std::string(who) + ": clip too large for one launch"); return AFX_ERR_UNSUPPORTED; }
    if ((rc = ensure(ctx->ld_clips, (size_t)n * sizeof(LoudClip))) != AFX_OK) return rc;
    if ((rc = ensure(ctx->ld_carry, (size_t)nt * kFiltB * kLoudZ * sizeof(double))) != AFX_OK) return rc;
    if ((rc = ensure(ctx->ld_part, (size_t)nt * kFiltB * 2 * sizeof(double))) != AFX_OK) return rc;
    if ((rc = ensure(ctx->ld_tpeak, (size_t)nt * sizeof(float))) != AFX_OK) return rc;
    if ((rc = ensure(ctx->ld_tbad, (size_t)nt * sizeof(uint32_t))) != AFX_OK) return rc;
    if ((rc = ensure(ctx->ld_seg, (size_t)std::max<int64_t>(segs, 1) * sizeof(double))) != AFX_OK) return rc;
    if ((rc = ensure(ctx->ld_z, (size_t)std::max<int64_t>(zs, 1) * sizeof(double))) != AFX_OK) return rc;
    if ((rc = ensure(ctx->ld_rec, (size_t)n * kLoudRec * sizeof(double))) != AFX_OK) return rc;
    const void* d_in = samples;
    if (h_in) {
      pieces.clear();
      for (int q = 0; q < n; ++q)
        pieces.push_back(clip_piece(samples, offsets[idx[q]], recs[q].in_off, recs[q].n, esz));
      if ((rc = stage_in(ctx, image, in_pos * (int64_t)esz, pieces, &d_in)) != AFX_OK) return rc;
    }
    float* d_out = nullptr;                    // a normalising mode writes it behind the chunk's first synchronise
    if (norm && (rc = out_buffer(ctx, out, out_mem_kind, out_pos, &d_out)) != AFX_OK) return rc;
    HIP_TRY(hipMemcpyAsync(ctx->ld_clips.p, recs.data(), (size_t)n * sizeof(LoudClip), hipMemcpyHostToDevice, s));
    const LoudClip* d_clips = (const LoudClip*)ctx->ld_clips.p;
    double *carry = (double*)ctx->ld_carry.p, *part = (double*)ctx->ld_part.p, *d_rec = (double*)ctx->ld_rec.p;
    HIP_TRY(launch_loud_ends(s, d_in, sample_fmt, d_tabs, d_clips, n, nt, carry, (float*)ctx->ld_tpeak.p, (uint32_t*)ctx->ld_tbad.p));
    HIP_TRY(launch_loud_scan(s, d_tabs, d_clips, n, carry));
    HIP_TRY(launch_loud_sums(s, d_in, sample_fmt, d_tabs, d_clips, n, nt, carry, part));
    HIP_TRY(launch_loud_gate(s, d_clips, n, part, (const float*)ctx->ld_tpeak.p, (const uint32_t*)ctx->ld_tbad.p, gate,
                             (double*)ctx->ld_seg.p, (double*)ctx->ld_z.p, d_rec));
    h_dev.resize((size_t)n * kLoudRec);
    HIP_TRY(hipMemcpyAsync(h_dev.data(), d_rec, h_dev.size() * sizeof(double), hipMemcpyDeviceToHost, s));
    if (out_blocks && zs > 0) {
      h_z.resize((size_t)zs);
      HIP_TRY(hipMemcpyAsync(h_z.data(), ctx->ld_z.p, (size_t)zs * sizeof(double), hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(hipStreamSynchronize(s));
    h_gain.assign((size_t)n, std::nanf(""));
    for (int q = 0; q < n; ++q) {
      const int i = idx[q];
      const double* d = h_dev.data() + (size_t)q * kLoudRec;
      if (d[kLdBad] != 0.0) { out_status[i] = AFX_CLIP_NONFINITE; continue; }   // its record stays NaN, its output range as the caller left it
      h_gain[q] = loud_finish(d, mode, target, out_rec + (size_t)AFX_LOUD_N * i);
      if (out_blocks && nbk[i] > 0) std::memcpy(out_blocks + zoff[i], h_z.data() + recs[q].z_off, (size_t)nbk[i] * sizeof(double));
    }
    if (!norm) continue;
    if ((rc = ensure(ctx->ld_gain, (size_t)n * sizeof(float))) != AFX_OK) return rc;
    HIP_TRY(hipMemcpyAsync(ctx->ld_gain.p, h_gain.data(), (size_t)n * sizeof(float), hipMemcpyHostToDevice, s));
    HIP_TRY(launch_loud_gain(s, d_in, sample_fmt, d_clips, n, nt, (const float*)ctx->ld_gain.p, d_out));
    if (h_out && (rc = fetch_out(ctx, d_out, out_pos, stage_out)) != AFX_OK) return rc;
    HIP_TRY(hipStreamSynchronize(s));
    pieces.clear();
    for (int q = 0; q < n; ++q)
      if (h_out && out_status[idx[q]] == AFX_CLIP_OK) pieces.push_back({stage_out.data() + recs[q].out_off, out_offsets[idx[q]] * 4, recs[q].n * 4});
    scatter_pieces(out, pieces);
  }
  return AFX_OK;
}

// ---- spectral-gating noise reduction (noisereduce's reduce_noise) -----------------------------------------------------------
// A chunk (cut_stft_chunk with the record of gate_cost over max(length, noise length)): the clips and their noise clips
// staged packed when they are the host's, both grids' records uploaded, the samples brought to float32 with their
// non-finite flags, then the passes of afx_gate.hip in order.  The flags, thr and the bit plane come back with the output.
extern "C" int afx_gate_batch(afx_ctx* ctx, const void* samples, int sample_fmt, int mem_kind,
                              const int64_t* offsets, const int64_t* lengths, int n_clips,
                              const int64_t* noise_offsets, const int64_t* noise_lengths, const afx_gate_opts* opts,
                              float* out, int out_mem_kind, const int64_t* out_offsets,
                              double* out_thresh, uint32_t* out_mask, int32_t* out_status) {
  const char* who = "afx_gate_batch";
  if (!ctx || !opts || n_clips < 0 || (n_clips > 0 && (!offsets || !lengths || !out_offsets || !out_status))) return null_arg(who);
  if ((noise_offsets == nullptr) != (noise_lengths == nullptr)) return null_arg(who);
  int rc;
  if ((rc = check_sample_format(who, sample_fmt, mem_kind)) != AFX_OK) return rc;
  if ((rc = check_sample_format(who, sample_fmt, out_mem_kind)) != AFX_OK) return rc;
  GateDerived gd;
  const char* why = "";
  if ((rc = gate_derive(*opts, gd, &why)) != AFX_OK) { set_error(std::string(who) + ": " + why); return rc; }
  const int n_fft = opts->n_fft, hop = opts->hop, pad = opts->padding;
  if ((n_fft != 1024 && n_fft != 2048) || hop != n_fft / 4) { set_error(std::string(who) + ": n_fft / hop must be 1024 / 256 or 2048 / 512"); return AFX_ERR_UNSUPPORTED; }
  if ((rc = check_clip_ranges(who, offsets, lengths, out_offsets, n_clips, INT64_MAX / 8)) != AFX_OK) return rc;
  const bool with_noise = noise_offsets != nullptr, stat = opts->stationary != 0;
  if (with_noise && (rc = check_clip_ranges(who, noise_offsets, noise_lengths, nullptr, n_clips, INT64_MAX / 8)) != AFX_OK) return rc;
  const int bins = gate_bins(n_fft), pitch = gate_pitch(n_fft), words = gate_words(n_fft), fpw = n_fft == 1024 ? 2 : 1;

  // the noise clip of clip i (stationary): its own, or the clip; cut to chunk_size samples on request
  auto noise_len = [&](int i) {
    int64_t l = with_noise ? noise_lengths[i] : lengths[i];
    if (opts->clip_noise && l > opts->chunk_size) l = opts->chunk_size;
    return l;
  };
  std::vector<int64_t> eff((size_t)n_clips), moff((size_t)n_clips);
  bool any = false;
  int64_t mpos = 0;
  for (int i = 0; i < n_clips; ++i) {
    const int64_t L = lengths[i];
    int st = AFX_CLIP_OK;
    if (L == 0 || (stat && with_noise && noise_lengths[i] == 0)) st = AFX_CLIP_TOO_SHORT;
    else if (L > opts->chunk_size) st = AFX_CLIP_TOO_LONG;
    else if (stat && noise_len(i) > kGateMaxChunk) { set_error(std::string(who) + ": a noise clip of more than 2^24 samples is not supported"); return AFX_ERR_UNSUPPORTED; }
    out_status[i] = st;
    eff[i] = st != AFX_CLIP_OK ? 0 : stat ? std::max(L, noise_len(i)) : L;
    moff[i] = mpos;
    if (st == AFX_CLIP_OK) mpos += gate_frames(L, hop, pad) * words;
    if (out_thresh) nan_row(out_thresh, bins, i);
    any = any || st == AFX_CLIP_OK;
  }
  if (!any) return AFX_OK;
  if (!samples || !out) { set_error(std::string(who) + ": null samples / out"); return AFX_ERR_INVALID; }

  (void)hipGetLastError();
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  GateTabs tb{};
  const int n_f = gd.smooth ? gd.n_f : 0, n_t = gd.smooth ? gd.n_t : 0;
  {
    constexpr size_t kTapDoubles = 2 * kGateMaxNf + 1 + 2 * kGateMaxNt + 1;
    std::vector<char> tab(kTapDoubles * sizeof(double) + ((size_t)n_fft + 4096) * sizeof(float));
    double* td = (double*)tab.data();
    float* tf = (float*)(tab.data() + kTapDoubles * sizeof(double));
    if (gd.smooth) {
      std::memcpy(td, gd.vf, (size_t)(2 * n_f + 1) * sizeof(double));
      std::memcpy(td + 2 * kGateMaxNf + 1, gd.vt, (size_t)(2 * n_t + 1) * sizeof(double));
    } else {
      td[0] = 1.0; td[2 * kGateMaxNf + 1] = 1.0;
    }
    for (int i = 0; i < n_fft; ++i) tf[i] = (float)(0.5 - 0.5 * std::cos(2.0 * M_PI * (double)i / (double)n_fft));
    for (int k = 0; k < 1024; ++k) {
      tf[n_fft + 2 * k] = (float)std::cos(2.0 * M_PI * k / 1024.0); tf[n_fft + 2 * k + 1] = (float)-std::sin(2.0 * M_PI * k / 1024.0);
      tf[n_fft + 2048 + 2 * k] = (float)std::cos(2.0 * M_PI * k / 2048.0); tf[n_fft + 2048 + 2 * k + 1] = (float)-std::sin(2.0 * M_PI * k / 2048.0);
    }
    if ((rc = ensure(ctx->gt_tab, tab.size())) != AFX_OK) return rc;
    HIP_TRY(hipMemcpyAsync(ctx->gt_tab.p, tab.data(), tab.size(), hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));                  // tab dies here
    tb.vf = (const double*)ctx->gt_tab.p;
    tb.vt = tb.vf + 2 * kGateMaxNf + 1;
    tb.window = (const float*)(tb.vf + kTapDoubles);
    tb.w1024 = tb.window + n_fft;
    tb.w2048 = tb.w1024 + 2048;
  }

  const size_t esz = sample_fmt == AFX_FMT_S16 ? 2 : 4;
  const bool h_in = mem_kind == AFX_MEM_HOST, h_out = out_mem_kind == AFX_MEM_HOST;
  StftCost cost;
  gate_cost(n_fft, stat, pad, sample_fmt, mem_kind, out_mem_kind, with_noise, cost);
  StftChunk ck;
  std::vector<GateGrid> sig, noi;
  std::vector<HpssClip> prs, prn;
  std::vector<HostPiece> pieces;
  std::vector<char> image, recs;
  std::vector<uint32_t> h_bad, h_bits;
  std::vector<double> h_thr;
  for (int c0 = 0; c0 < n_clips; c0 = ck.next) {
    cut_stft_chunk(offsets, eff.data(), n_clips, c0, dev_env().gate_budget, cost, ck);
    const int n = (int)ck.idx.size();
    if (n == 0) continue;
    sig.assign((size_t)n, GateGrid{}); noi.assign((size_t)n, GateGrid{});
    prs.assign((size_t)n, HpssClip{}); prn.clear();
    int64_t ypos = 0, in_pos = 0, rows = 0, nrows = 0, units = 0, nunits = 0, arows = 0, max_len = 0, max_nlen = 0;
    for (int q = 0; q < n; ++q) {
      const int i = ck.idx[q];
      const int64_t L = lengths[i];
      GateGrid& g = sig[q];
      g.y_off = ypos; g.len = L; g.out_off = h_out ? ypos : out_offsets[i];
      g.T = (int32_t)gate_frames(L, hop, pad);
      gate_active(L, n_fft, hop, pad, g.T, &g.ta, &g.na);
      g.row_base = rows; g.unit_base = units; g.arow_base = arows; g.shift = pad; g.clip = q;
      prs[q].in_off = h_in ? in_pos : offsets[i]; prs[q].y_off = ypos; prs[q].len = L;
      ypos += (L + 3) / 4 * 4; in_pos += (L + 3) / 4 * 4;
      rows += g.T; units += (g.na + fpw - 1) / fpw; arows += g.na; max_len = std::max(max_len, L);
    }
    if (stat)
      for (int q = 0; q < n; ++q) {
        const int i = ck.idx[q];
        const int64_t Ln = noise_len(i);
        GateGrid& g = noi[q];
        g.len = Ln; g.T = (int32_t)(1 + Ln / hop); g.ta = 0; g.na = g.T; g.shift = 0; g.clip = q;
        g.row_base = nrows; g.unit_base = nunits;
        if (with_noise) {
          HpssClip r{};
          r.in_off = h_in ? in_pos : noise_offsets[i]; r.y_off = ypos; r.len = Ln;
          prn.push_back(r);
          g.y_off = ypos;
          ypos += (Ln + 3) / 4 * 4; in_pos += (Ln + 3) / 4 * 4; max_nlen = std::max(max_nlen, Ln);
        } else {
          g.y_off = sig[q].y_off;
        }
        nrows += g.T; nunits += (g.na + fpw - 1) / fpw;
      }
    if (rows > INT32_MAX / 2 || nrows > INT32_MAX / 2) { set_error(std::string(who) + ": chunk too large for one launch"); return AFX_ERR_UNSUPPORTED; }

    // the records as one upload: both grids, then the prep records of the clips and of the noise clips
    const size_t o_noi = (size_t)n * sizeof(GateGrid), o_prs = 2 * o_noi, o_prn = o_prs + (size_t)n * sizeof(HpssClip);
    recs.assign(o_prn + prn.size() * sizeof(HpssClip), 0);
    std::memcpy(recs.data(), sig.data(), o_noi);
    std::memcpy(recs.data() + o_noi, noi.data(), o_noi);
    std::memcpy(recs.data() + o_prs, prs.data(), (size_t)n * sizeof(HpssClip));
    if (!prn.empty()) std::memcpy(recs.data() + o_prn, prn.data(), prn.size() * sizeof(HpssClip));
    if ((rc = ensure(ctx->gt_grids, recs.size())) != AFX_OK) return rc;
    if ((rc = ensure(ctx->gt_y, (size_t)std::max<int64_t>(ypos, 1) * sizeof(float))) != AFX_OK) return rc;
    if ((rc = ensure(ctx->gt_bad, (size_t)2 * n * sizeof(uint32_t))) != AFX_OK) return rc;
    if ((rc = ensure(ctx->gt_mag, (size_t)rows * pitch * sizeof(float))) != AFX_OK) return rc;
    if ((rc = ensure(ctx->gt_mask, (size_t)rows * pitch * sizeof(float))) != AFX_OK) return rc;
    if ((rc = ensure(ctx->gt_rows, (size_t)std::max<int64_t>(arows, 1) * n_fft * sizeof(float))) != AFX_OK) return rc;
    if (stat) {
      if ((rc = ensure(ctx->gt_nmag, (size_t)nrows * pitch * sizeof(float))) != AFX_OK) return rc;
      if ((rc = ensure(ctx->gt_bits, (size_t)rows * words * sizeof(uint32_t))) != AFX_OK) return rc;
      if ((rc = ensure(ctx->gt_thr, (size_t)n * pitch * sizeof(double))) != AFX_OK) return rc;
      if ((rc = ensure(ctx->gt_amp, (size_t)n * pitch * sizeof(double))) != AFX_OK) return rc;
    } else {
      if ((rc = ensure(ctx->gt_fwd, (size_t)rows * pitch * sizeof(double))) != AFX_OK) return rc;
    }
    const void* d_in = samples;
    if (h_in) {
      pieces.clear();
      for (int q = 0; q < n; ++q)
        pieces.push_back(clip_piece(samples, offsets[ck.idx[q]], prs[q].in_off, prs[q].len, esz));
      for (size_t q = 0; q < prn.size(); ++q)
        pieces.push_back(clip_piece(samples, noise_offsets[ck.idx[q]], prn[q].in_off, prn[q].len, esz));
      if ((rc = stage_in(ctx, image, in_pos * (int64_t)esz, pieces, &d_in)) != AFX_OK) return rc;
    }
    float* d_out;
    if ((rc = out_buffer(ctx, out, out_mem_kind, std::max<int64_t>(ypos, 1), &d_out)) != AFX_OK) return rc;
    HIP_TRY(hipMemcpyAsync(ctx->gt_grids.p, recs.data(), recs.size(), hipMemcpyHostToDevice, s));
    const GateGrid* d_sig = (const GateGrid*)ctx->gt_grids.p;
    const GateGrid* d_noi = (const GateGrid*)((const char*)ctx->gt_grids.p + o_noi);
    const HpssClip* d_prs = (const HpssClip*)((const char*)ctx->gt_grids.p + o_prs);
    const HpssClip* d_prn = (const HpssClip*)((const char*)ctx->gt_grids.p + o_prn);
    float *y = (float*)ctx->gt_y.p, *mag = (float*)ctx->gt_mag.p, *mask = (float*)ctx->gt_mask.p, *trows = (float*)ctx->gt_rows.p;
    uint32_t* bad = (uint32_t*)ctx->gt_bad.p;
    HIP_TRY(hipMemsetAsync(bad, 0, (size_t)2 * n * sizeof(uint32_t), s));
    HIP_TRY(hipMemsetAsync(mag, 0, (size_t)rows * pitch * sizeof(float), s));
    HIP_TRY(launch_hpss_prep(s, d_in, sample_fmt, 0, 0.f, d_prs, n, max_len, y, bad));
    if (!prn.empty()) HIP_TRY(launch_hpss_prep(s, d_in, sample_fmt, 0, 0.f, d_prn, n, max_nlen, y, bad + n));
    HIP_TRY(launch_gate_mag(s, n_fft, y, d_sig, bad, n, units, tb, mag));
    if (stat) {
      float* nmag = (float*)ctx->gt_nmag.p;
      double *thr = (double*)ctx->gt_thr.p, *amp = (double*)ctx->gt_amp.p;
      uint32_t* bits = (uint32_t*)ctx->gt_bits.p;
      HIP_TRY(launch_gate_mag(s, n_fft, y, d_noi, bad, n, nunits, tb, nmag));
      HIP_TRY(launch_gate_stats(s, n_fft, d_sig, d_noi, n, mag, nmag, opts->n_std_thresh, thr, amp));
      HIP_TRY(launch_gate_hard(s, n_fft, d_sig, n, rows, mag, amp, bits));
      HIP_TRY(launch_gate_smooth(s, n_fft, d_sig, n, rows, bits, nullptr, n_f, n_t, opts->prop_decrease, tb, mask));
    } else {
      HIP_TRY(launch_gate_recur(s, n_fft, d_sig, n, gd.beta, opts->thresh_n_mult, opts->sigmoid_slope, mag, (double*)ctx->gt_fwd.p));
      HIP_TRY(launch_gate_smooth(s, n_fft, d_sig, n, rows, nullptr, mag, n_f, n_t, opts->prop_decrease, tb, mask));
    }
    HIP_TRY(launch_gate_apply(s, n_fft, y, d_sig, bad, n, units, tb, mask, trows));
    HIP_TRY(launch_gate_ola(s, n_fft, trows, d_sig, bad, n, max_len, tb, d_out));
    h_bad.resize((size_t)2 * n);
    HIP_TRY(hipMemcpyAsync(h_bad.data(), bad, h_bad.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    if (stat && out_thresh) {
      h_thr.resize((size_t)n * pitch);
      HIP_TRY(hipMemcpyAsync(h_thr.data(), ctx->gt_thr.p, h_thr.size() * sizeof(double), hipMemcpyDeviceToHost, s));
    }
    if (stat && out_mask) {
      h_bits.resize((size_t)rows * words);
      HIP_TRY(hipMemcpyAsync(h_bits.data(), ctx->gt_bits.p, h_bits.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    }
    if (h_out)
      // straight to the caller's ranges, one copy per run of clips that lie back to back on both sides (gaps are not written)
      for (int q = 0; q < n;) {
        int e = q;
        int64_t cnt = sig[q].len;
        while (e + 1 < n && sig[e + 1].y_off == sig[q].y_off + cnt && out_offsets[ck.idx[e + 1]] == out_offsets[ck.idx[q]] + cnt) cnt += sig[++e].len;
        HIP_TRY(hipMemcpyAsync(out + out_offsets[ck.idx[q]], d_out + sig[q].y_off, (size_t)cnt * sizeof(float), hipMemcpyDeviceToHost, s));
        q = e + 1;
      }
    HIP_TRY(hipStreamSynchronize(s));
    for (int q = 0; q < n; ++q) {
      const int i = ck.idx[q];
      const bool nf = (h_bad[q] | h_bad[(size_t)n + q]) != 0;
      if (nf) out_status[i] = AFX_CLIP_NONFINITE;
      if (stat && out_thresh && !nf) std::memcpy(out_thresh + (size_t)bins * i, h_thr.data() + (size_t)q * pitch, (size_t)bins * sizeof(double));
      if (stat && out_mask) std::memcpy(out_mask + moff[i], h_bits.data() + sig[q].row_base * words, (size_t)sig[q].T * words * sizeof(uint32_t));
    }
  }
  return AFX_OK;
}

// ---- librosa-style stft / istft at n_fft 1024 and 2048 -----------------------------------------------------------------------
// The caller's window and the twiddles of both transforms, uploaded once per call (the window is the caller's to change).
static int stft_tables(afx_ctx* ctx, int n_fft, const float* window, StftTabs& tb) {
  std::vector<float> tab((size_t)n_fft + 4096);
  std::memcpy(tab.data(), window, (size_t)n_fft * sizeof(float));
  for (int k = 0; k < 1024; ++k) {
    tab[n_fft + 2 * k] = (float)std::cos(2.0 * M_PI * k / 1024.0); tab[n_fft + 2 * k + 1] = (float)-std::sin(2.0 * M_PI * k / 1024.0);
    tab[n_fft + 2048 + 2 * k] = (float)std::cos(2.0 * M_PI * k / 2048.0); tab[n_fft + 2048 + 2 * k + 1] = (float)-std::sin(2.0 * M_PI * k / 2048.0);
  }
  if (int rc = ensure(ctx->st_tab, tab.size() * sizeof(float))) return rc;
  HIP_TRY(hipMemcpyAsync(ctx->st_tab.p, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));            // tab dies here
  tb.window = (const float*)ctx->st_tab.p;
  tb.w1024 = tb.window + n_fft;
  tb.w2048 = tb.w1024 + 2048;
  return AFX_OK;
}

static int stft_opts_arg(const char* who, const afx_stft_opts* opts) {
  const char* why = "";
  const int rc = stft_check_opts(*opts, &why);
  if (rc != AFX_OK) set_error(std::string(who) + ": " + why);
  return rc;
}

// A chunk (cut_stft_chunk with the record of stft_cost over the lengths, 0 for a clip that is too short): the clips staged
// packed when they are the host's, the records uploaded, the samples brought to float32 with their non-finite flags
// (k_hpss_prep), then one launch of k_stft_frames into the caller's device memory or into the packed image that goes home.
extern "C" int afx_stft_batch(afx_ctx* ctx, const void* samples, int sample_fmt, int mem_kind,
                              const int64_t* offsets, const int64_t* lengths, int n_clips,
                              const afx_stft_opts* opts, const float* window,
                              void* out, int out_mem_kind, const int64_t* out_offsets, int32_t* out_status) {
  const char* who = "afx_stft_batch";
  int rc;
  if ((rc = clip_batch_args(who, ctx, sample_fmt, mem_kind, offsets, lengths, n_clips, out_mem_kind, out_offsets, out_status,
                            opts && window)) != AFX_OK) return rc;
  if (!opts || !window) return null_arg(who);
  if ((rc = stft_opts_arg(who, opts)) != AFX_OK) return rc;
  const afx_stft_opts o = *opts;
  const int n_fft = o.n_fft, bins = stft_bins(n_fft), fpw = n_fft == 1024 ? 2 : 1;
  const int fpe = o.out_kind == AFX_STFT_COMPLEX ? 2 : 1;        // floats per output element
  std::vector<int64_t> eff((size_t)n_clips), frames((size_t)n_clips);
  bool any = false;
  for (int i = 0; i < n_clips; ++i) {
    stft_frames(o, lengths[i], &frames[i], &out_status[i]);
    eff[i] = out_status[i] == AFX_CLIP_OK ? lengths[i] : 0;
    any = any || out_status[i] == AFX_CLIP_OK;
  }
  if (!any) return AFX_OK;
  if (!samples || !out) { set_error(std::string(who) + ": null samples / out"); return AFX_ERR_INVALID; }

  (void)hipGetLastError();
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  StftTabs tb{};
  if ((rc = stft_tables(ctx, n_fft, window, tb)) != AFX_OK) return rc;

  const size_t esz = sample_fmt == AFX_FMT_S16 ? 2 : 4;
  const bool h_in = mem_kind == AFX_MEM_HOST, h_out = out_mem_kind == AFX_MEM_HOST;
  StftCost cost;
  stft_cost(o, sample_fmt, mem_kind, out_mem_kind, 0, cost);
  StftChunk ck;
  std::vector<StftClip> recs;
  std::vector<HpssClip> prs;
  std::vector<HostPiece> pieces;
  std::vector<char> image, up;
  std::vector<uint32_t> h_bad;
  std::vector<float> stage_out;
  for (int c0 = 0; c0 < n_clips; c0 = ck.next) {
    cut_stft_chunk(offsets, eff.data(), n_clips, c0, dev_env().stft_budget, cost, ck);
    const int n = (int)ck.idx.size();
    if (n == 0) continue;
    recs.assign((size_t)n, StftClip{}); prs.assign((size_t)n, HpssClip{});
    int64_t ypos = 0, in_pos = 0, opos = 0, rows = 0, units = 0, max_len = 0;
    for (int q = 0; q < n; ++q) {
      const int i = ck.idx[q];
      const int64_t L = lengths[i], T = frames[i];
      StftClip& r = recs[q];
      r.y_off = ypos; r.len = L; r.out_off = h_out ? opos : out_offsets[i]; r.unit_base = units; r.T = (int32_t)T; r.clip = q;
      prs[q].in_off = h_in ? in_pos : offsets[i]; prs[q].y_off = ypos; prs[q].len = L;
      ypos += (L + 3) / 4 * 4; in_pos += (L + 3) / 4 * 4; opos += T * bins;
      rows += T; units += (T + fpw - 1) / fpw; max_len = std::max(max_len, L);
    }
    if (rows > INT32_MAX / 2) { set_error(std::string(who) + ": chunk too large for one launch"); return AFX_ERR_UNSUPPORTED; }

    const size_t o_prs = (size_t)n * sizeof(StftClip);
    up.assign(o_prs + (size_t)n * sizeof(HpssClip), 0);
    std::memcpy(up.data(), recs.data(), o_prs);
    std::memcpy(up.data() + o_prs, prs.data(), (size_t)n * sizeof(HpssClip));
    if ((rc = ensure(ctx->st_recs, up.size())) != AFX_OK) return rc;
    if ((rc = ensure(ctx->st_y, (size_t)std::max<int64_t>(ypos, 1) * sizeof(float))) != AFX_OK) return rc;
    if ((rc = ensure(ctx->st_bad, (size_t)n * sizeof(uint32_t))) != AFX_OK) return rc;
    const void* d_in = samples;
    if (h_in) {
      pieces.clear();
      for (int q = 0; q < n; ++q) pieces.push_back(clip_piece(samples, offsets[ck.idx[q]], prs[q].in_off, prs[q].len, esz));
      if ((rc = stage_in(ctx, image, in_pos * (int64_t)esz, pieces, &d_in)) != AFX_OK) return rc;
    }
    float* d_out;
    if ((rc = out_buffer(ctx, (float*)out, out_mem_kind, std::max<int64_t>(opos * fpe, 1), &d_out)) != AFX_OK) return rc;
    HIP_TRY(hipMemcpyAsync(ctx->st_recs.p, up.data(), up.size(), hipMemcpyHostToDevice, s));
    const StftClip* d_recs = (const StftClip*)ctx->st_recs.p;
    const HpssClip* d_prs = (const HpssClip*)((const char*)ctx->st_recs.p + o_prs);
    float* y = (float*)ctx->st_y.p;
    uint32_t* bad = (uint32_t*)ctx->st_bad.p;
    HIP_TRY(hipMemsetAsync(bad, 0, (size_t)n * sizeof(uint32_t), s));
    HIP_TRY(launch_hpss_prep(s, d_in, sample_fmt, 0, 0.f, d_prs, n, max_len, y, bad));
    HIP_TRY(launch_stft_frames(s, o, y, d_recs, bad, n, units, tb, d_out));
    h_bad.resize((size_t)n);
    HIP_TRY(hipMemcpyAsync(h_bad.data(), bad, h_bad.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    if (h_out && (rc = fetch_out(ctx, d_out, opos * fpe, stage_out)) != AFX_OK) return rc;
    HIP_TRY(hipStreamSynchronize(s));
    pieces.clear();
    for (int q = 0; q < n; ++q) {
      const int i = ck.idx[q];
      if (h_bad[q]) out_status[i] = AFX_CLIP_NONFINITE;
      if (h_out) pieces.push_back({stage_out.data() + recs[q].out_off * fpe, out_offsets[i] * 4 * fpe, frames[i] * bins * 4 * fpe});
    }
    scatter_pieces(out, pieces);
  }
  return AFX_OK;
}

// A chunk (cut_stft_chunk over istft_weight per clip): the kept rows staged packed when they are the host's, the records
// uploaded, k_istft_frames into the time rows, k_istft_ola into the caller's device memory or the packed image.
extern "C" int afx_istft_batch(afx_ctx* ctx, const void* spec, int mem_kind,
                               const int64_t* spec_offsets, const int64_t* n_frames, int n_clips,
                               const afx_stft_opts* opts, const float* window, const int64_t* lengths,
                               float* out, int out_mem_kind, const int64_t* out_offsets, int32_t* out_status) {
  const char* who = "afx_istft_batch";
  int rc;
  if ((rc = clip_batch_args(who, ctx, AFX_FMT_F32, mem_kind, spec_offsets, n_frames, n_clips, out_mem_kind, out_offsets, out_status,
                            opts && window)) != AFX_OK) return rc;
  if (!opts || !window) return null_arg(who);
  if ((rc = stft_opts_arg(who, opts)) != AFX_OK) return rc;
  const afx_stft_opts o = *opts;
  const int n_fft = o.n_fft, bins = stft_bins(n_fft), fpw = n_fft == 1024 ? 2 : 1;
  std::vector<int64_t> eff((size_t)n_clips), nfs((size_t)n_clips), nout((size_t)n_clips);
  bool any = false;
  for (int i = 0; i < n_clips; ++i) {
    const int64_t want = lengths && lengths[i] >= 0 ? lengths[i] : -1;
    if (want > (int64_t)1 << 31) { set_error(std::string(who) + ": lengths must be at most 2^31"); return AFX_ERR_INVALID; }
    out_status[i] = n_frames[i] == 0 ? AFX_CLIP_TOO_SHORT : AFX_CLIP_OK;
    nfs[i] = nout[i] = 0;
    if (out_status[i] == AFX_CLIP_OK) istft_samples(o, n_frames[i], want, &nfs[i], &nout[i]);
    eff[i] = nout[i] > 0 ? istft_weight(o, nfs[i], nout[i]) : 0;           // nothing to write: nothing to run
    any = any || eff[i] > 0;
  }
  if (!any) return AFX_OK;
  if (!spec || !out) { set_error(std::string(who) + ": null spec / out"); return AFX_ERR_INVALID; }

  (void)hipGetLastError();
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  StftTabs tb{};
  if ((rc = stft_tables(ctx, n_fft, window, tb)) != AFX_OK) return rc;

  const bool h_in = mem_kind == AFX_MEM_HOST, h_out = out_mem_kind == AFX_MEM_HOST;
  StftCost cost;
  stft_cost(o, AFX_FMT_F32, mem_kind, out_mem_kind, 1, cost);
  StftChunk ck;
  std::vector<IstftClip> recs;
  std::vector<HostPiece> pieces;
  std::vector<char> image;
  std::vector<float> stage_out;
  for (int c0 = 0; c0 < n_clips; c0 = ck.next) {
    cut_stft_chunk(spec_offsets, eff.data(), n_clips, c0, dev_env().stft_budget, cost, ck);
    const int n = (int)ck.idx.size();
    if (n == 0) continue;
    recs.assign((size_t)n, IstftClip{});
    int64_t in_pos = 0, opos = 0, rows = 0, units = 0, max_out = 0;
    for (int q = 0; q < n; ++q) {
      const int i = ck.idx[q];
      IstftClip& r = recs[q];
      r.spec_off = h_in ? in_pos : spec_offsets[i]; r.row_base = rows; r.unit_base = units;
      r.out_off = h_out ? opos : out_offsets[i]; r.n_out = nout[i]; r.n_frames = (int32_t)nfs[i];
      in_pos += nfs[i] * bins; opos += (nout[i] + 3) / 4 * 4;
      rows += nfs[i]; units += (nfs[i] + fpw - 1) / fpw; max_out = std::max(max_out, nout[i]);
    }
    if (rows > INT32_MAX / 2) { set_error(std::string(who) + ": chunk too large for one launch"); return AFX_ERR_UNSUPPORTED; }
    if ((rc = ensure(ctx->st_recs, (size_t)n * sizeof(IstftClip))) != AFX_OK) return rc;
    if ((rc = ensure(ctx->st_rows, (size_t)std::max<int64_t>(rows, 1) * n_fft * sizeof(float))) != AFX_OK) return rc;
    const void* d_in = spec;
    if (h_in) {
      pieces.clear();
      for (int q = 0; q < n; ++q) pieces.push_back(clip_piece(spec, spec_offsets[ck.idx[q]], recs[q].spec_off, (int64_t)recs[q].n_frames * bins, 8));
      if ((rc = stage_in(ctx, image, in_pos * 8, pieces, &d_in)) != AFX_OK) return rc;
    }
    float* d_out;
    if ((rc = out_buffer(ctx, out, out_mem_kind, std::max<int64_t>(opos, 1), &d_out)) != AFX_OK) return rc;
    HIP_TRY(hipMemcpyAsync(ctx->st_recs.p, recs.data(), (size_t)n * sizeof(IstftClip), hipMemcpyHostToDevice, s));
    const IstftClip* d_recs = (const IstftClip*)ctx->st_recs.p;
    float* trows = (float*)ctx->st_rows.p;
    HIP_TRY(launch_istft_frames(s, n_fft, (const float2*)d_in, d_recs, n, units, tb, trows));
    HIP_TRY(launch_istft_ola(s, o, trows, d_recs, n, max_out, tb, d_out));
    if (h_out && (rc = fetch_out(ctx, d_out, opos, stage_out)) != AFX_OK) return rc;
    HIP_TRY(hipStreamSynchronize(s));
    pieces.clear();
    for (int q = 0; q < n; ++q)
      if (h_out) pieces.push_back({stage_out.data() + recs[q].out_off, out_offsets[ck.idx[q]] * 4, recs[q].n_out * 4});
    scatter_pieces(out, pieces);
  }
  return AFX_OK;
}

// ---- librosa-style phase_vocoder and effects.time_stretch ------------------------------------------------------------------
static int pvoc_rates_arg(const char* who, const double* rates, int n_clips) {
  for (int i = 0; i < n_clips; ++i)
    if (!pvoc_rate_ok(rates[i])) { set_error(std::string(who) + ": clip " + std::to_string(i) + ": rate must be finite and > 0"); return AFX_ERR_INVALID; }
  return AFX_OK;
}

// The planes of a chunk's vocoder passes: angle and magnitude per input element, a sum per tile and bin
static int pvoc_planes(afx_ctx* ctx, int bins, int64_t rows, int64_t tiles) {
  int rc;
  if ((rc = ensure(ctx->pv_ang, (size_t)std::max<int64_t>(rows, 1) * bins * sizeof(double))) != AFX_OK) return rc;
  if ((rc = ensure(ctx->pv_mag, (size_t)std::max<int64_t>(rows, 1) * bins * sizeof(float))) != AFX_OK) return rc;
  return ensure(ctx->pv_sum, (size_t)std::max<int64_t>(tiles, 1) * bins * sizeof(double));
}

// k_pvoc_prep, k_pvoc_tiles, k_pvoc_carry, k_pvoc_apply over the n clips of a chunk
static int pvoc_passes(afx_ctx* ctx, int n_fft, int hop, const float2* spec, const PvocClip* d_recs, int n, int64_t rows,
                       int64_t tiles, uint32_t* bad, float2* out) {
  hipStream_t s = ctx->stream;
  const int bins = stft_bins(n_fft);
  double *ang = (double*)ctx->pv_ang.p, *sums = (double*)ctx->pv_sum.p;
  float* mag = (float*)ctx->pv_mag.p;
  HIP_TRY(launch_pvoc_prep(s, bins, spec, d_recs, n, rows, ang, mag, bad));
  HIP_TRY(launch_pvoc_tiles(s, n_fft, hop, d_recs, n, tiles, ang, sums));
  HIP_TRY(launch_pvoc_carry(s, bins, d_recs, n, ang, sums));
  HIP_TRY(launch_pvoc_apply(s, n_fft, hop, d_recs, n, tiles, ang, mag, sums, bad, out));
  return AFX_OK;
}

// A chunk (cut_stft_chunk with the record of pvoc_cost over rows in + rows out): the rows staged packed when they are the
// host's, the records uploaded, the four passes into the caller's device memory or into the packed image that goes home.
extern "C" int afx_pvoc_batch(afx_ctx* ctx, const void* spec, int mem_kind, const int64_t* spec_offsets, const int64_t* n_frames,
                              const double* rates, int n_clips, int n_fft, int hop,
                              void* out, int out_mem_kind, const int64_t* out_offsets, int32_t* out_status) {
  const char* who = "afx_pvoc_batch";
  int rc;
  if ((rc = clip_batch_args(who, ctx, AFX_FMT_F32, mem_kind, spec_offsets, n_frames, n_clips, out_mem_kind, out_offsets, out_status,
                            rates != nullptr)) != AFX_OK) return rc;
  if ((rc = pvoc_rates_arg(who, rates, n_clips)) != AFX_OK) return rc;
  const char* why = "";
  if ((rc = pvoc_check(n_fft, hop, &why)) != AFX_OK) { set_error(std::string(who) + ": " + why); return rc; }
  const int bins = stft_bins(n_fft);
  std::vector<int64_t> eff((size_t)n_clips), tout((size_t)n_clips);
  bool any = false;
  for (int i = 0; i < n_clips; ++i) {
    out_status[i] = n_frames[i] == 0 ? AFX_CLIP_TOO_SHORT : AFX_CLIP_OK;
    tout[i] = eff[i] = 0;
    if (out_status[i] != AFX_CLIP_OK) continue;
    if (!pvoc_frames(n_fft, n_frames[i], rates[i], &tout[i])) {
      set_error(std::string(who) + ": clip " + std::to_string(i) + ": T_out x bins must be below 2^31");
      return AFX_ERR_UNSUPPORTED;
    }
    eff[i] = pvoc_weight(n_frames[i], tout[i]);
    any = true;
  }
  if (!any) return AFX_OK;
  if (!spec || !out) { set_error(std::string(who) + ": null spec / out"); return AFX_ERR_INVALID; }

  (void)hipGetLastError();
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const bool h_in = mem_kind == AFX_MEM_HOST, h_out = out_mem_kind == AFX_MEM_HOST;
  StftCost cost;
  pvoc_cost(n_fft, mem_kind, out_mem_kind, cost);
  StftChunk ck;
  std::vector<PvocClip> recs;
  std::vector<HostPiece> pieces;
  std::vector<char> image;
  std::vector<uint32_t> h_bad;
  std::vector<float> stage_out;
  for (int c0 = 0; c0 < n_clips; c0 = ck.next) {
    cut_stft_chunk(spec_offsets, eff.data(), n_clips, c0, dev_env().stft_budget, cost, ck);
    const int n = (int)ck.idx.size();
    if (n == 0) continue;
    recs.assign((size_t)n, PvocClip{});
    int64_t in_pos = 0, opos = 0, rows = 0, tiles = 0;
    for (int q = 0; q < n; ++q) {
      const int i = ck.idx[q];
      PvocClip& r = recs[q];
      r.spec_off = h_in ? in_pos : spec_offsets[i]; r.row_base = rows; r.out_off = h_out ? opos : out_offsets[i];
      r.tile_base = tiles; r.rate = rates[i]; r.T = (int32_t)n_frames[i]; r.T_out = (int32_t)tout[i]; r.clip = q;
      in_pos += n_frames[i] * bins; opos += tout[i] * bins; rows += n_frames[i]; tiles += (tout[i] + kPvocTile - 1) / kPvocTile;
    }
    if (rows > INT32_MAX / 2 || tiles > INT32_MAX / 2) { set_error(std::string(who) + ": chunk too large for one launch"); return AFX_ERR_UNSUPPORTED; }
    if ((rc = ensure(ctx->pv_recs, (size_t)n * sizeof(PvocClip))) != AFX_OK) return rc;
    if ((rc = ensure(ctx->pv_bad, (size_t)n * sizeof(uint32_t))) != AFX_OK) return rc;
    if ((rc = pvoc_planes(ctx, bins, rows, tiles)) != AFX_OK) return rc;
    const void* d_in = spec;
    if (h_in) {
      pieces.clear();
      for (int q = 0; q < n; ++q) pieces.push_back(clip_piece(spec, spec_offsets[ck.idx[q]], recs[q].spec_off, (int64_t)recs[q].T * bins, 8));
      if ((rc = stage_in(ctx, image, in_pos * 8, pieces, &d_in)) != AFX_OK) return rc;
    }
    float* d_out;
    if ((rc = out_buffer(ctx, (float*)out, out_mem_kind, std::max<int64_t>(opos * 2, 1), &d_out)) != AFX_OK) return rc;
    HIP_TRY(hipMemcpyAsync(ctx->pv_recs.p, recs.data(), (size_t)n * sizeof(PvocClip), hipMemcpyHostToDevice, s));
    uint32_t* bad = (uint32_t*)ctx->pv_bad.p;
    HIP_TRY(hipMemsetAsync(bad, 0, (size_t)n * sizeof(uint32_t), s));
    if ((rc = pvoc_passes(ctx, n_fft, hop, (const float2*)d_in, (const PvocClip*)ctx->pv_recs.p, n, rows, tiles, bad, (float2*)d_out)) != AFX_OK) return rc;
    h_bad.resize((size_t)n);
    HIP_TRY(hipMemcpyAsync(h_bad.data(), bad, h_bad.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    if (h_out && (rc = fetch_out(ctx, d_out, opos * 2, stage_out)) != AFX_OK) return rc;
    HIP_TRY(hipStreamSynchronize(s));
    pieces.clear();
    for (int q = 0; q < n; ++q) {
      const int i = ck.idx[q];
      if (h_bad[q]) out_status[i] = AFX_CLIP_NONFINITE;
      if (h_out) pieces.push_back({stage_out.data() + recs[q].out_off * 2, out_offsets[i] * 8, tout[i] * bins * 8});
    }
    scatter_pieces(out, pieces);
  }
  return AFX_OK;
}

// A chunk (cut_stft_chunk with the record of stretch_cost over stretch_weight): afx_stft_batch's launches into a spectrum
// that stays in the workspace, the vocoder's four passes over it, afx_istft_batch's two launches on the vocoded rows -- the
// same kernels on the same records as the three entry points, so the same bits.
extern "C" int afx_time_stretch_batch(afx_ctx* ctx, const void* samples, int sample_fmt, int mem_kind,
                                      const int64_t* offsets, const int64_t* lengths, const double* rates, int n_clips,
                                      const afx_stft_opts* opts, const float* window,
                                      float* out, int out_mem_kind, const int64_t* out_offsets, int32_t* out_status) {
  const char* who = "afx_time_stretch_batch";
  int rc;
  if ((rc = clip_batch_args(who, ctx, sample_fmt, mem_kind, offsets, lengths, n_clips, out_mem_kind, out_offsets, out_status,
                            opts && window && rates)) != AFX_OK) return rc;
  if (!opts || !window) return null_arg(who);
  if ((rc = pvoc_rates_arg(who, rates, n_clips)) != AFX_OK) return rc;
  if ((rc = stft_opts_arg(who, opts)) != AFX_OK) return rc;
  afx_stft_opts o = *opts;
  o.out_kind = AFX_STFT_COMPLEX;
  const int n_fft = o.n_fft, bins = stft_bins(n_fft), fpw = n_fft == 1024 ? 2 : 1;
  std::vector<int64_t> eff((size_t)n_clips), frames((size_t)n_clips), tout((size_t)n_clips), nfs((size_t)n_clips), nout((size_t)n_clips);
  bool any = false;
  for (int i = 0; i < n_clips; ++i) {
    stft_frames(o, lengths[i], &frames[i], &out_status[i]);
    eff[i] = tout[i] = nfs[i] = nout[i] = 0;
    if (out_status[i] != AFX_CLIP_OK) continue;
    if (!stretch_length(lengths[i], rates[i], &nout[i])) {
      set_error(std::string(who) + ": clip " + std::to_string(i) + ": length / rate must be at most 2^31");
      return AFX_ERR_INVALID;
    }
    if (!pvoc_frames(n_fft, frames[i], rates[i], &tout[i])) {
      set_error(std::string(who) + ": clip " + std::to_string(i) + ": T_out x bins must be below 2^31");
      return AFX_ERR_UNSUPPORTED;
    }
    if (nout[i] == 0) continue;                                  // nothing to write: nothing to run
    int64_t n_out = 0;
    istft_samples(o, tout[i], nout[i], &nfs[i], &n_out);
    eff[i] = stretch_weight(o, lengths[i], frames[i], tout[i], nout[i]);
    any = true;
  }
  if (!any) return AFX_OK;
  if (!samples || !out) { set_error(std::string(who) + ": null samples / out"); return AFX_ERR_INVALID; }

  (void)hipGetLastError();
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  StftTabs tb{};
  if ((rc = stft_tables(ctx, n_fft, window, tb)) != AFX_OK) return rc;

  const size_t esz = sample_fmt == AFX_FMT_S16 ? 2 : 4;
  const bool h_in = mem_kind == AFX_MEM_HOST, h_out = out_mem_kind == AFX_MEM_HOST;
  StftCost cost;
  stretch_cost(o, sample_fmt, mem_kind, out_mem_kind, cost);
  StftChunk ck;
  std::vector<StftClip> fwd;
  std::vector<HpssClip> prs;
  std::vector<PvocClip> pvs;
  std::vector<IstftClip> inv;
  std::vector<HostPiece> pieces;
  std::vector<char> image, up;
  std::vector<uint32_t> h_bad;
  std::vector<float> stage_out;
  for (int c0 = 0; c0 < n_clips; c0 = ck.next) {
    cut_stft_chunk(offsets, eff.data(), n_clips, c0, dev_env().stft_budget, cost, ck);
    const int n = (int)ck.idx.size();
    if (n == 0) continue;
    fwd.assign((size_t)n, StftClip{}); prs.assign((size_t)n, HpssClip{}); pvs.assign((size_t)n, PvocClip{}); inv.assign((size_t)n, IstftClip{});
    int64_t ypos = 0, in_pos = 0, dpos = 0, ppos = 0, opos = 0, rows = 0, units = 0, tiles = 0, irows = 0, iunits = 0, max_len = 0, max_out = 0;
    for (int q = 0; q < n; ++q) {
      const int i = ck.idx[q];
      const int64_t L = lengths[i], T = frames[i], nf = nfs[i];
      StftClip& f = fwd[q];
      f.y_off = ypos; f.len = L; f.out_off = dpos; f.unit_base = units; f.T = (int32_t)T; f.clip = q;
      prs[q].in_off = h_in ? in_pos : offsets[i]; prs[q].y_off = ypos; prs[q].len = L;
      PvocClip& p = pvs[q];                                      // only the rows istft keeps are made
      p.spec_off = dpos; p.row_base = rows; p.out_off = ppos; p.tile_base = tiles; p.rate = rates[i]; p.T = (int32_t)T; p.T_out = (int32_t)nf; p.clip = q;
      IstftClip& r = inv[q];
      r.spec_off = ppos; r.row_base = irows; r.unit_base = iunits; r.out_off = h_out ? opos : out_offsets[i]; r.n_out = nout[i]; r.n_frames = (int32_t)nf;
      ypos += (L + 3) / 4 * 4; in_pos += (L + 3) / 4 * 4; dpos += T * bins; ppos += nf * bins; opos += (nout[i] + 3) / 4 * 4;
      rows += T; units += (T + fpw - 1) / fpw; tiles += (nf + kPvocTile - 1) / kPvocTile; irows += nf; iunits += (nf + fpw - 1) / fpw;
      max_len = std::max(max_len, L); max_out = std::max(max_out, nout[i]);
    }
    if (rows > INT32_MAX / 2 || irows > INT32_MAX / 2 || tiles > INT32_MAX / 2) { set_error(std::string(who) + ": chunk too large for one launch"); return AFX_ERR_UNSUPPORTED; }

    const size_t o_prs = (size_t)n * sizeof(StftClip), o_pvs = o_prs + (size_t)n * sizeof(HpssClip), o_inv = o_pvs + (size_t)n * sizeof(PvocClip);
    up.assign(o_inv + (size_t)n * sizeof(IstftClip), 0);
    std::memcpy(up.data(), fwd.data(), o_prs);
    std::memcpy(up.data() + o_prs, prs.data(), (size_t)n * sizeof(HpssClip));
    std::memcpy(up.data() + o_pvs, pvs.data(), (size_t)n * sizeof(PvocClip));
    std::memcpy(up.data() + o_inv, inv.data(), (size_t)n * sizeof(IstftClip));
    if ((rc = ensure(ctx->pv_recs, up.size())) != AFX_OK) return rc;
    if ((rc = ensure(ctx->pv_bad, (size_t)n * sizeof(uint32_t))) != AFX_OK) return rc;
    if ((rc = ensure(ctx->st_y, (size_t)std::max<int64_t>(ypos, 1) * sizeof(float))) != AFX_OK) return rc;
    if ((rc = ensure(ctx->pv_spec, (size_t)std::max<int64_t>(dpos, 1) * 8)) != AFX_OK) return rc;
    if ((rc = ensure(ctx->pv_out, (size_t)std::max<int64_t>(ppos, 1) * 8)) != AFX_OK) return rc;
    if ((rc = ensure(ctx->st_rows, (size_t)std::max<int64_t>(irows, 1) * n_fft * sizeof(float))) != AFX_OK) return rc;
    if ((rc = pvoc_planes(ctx, bins, rows, tiles)) != AFX_OK) return rc;
    const void* d_in = samples;
    if (h_in) {
      pieces.clear();
      for (int q = 0; q < n; ++q) pieces.push_back(clip_piece(samples, offsets[ck.idx[q]], prs[q].in_off, prs[q].len, esz));
      if ((rc = stage_in(ctx, image, in_pos * (int64_t)esz, pieces, &d_in)) != AFX_OK) return rc;
    }
    float* d_out;
    if ((rc = out_buffer(ctx, out, out_mem_kind, std::max<int64_t>(opos, 1), &d_out)) != AFX_OK) return rc;
    HIP_TRY(hipMemcpyAsync(ctx->pv_recs.p, up.data(), up.size(), hipMemcpyHostToDevice, s));
    const char* base = (const char*)ctx->pv_recs.p;
    const StftClip* d_fwd = (const StftClip*)base;
    const HpssClip* d_prs = (const HpssClip*)(base + o_prs);
    const PvocClip* d_pvs = (const PvocClip*)(base + o_pvs);
    const IstftClip* d_inv = (const IstftClip*)(base + o_inv);
    float* y = (float*)ctx->st_y.p;
    uint32_t* bad = (uint32_t*)ctx->pv_bad.p;
    float2 *D = (float2*)ctx->pv_spec.p, *P = (float2*)ctx->pv_out.p;
    float* trows = (float*)ctx->st_rows.p;
    HIP_TRY(hipMemsetAsync(bad, 0, (size_t)n * sizeof(uint32_t), s));
    HIP_TRY(launch_hpss_prep(s, d_in, sample_fmt, 0, 0.f, d_prs, n, max_len, y, bad));
    HIP_TRY(launch_stft_frames(s, o, y, d_fwd, bad, n, units, tb, D));
    if ((rc = pvoc_passes(ctx, n_fft, o.hop, D, d_pvs, n, rows, tiles, bad, P)) != AFX_OK) return rc;
    HIP_TRY(launch_istft_frames(s, n_fft, P, d_inv, n, iunits, tb, trows));
    HIP_TRY(launch_istft_ola(s, o, trows, d_inv, n, max_out, tb, d_out));
    h_bad.resize((size_t)n);
    HIP_TRY(hipMemcpyAsync(h_bad.data(), bad, h_bad.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    if (h_out && (rc = fetch_out(ctx, d_out, opos, stage_out)) != AFX_OK) return rc;
    HIP_TRY(hipStreamSynchronize(s));
    pieces.clear();
    for (int q = 0; q < n; ++q) {
      const int i = ck.idx[q];
      if (h_bad[q]) out_status[i] = AFX_CLIP_NONFINITE;
      if (h_out) pieces.push_back({stage_out.data() + inv[q].out_off, out_offsets[i] * 4, inv[q].n_out * 4});
    }
    scatter_pieces(out, pieces);
  }
  return AFX_OK;
}
