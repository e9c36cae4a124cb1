/*
 * afx.h -- C ABI of libafx.so, the MI355X (gfx950) MFCC / RMS engine.
 *
 * The reference (chiy48308/audio_feature_extraction) has no FFI: its hot path is
 * three Python methods that call librosa.  This header is the seam a maintainer
 * binds with ctypes; each entry point names the reference
 * call(s) it replaces.  Paths are relative to the reference root,
 *   F = audio_feature_extraction_toolkit/core/feature_extractor.py
 *
 * Conventions
 *   - plain C, plain pointers and sizes, no torch / HIP types in signatures;
 *   - every function returns 0 (AFX_OK) or a negative afx_status; nothing throws
 *     across the ABI; afx_last_error() gives the text of the last failure on the
 *     calling thread;
 *   - the caller owns every buffer it passes; the library never frees them;
 *   - an afx_ctx is bound to one HIP device and owns one stream; it is not
 *     thread-safe -- use one ctx per worker thread (one per GPU);
 *   - all entry points are synchronous on return, except afx_extract_submit (its results are
 *     handed out by afx_extract_collect);
 *   - a per-clip failure is reported in out_status[] and never fails the batch
 *     (maps onto batch_process's per-file try/except, F:229-235).
 */
#ifndef AFX_H
#define AFX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AFX_VERSION 107      /* 107: afx_resample_design, afx_resample_batch; 106: afx_hpss_batch; 105: afx_dtw_batch; 104: afx_batch_geometry, afx_host_alloc / afx_host_free */

typedef enum afx_status {
  AFX_OK = 0,
  AFX_ERR_INVALID = -1,     /* bad argument / unsupported parameter combination */
  AFX_ERR_NO_DEVICE = -2,   /* no usable HIP device */
  AFX_ERR_HIP = -3,         /* a HIP runtime call or kernel launch failed */
  AFX_ERR_NOMEM = -4,
  AFX_ERR_UNSUPPORTED = -5  /* e.g. n_fft outside the supported set (see afx_rfft_host) */
} afx_status;

/* per-clip status written to out_status[] */
typedef enum afx_clip_status {
  AFX_CLIP_OK = 0,
  AFX_CLIP_TOO_SHORT = 1,  /* fewer than delta_width frames, or < 2 samples:
                              librosa.feature.delta raises ParameterError (F:137) */
  AFX_CLIP_NONFINITE = 2   /* NaN/Inf sample: librosa.util.valid_audio raises */
} afx_clip_status;

/* per-pair status of afx_dtw_batch */
typedef enum afx_dtw_status {
  AFX_DTW_OK = 0,
  AFX_DTW_NONFINITE = 1,   /* NaN / inf feature, or a zero-norm frame under AFX_DTW_COSINE (librosa raises) */
  AFX_DTW_NO_PATH = 2      /* D[N-1, M-1] (subseq: all of row N-1) is inf: the band or the step list admits no path */
} afx_dtw_status;

/* local cost of afx_dtw_batch: scipy.spatial.distance.cdist's metrics of the same names */
enum { AFX_DTW_EUCLIDEAN = 0, AFX_DTW_SQEUCLIDEAN = 1, AFX_DTW_COSINE = 2 };
/* flags for afx_dtw_batch */
enum { AFX_DTW_BACKTRACK = 1, AFX_DTW_STORE_D = 2, AFX_DTW_SUBSEQ = 4 /* afx_dtw_steps_batch only */ };
/* afx_hpss_batch: with the AFX_FLAG_* bits, the debug output of the median stage */
enum { AFX_HPSS_STORE_SPEC = 4 };

enum { AFX_WINDOW_HAMMING = 0, AFX_WINDOW_HANN = 1 };
enum { AFX_FMT_F32 = 0, AFX_FMT_S16 = 1 };           /* S16: value / 32768 (libsndfile) */
enum { AFX_MEM_HOST = 0, AFX_MEM_DEVICE = 1 };

/* flags for afx_extract_batch */
enum {
  AFX_FLAG_PREEMPH = 1,    /* apply pre-emphasis (F:69); off for extract_mfcc(y)/extract_energy(y) */
  AFX_FLAG_TRIM = 2        /* apply silence trim (F:72) */
};

/* Constructor arguments of AudioFeatureExtractor (F:10-17) plus the values the
 * reference hard-codes at its librosa call sites. */
typedef struct afx_params {
  int32_t sr;            /* F:11  */
  int32_t n_fft;         /* frame_length, F:12 -> n_fft of librosa.feature.mfcc (F:131) */
  int32_t hop;           /* F:13  */
  int32_t n_mfcc;        /* F:14  */
  int32_t n_mels;        /* librosa default 128 (the reference never passes it) */
  int32_t window;        /* AFX_WINDOW_HAMMING: F:133 */
  float   preemph;       /* F:17, 0.97 */
  float   trim_top_db;   /* 30, F:72 */
  int32_t trim_frame;    /* 2048, librosa.effects.trim default */
  int32_t trim_hop;      /* 512 */
  float   top_db;        /* 80, librosa.power_to_db default */
  float   amin;          /* 1e-10 */
  int32_t delta_width;   /* 9, librosa.feature.delta default */
  int32_t reserved;
  /* mel / MFCC option variants the reference's experiment extractors pass to librosa.filters.mel and
   * librosa.feature.mfcc (04_feature_extraction_experiment/audio_feature_extraction 2/audio_feature_extraction/
   * feature_extractor.py:148-181); the packaged class passes none, i.e. the defaults below */
  float   fmin;          /* 0: lowest mel band edge, Hz */
  float   fmax;          /* 0 = sr / 2: highest band edge, Hz */
  int32_t htk;           /* 0: Slaney mel scale; 1: HTK formula */
  float   lifter;        /* 0: none; L > 0: coefficient n (1-based) scaled by 1 + (L / 2) sin(pi n / L) */
} afx_params;

typedef struct afx_ctx afx_ctx;
typedef struct afx_plan afx_plan;

/* ---- library / device ---------------------------------------------------- */
int afx_version(void);
int afx_device_count(void);                       /* 0 when no GPU is visible */
const char* afx_last_error(void);                 /* thread-local, never NULL */

int afx_init(int device, afx_ctx** out);          /* binds device, creates the stream */
void afx_destroy(afx_ctx* ctx);

/* device memory helpers so that a binding needs no HIP API of its own */
int afx_malloc(afx_ctx* ctx, size_t bytes, void** out_dptr);
int afx_free(afx_ctx* ctx, void* dptr);
/* Page-locked host memory for batch buffers that are uploaded (batch_process packs a window of decoded files into one,
 * F:228-235): afx_memcpy_h2d from it is one DMA at link rate, from pageable memory the runtime stages it through its own
 * pinned buffer first (a host copy at a fifth of that).  Free with afx_host_free before afx_destroy. */
int afx_host_alloc(afx_ctx* ctx, size_t bytes, void** out);
int afx_host_free(afx_ctx* ctx, void* hptr);
int afx_memcpy_h2d(afx_ctx* ctx, void* dst_d, const void* src_h, size_t bytes);
int afx_memcpy_d2h(afx_ctx* ctx, void* dst_h, const void* src_d, size_t bytes);
int afx_synchronize(afx_ctx* ctx);

/* ---- plan: window / twiddle / sparse-mel / DCT tables for one parameter set  */
void afx_default_params(afx_params* p);           /* reference defaults (F:10-17, F:72, F:133) */
int afx_plan_create(afx_ctx* ctx, const afx_params* p, afx_plan** out);
void afx_plan_destroy(afx_plan* plan);

/* Host-only table builders (no device needed) -- what afx_plan_create uploads.
 * window[n_fft]; mel_dense[n_mels * (n_fft/2+1)] row-major (librosa.filters.mel
 * float32 values); dct[n_mfcc * n_mels] (ortho DCT-II rows).  Any pointer may be
 * NULL.  Replaces scipy.signal.get_window / librosa.filters.mel / scipy.fft.dct
 * table construction under librosa.feature.mfcc (F:127). */
int afx_build_tables(const afx_params* p, float* window, float* mel_dense, float* dct);

/* Host-only: the mel schedule of the wave-level frame kernel (k_frames3), for inspection and tests.
 * One frame pair at a time, a lane accumulates 4 * nb consecutive taps of one filter of librosa.filters.mel
 * (F:127); `width` adjacent lanes share a filter.  info[26] = rounds, weight floats, then per round (8 slots)
 * nb, width, weight offset; weights[info[1]] as [round][batch][lane][4]; meta[64 * rounds] per lane:
 * first bin | filter << 11 | owner << 20.  Any pointer may be NULL.  AFX_ERR_UNSUPPORTED when the
 * configuration has no such schedule. */
int afx_build_mel_schedule(const afx_params* p, int32_t* info, float* weights, int32_t* meta);

/* Host-only: the frame geometry of a ragged batch, as every batch entry point lays it out (batch_process hands over
 * files of any length, F:228-235).  records[4 * n_clips]: per clip the first frame slot, Tmax = 1 + length / hop, Tmax
 * padded to whole 16-frame blocks, first block index; totals[4]: frame slots, 16-frame blocks, trim blocks, largest
 * Tmax.  Either pointer may be NULL.  AFX_ERR_INVALID for negative or oversized offsets / lengths (the same check the
 * batch entry points make before anything is uploaded). */
int afx_batch_geometry(const afx_params* p, const int64_t* offsets, const int64_t* lengths, int n_clips,
                       int64_t* records, int64_t* totals);

/* ---- the hot path ---------------------------------------------------------
 * One pass of preprocess_audio -> extract_mfcc + extract_energy (F:194,198,199)
 * over a ragged batch of clips.
 *
 *   samples   packed clips (AFX_FMT_F32 float or AFX_FMT_S16 int16_t), in host
 *             or device memory (mem_kind); clip i is
 *             samples[offsets[i] .. offsets[i]+lengths[i])  (element units)
 *   offsets, lengths   host arrays, n_clips entries
 *   flags     AFX_FLAG_PREEMPH | AFX_FLAG_TRIM for extract_features semantics
 *   out_stats host, n_clips * (4*n_mfcc + 3) floats per clip:
 *             mfcc_mean[K] mfcc_std[K] mfcc_delta_mean[K] mfcc_delta2_mean[K]
 *             energy_mean energy_std energy_range        (F:141-150, F:171-178)
 *             A clip whose status is AFX_CLIP_TOO_SHORT because it has fewer than nine frames (the
 *             width-9 delta of F:137 cannot be formed) but at least two samples still has its three
 *             energy statistics, on every plan shape: extract_energy (F:153-179) only calls
 *             librosa.feature.rms.  Its MFCC entries are zero.  Every other non-OK clip: all zero.
 *   out_status host int32[n_clips]  (afx_clip_status)
 *   out_trim  host int64[2*n_clips] (start, end) of the kept span, or NULL
 *   out_nframes host int32[n_clips] T = 1 + (end-start)/hop, or NULL
 *   out_frames  NULL, or host float buffer for the per-frame matrices the
 *             reference computes and then reduces (F:127-138, F:164): clip i
 *             occupies rows of stride Tmax_i = 1 + lengths[i]/hop starting at
 *             float index frame_offsets[i]: (3*n_mfcc + 1) rows
 *             [mfcc K | delta K | delta2 K | rms 1], first T_i entries valid.
 *   frame_offsets host int64[n_clips] (ignored when out_frames is NULL)
 */
int afx_extract_batch(afx_plan* plan,
                      const void* samples, int sample_fmt, int mem_kind,
                      const int64_t* offsets, const int64_t* lengths, int n_clips,
                      int flags,
                      float* out_stats, int32_t* out_status,
                      int64_t* out_trim, int32_t* out_nframes,
                      float* out_frames, const int64_t* frame_offsets);

/* The same pass in two halves, for callers that keep the device busy across batches (batch_process walks its
 * files in windows, F:204-211): afx_extract_submit queues everything a batch needs -- kernels and the copies of its
 * results -- on the plan's stream and returns; afx_extract_collect waits for THAT batch only and fills the out_*
 * arrays given at submit (which, like `samples`, `offsets` and `lengths`, must stay valid until then).  Two plans of
 * one context submitted alternately from one thread run back to back on the device: the host's share of a batch
 * (collect, hand-out, next submit) falls under the other plan's kernels.  One batch per plan may be pending; n_clips
 * must be in [1, 32768]; afx_extract_batch(plan, ...) == submit + collect per 32768-clip chunk.
 * A batch whose clip offsets / lengths differ from the plan's previous batch costs the host one 48-byte record per
 * clip (pinned staging, asynchronous upload); the per-block work list is built on the device.  No stream
 * synchronisation happens inside submit unless workspace has to grow.  With out_frames given, the copy of the
 * per-frame matrices into the caller's (pageable) buffer is queued by submit and may make it block. */
int afx_extract_submit(afx_plan* plan,
                       const void* samples, int sample_fmt, int mem_kind,
                       const int64_t* offsets, const int64_t* lengths, int n_clips,
                       int flags,
                       float* out_stats, int32_t* out_status,
                       int64_t* out_trim, int32_t* out_nframes,
                       float* out_frames, const int64_t* frame_offsets);
int afx_extract_collect(afx_plan* plan);

/* extract_f0 (F:76-114): librosa.pyin(y, fmin, fmax, frame_length=n_fft, hop_length=hop, sr)
 * at librosa's defaults, of the same preprocessed clips (flags as for
 * afx_extract_batch: the reference feeds y_processed, F:195), reduced as F:97-107.
 *   out_f0stats host double[4 * n_clips]: f0_mean, f0_std, f0_missing_rate, f0_quality
 *             (0, 0, 1, 0 when no frame is voiced -- the reference's own branch F:103-107)
 *   out_status host int32[n_clips]: AFX_CLIP_OK or AFX_CLIP_NONFINITE
 *   out_f0    NULL, or host double buffer: clip i's per-frame f0 (NaN = unvoiced) in
 *             out_f0[f0_offsets[i] .. + T_i), T_i = 1 + kept_length_i / hop; the rest of the clip's
 *             1 + length_i / hop slots (frames trimmed away) is set to NaN
 * Device workspace inside the plan: about 14 KB per frame (the Viterbi value columns, 2 * n_bins
 * doubles per frame, are kept for back-tracking); batches are processed in chunks of at most
 * 1.28 M frames (about 18 GB).
 * Float64 throughout, except the running frame energy, which numpy accumulates in
 * float32 and which is reproduced add for add. */
int afx_f0_batch(afx_plan* plan,
                 const void* samples, int sample_fmt, int mem_kind,
                 const int64_t* offsets, const int64_t* lengths, int n_clips,
                 int flags, double fmin, double fmax,
                 double* out_f0stats, int32_t* out_status,
                 double* out_f0, const int64_t* f0_offsets);

/* Zero-crossing rate per frame of the same preprocessed clips (librosa.feature.zero_crossing_rate with
 * frame_length = n_fft, hop_length = hop, center=True): the frame-level feature the reference's experiment
 * scripts store beside mfcc / f0 / energy (04_feature_extraction_experiment/feature_extraction.py:340-352).
 *   out_zcr   host double buffer: clip i's T_i rates at out_zcr[zcr_offsets[i] ..]; at most 32768 clips per call */
int afx_zcr_batch(afx_plan* plan,
                  const void* samples, int sample_fmt, int mem_kind,
                  const int64_t* offsets, const int64_t* lengths, int n_clips, int flags,
                  double* out_zcr, const int64_t* zcr_offsets, int32_t* out_status);

/* Frame-level spectral descriptors the reference's experiment extractor takes from librosa at its defaults
 * (04_feature_extraction_experiment/feature_extractor.py:497-506: spectral_centroid, spectral_bandwidth,
 * spectral_rolloff, spectral_contrast; n_fft 2048, hop 512, centred, magnitude spectrum) of the given clips
 * (flags: AFX_FLAG_PREEMPH or 0; no trim -- pass the preprocessed signal, as the reference does).  The plan must have
 * n_fft 2048 / hop 512 (the reference calls librosa with its default Hann window: create the plan with AFX_WINDOW_HANN).
 *   out_desc  host float buffer: clip i has T_i = 1 + length_i / 512 rows of 17 floats at out_desc[desc_offsets[i] ..]:
 *             centroid (Hz), bandwidth (Hz, p = 2), rolloff (Hz, 85 %), then per octave band k = 0..6 of
 *             spectral_contrast(fmin = 200, n_bands = 6, quantile = 0.02) the valley[k] (mean of the smallest
 *             magnitudes) and after those the peak[k]; contrast = power_to_db(peak) - power_to_db(valley) with
 *             librosa's clip-global top_db clamp is left to the caller (it needs the maximum over the whole clip).
 *   AFX_ERR_UNSUPPORTED when sr <= 12800 (librosa: "Frequency band exceeds Nyquist") or the plan has another shape. */
int afx_spectral_batch(afx_plan* plan,
                       const void* samples, int sample_fmt, int mem_kind,
                       const int64_t* offsets, const int64_t* lengths, int n_clips, int flags,
                       float* out_desc, const int64_t* desc_offsets, int32_t* out_status);

/* Batched DTW alignment (librosa.sequence.dtw at its defaults: step sizes (1,1), (0,1), (1,0) in that order, the first
 * minimum winning a tie), the step the reference's aligner runs on pairs of MFCC(+delta+delta2) frame matrices
 * (05_dtw_alignment_experiment/dtw_alignment.py:930-970, :1092-1130, :1206-1250).
 *   feats     host float32, frame-major: frame t is feats[t * dim .. t * dim + dim); X and Y of pair p are the frames
 *             x_off[p] .. + x_len[p] and y_off[p] .. + y_len[p] (a teacher shared by many students is held once)
 *   dim       1 .. 128 (AFX_ERR_UNSUPPORTED above); every N * M must be <= 2^31 and N, M <= 2^30
 *             (AFX_ERR_UNSUPPORTED otherwise)
 *   band_r    NULL, or per pair the band radius r = round_half_even(band_rad * min(N, M)) of librosa's
 *             global_constraints (fill_off_diagonal); r < 0: unconstrained
 *   metric    AFX_DTW_EUCLIDEAN / AFX_DTW_SQEUCLIDEAN / AFX_DTW_COSINE, evaluated in float32 from direct differences;
 *             the accumulation is float64
 *   flags     AFX_DTW_BACKTRACK: the warping path; AFX_DTW_STORE_D: the accumulated cost matrix
 *   out_cost  host double[n_pairs]: D[N-1, M-1]   (NaN for a NONFINITE pair, inf for NO_PATH)
 *   out_status host int32[n_pairs]: afx_dtw_status; a failed pair never affects the others
 *   out_path, path_off, out_path_len  (AFX_DTW_BACKTRACK) pair p's path as L int32 (i, j) pairs at
 *             out_path[2 * path_off[p] ..], end to start (wp[0] = (N-1, M-1), wp[L-1] = (0, 0)); N + M - 1 pairs
 *             must be reserved; out_path_len[p] = L (0 for a failed pair)
 *   out_D, d_off  (AFX_DTW_STORE_D) row-major float64 N x M at out_D[d_off[p] ..], inf outside the band
 * The batch runs in chunks whose device workspace (step codes at 2 bits per cell, D when stored, one boundary row per
 * pair) stays within 2 GiB; a pair larger than that runs alone. */
int afx_dtw_batch(afx_ctx* ctx, const float* feats, int dim,
                  const int64_t* x_off, const int64_t* x_len, const int64_t* y_off, const int64_t* y_len,
                  const int32_t* band_r, int n_pairs, int metric, int flags,
                  double* out_cost, int32_t* out_status,
                  int32_t* out_path, const int64_t* path_off, int32_t* out_path_len,
                  double* out_D, const int64_t* d_off);

/* afx_dtw_batch with librosa.sequence.dtw's step_sizes_sigma, weights_add, weights_mul and subseq.  Everything
 * afx_dtw_batch takes means the same; in addition:
 *   steps, n_steps  NULL: the default steps (1,1), (0,1), (1,0), with w_add / w_mul of 3 entries (n_steps is ignored).
 *             Otherwise int32[n_steps][2], the caller's (di, dj) list: 1 .. 5 steps, components 0 .. 2
 *             (AFX_ERR_UNSUPPORTED above either), no negative component and no (0, 0) (AFX_ERR_INVALID).  As in librosa
 *             the list follows the three defaults, whose inf weights never win: the recorded step indices start at 3.
 *             The list [(1,1)] alone needs N <= M for every pair (AFX_ERR_INVALID, as librosa raises).
 *   w_add, w_mul  NULL (zeros / ones), or one double per step: candidate = D[i-di, j-dj] + (w_mul * C[i, j] + w_add), the
 *             multiply and the add both rounded to float64, compared in list order with a strict <.  Negative, NaN and inf
 *             weights are AFX_ERR_INVALID.
 *   flags     also AFX_DTW_SUBSEQ: row 0 of D is seeded with C[0, :], the path ends at (N-1, j*) with j* the first argmin
 *             of D[N-1, :] and is walked back to the first cell of row 0.  X is aligned inside Y as given: librosa's
 *             swap for N > M is the caller's.
 *   out_cost  D[N-1, M-1], or D[N-1, j*] under AFX_DTW_SUBSEQ
 *   out_end   NULL, or host int32[n_pairs]: j* (M - 1 without AFX_DTW_SUBSEQ; -1 for a NONFINITE pair)
 * Argument errors are reported before any device work.  Step codes take 4 bits per cell and a pair has two boundary
 * rows; the chunks are cut with those sizes.  A call with steps == NULL, unit weights and no AFX_DTW_SUBSEQ computes what
 * afx_dtw_batch computes, with this entry point's kernel.  Newer than AFX_VERSION 107 says: a binding detects it by its
 * presence. */
int afx_dtw_steps_batch(afx_ctx* ctx, const float* feats, int dim,
                        const int64_t* x_off, const int64_t* x_len, const int64_t* y_off, const int64_t* y_len,
                        const int32_t* band_r, int n_pairs, int metric, int flags,
                        const int32_t* steps, int n_steps, const double* w_add, const double* w_mul,
                        double* out_cost, int32_t* out_status,
                        int32_t* out_path, const int64_t* path_off, int32_t* out_path_len,
                        double* out_D, const int64_t* d_off, int32_t* out_end);

/* librosa.effects.hpss / harmonic at librosa 0.11's defaults (kernel_size 31, power 2, margin 1) and the harmonic
 * features of 04_feature_extraction_experiment/feature_extractor.py:525-556 (librosa.effects.harmonic, then
 * librosa.feature.spectral_centroid of the harmonic signal at its defaults).  The plan must be n_fft 2048 / hop 512 with
 * AFX_WINDOW_HANN; flags: AFX_FLAG_PREEMPH (the plan's pre-emphasis is applied to the input first) and / or
 * AFX_HPSS_STORE_SPEC (AFX_FLAG_TRIM is unsupported).  The time-axis median follows scipy's 'reflect' mirror repeated
 * with period 2T for every clip of T frames.
 *   out_harm / out_perc  NULL or host float: clip i's signal at out_*[offsets[i] .. + lengths[i]]
 *   out_stats            NULL or host double[4 n_clips]: sum h^2, sum y^2, mean and std (ddof 0) of h's spectral
 *                        centroid (Hz); NaN for a failed clip, centroid fields NaN for a clip of one sample
 *   out_spec, spec_off   AFX_HPSS_STORE_SPEC only (no performance requirement): S, Hm, Pm as float32 3 x 1025 x T_i
 *                        (bin-major) at out_spec[spec_off[i] ..], T_i = 1 + lengths[i] / 512
 *   out_status           afx_clip_status per clip: AFX_CLIP_TOO_SHORT for length 0, AFX_CLIP_NONFINITE for a NaN / inf
 *                        sample; a failed clip's signals are zero and never affect the other clips
 * The batch runs in chunks whose device workspace stays within 2 GiB; a clip larger than that runs alone. */
int afx_hpss_batch(afx_plan* plan, const void* samples, int sample_fmt, int mem_kind,
                   const int64_t* offsets, const int64_t* lengths, int n_clips, int flags,
                   float* out_harm, float* out_perc, double* out_stats,
                   float* out_spec, const int64_t* spec_off, int32_t* out_status);

/* The timbre group of 04_feature_extraction_experiment/feature_extractor.py:558-590: librosa.feature.chroma_stft (with
 * librosa.estimate_tuning when no tuning is given) and librosa.feature.melspectrogram at librosa's defaults (n_fft 2048,
 * hop 512, centred, periodic Hann, power 2; piptrack fmin 150 / fmax 4000 / threshold 0.1, tuning resolution 0.01, 12
 * chroma, ctroct 5, octwidth 2, norm 2 / inf, base_c), as tests/chroma_ref.py restates them.  Both symbols are newer than
 * AFX_VERSION 107 says: a binding detects them by their presence.  The plan must be n_fft 2048 / hop 512 with
 * AFX_WINDOW_HANN and at most 128 mel bands (AFX_ERR_UNSUPPORTED otherwise); sr and the mel bank are the plan's.
 *   flags       AFX_FLAG_PREEMPH or 0, plus AFX_CHROMA_STORE_HIST (AFX_FLAG_TRIM is unsupported)
 *   tuning_in   NULL: the tuning of every clip is estimated on the device; else n_clips values (fractions of a semitone)
 *   out_chroma, chroma_off   NULL or host float: clip i's 12 x T_i matrix, row-major, at out_chroma[chroma_off[i] ..],
 *               T_i = 1 + lengths[i] / 512; every frame divided by its maximum (a frame below FLT_MIN stays zero)
 *   out_mel, mel_off         NULL or host float: n_mels x T_i mel power at out_mel[mel_off[i] ..]
 *   out_tuning  NULL or host double[n_clips]: the tuning used (an estimate is one of -0.5 + 0.01 k, k < 100; 0 when the
 *               clip has no pitch peak)
 *   out_stats   NULL or host double[4 n_clips]: mean and std (ddof 0) of the mel matrix, then of the chroma matrix;
 *               NaN for a failed clip
 *   out_hist    AFX_CHROMA_STORE_HIST only (no performance requirement; zeros where tuning_in is given): int32[102
 *               n_clips]: pitch peaks, peaks at or above the median magnitude, their 100 residual counts
 *   out_status  AFX_CLIP_TOO_SHORT for length 0, AFX_CLIP_NONFINITE for a NaN / inf sample; a failed clip's matrices are
 *               zero and it never affects the other clips
 * No float atomics: results are bit-reproducible and independent of what else is in the batch.  The batch runs in chunks
 * whose device workspace stays within 2 GiB; a clip larger than that runs alone.
 *
 * afx_chroma_filters (host-only): librosa.filters.chroma(sr, 2048, tuning) as 12 x 1025 float32, row-major. */
enum { AFX_CHROMA_STORE_HIST = 8 };
int afx_chroma_batch(afx_plan* plan, const void* samples, int sample_fmt, int mem_kind,
                     const int64_t* offsets, const int64_t* lengths, int n_clips, int flags,
                     const double* tuning_in,
                     float* out_chroma, const int64_t* chroma_off,
                     float* out_mel, const int64_t* mel_off,
                     double* out_tuning, double* out_stats, int32_t* out_hist, int32_t* out_status);
int afx_chroma_filters(int sr, double tuning, float* out /*[12 * 1025]*/);

/* The rhythm group of 04_feature_extraction_experiment/feature_extractor.py:592-622: librosa.onset.onset_strength, the
 * tempogram librosa.beat.beat_track asks librosa.feature.tempo for (win = int(8 sr) // 512 lags) and tempo's decision, at
 * librosa 0.11's defaults (mel power of n_fft 2048 / hop 512, power_to_db with ref 1 and top_db 80, lag 1, the mean over
 * the bands, centred; Hann autocorrelation window, linear_ramp padding, norm inf; start_bpm 120, std_bpm 1, max_tempo 320,
 * mean aggregate), as tests/rhythm_ref.py restates them.  Beat positions are afx_beat_batch's, below.  Both symbols are newer than
 * AFX_VERSION 107 says: a binding detects them by their presence.  The plan must be n_fft 2048 / hop 512 with
 * AFX_WINDOW_HANN, at most 128 mel bands and 128 <= sr <= 49215 (2 <= win <= 768) -- AFX_ERR_UNSUPPORTED otherwise; sr and the
 * mel bank are the plan's.  With T_i = 1 + lengths[i] / 512:
 *   flags          AFX_FLAG_PREEMPH or 0 (AFX_FLAG_TRIM is unsupported)
 *   out_env, env_off         NULL or host float: clip i's onset envelope, T_i values at out_env[env_off[i] ..]; its first
 *                  three are 0, so a clip of T_i <= 3 has an all-zero envelope
 *   out_tempogram, tg_off    NULL or host float (no performance requirement): win x T_i, row-major, at
 *                  out_tempogram[tg_off[i] ..]; every frame divided by its largest magnitude (a frame below FLT_MIN is left)
 *   out_acmean     NULL or host double[win * n_clips]: the mean of the tempogram over the frames
 *   out_tempo, out_lag       host double / int32 [n_clips]: lag = the first maximum of log1p(1e6 acmean) + logprior,
 *                  tempo = bpm[lag] (afx_tempo_table); lag 0 and tempo 0.0 when the envelope is all zero
 *   out_stats      NULL or host double[2 n_clips]: mean and std (ddof 0) of the envelope
 *   out_status     AFX_CLIP_TOO_SHORT for length 0 (one zero frame), AFX_CLIP_NONFINITE for a NaN / inf sample; a failed
 *                  clip's envelope, tempogram and acmean are zero, its lag 0, its tempo and statistics NaN, and it never
 *                  affects the other clips
 * No float atomics: results are bit-reproducible and independent of what else is in the batch.  The batch runs in chunks
 * whose device workspace stays within 2 GiB; a clip larger than that runs alone.
 *
 * afx_tempo_table (host-only): win, kmin (the first lag slower than 320 bpm), bpm[win] (bpm[0] = inf) and logprior[win]
 * (-inf below kmin) for a sample rate at hop 512; any pointer may be NULL.  AFX_ERR_UNSUPPORTED when win is not in 2 .. 768. */
int afx_tempo_table(int sr, int32_t* out_win, int32_t* out_kmin, double* out_bpm, double* out_logprior);
int afx_rhythm_batch(afx_plan* plan, const void* samples, int sample_fmt, int mem_kind,
                     const int64_t* offsets, const int64_t* lengths, int n_clips, int flags,
                     float* out_env, const int64_t* env_off,
                     float* out_tempogram, const int64_t* tg_off,
                     double* out_acmean,
                     double* out_tempo, int32_t* out_lag,
                     double* out_stats,
                     int32_t* out_status);

/* Beat positions: the second half of librosa.beat.beat_track(onset_envelope=env, sr=sr) (hop 512, trim by Ellis's
 * beat-indexed rule), as tests/beat_ref.py restates it.  Both symbols are newer than AFX_VERSION 107 says: a binding detects
 * them by their presence.  For an envelope env[T], fps = sr / 512 and a tempo bpm:
 *   no beats       T < 2, an all-zero envelope, or bpm == 0 (librosa is undefined for T == 1; ours is no beats)
 *   fpb            round(fps 60 / bpm), half to even, in [1, 768]; a tempo afx_rhythm_batch decided gives fpb == its lag
 *   localscore     x = env / (std(env, ddof 1) + DBL_MIN) convolved ("same") with exp(-0.5 ((k - fpb) 32 / fpb)^2), k = 0 .. 2 fpb
 *   cumscore[i]    localscore[i] + the largest of cumscore[loc] - tightness (log(i - loc) - log(fpb))^2 over loc = i - lo,
 *                  i - lo - 1, .. i - 2 fpb (loc >= 0; lo = round(fpb / 2) half to even); the nearest predecessor wins a tie
 *   backlink[i]    that loc, -1 without one and -1 until the first frame whose localscore reaches 0.01 max(localscore)
 *   last beat      the largest local maximum of cumscore (> left, >= right; never frame 0) that reaches half the median of
 *                  the local maxima; none: no beats
 *   trim           with s[j] = localscore at beat j: smooth[j] = 0.5 s[j-1] + s[j] + 0.5 s[j+1]; the beats from the first to
 *                  the last with smooth[j] > 0.5 sqrt(mean(smooth^2)) are kept
 * all in float64.  A clip the dynamic programme does not run for has localscore and cumscore zero and every backlink -1.
 *
 * afx_beat_track_host (host-only): one envelope on the CPU -- the specification of the kernels.  out_mask[T]: 1 at a beat.
 * AFX_ERR_INVALID for bpm < 0, a non-finite bpm, fps, tightness or envelope value, fps or tightness <= 0, or fpb outside
 * [1, 768] when bpm > 0; AFX_ERR_UNSUPPORTED for more than 2^22 frames.
 *
 * afx_beat_batch: plan limits are afx_rhythm_batch's.  Without AFX_BEAT_INPUT_ENVELOPE the clips are samples and the
 * envelope and the tempo are the ones afx_rhythm_batch computes for them (array-equal), T_i = 1 + lengths[i] / 512.  With it,
 * samples holds float32 envelopes, lengths[i] = T_i <= 2^22, and the tempo is decided from the envelope the same way;
 * AFX_FLAG_PREEMPH is refused (AFX_ERR_INVALID) and a NaN / inf value gives AFX_CLIP_NONFINITE.
 *   in_bpm         NULL: every clip is tracked at the decided tempo; else per clip a tempo, 0 = the decided one
 *                  (AFX_ERR_INVALID as for afx_beat_track_host)
 *   out_beats, frame_off     host uint8: T_i flags at out_beats[frame_off[i] ..], 1 at a beat
 *   out_n_beats, out_tempo, out_fpb      host [n_clips]: the count, the tempo tracked at, fpb (0 for tempo 0)
 *   out_env, out_localscore, out_cumscore, out_backlink      NULL or host, T_i values at frame_off[i]
 *   out_status     as afx_rhythm_batch's (AFX_CLIP_TOO_SHORT for a clip of 0 samples: one frame, no beats; an envelope of 0
 *                  frames is AFX_CLIP_OK and writes nothing); a clip with tempo 0 or T < 2 has no beats and is AFX_CLIP_OK; a
 *                  failed clip's outputs are zero, its tempo NaN, and it never affects another clip
 * No float atomics: results are bit-reproducible and depend neither on the rest of the batch nor on the chunk cut. */
enum { AFX_BEAT_INPUT_ENVELOPE = 64 };   /* in flags, beside AFX_FLAG_PREEMPH */
int afx_beat_track_host(const float* env, int64_t T, double fps, double bpm, double tightness, int trim,
                        uint8_t* out_mask /*[T]*/, int64_t* out_n_beats,
                        double* out_localscore /*NULL ok, [T]*/, double* out_cumscore /*NULL ok*/, int32_t* out_backlink /*NULL ok*/);
int afx_beat_batch(afx_plan* plan, const void* samples, int sample_fmt, int mem_kind,
                   const int64_t* offsets, const int64_t* lengths, int n_clips, int flags,
                   const double* in_bpm, double tightness, int trim,
                   uint8_t* out_beats, const int64_t* frame_off,
                   int32_t* out_n_beats, double* out_tempo, int32_t* out_fpb,
                   float* out_env,
                   double* out_localscore, double* out_cumscore, int32_t* out_backlink,
                   int32_t* out_status);

/* Host-only: how afx_hpss_batch, afx_chroma_batch and afx_rhythm_batch cut a batch into chunks (one rule, the entry points
 * differ in the cost record).  A clip of T = 1 + length / 512 frames costs T cost[0] + ceil(T / cost[4]) cost[1] +
 * length cost[2] + cost[3] bytes of workspace; a chunk holds at least one clip and ends before the clip that would take
 * its bytes past budget or its tiles (of cost[4] frames) past cost[5], or at 32768 clips.  chunk_of[i] = the chunk of
 * clip i, -1 for a clip of length 0 (it is in no chunk and costs nothing).  Newer than AFX_VERSION 107 says: a binding
 * detects it by its presence.  AFX_ERR_INVALID for a length outside [0, 2^31], a budget outside [1, 2^62], cost[0 .. 2]
 * outside [0, 2^20], cost[3] outside [0, 2^30] (afx_gate_batch's clip carries its padding's frames) or cost[4], cost[5]
 * outside [1, 2^31 - 1]. */
int afx_stft_chunks(const int64_t* lengths, int n_clips, const int64_t* cost /*[6]*/, int64_t budget, int32_t* chunk_of);

/* The spectral, harmonic, timbre and rhythm groups of the experiment extractor in one pass
 * (04_feature_extraction_experiment/feature_extractor.py:624-687 hands one preprocessed (y, sr) to all four): one upload,
 * the preprocess on the device, one STFT of y per chunk, every group reading the same rows, scalars back.  All four symbols
 * are newer than AFX_VERSION 107 says: a binding detects them by their presence.
 *
 * Plan: frame_length 2048, hop_length 512, Hann, as afx_hpss_batch; with AFX_GROUP_SPECTRAL sr > 12800 (six octave bands
 * from 200 Hz), with AFX_GROUP_RHYTHM 128 <= sr <= 49215, with AFX_GROUP_TIMBRE or _RHYTHM at most 128 mel bands
 * (AFX_ERR_UNSUPPORTED otherwise, as for AFX_FLAG_TRIM; AFX_ERR_INVALID for groups == 0, an unknown group or flag).
 * flags: AFX_GROUPS_PREPROCESS runs afx_sosfiltfilt_batch's AFX_FILT_EXPERIMENT first (afx_butter_sos(5, 200 / (sr / 2),
 * high-pass), padlen 18, pre-emphasis 0.98) and the groups see that call's output bit for bit; without it the samples are
 * taken as given and AFX_FLAG_PREEMPH means what it means for afx_hpss_batch (with it, AFX_FLAG_PREEMPH is refused).
 *
 * out_stats[24 i ..], NaN for a group that was not asked for:
 *   [0..8)    mean, std (ddof 0) of spectral_centroid, _bandwidth, _rolloff and _contrast (power_to_db(peak) -
 *             power_to_db(valley), each matrix clamped 80 dB below its own maximum) at librosa's defaults
 *   [8..12)   afx_hpss_batch's record: sum h^2, sum y^2, mean and std of spectral_centroid(h)
 *   [12..16)  afx_chroma_batch's record: mean, std of the mel power matrix, mean, std of chroma_stft
 *   [16..18)  mean, std of the 13 x T matrix librosa.feature.mfcc(y, sr, n_mfcc=13) (from one frame up)
 *   [18..22)  tempo, mean and std of the onset envelope, the mean tempogram at the chosen lag
 *   [22..24)  the preprocess's max|x| and max|y| (0 without AFX_GROUPS_PREPROCESS)
 * out_tuning, out_lag (NULL ok): the tuning estimated for the clip (0.0 without AFX_GROUP_TIMBRE), the chosen tempogram
 * lag.  out_status: AFX_CLIP_NONFINITE for a NaN / inf sample, AFX_CLIP_TOO_SHORT for length 0 and, with the preprocess,
 * for 18 samples or fewer; such a clip's record is all NaN and it never affects another clip.  The centroid fields
 * ([0..8), [10], [11]) of a clip of one sample are NaN.  Results are bit-reproducible and depend neither on the rest of
 * the batch nor on how it was cut into chunks (2 GiB of workspace each).
 *
 * afx_groups_cost (host-only): the cost record afx_groups_batch cuts with, for afx_stft_chunks; it is an upper bound over
 * plans (768 lags, 128 mel bands, float32 host samples) and so needs none.
 * afx_groups_dct_table (host-only): rows 0 .. 12 of the orthonormal DCT-II of n_mels <= 128 points as out[13][128]
 * (float64 rounded once; columns past n_mels are zero), the table of [16..18).
 * afx_groups_debug_rows: with AFX_GROUPS_STORE_DESC and AFX_GROUP_SPECTRAL the call keeps the 17 floats per frame of
 * afx_spectral_batch's layout on the host, clip after clip (a clip of status AFX_CLIP_TOO_SHORT has none); this copies the first
 * min(n_floats, *count) of them out and sets *count to how many the last call kept. */
enum { AFX_GROUP_SPECTRAL = 1, AFX_GROUP_HARMONIC = 2, AFX_GROUP_TIMBRE = 4, AFX_GROUP_RHYTHM = 8 };
enum { AFX_GROUPS_PREPROCESS = 16, AFX_GROUPS_STORE_DESC = 32 };   /* in flags, beside AFX_FLAG_PREEMPH */
int afx_groups_batch(afx_plan* plan, const void* samples, int sample_fmt, int mem_kind,
                     const int64_t* offsets, const int64_t* lengths, int n_clips,
                     int flags, int groups,
                     double* out_stats /*[n_clips][24]*/, double* out_tuning, int32_t* out_lag,
                     int32_t* out_status);
int afx_groups_cost(int groups, int flags, int64_t* cost /*[6]*/);
int afx_groups_dct_table(int n_mels, float* out /*[13][128]*/);
int afx_groups_debug_rows(afx_plan* plan, float* out, int64_t n_floats, int64_t* count);

/* STFT-domain noise reduction: spectral_subtraction and wiener_filter of
 * 00_audio_data_collection_experiment/noise_reduction.py:15-92 and the aligner's preprocess of
 * 05_dtw_alignment_experiment/process_audio.py:9-54, as tests/denoise_ref.py restates them.  Both symbols are newer than
 * AFX_VERSION 107 says: a binding detects them by their presence.  The plan must be n_fft 2048 / hop 512 with
 * AFX_WINDOW_HANN (AFX_ERR_UNSUPPORTED otherwise, as for AFX_FLAG_TRIM).
 *
 * X is the centred (zero-padded) STFT of the clip, T = 1 + length / 512 frames, n = min(T, noise_frames):
 *   AFX_DENOISE_SPECSUB  N[b] = mean over t < n of |X[b, t]|;    Y = X max(|X| - beta N, 0) / |X|, 0 where |X| = 0
 *   AFX_DENOISE_WIENER   Np[b] = mean over t < n of |X[b, t]|^2; Y = X P / (P + Np + 2^-52), P = |X|^2 (beta is not read)
 * then librosa.istft(Y, hop_length=512): window x irfft, overlap-add in increasing frame order, division by the window
 * sum-square where it exceeds the float32 tiny.  That gives L' = 512 (length / 512) samples; out[L' .. length) is zero (the
 * reference pads), and a clip shorter than 512 samples is all zero with status AFX_CLIP_OK.
 *   flags  AFX_FLAG_PREEMPH (the plan's pre-emphasis first, as for afx_hpss_batch) and / or
 *          AFX_DENOISE_RMS_GAIN  the STFT sees fl32(y g), g = fl32(0.1 / (sqrt(mean y^2) + 1e-6)), sum y^2 in float64
 *          AFX_DENOISE_VAD       on the L' denoised samples d: e = librosa.feature.rms(d, frame_length int(0.025 sr),
 *                                hop_length int(0.010 sr), center=True, zero padding), thr = 0.5 mean(e); out[j] = d[j] iff a
 *                                frame i with e[i] > thr has i hop <= j < i hop + fl and i hop + fl <= L' (the copy windows
 *                                are not centred although the RMS frames are), else 0; sr is the plan's
 *          The aligner's preprocess is AFX_DENOISE_SPECSUB with both flags, beta 1, noise_frames 10; its result is out[0, L').
 *   out       host float: clip i at out[offsets[i] .. + lengths[i]]
 *   out_info  NULL or host double[n_clips][4]: the gain (1.0 without AFX_DENOISE_RMS_GAIN), the VAD threshold, the speech
 *             frames and the VAD frames (NaN, 0, 0 without AFX_DENOISE_VAD); all NaN for a failed clip
 *   out_status  AFX_CLIP_TOO_SHORT for length 0 and, with AFX_DENOISE_VAD, for fewer than 512 samples; AFX_CLIP_NONFINITE
 *             for a NaN / inf sample; a failed clip's output is zero and it never affects another clip
 * AFX_ERR_INVALID for an unknown mode or flag, beta negative or not finite, noise_frames outside [1, 64] and
 * AFX_DENOISE_VAD with int(0.010 sr) < 1.  Results are bit-reproducible and depend neither on the rest of the batch, nor on
 * how it was cut into chunks (2 GiB of workspace each), nor on the layout of the input.
 *
 * afx_denoise_cost (host-only): the cost record afx_denoise_batch cuts with, for afx_stft_chunks. */
enum { AFX_DENOISE_SPECSUB = 0, AFX_DENOISE_WIENER = 1 };
enum { AFX_DENOISE_RMS_GAIN = 128, AFX_DENOISE_VAD = 256 };   /* in flags, beside AFX_FLAG_PREEMPH */
int afx_denoise_batch(afx_plan* plan, const void* samples, int sample_fmt, int mem_kind,
                      const int64_t* offsets, const int64_t* lengths, int n_clips,
                      int flags, int mode, double beta, int noise_frames,
                      float* out, double* out_info /*[n_clips][4]*/, int32_t* out_status);
int afx_denoise_cost(int flags, int sample_fmt, int mem_kind, int64_t* cost /*[6]*/);

/* Host-only (no device needed): the tables afx_f0_batch uploads, for inspection and tests.
 * info[8] = min_period, max_period, n_pitch_bins, band (transition half-width), candidate
 * capacity, lags kept, lags per lane, trough slots per lane.  beta[100] = Beta(2,18) mass of
 * each threshold interval; lt[2][2*band+1][2*band+1] = log(switch * local + tiny) per source-row
 * class (0 interior, 1..band low edge, band+1..2*band high edge) and offset; freqs[n_pitch_bins].
 * Any pointer may be NULL. */
int afx_f0_build_tables(int sr, int n_fft, int hop, double fmin, double fmax, int32_t* info,
                        double* beta, double* lt, double* freqs);

/* Host-only: which instantiation of each pYIN kernel afx_f0_batch launches for a configuration -- the launchers switch on
 * the same record.  out[12] = energy kernel (0 k_f0_energy, otherwise the LPW of k_f0_energy2), its frames per workgroup;
 * k_f0_yin's N, FPB, SH; k_f0_viterbi's NBT, BANDT (0, 0: generic); Viterbi targets per thread; k_f0_backtrack's ring depth;
 * then band, n_pitch_bins and the LDS bytes of the k_f0_yin launch.  AFX_ERR_UNSUPPORTED, with the reason afx_f0_batch
 * gives, for a configuration extract_f0 refuses (transition band wider than 64 bins, more than 160 KiB of LDS). */
int afx_f0_dispatch(int sr, int n_fft, int hop, double fmin, double fmax, int32_t* out);

/* Host-only ingest for batch_process (load_audio, F:52 -> librosa.load -> soundfile), by `threads` native threads.
 * afx_wav_probe walks the RIFF chunks of n files: info[4 i ..] = format tag (1 PCM, 3 IEEE float; the sub-format of
 * WAVE_FORMAT_EXTENSIBLE), channels, sample rate, bits per sample; frames[i], data_off[i] = sample frames and byte offset
 * of the data chunk (cut at the file's end); status[i] = 0 ok, 1 not a usable RIFF/WAVE file, 2 cannot be opened / read.
 * afx_wav_read_s16 copies frames[i] 16-bit samples of file i from data_off[i] to out[offsets[i] ..] (for files the probe
 * found to be 16-bit PCM mono: a batch packed in place, uploaded as AFX_FMT_S16); status[i] = 0 or 2.  Every other sample
 * type or channel count goes through afx_wav_read_raw / afx_decode_batch below, or the caller's own decoder. */
int afx_wav_probe(const char* const* paths, int n, int threads, int32_t* info /*[4n]*/, int64_t* frames,
                  int64_t* data_off, int32_t* status);
int afx_wav_read_s16(const char* const* paths, int n, int threads, const int64_t* data_off, const int64_t* frames,
                     int16_t* out, int64_t out_len, const int64_t* offsets, int32_t* status);

/* Every other WAVE layout of load_audio (F:52 -> librosa.load -> soundfile, mono=True): the raw data chunk is read as
 * bytes, uploaded as it is, and converted and mixed down on the device.  Both symbols are newer than AFX_VERSION 107 says:
 * a binding detects them by their presence.
 *
 * afx_wav_read_raw (host-only) is afx_wav_read_s16 in bytes: nbytes[i] bytes of file i from data_off[i] go to
 * out[offsets[i] ..]; status[i] = 0 or 2.  AFX_ERR_INVALID, with nothing read, when a clip does not fit out_len bytes.
 *
 * afx_decode_batch: clip i is frames[i] interleaved sample frames of channels[i] channels of sample kind kinds[i]
 * (little-endian, as in the file) from byte byte_offsets[i] of raw (host or device memory); its mono float32 signal goes to
 * out[out_offsets[i] .. + frames[i]) in host or device memory (out_mem_kind), the elements from there to the next multiple
 * of 4 are written as 0, nothing else is written.  byte_offsets must be multiples of 16, out_offsets multiples of 4
 * (AFX_ERR_INVALID otherwise; device pointers are taken to be 16-byte aligned); device-resident raw is read in whole
 * 4-byte words, so the buffer must reach the next multiple of 4 behind the last clip.  A batch may mix kinds and channel
 * counts; a clip of 0 frames writes nothing.  Host-resident raw / out are staged through pageable copies inside the call (as
 * afx_resample_batch stages them): the path that uploads a page-locked window once is device memory on both sides.
 *   u8   float32(v - 128) * 2^-7        s16  float32(v) * 2^-15        s24  float32(v) * 2^-23 (sign-extended)
 *   s32  float32(v), rounded to nearest even, * 2^-31      f32  the bits as they are      f64  rounded to nearest even
 * (libsndfile's scaling, wavio.to_float32); 2 to 7 channels: the float32 sum in channel order ((c0 + c1) + c2) ... divided
 * by float32(channels) (numpy's mean over the channel axis for fewer than 8 channels, wavio.to_mono).  Denormals are kept.
 * No atomics: results are bit-reproducible.  AFX_ERR_UNSUPPORTED for more than 7 channels; AFX_ERR_INVALID, before anything
 * is uploaded, for negative offsets or sizes, an unknown kind, fewer than 1 channel, or clips whose output slots overlap. */
enum { AFX_SMP_U8 = 0, AFX_SMP_S16 = 1, AFX_SMP_S24 = 2, AFX_SMP_S32 = 3, AFX_SMP_F32 = 4, AFX_SMP_F64 = 5 };
int afx_wav_read_raw(const char* const* paths, int n, int threads, const int64_t* data_off, const int64_t* nbytes,
                     uint8_t* out, int64_t out_len, const int64_t* offsets /*bytes*/, int32_t* status);
int afx_decode_batch(afx_ctx* ctx, const void* raw, int mem_kind, const int64_t* byte_offsets, const int64_t* frames,
                     const int32_t* kinds, const int32_t* channels, int n_clips,
                     float* out, int out_mem_kind, const int64_t* out_offsets);

/* Resampling to the extractor's rate, the other half of load_audio (F:52: librosa.load(path, sr=self.sr)).  The filter is
 * the engine's own (parity with librosa's soxr_hq is not claimed): a linear-phase Kaiser-windowed sinc, 125 dB, transition
 * band 0.913 .. 1.0 of the lower Nyquist rate, applied as a polyphase filter.  With g = gcd(sr_in, sr_out), up = sr_out / g,
 * down = sr_in / g, taps h[0 .. L) of odd length L and half = (L - 1) / 2, a clip x[0 .. n) gives ceil(n * up / down) samples
 *   out[m] = float32( sum_i x[i] * (up * h[m * down + half - i * up]) ),    0 <= i < n, tap index within [0, L)
 * with x taken as float64 (S16: value / 32768), the products and the sum in float64, one rounding to float32; samples
 * outside the clip are zero.
 *
 * afx_resample_design (host-only, no device needed): info[4] = up, down, L, half; taps[L] (NULL: sizes only) from
 * scipy.signal.kaiserord(125, ...) / firwin with a Kaiser window, unity DC gain.  sr_in == sr_out: 1, 1, 1, 0 and the tap 1.
 * AFX_ERR_INVALID for a non-positive rate; AFX_ERR_UNSUPPORTED for a rate pair outside the table bounds of the device
 * resampler: up <= 2048, L <= 2^21 (22051 -> 22050 has up = 22050 and 10^7 taps).
 *
 * afx_resample_batch: clip i = samples[offsets[i] .. + lengths[i]) (AFX_FMT_F32 / AFX_FMT_S16, host or device memory) is
 * written as float32 to out[out_offsets[i] .. + ceil(lengths[i] * up / down)) in host or device memory (out_mem_kind);
 * out_lengths (host, NULL ok) receives those lengths.  A clip of length 0 writes nothing.  taps: NULL = the design above,
 * else n_taps (odd) caller-supplied taps of unity DC gain.  sr_in == sr_out converts / copies.  A clip's sum never reads
 * its neighbours in the packed buffer.  NaN / inf samples propagate into the outputs whose filter span (widened to the
 * eight adjacent outputs a lane computes together) holds them; there is no per-clip status -- the extract passes behind
 * report AFX_CLIP_NONFINITE.  Results are bit-reproducible (no atomics, one fixed summation order).
 * AFX_ERR_UNSUPPORTED beyond the bounds above, when ceil(8 / up) * down > 2048, or when the filter's span does not fit the
 * kernel's LDS tile; AFX_ERR_INVALID for negative offsets / lengths or an even n_taps. */
int afx_resample_design(int sr_in, int sr_out, int32_t* info /*[4]*/, double* taps);
int afx_resample_batch(afx_ctx* ctx, const void* samples, int sample_fmt, int mem_kind,
                       const int64_t* offsets, const int64_t* lengths, int n_clips, int sr_in, int sr_out,
                       const double* taps, int n_taps, float* out, int out_mem_kind,
                       const int64_t* out_offsets, int64_t* out_lengths);

/* Zero-phase IIR filtering with scipy.signal.filtfilt semantics on cascaded second-order sections, and the experiment
 * extractor's preprocess_audio (04_feature_extraction_experiment/feature_extractor.py:133-154) around it.  All four symbols
 * are newer than AFX_VERSION 107 says: a binding detects them by their presence.
 *
 * The filter.  For a clip x[0 .. n) of float32 samples (S16: value / 32768), sections sos[S][6] = b0 b1 b2 1 a1 a2 (float64,
 * a0 == 1, 1 <= S <= 4) and padlen (0 .. 4096; 18 is scipy's default for the experiment's 5th-order filter):
 *   - odd extension by padlen on both sides, 2 x[0] - x[padlen .. 1] and 2 x[n - 1] - x[n - 2 .. n - padlen - 1], in the
 *     samples' float32 (what scipy computes for a float32 array);
 *   - a forward pass of the cascade in float64 from its step steady state (scipy.signal.sosfilt_zi) times the first extended
 *     sample, a backward pass from the steady state times the forward pass's last output, the extension stripped;
 *   - AFX_FILT_PLAIN: one rounding to float32.
 * AFX_FILT_EXPERIMENT does the whole preprocess_audio: x / max|x| in float32 (unchanged when the peak is below FLT_MIN);
 * librosa's pre-emphasis in float32 with its initial state (u[0] = x[0] + (2 x[0] - x[1]), u[i] = x[i] + (-preemph) x[i - 1],
 * product and sum rounded separately); the filter above in float64; y / max|y| in float64 (unchanged below DBL_MIN); one
 * rounding to float32.
 * Per clip: AFX_CLIP_TOO_SHORT for n <= padlen (scipy raises; length 0 included) and AFX_CLIP_NONFINITE for a NaN / inf
 * sample -- the output range of such a clip is not written; an all-zero clip is AFX_CLIP_OK with zeros out.
 * The passes are computed in blocks of 64 samples whose end states are carried in the per-section state basis (see
 * afx_filtfilt_geometry and DESIGN.md); results are bit-reproducible (no atomics, one fixed order of fused multiply-adds),
 * a clip never reads its neighbours in the packed buffer, and its result depends neither on the rest of the batch nor on how
 * the batch was cut into chunks.
 *
 * afx_butter_sos (host-only): the digital Butterworth filter of scipy.signal.butter(order, wn, output='sos') by the bilinear
 * transform, (order + 1) / 2 rows of six; every section has unit gain at the far end of the pass band, so the rows are not
 * scipy's but their product is.  order 1 .. 8 (AFX_ERR_UNSUPPORTED above), 0 < wn < 1 (1 = Nyquist; AFX_ERR_INVALID otherwise).
 * afx_filtfilt_geometry (host-only): info[4] = samples per block, blocks per tile, most sections, largest padlen.
 * afx_sosfiltfilt_host (host-only): one host clip through the same block decomposition, tables and fused operations in
 * float64 on the CPU -- the specification of the kernels.  out_peak (NULL ok): max|x|, max|y| before the last scaling.
 * afx_sosfiltfilt_batch: clip i = samples[offsets[i] .. + lengths[i]) (AFX_FMT_F32 / AFX_FMT_S16, host or device memory) is
 * written to out[out_offsets[i] .. + lengths[i]) in host or device memory (out_mem_kind); out_peak (host, NULL ok) receives
 * max|x| and max|y| per clip (zeros for a failed one), out_status (host) the afx_clip_status.  AFX_ERR_UNSUPPORTED for more
 * than 4 sections or padlen > 4096; AFX_ERR_INVALID for negative offsets / lengths, an unknown mode, or sections that are
 * not finite, not normalised to a0 = 1, or have a pole at z = 1. */
enum { AFX_FILT_PLAIN = 0, AFX_FILT_EXPERIMENT = 1 };
int afx_butter_sos(int order, double wn, int highpass, double* sos /*[(order + 1) / 2][6]*/);
int afx_filtfilt_geometry(int32_t* info /*[4]*/);
int afx_sosfiltfilt_host(const void* samples, int sample_fmt, int64_t n, const double* sos, int n_sections, int padlen,
                         int mode, float preemph, float* out, double* out_peak /*[2]*/, int32_t* out_status);
int afx_sosfiltfilt_batch(afx_ctx* ctx, const void* samples, int sample_fmt, int mem_kind,
                          const int64_t* offsets, const int64_t* lengths, int n_clips,
                          const double* sos, int n_sections, int padlen, int mode, float preemph,
                          float* out, int out_mem_kind, const int64_t* out_offsets,
                          double* out_peak /*[n_clips][2]*/, int32_t* out_status);

/* Sample-domain smoothers with scipy semantics, and the experiment extractor's energy and ZCR groups
 * (04_feature_extraction_experiment/feature_extractor.py:341-483) built on them.  All eight symbols are newer than AFX_VERSION
 * 107 says: a binding detects them by their presence.  Clips, formats and memory kinds are those of afx_sosfiltfilt_batch;
 * outputs are float32 of their inputs' lengths.  Results are bit-reproducible, a clip never reads its neighbours in the
 * packed buffer, and its result depends neither on the rest of the batch nor on how the batch was cut into chunks.
 *
 * afx_medfilt_batch: scipy.signal.medfilt(x, kernel_size).  kernel_size odd, 1 .. 31 (an even or non-positive one is
 * AFX_ERR_INVALID, a larger one AFX_ERR_UNSUPPORTED); out[i] = the median of x[i - h .. i + h], h = kernel_size / 2, with
 * zeros outside [0, n), so a kernel longer than the clip is legal.  The result is one of the inputs or 0: value-exact; a
 * zero result is always +0.  Per clip: AFX_CLIP_TOO_SHORT for length 0, AFX_CLIP_NONFINITE for a NaN / inf sample -- the
 * output range of such a clip is not written.
 *
 * afx_savgol_batch: scipy.signal.savgol_filter(x, window_length, polyorder, deriv=deriv, delta=delta, mode='interp') of the
 * float32 samples widened to float64.  window_length odd, 3 .. 31; 0 <= polyorder <= 5, polyorder < window_length;
 * deriv 0 .. 2; delta finite and not 0.  AFX_ERR_INVALID for a negative or zero window_length, a negative polyorder or deriv,
 * polyorder >= window_length or a bad delta; AFX_ERR_UNSUPPORTED for an even window_length, window_length 1 or above 31,
 * polyorder above 5, deriv above 2 -- all before any device work.  Interior outputs are the window_length taps of
 * scipy.signal.savgol_coeffs; the first and last window_length / 2 outputs are the degree-polyorder least-squares polynomial
 * through the clip's first / last window_length samples, evaluated (deriv times differentiated) at the output's position.
 * Every output is one chain of float64 fused multiply-adds over window_length samples in ascending order, rounded once to
 * float32.  Per clip: AFX_CLIP_TOO_SHORT for n < window_length (scipy raises), AFX_CLIP_NONFINITE as above.
 * afx_savgol_tables (host-only): the interior taps in scipy.signal.savgol_coeffs' (convolution) order and the two edge
 * matrices, row r = output r (left) / n - window_length / 2 + r (right) as weights over the first / last window_length
 * samples in ascending order; float64, from a centred and scaled abscissa.
 * afx_medfilt_host, afx_savgol_host (host-only): one host clip through the same code on the CPU -- the specification of the
 * kernels, bit for bit.
 * afx_smooth_geometry (host-only): info[4] = samples per tile, largest kernel_size / window_length, largest polyorder,
 * largest deriv.
 *
 * afx_energy_zcr_batch: the energy group (:341-403) and the ZCR group (:405-483) of clips at rate sr in one call: one
 * upload, AFX_EZ_N doubles per clip back.  flags: AFX_EZ_PREPROCESS runs afx_sosfiltfilt_batch's AFX_FILT_EXPERIMENT first
 * (afx_butter_sos(5, 200 / (sr / 2), 1), padlen 18, pre-emphasis 0.98; the groups see that call's float32 output bit for
 * bit; clips of 18 samples or fewer are AFX_CLIP_TOO_SHORT); without it only an empty clip is.  AFX_EZ_ENERGY, AFX_EZ_ZCR:
 * the groups to compute; the fields of a group not asked for, and every field of a failed clip, are NaN.
 * Framing per clip (:42-60): fl = frame_length when n >= frame_length, else max(64, 2^floor(log2 n));
 * hop = min(hop_length, fl / 4); T = 1 + n / hop.  frame_length: a power of two in [64, 2048]; hop_length >= 1; sr >= 1 and,
 * with AFX_EZ_PREPROCESS, above 400 (the cutoff must lie below Nyquist): AFX_ERR_INVALID otherwise.
 *   energy  librosa.feature.rms(center=True, zero padding): the squares of the float32 samples summed in float64, mean
 *           square over fl, square root in float64; its mean, population standard deviation and np.percentile(energy, 10)
 *           (numpy's linear rule on the two exact order statistics).
 *   ZCR     afx_medfilt_batch(3), then afx_savgol_batch(11, 3, 0, 1.0) when n > 11, float32 between the stages;
 *           peak = max |s|; a sample counts as +0 when fabs((double)s / (double)peak) <= 1e-10, and every sample does when
 *           the peak is below FLT_MIN (librosa.util.normalize leaves such a signal as it is); frames are centred with edge
 *           padding, a crossing is a change of sign bit between neighbours, a frame's first sample never is one, the rate is
 *           count / fl in float64; the mean and population standard deviation of the rates, and local_stability: the mean
 *           over i in 0 .. T - w of the population standard deviation of rates[i .. i + w), w = min(10, T); the standard
 *           deviation itself when w == 1.  (The reference passes pad_mode='reflect', a keyword librosa.feature.
 *           zero_crossing_rate does not have; this is librosa's own edge padding.)
 * Sums run in one fixed order: a lane's own terms ascending, then a halving tree over the lanes.
 * afx_energy_zcr_host (host-only): one float32 clip, already preprocessed, through the same operations on the CPU;
 * rec[AFX_EZ_PEAK_IN] and rec[AFX_EZ_PEAK_FILT] stay NaN. */
enum { AFX_EZ_PREPROCESS = 1, AFX_EZ_ENERGY = 2, AFX_EZ_ZCR = 4 };
enum {
  AFX_EZ_T = 0,            /* frames */
  AFX_EZ_FL = 1,           /* the clip's frame length */
  AFX_EZ_HOP = 2,          /* the clip's hop */
  AFX_EZ_ENERGY_MEAN = 3,
  AFX_EZ_ENERGY_STD = 4,
  AFX_EZ_ENERGY_P10 = 5,
  AFX_EZ_ZCR_MEAN = 6,
  AFX_EZ_ZCR_STD = 7,
  AFX_EZ_ZCR_LOCAL = 8,    /* local_stability */
  AFX_EZ_PEAK_SMOOTH = 9,  /* max |s| of the smoothed signal (ZCR group) */
  AFX_EZ_PEAK_IN = 10,     /* the preprocess's max |x| */
  AFX_EZ_PEAK_FILT = 11,   /* the preprocess's max |y| before its last scaling */
  AFX_EZ_N = 12
};
int afx_smooth_geometry(int32_t* info /*[4]*/);
int afx_savgol_tables(int window_length, int polyorder, int deriv, double delta, double* coeffs /*[W]*/,
                      double* left /*[W / 2][W]*/, double* right /*[W / 2][W]*/);
int afx_medfilt_host(const void* samples, int sample_fmt, int64_t n, int kernel_size, float* out, int32_t* out_status);
int afx_savgol_host(const void* samples, int sample_fmt, int64_t n, int window_length, int polyorder, int deriv, double delta,
                    float* out, int32_t* out_status);
int afx_energy_zcr_host(const float* samples, int64_t n, int frame_length, int hop_length, int flags,
                        double* out_rec /*[AFX_EZ_N]*/, int32_t* out_status);
int afx_medfilt_batch(afx_ctx* ctx, const void* samples, int sample_fmt, int mem_kind,
                      const int64_t* offsets, const int64_t* lengths, int n_clips, int kernel_size,
                      float* out, int out_mem_kind, const int64_t* out_offsets, int32_t* out_status);
int afx_savgol_batch(afx_ctx* ctx, const void* samples, int sample_fmt, int mem_kind,
                     const int64_t* offsets, const int64_t* lengths, int n_clips,
                     int window_length, int polyorder, int deriv, double delta,
                     float* out, int out_mem_kind, const int64_t* out_offsets, int32_t* out_status);
int afx_energy_zcr_batch(afx_ctx* ctx, const void* samples, int sample_fmt, int mem_kind,
                         const int64_t* offsets, const int64_t* lengths, int n_clips,
                         int sr, int frame_length, int hop_length, int flags,
                         double* out_rec /*[n_clips][AFX_EZ_N]*/, int32_t* out_status);

/* ITU-R BS.1770-4 integrated (gated) loudness of mono clips and loudness / peak normalisation, with the semantics of
 * pyloudnorm 0.1.x Meter(rate, block_size).integrated_loudness and normalize.loudness / normalize.peak at the experiment's
 * call sites (04_feature_extraction_experiment/process_audio.py:134-147: K-weighting, mono).  All seven symbols are newer
 * than AFX_VERSION 107 says: a binding detects them by their presence.
 *
 * The measure.  For a clip x[0 .. n) of float32 samples (S16: value / 32768) at `rate` and T_g = block_size seconds:
 *   - K-weighting: the two sections of afx_kweight_sos, a causal cascade from zero state (scipy.signal.lfilter without zi),
 *     both sections in float64 with no rounding between them (pyloudnorm rounds each stage to the array's float32);
 *   - gating blocks: numBlocks = int(round_half_even((n / rate - T_g) / (T_g / 4)) + 1); block j covers the samples
 *     [b_j, b_{j + 4}) cut at n, b_k = int(T_g * (k * 0.25) * rate) in float64 left to right -- four consecutive segments
 *     --, z_j = sum y^2 / (T_g * rate), the divisor the same for a last block that the rounding left partial;
 *   - gates in the linear domain: the first set z_j >= 10^((-70 + 0.691) / 10); the second z_j > (first-set mean) / 10 and
 *     z_j > 10^((-70 + 0.691) / 10); LUFS = -0.691 + 10 log10(second-set mean), -inf when the set is empty.
 * The K-weighted samples are never stored: the filter runs in the blocks of afx_sosfiltfilt_batch (64 samples, states
 * carried in the per-section basis), once for the blocks' end states and once, from the true entry states, for the sums of
 * squares (afx_loudness_geometry and DESIGN.md).  The sums are float64 in one fixed order; log10 and the gain are host
 * double arithmetic on the gated means, the same code for the device path and the host executor.
 *
 * mode: AFX_LOUD_MEASURE (out may be NULL and is not written); AFX_LOUD_NORM_LOUDNESS: out = float32(gain) * x with
 * gain = 10^((target - LUFS) / 20); AFX_LOUD_NORM_PEAK: gain = 10^(target / 20) / max|x| (the gain needs no level: the loudness
 * fields are the measure's when the clip is long enough for it, NaN otherwise).  One rounded float32 product per sample (numpy
 * 1.24: a float32 array times a float64 scalar).  A clip without a level -- LUFS = -inf, or a zero peak -- comes back
 * unchanged with gain 1 (pyloudnorm would multiply by inf).
 * out_rec holds AFX_LOUD_N doubles per clip (AFX_LOUD_*); GAIN and PEAK_OUT are NaN in AFX_LOUD_MEASURE.  out_blocks (host,
 * NULL ok) receives every z_j of clip i at out_block_offsets[i] (NULL: packed, clip after clip; afx_loudness_blocks
 * gives the counts).  out_status (host): AFX_CLIP_TOO_SHORT for n < block_size * rate (pyloudnorm raises; AFX_LOUD_NORM_PEAK:
 * for n == 0 only) and AFX_CLIP_NONFINITE for a NaN / inf sample -- the record of such a clip is NaN and its output range is
 * not written.  Results are bit-reproducible (no atomics), a clip never reads its neighbours in the packed buffer, and
 * its result depends neither on the rest of the batch nor on how the batch was cut into chunks (afx_stft_chunks with the
 * record of afx_loudness_cost).
 * rates[i] is clip i's own rate: a batch may hold up to 16 distinct rates (AFX_ERR_UNSUPPORTED above).  Rates from 4000 to
 * 192000 Hz; block_size * rate / 4 must exceed 64 samples and block_size 3600 s at most (AFX_ERR_UNSUPPORTED); a rate < 1, a
 * block_size that is not positive and finite, a target that is not finite, an unknown mode: AFX_ERR_INVALID.
 *
 * afx_kweight_sos (host-only): the high shelf (+4 dB, Q = 1 / sqrt 2, 1500 Hz) and the high pass (Q = 0.5, 38 Hz) in RBJ
 * form, divided through by a0: rows b0 b1 b2 1 a1 a2.  AFX_ERR_INVALID for a rate outside 4000 .. 192000.
 * afx_loudness_geometry (host-only): info[5] = samples per block, blocks per tile, lowest rate, highest rate, most distinct
 * rates of a call.
 * afx_loudness_blocks (host-only): numBlocks of a clip of n samples (0: too short to measure).
 * afx_loudness_host (host-only): one host clip through the same block decomposition, tables, operations and summation
 * order on the CPU -- the specification of the kernels, bit for bit.  out_blocks (NULL ok): its z_j.
 * afx_loudness_cost (host-only): cost[6] for afx_stft_chunks (bytes per frame, tile, sample, clip; frames per tile, most
 * tiles): 64 bytes per block of 64 samples (512 per frame of the chunk rule), the uploads, 8 per tile, 3648 per clip. */
enum { AFX_LOUD_MEASURE = 0, AFX_LOUD_NORM_LOUDNESS = 1, AFX_LOUD_NORM_PEAK = 2 };
enum {
  AFX_LOUD_LUFS = 0,        /* integrated loudness; -inf when the second set is empty */
  AFX_LOUD_BLOCKS = 1,      /* gating blocks */
  AFX_LOUD_N1 = 2,          /* blocks of the first set (absolute gate) */
  AFX_LOUD_N2 = 3,          /* blocks of the second set (both gates) */
  AFX_LOUD_GAMMA_R = 4,     /* the relative threshold, dB */
  AFX_LOUD_GATED_MS = 5,    /* mean of z_j over the second set (0 when empty) */
  AFX_LOUD_PEAK = 6,        /* max |x| */
  AFX_LOUD_GAIN = 7,        /* the float32 gain applied */
  AFX_LOUD_PEAK_OUT = 8,    /* max |out| */
  AFX_LOUD_FIRST_MS = 9,    /* mean of z_j over the first set (0 when empty) */
  AFX_LOUD_UNGATED_MS = 10, /* mean of every z_j */
  AFX_LOUD_N = 11
};
int afx_kweight_sos(int rate, double* sos /*[2][6]*/);
int afx_loudness_geometry(int32_t* info /*[5]*/);
int afx_loudness_blocks(int64_t n, int rate, double block_size, int64_t* n_blocks);
int afx_loudness_cost(int sample_fmt, int mem_kind, int out_mem_kind, int mode, int64_t* cost /*[6]*/);
int afx_loudness_host(const void* samples, int sample_fmt, int64_t n, int rate, double block_size, double target, int mode,
                      double* out_rec /*[AFX_LOUD_N]*/, double* out_blocks, float* out, int32_t* out_status);
int afx_loudness_batch(afx_ctx* ctx, const void* samples, int sample_fmt, int mem_kind,
                       const int64_t* offsets, const int64_t* lengths, const int32_t* rates, int n_clips,
                       double block_size, int mode, double target,
                       double* out_rec /*[n_clips][AFX_LOUD_N]*/, double* out_blocks, const int64_t* out_block_offsets,
                       float* out, int out_mem_kind, const int64_t* out_offsets, int32_t* out_status);

/* Spectral-gating noise reduction with the semantics of noisereduce 3.0.3's reduce_noise for one mono clip of at most
 * chunk_size samples, as the experiment's audio processor calls it (04_feature_extraction_experiment/process_audio.py:82-98).
 * DESIGN.md section 25 is the definition and tests/gate_ref.py its float64 restatement.  All three symbols are newer than
 * AFX_VERSION 107 says: a binding detects them by their presence.
 *
 * The grid: chunk = padding zeros, the clip, padding zeros; scipy.signal.stft(nperseg = n_fft, noverlap = n_fft - hop,
 * padded = False): periodic Hann, n_fft / 2 zeros at each end, X = rfft(frame w) / sum w, T = 1 + (length + 2 padding) / hop
 * frames; the matching istft, and the samples [padding, padding + length) of it as float32.
 * stationary: the noise clip (noise_offsets / noise_lengths in the same buffer, or the clip itself when both are NULL; cut to
 * chunk_size samples with clip_noise) has its own grid without the padding; N = dB of |X_n|, 20 log10(a + 2^-52) floored per
 * bin at the row's maximum - 80; thr[b] = mean_t N + n_std_thresh std_t N (float64, one fixed order); hard[b][t] =
 * dB of |X| (floored the same way on the signal grid) > thr[b], taken as |X| + 2^-52 > 10^(thr / 20) or floor > thr;
 * mask = hard p + (1 - p), smoothed.
 * non-stationary: S = scipy.signal.filtfilt([beta], [1, beta - 1], |X|, padtype=None) along time in float64,
 * mask = 1 / (1 + exp(-((|X| - S) / S - thresh_n_mult) sigmoid_slope)), 0 where S = 0; smoothed; then mask p + (1 - p).
 * The smoothing: the outer product of two triangles of 2 n_f + 1 bins and 2 n_t + 1 frames (afx_gate_params), normalised,
 * with zeros beyond the array's four edges, float64; none when n_f = n_t = 1.  Y = X mask, float32.
 *
 * n_fft / hop must be 1024 / 256 or 2048 / 512 with win_length == n_fft (AFX_ERR_UNSUPPORTED otherwise, as for a filter of
 * more than 128 bins or 64 frames a side, padding above 2^20 and chunk_size above 2^24); AFX_ERR_INVALID where noisereduce
 * raises (a smoothing width below one bin / frame) and for prop_decrease outside [0, 1], a time constant that is not
 * positive, or a value that is not finite.
 *   out          float32, clip i at out_offsets[i], host or device memory (out_mem_kind)
 *   out_thresh   host, NULL ok: double[n_clips][n_fft / 2 + 1], thr in dB (stationary; NaN for a failed clip)
 *   out_mask     host, NULL ok: the hard mask on the signal grid (stationary), clip after clip in batch order, a clip of
 *                status AFX_CLIP_OK or AFX_CLIP_NONFINITE taking T rows of ceil((n_fft / 2 + 1) / 32) uint32, frame after
 *                frame; bin b is bit (b & 31) of word b >> 5.  Any other clip takes none.
 *   out_status   host: AFX_CLIP_TOO_SHORT for length 0 (or a noise clip of length 0), AFX_CLIP_TOO_LONG for more than
 *                chunk_size samples (noisereduce's chunk loop is not restated) -- neither clip's output range is written --
 *                and AFX_CLIP_NONFINITE for a NaN / inf sample in the clip or its noise clip: zeros out.
 * No atomics: results are bit-reproducible, and a clip's result depends neither on the rest of the batch, on the input
 * layout, nor on how the batch was cut into chunks (afx_stft_chunks with the record of afx_gate_cost over
 * max(length, noise length) per clip, 0 for a clip that is too long).
 *
 * afx_gate_params (host-only): info[4] = n_f, n_t, T of a clip of `length` samples, 1 when the mask is smoothed; beta; the
 * taps of each axis, each normalised to sum 1 (their outer product is the filter; room for 257 and 129 doubles).  Any n_fft
 * and hop.  beta, taps_f, taps_t may be NULL.
 * afx_gate_cost (host-only): cost[6] for afx_stft_chunks. */
typedef struct afx_gate_opts {
  int32_t sr, n_fft, win_length, hop;
  int32_t stationary;         /* 0: non-stationary */
  int32_t clip_noise;         /* clip_noise_stationary */
  int32_t padding, chunk_size;
  double prop_decrease, time_constant_s, freq_mask_smooth_hz, time_mask_smooth_ms;
  double thresh_n_mult, sigmoid_slope, n_std_thresh;
} afx_gate_opts;
enum { AFX_CLIP_TOO_LONG = 3 };   /* afx_gate_batch: more than chunk_size samples */
int afx_gate_params(const afx_gate_opts* opts, int64_t length, int64_t* info /*[4]*/, double* beta, double* taps_f, double* taps_t);
int afx_gate_cost(const afx_gate_opts* opts, int sample_fmt, int mem_kind, int out_mem_kind, int with_noise, int64_t* cost /*[6]*/);
int afx_gate_batch(afx_ctx* ctx, const void* samples, int sample_fmt, int mem_kind,
                   const int64_t* offsets, const int64_t* lengths, int n_clips,
                   const int64_t* noise_offsets, const int64_t* noise_lengths, const afx_gate_opts* opts,
                   float* out, int out_mem_kind, const int64_t* out_offsets,
                   double* out_thresh, uint32_t* out_mask, int32_t* out_status);

/* librosa.stft / librosa.istft (librosa 0.11) of mono clips at n_fft 1024 or 2048, the transforms behind the reference's
 * own spectral steps (00_audio_data_collection_experiment/noise_reduction.py:31-84, 05_dtw_alignment_experiment/
 * process_audio.py:21-33, visualization.py:194-208).  DESIGN.md section 26 is the definition and tests/stft_ref.py its
 * numpy restatement.  All five symbols are newer than AFX_VERSION 107 says: a binding detects them by their presence.
 *
 * window: n_fft floats in host memory, the caller's window already zero-padded centred to n_fft (librosa.util.pad_center).
 * hop in [1, n_fft]; any other n_fft or hop is AFX_ERR_UNSUPPORTED; a center, pad_mode or out_kind that is none of the
 * values below is AFX_ERR_INVALID.
 *
 * Forward: with center the clip is padded by n_fft / 2 at each end, with zeros (AFX_PAD_CONSTANT) or as
 * np.pad(mode="reflect") does (AFX_PAD_REFLECT, clips longer than n_fft / 2 only); T = 1 + (padded length - n_fft) / hop
 * frames, frame t = padded[t hop .. t hop + n_fft), D[:, t] = rfft(frame x window) in float32.  Clip i takes T rows of
 * n_fft / 2 + 1 elements at element out_offsets[i] of out, frame after frame with nothing between the rows -- the memory
 * of the Fortran-ordered [1 + n_fft / 2, T] array librosa returns: complex64 (AFX_STFT_COMPLEX; out must be 8-byte
 * aligned), or float32 |D| (AFX_STFT_MAG: sqrt(re re + im im), each operation rounded once) or |D|^2 (AFX_STFT_POWER).
 * out_status: AFX_CLIP_TOO_SHORT (nothing written) for length 0, for length < n_fft without center and for
 * length <= n_fft / 2 under AFX_PAD_REFLECT; AFX_CLIP_NONFINITE for a NaN / inf sample: zeros out.
 *
 * Inverse: clip i is n_frames[i] rows of n_fft / 2 + 1 complex64 at element spec_offsets[i] of spec, laid out as above.
 * s = n_fft / 2 with center, else 0; with a length >= 0 only the first min(T, ceil((length + 2 s) / hop)) frames are used;
 * full = n_fft + hop (frames - 1); acc[m] = sum_t window[m - t hop] irfft(D[:, t])[m - t hop] and wss[m] = sum_t
 * float32(window^2)[m - t hop] over the frames that cover m, in increasing t, in float32 (the imaginary parts of bins 0 and
 * n_fft / 2 are ignored); out[j] = acc[s + j] / wss[s + j] where wss > FLT_MIN, acc[s + j] elsewhere, 0 for s + j >= full,
 * for j < length, or j < full - 2 s when none is given.  There is no non-finite check: a frame with a NaN / inf bin makes
 * the samples it covers NaN and no others.  out_status: AFX_CLIP_TOO_SHORT for no frames.
 *
 * No atomics in any sum: results are bit-reproducible, and a clip's result depends neither on the rest of the batch, on the
 * input layout, on host or device memory, nor on how the batch was cut into chunks (afx_stft_chunks with the record of
 * afx_stft_cost: forward over the lengths, 0 for a clip that is too short; inverse over frames used + ceil(samples written
 * / hop) per clip).
 *
 * afx_stft_frames (host-only): T and the status of a clip of `length` samples (T = 0 unless AFX_CLIP_OK).
 * afx_istft_samples (host-only): the frames used and the samples written for T frames (both 0 for T = 0).
 * afx_stft_cost (host-only): cost[6] for afx_stft_chunks; every byte is charged per unit of length and per clip. */
enum { AFX_PAD_CONSTANT = 0, AFX_PAD_REFLECT = 1 };
enum { AFX_STFT_COMPLEX = 0, AFX_STFT_MAG = 1, AFX_STFT_POWER = 2 };
typedef struct afx_stft_opts { int32_t n_fft, hop, center, pad_mode, out_kind, reserved[3]; } afx_stft_opts;
int afx_stft_frames(const afx_stft_opts* opts, int64_t length, int64_t* T, int32_t* clip_status);
int afx_istft_samples(const afx_stft_opts* opts, int64_t T, int64_t length /* < 0: none */, int64_t* n_frames, int64_t* n_out);
int afx_stft_cost(const afx_stft_opts* opts, int sample_fmt, int mem_kind, int out_mem_kind, int inverse, int64_t* cost /*[6]*/);
int afx_stft_batch(afx_ctx* ctx, const void* samples, int sample_fmt, int mem_kind,
                   const int64_t* offsets, const int64_t* lengths, int n_clips,
                   const afx_stft_opts* opts, const float* window /*[n_fft], host*/,
                   void* out, int out_mem_kind, const int64_t* out_offsets /* in output elements */, int32_t* out_status);
int afx_istft_batch(afx_ctx* ctx, const void* spec /* complex64 rows */, int mem_kind,
                    const int64_t* spec_offsets /* complex elements */, const int64_t* n_frames, int n_clips,
                    const afx_stft_opts* opts, const float* window,
                    const int64_t* lengths /* NULL, or per clip, < 0: none */,
                    float* out, int out_mem_kind, const int64_t* out_offsets, int32_t* out_status);

/* librosa.phase_vocoder and librosa.effects.time_stretch (librosa 0.11) of mono clips: what brings a student take to a
 * teacher's duration without changing its pitch.  DESIGN.md section 27 is the definition and tests/pvoc_ref.py its numpy
 * restatement.  All seven symbols are newer than AFX_VERSION 107 says: a binding detects them by their presence.
 *
 * phase_vocoder: clip i is n_frames[i] = T rows of bins = n_fft / 2 + 1 complex64 at element spec_offsets[i] of spec, frame
 * after frame (afx_stft_batch's layout); n_fft even in [2, 4096], hop in [1, n_fft] (anything else: AFX_ERR_UNSUPPORTED).
 * rates[i] must be finite and > 0 (AFX_ERR_INVALID before any device work).  T_out = ceil(T / rate) in float64 rows go to
 * element out_offsets[i] of out; T_out x bins >= 2^31 is AFX_ERR_UNSUPPORTED.  Step t: s = double(t) rate, j = floor(s),
 * a = s - j; c0 = D[:, j], c1 = D[:, j + 1], columns T and beyond being +0 + 0i; mag = float32(1 - a) |c0| + float32(a) |c1|
 * in float32 (|c| = sqrt(re re + im im), every operation rounded once); the phase in float64: phi[k] = 2 pi hop k / n_fft,
 * acc_0 = angle(D[:, 0]), acc_{t+1} = acc_t + phi + wrap(angle(c1) - angle(c0) - phi), wrap(d) = d - 2 pi rint(d / 2 pi);
 * out[:, t] = complex64(mag cos(acc_t), mag sin(acc_t)).  The sum runs in a fixed order: within a tile of AFX_PVOC_TILE
 * steps in increasing t from 0.0, then tile after tile, and the accumulator is reduced to [-pi, pi] after every tile
 * (only acc mod 2 pi is observable).  out_status: AFX_CLIP_TOO_SHORT (nothing written) for T = 0; AFX_CLIP_NONFINITE for a
 * NaN / inf bin anywhere in the clip's D: zeros out, where librosa lets the bin poison its row from there on.
 *
 * time_stretch: stft -> phase_vocoder -> istft(length = n_out), n_out = rint(length / rate) in float64, halves to even, in
 * one call on one workspace with the kernels and records of the three entry points, so bit for bit what they give one after
 * another; the spectra never leave the device.  opts and window as afx_stft_batch takes them (out_kind AFX_STFT_COMPLEX);
 * out_status as afx_stft_batch gives it, and AFX_CLIP_NONFINITE (zeros out) for a spectrum that overflowed as well.
 *
 * No atomics in any sum: a clip's result is bit-identical whatever the rest of the batch, the order of the clips, host or
 * device memory and the chunk cut (afx_stft_chunks with the record of afx_pvoc_cost over T + T_out per clip, or of
 * afx_time_stretch_cost over T + T_out + ceil(length / hop) + ceil(n_out / hop); 0 for a clip with nothing to run).
 *
 * afx_pvoc_frames (host-only): T_out and the status of a clip of T rows.
 * afx_time_stretch_samples (host-only): the frames of the clip, the rows of the stretch and the samples written.
 * afx_pvoc_host (host-only): the same definition in plain C++ for one clip, the kernels' specification; out holds T_out
 * rows.  The kernels agree with it to rounding (libm's atan2 / cos / sin against the device's). */
enum { AFX_PVOC_TILE = 32 };
int afx_pvoc_frames(int n_fft, int hop, int64_t T, double rate, int64_t* T_out, int32_t* clip_status);
int afx_time_stretch_samples(const afx_stft_opts* opts, int64_t length, double rate, int64_t* T, int64_t* T_out, int64_t* n_out,
                             int32_t* clip_status);
int afx_pvoc_cost(int n_fft, int mem_kind, int out_mem_kind, int64_t* cost /*[6]*/);
int afx_time_stretch_cost(const afx_stft_opts* opts, int sample_fmt, int mem_kind, int out_mem_kind, int64_t* cost /*[6]*/);
int afx_pvoc_host(const void* spec /* complex64 rows */, int64_t T, double rate, int n_fft, int hop, void* out, int32_t* clip_status);
int afx_pvoc_batch(afx_ctx* ctx, const void* spec /* complex64 rows */, int mem_kind,
                   const int64_t* spec_offsets /* complex elements */, const int64_t* n_frames, const double* rates, int n_clips,
                   int n_fft, int hop, void* out, int out_mem_kind, const int64_t* out_offsets, int32_t* out_status);
int afx_time_stretch_batch(afx_ctx* ctx, const void* samples, int sample_fmt, int mem_kind,
                           const int64_t* offsets, const int64_t* lengths, const double* rates, int n_clips,
                           const afx_stft_opts* opts, const float* window /*[n_fft], host*/,
                           float* out, int out_mem_kind, const int64_t* out_offsets, int32_t* out_status);

/* The recording screen of00_audio_data_collection_experiment/audio_format_assessment.py:143-300 (detect_silence,
 * check_volume_levels, check_amplitude_stability, estimate_snr) and the sums behind the scores of
 * audio_quality_assessment.py:150-280 (SNR of the difference, Pearson correlation, MSE), as per-clip reductions.  All five
 * symbols are newer than AFX_VERSION 107 says: a binding detects them by their presence.
 *
 * afx_assess_batch: clip i = samples[offsets[i] .. + lengths[i]) (AFX_FMT_F32 / AFX_FMT_S16 taken as value / 32768, host or
 * device memory) with its own frame lengths frame_short[i], frame_long[i] >= 1 (the screen's int(0.01 sr) and int(0.1 sr) at
 * the clip's own rate: a batch may mix rates).  Framing is librosa.feature.rms(frame_length = hop_length = fl, center=True)
 * with zero padding: 1 + (len + 2 (fl / 2) - fl) / fl frames -- 1 + len / fl for an even fl, 1 + (len - 1) / fl for an odd
 * one such as 441 --, frame t = samples [t fl - fl / 2, t fl - fl / 2 + fl) cut to the clip, its mean square
 * p_t = sum y^2 / fl.  out_rec holds AFX_ASSESS_N doubles per clip:
 *   [0] n_short        the frames of frame_short
 *   [1] silent         short frames with rms_db < threshold_db, rms_db = librosa.amplitude_to_db(rms, ref=np.max) =
 *                      max(10 log10(max(1e-10, p_t)) - 10 log10(max(1e-10, max p)), -80); decided in float64 as
 *                      max(1e-10, p_t) < max(1e-10, max p) 10^(threshold_db / 10), never when threshold_db <= -80
 *   [2] longest_run    longest run of consecutive silent frames, in frames (a run that reaches the last frame counts)
 *   [3] max_rms_short  sqrt(max p)
 *   [4] mean_square    sum y^2 / len
 *   [5] peak           max |y| (exact)
 *   [6] noise_mean_square   mean of y^2 over the first min(int(0.1 len), noise_cap) samples; NaN when there are none
 *   [7] n_long, [8] rms_long_mean, [9] rms_long_std   the long framing: frames, mean and population standard deviation
 *                      (around that mean) of sqrt(p_t)
 * Squares of float32 samples are exact in float64 and are summed there.  out_status (host): AFX_CLIP_TOO_SHORT for length 0,
 * AFX_CLIP_NONFINITE for a NaN / inf sample; the record of a failed clip is NaN and no other clip is affected.  The samples
 * are read from device memory once; no atomics: a clip's record is bit-reproducible and depends neither on the rest of the
 * batch, nor on the clip's place in it or in the buffer, nor on how the batch is cut into chunks (afx_stft_chunks with the
 * record of afx_assess_cost).  AFX_ERR_INVALID for a frame length < 1, negative offsets / lengths / noise_cap, a threshold
 * that is not finite.
 *
 * afx_compare_batch: pair i = ref[ref_offsets[i] .. + ref_lengths[i]) and deg[deg_offsets[i] .. + deg_lengths[i]), both of
 * sample_fmt in mem_kind (they may be one buffer); n = min of the two lengths samples of each are used.  out_rec holds
 * AFX_COMPARE_N doubles per pair: n, sum r, sum d, sum r^2, sum d^2, sum r d, sum (d - r)^2 -- float64 sums of float32
 * samples, the difference d - r alone taken in float32 first (numpy's degraded - reference) -- and, for the correlation of
 * signals with an offset, which those sums cancel in, the centred sums [7] sum (r - mean r)^2, [8] sum (d - mean d)^2,
 * [9] sum (r - mean r)(d - mean d): centred per span of 4096 samples on the span's means and joined around the pair's
 * (sum M_i + n_i (mean_i - mean)^2), still in one read.  Status values, reproducibility and independence as above
 * (AFX_CLIP_TOO_SHORT: n == 0).
 *
 * afx_assess_host / afx_compare_host (host-only): one clip / one pair through the same definitions in plain C++, sums in
 * sample order -- the specification of the kernels; they agree with them to rounding of the float64 sums, counts exactly.
 * afx_assess_cost (host-only): cost[6] for afx_stft_chunks, what = AFX_COST_ASSESS or AFX_COST_COMPARE (bytes per frame,
 * tile, sample, clip; frames per tile, most tiles).  The frame lengths are the caller's, so the record bounds the
 * workspace by the clip's samples: 17 bytes each (+ the upload) and 256 per clip; 1 (+ both uploads) for a pair. */
enum { AFX_ASSESS_N = 10, AFX_COMPARE_N = 10 };
enum { AFX_COST_ASSESS = 0, AFX_COST_COMPARE = 1 };
int afx_assess_cost(int what, int sample_fmt, int mem_kind, int64_t* cost /*[6]*/);
int afx_assess_host(const void* samples, int sample_fmt, int64_t n, int32_t frame_short, int32_t frame_long,
                    double threshold_db, int64_t noise_cap, double* out_rec /*[AFX_ASSESS_N]*/, int32_t* out_status);
int afx_compare_host(const void* ref, const void* deg, int sample_fmt, int64_t n_ref, int64_t n_deg,
                     double* out_rec /*[AFX_COMPARE_N]*/, int32_t* out_status);
int afx_assess_batch(afx_ctx* ctx, const void* samples, int sample_fmt, int mem_kind,
                     const int64_t* offsets, const int64_t* lengths, const int32_t* frame_short, const int32_t* frame_long,
                     int n_clips, double threshold_db, int64_t noise_cap,
                     double* out_rec /*[n_clips][AFX_ASSESS_N]*/, int32_t* out_status);
int afx_compare_batch(afx_ctx* ctx, const void* ref, const void* deg, int sample_fmt, int mem_kind,
                      const int64_t* ref_offsets, const int64_t* ref_lengths, const int64_t* deg_offsets,
                      const int64_t* deg_lengths, int n_pairs, double* out_rec /*[n_pairs][AFX_COMPARE_N]*/, int32_t* out_status);

/* The DFT of a whole clip, of any length, in float64, and the third term of the reference's PESQ-like score
 * (audio_quality_assessment.py:150-201, calculate_pesq_alternative): spec_dist = mean_k(| |R_k| - |D_k| | / (|R_k| + 1e-10))
 * over all N bins of R = np.fft.fft(reference), D = np.fft.fft(degraded).  All five symbols are newer than AFX_VERSION 107
 * says: a binding detects them by their presence.
 *
 * The transform is Bluestein's algorithm over the power of two M >= 2 N - 1: the chirp exp(-i pi k^2 / N) with its phase
 * reduced in integers (k^2 mod 2 N), three radix-2 transforms of M points in float64, the spectrum of the chirp filter
 * computed once per distinct N of a chunk.  N <= AFX_CFFT_MAX_N = 2^21 samples on the device (AFX_ERR_UNSUPPORTED above:
 * nothing is computed); the host executors take up to 2^27.
 *
 * afx_specdist_batch: the pairs of afx_compare_batch (same arguments; n = min of the two lengths).  The two real signals
 * of a pair go through ONE transform, Z = DFT(r + i d), R_k = (Z_k + conj Z_{N-k}) / 2, D_k = (Z_k - conj Z_{N-k}) / 2i.
 * out_rec holds AFX_SPECDIST_N doubles per pair: n, sum_k | |R_k| - |D_k| | / (|R_k| + 1e-10), sum_k |R_k|^2,
 * sum_k |D_k|^2 (Parseval: sum_k |R_k|^2 = n sum r^2), each over all n bins in an order that depends on n alone.  A pair
 * whose sides are equal sample for sample has D = R by definition, not to rounding: its distance is exactly 0, as numpy's is.
 * out_status (host): AFX_CLIP_TOO_SHORT for n == 0, AFX_CLIP_NONFINITE for a NaN / inf sample; the record of a failed pair is
 * NaN and no other pair is affected.  No atomics: a record is bit-reproducible and depends neither on the rest of the batch,
 * nor on the pair's place in it or in the buffer, nor on how the batch is cut into chunks (afx_stft_chunks with the record
 * of afx_specdist_cost).
 *
 * afx_clip_fft_batch: np.fft.rfft of clip i = samples[offsets[i] .. + lengths[i]): bins 0 .. N / 2 as interleaved float64
 * (re, im) at out[2 out_offsets[i] ..) in host memory, 2 (N / 2 + 1) doubles (NaN for a clip with a NaN / inf sample;
 * nothing is written for length 0).  The same transform with a zero imaginary part.
 *
 * afx_specdist_host / afx_clip_fft_host (host-only): one pair / one clip through the same definitions in plain C++ -- the
 * specification of the kernels; they agree with them to rounding.
 * afx_specdist_cost (host-only): cost[6] for afx_stft_chunks (bytes per frame, tile, sample, clip; frames per tile, most
 * tiles).  M < 4 n, so the work and the filter spectrum (counted for every pair, though pairs of one n share it) are
 * bounded by 128 bytes a sample, plus the uploads of both sides; 256 per pair. */
enum { AFX_SPECDIST_N = 4 };
#define AFX_CFFT_MAX_N (1 << 21)
int afx_specdist_cost(int sample_fmt, int mem_kind, int64_t* cost /*[6]*/);
int afx_specdist_host(const void* ref, const void* deg, int sample_fmt, int64_t n_ref, int64_t n_deg,
                      double* out_rec /*[AFX_SPECDIST_N]*/, int32_t* out_status);
int afx_clip_fft_host(const void* samples, int sample_fmt, int64_t n, double* out /*[2 * (n / 2 + 1)]*/, int32_t* out_status);
int afx_specdist_batch(afx_ctx* ctx, const void* ref, const void* deg, int sample_fmt, int mem_kind,
                       const int64_t* ref_offsets, const int64_t* ref_lengths, const int64_t* deg_offsets,
                       const int64_t* deg_lengths, int n_pairs, double* out_rec /*[n_pairs][AFX_SPECDIST_N]*/, int32_t* out_status);
int afx_clip_fft_batch(afx_ctx* ctx, const void* samples, int sample_fmt, int mem_kind, const int64_t* offsets,
                       const int64_t* lengths, int n_clips, double* out, const int64_t* out_offsets, int32_t* out_status);

/* Host-only (no device needed): the real FFT the frame kernel of the frame lengths that are not powers of two runs
 * (k_frames_mr), executed in float32 on the CPU with the same radix schedule, twiddle tables and operation order:
 * n_fft / 2 complex points through Stockham passes of radix 3, 5, 4, 8, then the real-FFT split.  out holds the
 * n_fft / 2 + 1 bins as (re, im) pairs.  For tests of the schedule and for bisecting a device mismatch.
 * AFX_ERR_UNSUPPORTED unless n_fft is a multiple of 16 in [256, 2048] with no prime factor other than 2, 3 and 5
 * (the set afx_plan_create accepts). */
int afx_rfft_host(int n_fft, const float* x /*[n_fft]*/, float* out /*[2 * (n_fft / 2 + 1)]*/);

/* preprocess_audio(y) (F:58-74): pre-emphasis + trim of ONE host clip.
 * out_y receives the n pre-emphasised samples (host, n floats); the kept span
 * is out_y[*start .. *end). */
int afx_preprocess(afx_plan* plan, const float* y, int64_t n,
                   float* out_y, int64_t* start, int64_t* end, int32_t* status);

/* ---- measurement ---------------------------------------------------------
 * When enabled, afx_extract_batch brackets every kernel with HIP events on the
 * plan's stream.  afx_plan_get_timings returns, per kernel slot, the summed
 * milliseconds and launch count since the last reset. */
enum {
  AFX_K_TRIM_BLOCKS = 0,   /* two-pass pipeline: per-512-sample block sums of squares of y_pre; samples-read-once pipeline
                              (n_fft 1024 / hop 256): the second frame-kernel launch over the frames a trim cut touches */
  AFX_K_TRIM_DECIDE = 1,   /* per-clip max / threshold scan -> [start,end), T */
  AFX_K_FRAMES = 2,        /* fused framing+window+rFFT+power+mel+dB (+RMS)  -- dominant */
  AFX_K_DCT = 3,           /* top_db clamp + DCT-II */
  AFX_K_STATS = 4,         /* delta/delta2 + per-clip statistics */
  AFX_K_COUNT = 5
};
/* enable: 0 off, 1 every kernel, 2 the frame kernel (AFX_K_FRAMES) only -- an event pair per kernel costs stream time
 * (about 5 us each, more with several batches in flight), so a throughput run times the one kernel it reports */
int afx_plan_set_timing(afx_plan* plan, int enable);
int afx_plan_get_timings(afx_plan* plan, float* ms_sum /*[AFX_K_COUNT]*/,
                         int32_t* launches /*[AFX_K_COUNT]*/, int reset);
/* The same launches as (start, end) intervals in milliseconds on a clock common to every plan of the device (one
 * reference event per device), newest `cap` of them, oldest first; *count = intervals held since the last reset.
 * With several plans (streams) in flight on one GPU their kernels overlap: the time the GPU spends in a kernel is
 * the union of the plans' intervals, not their sum -- bench.py merges them for `roofline.avg_launch_ms`. */
int afx_plan_get_intervals(afx_plan* plan, int kernel_slot, double* start_ms, double* end_ms, int cap, int32_t* count);

#ifdef __cplusplus
}
#endif
#endif /* AFX_H */
