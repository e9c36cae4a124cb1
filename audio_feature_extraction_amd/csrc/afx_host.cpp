// Host-only part of libafx.so: the error string, the version, and the builders that need no device -- the clip records of
// a batch (what prepare_descriptors uploads), the packed image of a host batch (pack_pieces, scatter_pieces), the chunk cut
// of the STFT-based groups (cut_stft_chunk, afx_stft_chunks), the
// pYIN tables, the pYIN kernel dispatch (afx_f0_dispatch), the chroma filterbank (afx_chroma_filters) and the tempo table
// (afx_tempo_table).  Together with afx_tables.cpp, afx_f0_tables.cpp and afx_wav.cpp this is everything that parses
// caller- or file-supplied data on the host; `make asan` builds exactly these files (plus afx_host_stubs.cpp) with
// g++ -fsanitize=address,undefined as libafx_host_asan.so.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <string>

#include "afx_device.h"
#include "afx_f0.h"
#include "afx_groups.h"
#include "afx_denoise.h"
#include "afx_hpss.h"
#include "afx_internal.h"
#include "afx_mr.h"

namespace afx {

static thread_local std::string g_err;
void set_error(const std::string& s) { g_err = s; }

// The per-clip records of a ragged batch (reference: batch_process walks files of any length,
// audio_feature_extraction_toolkit/core/feature_extractor.py:228-235): frame slots padded to whole 16-frame blocks,
// trim-block slots, block indices.  false + `why` on input the kernels' 32-bit frame arithmetic cannot hold.
bool build_clip_descs(int hop, int trim_hop, const int64_t* offsets, const int64_t* lengths, int n, ClipDesc* out,
                      BatchGeom& g, std::string& why) {
  g = BatchGeom{};
  if (hop <= 0 || trim_hop <= 0) { why = "hop / trim hop must be positive"; return false; }
  int64_t fb = 0, tb = 0, nblk = 0;
  int max_tb = 0, max_tm = 0;
  const int64_t kMaxElems = (int64_t)1 << 46;                 // offsets + lengths stay far from overflow
  for (int i = 0; i < n; ++i) {
    if (lengths[i] < 0 || offsets[i] < 0) { why = "negative clip offset/length"; return false; }
    if (offsets[i] > kMaxElems) { why = "clip offset too large"; return false; }
    if (lengths[i] / hop > (int64_t)1 << 30 || lengths[i] > kMaxElems) { why = "clip too long"; return false; }
    ClipDesc& c = out[i];
    c.off = offsets[i]; c.len = lengths[i];
    c.tmax = (int32_t)(1 + lengths[i] / hop);
    c.tpad = (c.tmax + kFramesPerBlock - 1) / kFramesPerBlock * kFramesPerBlock;
    c.frame_base = fb; c.tblk_base = tb;
    fb += c.tpad;
    const int64_t ntb = (lengths[i] + trim_hop - 1) / trim_hop;
    tb += ntb;
    max_tb = (int)std::max<int64_t>(max_tb, std::min<int64_t>(ntb, INT32_MAX));
    max_tm = std::max<int>(max_tm, c.tmax);
    c.blk_base = (int32_t)nblk; c.pad_ = 0;
    nblk += c.tpad / kFramesPerBlock;
    if (nblk > (int64_t)1 << 30 || tb > (int64_t)1 << 40) { why = "batch too large"; return false; }
  }
  g.total_tpad = fb; g.total_tblk = tb; g.max_tblocks = std::max(max_tb, 1); g.max_tmax = max_tm; g.nblocks = (int)nblk;
  return true;
}

void cut_stft_chunk(const int64_t* offsets, const int64_t* lengths, int n_clips, int first, int64_t budget,
                    const StftCost& cost, StftChunk& ck) {
  ck.recs.clear(); ck.idx.clear();
  ck.frames = ck.samples = ck.spec_floats = ck.hi = ck.max_len = 0; ck.lo = INT64_MAX; ck.tiles = 0;
  int64_t bytes = 0;
  int c1 = first;
  for (; c1 < n_clips && (int)ck.recs.size() < kStftChunkClips; ++c1) {
    const int64_t L = lengths[c1];
    if (L == 0) continue;
    const int64_t T = 1 + L / 512, nt = (T + cost.tile - 1) / cost.tile;
    const int64_t pb = T * cost.per_frame + nt * cost.per_tile + L * cost.per_sample + cost.per_clip;
    if (!ck.recs.empty() && (bytes + pb > budget || (int64_t)ck.tiles + nt > cost.tile_cap)) break;
    HpssClip r{};
    r.in_off = offsets[c1]; r.y_off = ck.samples; r.len = L; r.frame_base = ck.frames; r.spec_off = ck.spec_floats;
    r.T = (int32_t)T; r.tile_base = ck.tiles;
    ck.recs.push_back(r); ck.idx.push_back(c1);
    ck.frames += T; ck.samples += L; ck.spec_floats += cost.spec_floats * T; ck.tiles += (int)nt; bytes += pb;
    ck.lo = std::min(ck.lo, offsets[c1]); ck.hi = std::max(ck.hi, offsets[c1] + L); ck.max_len = std::max(ck.max_len, L);
  }
  ck.next = c1;
}

// What a clip costs a chunk of afx_groups_batch.  Buffers whose lifetimes do not overlap share space: the power rows of h lie
// where X lay (dead behind k_hpss_mask), so the harmonic group adds no power rows of its own.
void groups_cost(int groups, bool preprocess, StftCost& cost) {
  const bool sp = groups & AFX_GROUP_SPECTRAL, ha = groups & AFX_GROUP_HARMONIC, ti = groups & AFX_GROUP_TIMBRE, rh = groups & AFX_GROUP_RHYTHM;
  constexpr int64_t kWin = kRhMaxWin, kBand = 1023, kDesc = kSpecFloats * 4;
  cost = StftCost{};
  cost.per_frame = ((sp || ti || rh) ? kHpssPowPitch * 4 : 0)              // the power rows of y
                   + (sp ? kDesc : 0)                                      // its descriptor rows
                   + (ha ? 2 * kHpssPitch * 8 + kDesc : 0)                 // X, Yh; the centroid rows of h
                   + (ti ? kBand * 5 + 4 * 8 + 2 * 8 : 0)                  // piptrack's peaks, k_chroma_apply's and k_mfcc_rows' sums
                   + ((ti || rh) ? kRhMels * 4 : 0)                        // the mel dB rows
                   + (rh ? 4 : 0);                                         // the envelope
  cost.per_tile = rh ? kWin * 8 : 0;
  cost.per_sample = 4 + 4 + (ha ? 4 : 0)                                   // the upload, y, h
                    + (preprocess ? 4 + 10 : 0);                           // the filter's output; its tiles (36 872 B per 4096 samples)
  cost.per_clip = 128 + 8 * 4 + kGroupsStats * 8 + 2 * 4 + (sp ? 8 * 8 : 0) + (ha ? sizeof(HpssClip) + 4 * 8 : 0)
                  + (ti ? kChromaHist * 4 + 4 * 8 + 2 * 8 : 0) + (rh ? kWin * 8 + 4 * 8 : 0)
                  + (preprocess ? 2 * ((int64_t)kFiltTile * 8 + (int64_t)kFiltB * kFiltZ * 8 + 8) + sizeof(FiltClip) + sizeof(FiltState) : 0);
  cost.tile = 16;
  cost.tile_cap = ha ? 65535 : INT32_MAX / 2;             // k_hpss_mask's grid holds 65535 tiles of 64 frames: never more than these
}

// What a clip costs a chunk of afx_denoise_batch: the rows k_dn_frames writes and k_hpss_ola reads; y, the output and the
// upload; with the VAD the energies, which a clip of L samples has at most L + 1 of; the profile row, the record, the info.
void denoise_cost(int flags, int sample_fmt, int mem_kind, StftCost& cost) {
  const bool vad = (flags & AFX_DENOISE_VAD) != 0;
  cost = StftCost{};
  cost.per_frame = kHpssPitch * 8;
  cost.per_sample = 4 + 4 + (mem_kind != AFX_MEM_HOST ? 0 : sample_fmt == AFX_FMT_S16 ? 2 : 4) + (vad ? 4 : 0);
  cost.per_clip = 128 + kDnProfPitch * 4 + kDnInfo * 8 + (vad ? 4 : 0);
  cost.tile = kHpssTile;                                  // no kernel here works in tiles; the count only has to fit an int
  cost.tile_cap = INT32_MAX / 2;
}

void groups_dct_table(int n_mels, float* out) {
  std::fill(out, out + kGroupsMfcc * kRhMels, 0.f);
  const double M = (double)n_mels;
  for (int k = 0; k < kGroupsMfcc; ++k)
    for (int m = 0; m < n_mels; ++m)
      out[k * kRhMels + m] = (float)(std::sqrt((k == 0 ? 1.0 : 2.0) / M) * std::cos(M_PI * (double)k * (2.0 * m + 1.0) / (2.0 * M)));
}

// The packed image a context entry point uploads for a host batch, and the way back of a downloaded one.
void scatter_pieces(void* dst, const std::vector<HostPiece>& pieces) {
  for (const HostPiece& p : pieces)
    if (p.n_bytes > 0) std::memcpy((char*)dst + p.dst_bytes, p.src, (size_t)p.n_bytes);
}

void pack_pieces(std::vector<char>& image, int64_t total_bytes, const std::vector<HostPiece>& pieces) {
  image.assign((size_t)total_bytes, 0);
  scatter_pieces(image.data(), pieces);
}

// One Stockham pass of radix R over N2 points, butterfly by butterfly as k_frames_mr's lanes take them.
template <int R>
static void mr_host_pass(const mrc* in, mrc* out, const mrc* tw, int N2, int NS) {
  const int nbf = N2 / R, step = N2 / (NS * R);
  for (int j = 0; j < nbf; ++j) {
    mrc x[R];
    for (int r = 0; r < R; ++r) x[r] = in[j + r * nbf];
    const int jm = j % NS;
    mr_butterfly<R>(x, tw, jm, step, NS == 1);
    for (int r = 0; r < R; ++r) out[(j - jm) * R + jm + r * NS] = x[r];
  }
}

}  // namespace afx

using namespace afx;

// The kernel's real FFT on the CPU, float32 throughout: z[n] = x[2n] + i x[2n+1], the schedule's passes, the split.
extern "C" int afx_rfft_host(int n_fft, const float* x, float* out) {
  if (!x || !out) { set_error("afx_rfft_host: null argument"); return AFX_ERR_INVALID; }
  if (!mr_supported(n_fft)) {
    set_error("afx_rfft_host: frame_length must be a multiple of 16 in [256, 2048] with no prime factor other than 2, 3 and 5");
    return AFX_ERR_UNSUPPORTED;
  }
  const int N2 = n_fft / 2;
  std::vector<float> twf, postf;
  build_fft_tables(n_fft, twf, postf);
  const mrc* tw = reinterpret_cast<const mrc*>(twf.data());
  const mrc* post = reinterpret_cast<const mrc*>(postf.data());
  std::vector<mrc> a((size_t)N2), b((size_t)N2);
  for (int n = 0; n < N2; ++n) a[n] = mr_mk(x[2 * n], x[2 * n + 1]);
  const MrSchedule sc = mr_schedule(N2);
  int NS = 1;
  for (int p = 0; p < sc.n; ++p) {
    switch (sc.radix(p)) {
      case 3: mr_host_pass<3>(a.data(), b.data(), tw, N2, NS); break;
      case 4: mr_host_pass<4>(a.data(), b.data(), tw, N2, NS); break;
      case 5: mr_host_pass<5>(a.data(), b.data(), tw, N2, NS); break;
      default: mr_host_pass<8>(a.data(), b.data(), tw, N2, NS); break;
    }
    NS *= sc.radix(p);
    a.swap(b);
  }
  for (int k = 0; k < N2; ++k) {
    const mrc X2 = mr_split2(a[k], a[(N2 - k) % N2], post[k]);
    out[2 * k] = 0.5f * X2.x; out[2 * k + 1] = 0.5f * X2.y;
  }
  out[2 * N2] = a[0].x - a[0].y; out[2 * N2 + 1] = 0.f;
  return AFX_OK;
}

extern "C" int afx_version(void) { return AFX_VERSION; }

extern "C" const char* afx_last_error(void) { return g_err.c_str(); }

extern "C" int afx_batch_geometry(const afx_params* p, const int64_t* offsets, const int64_t* lengths, int n_clips,
                                  int64_t* records, int64_t* totals) {
  if (!p || n_clips < 0 || (n_clips > 0 && (!offsets || !lengths))) { set_error("afx_batch_geometry: null/invalid argument"); return AFX_ERR_INVALID; }
  std::string msg;
  int st = validate_params(*p, msg);
  if (st != AFX_OK) { set_error(msg); return st; }
  std::vector<ClipDesc> cd((size_t)std::max(n_clips, 1));
  BatchGeom g;
  if (!build_clip_descs(p->hop, p->trim_hop, offsets, lengths, n_clips, cd.data(), g, msg)) { set_error("afx_batch_geometry: " + msg); return AFX_ERR_INVALID; }
  if (records)
    for (int i = 0; i < n_clips; ++i) {
      int64_t* r = records + 4 * (size_t)i;
      r[0] = cd[i].frame_base; r[1] = cd[i].tmax; r[2] = cd[i].tpad; r[3] = cd[i].blk_base;
    }
  if (totals) { totals[0] = g.total_tpad; totals[1] = g.nblocks; totals[2] = g.total_tblk; totals[3] = g.max_tmax; }
  return AFX_OK;
}

extern "C" int afx_f0_build_tables(int sr, int n_fft, int hop, double fmin, double fmax, int32_t* info,
                                   double* beta, double* lt, double* freqs) {
  HostF0Tables t;
  std::string why;
  if (!build_f0_tables(sr, n_fft, hop, fmin, fmax, t, why)) { set_error("afx_f0_build_tables: " + why); return AFX_ERR_UNSUPPORTED; }
  if (info) {
    const int32_t v[8] = {t.p.min_period, t.p.max_period, t.p.n_bins, t.p.band, t.p.cap, t.p.n_lag, t.p.R, t.p.slots};
    std::memcpy(info, v, sizeof(v));
  }
  if (beta) std::memcpy(beta, t.beta.data(), t.beta.size() * sizeof(double));
  if (lt) std::memcpy(lt, t.lt.data(), t.lt.size() * sizeof(double));
  if (freqs) std::memcpy(freqs, t.freqs.data(), t.freqs.size() * sizeof(double));
  return AFX_OK;
}


extern "C" int afx_f0_dispatch(int sr, int n_fft, int hop, double fmin, double fmax, int32_t* out) {
  if (!out) { set_error("afx_f0_dispatch: null argument"); return AFX_ERR_INVALID; }
  if (sr <= 0 || hop <= 0 || n_fft < 2 || n_fft > 4096) { set_error("afx_f0_dispatch: sr, hop_length must be positive and frame_length in [2, 4096]"); return AFX_ERR_INVALID; }
  HostF0Tables t;
  F0Dispatch d;
  std::string why;
  if (!f0_plan(sr, n_fft, hop, fmin, fmax, t, d, why)) { set_error("afx_f0_dispatch: " + why); return AFX_ERR_UNSUPPORTED; }
  const int32_t v[12] = {d.energy_lpw, d.epb, d.yin_n, d.yin_fpb, d.yin_sh, d.vit_nbt, d.vit_bandt, d.vit_tpt, d.bt_depth,
                         t.p.band, t.p.n_bins, d.yin_lds};
  std::memcpy(out, v, sizeof(v));
  return AFX_OK;
}

extern "C" int afx_stft_chunks(const int64_t* lengths, int n_clips, const int64_t* cost, int64_t budget, int32_t* chunk_of) {
  if (n_clips < 0 || !cost || (n_clips > 0 && (!lengths || !chunk_of))) { set_error("afx_stft_chunks: null/invalid argument"); return AFX_ERR_INVALID; }
  // the sums of a chunk stay below 2^63: a clip costs less than 2^55 bytes, and a chunk is cut before it passes the budget
  for (int k = 0; k < 6; ++k)
    if (cost[k] < (k >= 4 ? 1 : 0) || cost[k] > (k >= 4 ? INT32_MAX : k == 3 ? 1 << 30 : 1 << 20)) { set_error("afx_stft_chunks: cost out of range"); return AFX_ERR_INVALID; }
  if (budget < 1 || budget > (int64_t)1 << 62) { set_error("afx_stft_chunks: budget must be in [1, 2^62]"); return AFX_ERR_INVALID; }
  for (int i = 0; i < n_clips; ++i)
    if (lengths[i] < 0 || lengths[i] > (int64_t)1 << 31) { set_error("afx_stft_chunks: lengths must be in [0, 2^31]"); return AFX_ERR_INVALID; }
  const StftCost c{cost[0], cost[1], cost[2], cost[3], cost[4], cost[5], 0};
  const std::vector<int64_t> offsets((size_t)n_clips, 0);
  std::fill(chunk_of, chunk_of + n_clips, -1);
  StftChunk ck;
  int32_t chunk = 0;
  for (int c0 = 0; c0 < n_clips; c0 = ck.next) {
    cut_stft_chunk(offsets.data(), lengths, n_clips, c0, budget, c, ck);
    if (ck.idx.empty()) continue;
    for (int i : ck.idx) chunk_of[i] = chunk;
    ++chunk;
  }
  return AFX_OK;
}

extern "C" int afx_groups_cost(int groups, int flags, int64_t* cost) {
  if (!cost) { set_error("afx_groups_cost: null argument"); return AFX_ERR_INVALID; }
  if (groups <= 0 || (groups & ~kGroupsAll)) { set_error("afx_groups_cost: groups must be a non-empty set of AFX_GROUP_* bits"); return AFX_ERR_INVALID; }
  StftCost c;
  groups_cost(groups, (flags & AFX_GROUPS_PREPROCESS) != 0, c);
  const int64_t v[6] = {c.per_frame, c.per_tile, c.per_sample, c.per_clip, c.tile, c.tile_cap};
  std::memcpy(cost, v, sizeof(v));
  return AFX_OK;
}

extern "C" int afx_denoise_cost(int flags, int sample_fmt, int mem_kind, int64_t* cost) {
  if (!cost) { set_error("afx_denoise_cost: null argument"); return AFX_ERR_INVALID; }
  if (flags & AFX_FLAG_TRIM) { set_error("afx_denoise_cost: trim is not applied here; pass the preprocessed signal"); return AFX_ERR_UNSUPPORTED; }
  if (flags & ~(AFX_FLAG_PREEMPH | AFX_DENOISE_RMS_GAIN | AFX_DENOISE_VAD)) { set_error("afx_denoise_cost: unknown flag"); return AFX_ERR_INVALID; }
  if ((sample_fmt != AFX_FMT_F32 && sample_fmt != AFX_FMT_S16) || (mem_kind != AFX_MEM_HOST && mem_kind != AFX_MEM_DEVICE)) {
    set_error("afx_denoise_cost: unknown sample format or memory kind");
    return AFX_ERR_INVALID;
  }
  StftCost c;
  denoise_cost(flags, sample_fmt, mem_kind, c);
  const int64_t v[6] = {c.per_frame, c.per_tile, c.per_sample, c.per_clip, c.tile, c.tile_cap};
  std::memcpy(cost, v, sizeof(v));
  return AFX_OK;
}

extern "C" int afx_groups_dct_table(int n_mels, float* out) {
  if (!out) { set_error("afx_groups_dct_table: null argument"); return AFX_ERR_INVALID; }
  if (n_mels < 1 || n_mels > kRhMels) { set_error("afx_groups_dct_table: n_mels must be in 1 .. 128"); return AFX_ERR_INVALID; }
  groups_dct_table(n_mels, out);
  return AFX_OK;
}

// librosa.filters.chroma(sr, 2048, tuning, n_chroma=12, ctroct=5, octwidth=2, norm=2, base_c=True): float64 throughout, one
// rounding to float32 (tests/chroma_ref.py chroma_filters is the spec).  Column j's width needs q[j + 1] only, and the norm
// is per column, so the 1025 columns kept are all that is computed.
extern "C" int afx_chroma_filters(int sr, double tuning, float* out) {
  if (!out) { set_error("afx_chroma_filters: null argument"); return AFX_ERR_INVALID; }
  if (sr <= 0 || !std::isfinite(tuning)) { set_error("afx_chroma_filters: sr must be positive and tuning finite"); return AFX_ERR_INVALID; }
  constexpr int NB = 1025;
  const double a440 = 440.0 * std::pow(2.0, tuning / 12.0) / 16.0, step = (double)sr / 2048.0;
  double q[NB + 1];
  for (int j = 1; j <= NB; ++j) q[j] = 12.0 * std::log2(((double)j * step) / a440);
  q[0] = q[1] - 18.0;
  for (int j = 0; j < NB; ++j) {
    const double bw = std::max(q[j + 1] - q[j], 1.0);
    double w[12], ss = 0.0;
    for (int c = 0; c < 12; ++c) {
      const double d = std::fmod(q[j] - (double)c + 6.0 + 120.0, 12.0) - 6.0, e = 2.0 * d / bw;
      w[c] = std::exp(-0.5 * (e * e));
      ss += w[c] * w[c];
    }
    const double norm = std::max(std::sqrt(ss), DBL_MIN), o = (q[j] / 12.0 - 5.0) / 2.0, oct = std::exp(-0.5 * (o * o));
    for (int c = 0; c < 12; ++c) out[c * NB + j] = (float)(w[(c + 3) % 12] / norm * oct);     // roll(-3): row c is pitch class c + 3
  }
  return AFX_OK;
}

// librosa.feature.tempo's table for librosa.beat.beat_track's call (hop 512, ac_size 8, start_bpm 120, std_bpm 1,
// max_tempo 320): win = int(8 sr) // 512 lags, bpm = tempo_frequencies, the log-normal prior with every lag faster than
// max_tempo removed (tests/rhythm_ref.py tempo_table is the spec).  float64 in the order numpy evaluates it.
extern "C" int afx_tempo_table(int sr, int32_t* out_win, int32_t* out_kmin, double* out_bpm, double* out_logprior) {
  if (sr <= 0) { set_error("afx_tempo_table: sr must be positive"); return AFX_ERR_INVALID; }
  const int64_t win = ((int64_t)8 * sr) / 512;
  if (win < 2 || win > 768) {
    set_error("afx_tempo_table: the 8 s tempogram window must hold 2 .. 768 frames of hop 512 (128 <= sr <= 49215)");
    return AFX_ERR_UNSUPPORTED;
  }
  int kmin = 0;
  for (int k = 0; k < (int)win; ++k) {
    const double bpm = k == 0 ? INFINITY : (60.0 * (double)sr) / (512.0 * (double)k);
    if (kmin == 0 && bpm < 320.0) kmin = k;              // the first lag slower than max_tempo (0 when there is none)
    const double d = std::log2(bpm) - std::log2(120.0);
    if (out_bpm) out_bpm[k] = bpm;
    if (out_logprior) out_logprior[k] = -0.5 * (d * d);
  }
  if (out_logprior) for (int k = 0; k < kmin; ++k) out_logprior[k] = -INFINITY;
  if (out_win) *out_win = (int32_t)win;
  if (out_kmin) *out_kmin = kmin;
  return AFX_OK;
}
