// extract_f0 (pYIN) on the device: structures shared by afx_f0.hip, afx_tables.cpp and afx_api.cpp.
// Reference: audio_feature_extraction_toolkit/core/feature_extractor.py:76-114 (librosa.pyin at its defaults).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "afx_device.h"

namespace afx {

constexpr int kF0Thresholds = 100;     // librosa.pyin n_thresholds
constexpr int kF0FramesPerBlock = 16;  // frames one workgroup of k_f0_yin owns at most (8 where that fits a third workgroup per CU)

struct F0Params {
  int32_t n_fft, hop, W;               // frame_length, hop_length, win_length = frame_length / 2
  int32_t min_period, max_period;      // floor(sr / fmax), min(ceil(sr / fmin), n_fft - W - 1)
  int32_t n_tau;                       // max_period + 1 lags of the difference function
  int32_t n_tau_pad;                   // row stride of the energy rows (multiple of 64)
  int32_t n_lag;                       // max_period - min_period + 1 lags kept after normalisation
  int32_t n_bins;                      // pitch bins (10 per semitone from fmin)
  int32_t R;                           // ceil(n_tau / 64): lags per lane
  int32_t slots;                       // ceil(n_lag / 64): trough slots per lane
  int32_t cap;                         // candidate capacity per frame (>= number of possible troughs)
  int32_t band;                        // max_semitones_per_frame * bins_per_semitone (transition half-width)
  int32_t epb;                         // frames per block of k_f0_energy (64, 32 or 16)
  int32_t debug;                       // AFX_F0_DEBUG: timing-only ablation switches (results are wrong when set)
  double sr, fmin;
  double tiny;                         // np.finfo(float64).tiny
  double c0;                           // log(tiny): log of a zero probability
  double no_trough_prob;
  double bins_per_octave;              // 12 * bins_per_semitone
};

struct F0Tables {
  const double* thr;      // [101] np.linspace(0, 1, 101)
  const double* beta;     // [100] diff(beta.cdf(thr, 2, 18))
  const double* cumbeta;  // [101] cumbeta[n] = sum(beta[:n])
  const double* bfact;    // [cap + 1] (1 - e^-2) / (1 - e^-2n)  (scipy.stats.boltzmann.pmf normaliser)
  const double* bexp;     // [cap + 1] e^-2k
  const double* lt;       // [2][2 * band + 1][2 * band + 1] log(switch * local[row class][d] + tiny)
  const double* ltw;      // [2][2 * band + 1] the interior row as the band walk meets it: entry 2 band - e; stay row, then switch row
                          // (contiguous, so that the walk's scalar loads take several weights at once)
  const double* freqs;    // [n_bins] fmin * 2^(b / 120)
};

// (maximum, first arg-max) of one Viterbi value column: the best out-of-band source of the next step
struct VitBest { double value; int32_t arg; int32_t pad; };

struct HostF0Tables {
  F0Params p{};
  std::vector<double> thr, beta, cumbeta, bfact, bexp, lt, ltw, freqs;
};

// builds every table from (sr, n_fft, hop, fmin, fmax); returns false when the combination is unsupported
bool build_f0_tables(int sr, int n_fft, int hop, double fmin, double fmax, HostF0Tables& t, std::string& why);

// ---------------------------------------------------------------------------------------------
// Which kernels a configuration runs.  Everything from here to f0_dispatch is host arithmetic on F0Params (the kernels read
// the same layouts): the launchers of afx_f0.hip switch on the F0Dispatch it fills, afx_f0_dispatch (afx_host.cpp) hands it
// to the tests, and f0_plan applies the refusals -- one statement of the choice for all three.
// ---------------------------------------------------------------------------------------------
constexpr int kEnergyWaves = 4;       // waves per workgroup of k_f0_energy
constexpr int kE2Tile = 32;
constexpr int kVitThreads = 640;
constexpr int kBtWaves = 4;
constexpr int kBtWin = 256;                       // doubles per half column in a ring slot: two 1 KB DMA instructions
constexpr size_t kF0LdsLimit = 160 * 1024;

inline size_t f0_energy_lds_bytes(const F0Params& fp) {
  const size_t span = (size_t)(fp.epb - 1) * fp.hop + fp.W + fp.n_tau;
  return (span + span / fp.hop + 8) * 4 + (size_t)fp.n_tau * (fp.epb + 1) * 4;
}
__host__ __device__ inline size_t f0_energy2_span(const F0Params& fp, int lpw) {
  return (size_t)(kEnergyWaves * lpw - 1) * fp.hop + fp.W + fp.n_tau;
}
inline size_t f0_energy2_lds_bytes(const F0Params& fp, int lpw) {
  const size_t span = f0_energy2_span(fp, lpw);
  return (span + span / fp.hop + 8 + (size_t)kEnergyWaves * lpw * (kE2Tile + 1)) * 4;
}

struct YinLds { size_t span, per_wave, tables, total; };
// compact (the REF instantiation): the trough / candidate arrays CP, CB live in the D row behind its 64 event flags -- D is
// idle once the normalised difference is formed -- and the two tables that are only read with uniform indices (beta,
// cumbeta) come through the scalar cache: 39.7 KB per workgroup, a fourth workgroup per CU
__host__ __device__ inline YinLds yin_lds_i(int hop_, int n_fft_, int n_tau_pad_, int slots_, int cap_, int fpb, bool yf, bool compact = false) {
  YinLds L;
  L.span = (size_t)(fpb - 1) * hop_ + n_fft_ + 64;
  // per wave (doubles): D[n_tau_pad] | X[slots*64 + 2] | CP[cap] | CB[cap] (ints, cap/2 doubles)
  L.per_wave = (size_t)n_tau_pad_ + (size_t)slots_ * 64 + 2 + cap_ + (cap_ + 1) / 2;
  // shared tables: thr[101] | beta[100] | cumbeta[101] | bfact[cap+1] | bexp[cap+1]
  L.tables = 101 + 100 + 101 + 2 * ((size_t)cap_ + 1);
  // the staged signal is kept as the float32 it is (converted on read: half the bytes of the autocorrelation's LDS reads and
  // 20 KB less per workgroup); span is rounded up to an even count so that the double arrays behind it stay 8-byte aligned
  // (yf: the instantiations with at most 6 lags per lane; the lag-heavy ones re-read the signal 11..16 times per step and keep it
  // as float64 -- a conversion per read costs them more than the bytes)
  L.span = (L.span + 1) & ~(size_t)1;
  if (compact) {
    L.per_wave = (size_t)n_tau_pad_ + (size_t)slots_ * 64 + 2;
    L.tables = 101 + 2 * ((size_t)cap_ + 1);
  }
  L.total = L.span * (yf ? sizeof(float) : sizeof(double)) + (4 * L.per_wave + L.tables) * sizeof(double);
  return L;
}
__host__ __device__ inline YinLds yin_lds(const F0Params& fp, int fpb, bool yf) {
  return yin_lds_i(fp.hop, fp.n_fft, fp.n_tau_pad, fp.slots, fp.cap, fpb, yf);
}
// frames one workgroup owns: 16, or 8 where that (and only that) lets a third workgroup onto the CU -- the kernel is bound by
// how often a wave gets to issue, and the lag-heavy instantiations (more than 6 lags per lane) cannot use a third wave anyway
inline int f0_yin_frames_per_block(const F0Params& fp) {
  const int need = fp.R > fp.slots ? fp.R : fp.slots;
  const size_t third = 160 * 1024 / 3;
  return (need <= 6 && yin_lds(fp, 16, true).total > third && yin_lds(fp, 8, true).total <= third) ? 8 : 16;
}
inline size_t f0_yin_lds_bytes(const F0Params& fp) {
  const int need = fp.R > fp.slots ? fp.R : fp.slots;
  return yin_lds(fp, f0_yin_frames_per_block(fp), need <= 6).total;
}

// The shapes k_f0_yin has compiled in (its template parameter SH; 0: any shape, from the parameters): 1 the reference's
// (22050 Hz, frame_length 1024, C2..C7), 2 the same pitch range at 16 kHz, frame_length 512 (BASELINE configs[2]), 3 the same at
// 44.1 kHz, frame_length 2048 (configs[4]).
template <int SH> struct YinShape { static constexpr int hop = 0, W = 0, n_fft = 0, R = 0, slots = 0, n_lag = 0, n_tau = 0, n_tau_pad = 0, min_period = 0, max_period = 0, cap = 0, n_bins = 0; };
template <> struct YinShape<1> { static constexpr int hop = 256, W = 512, n_fft = 1024, R = 6, slots = 6, n_lag = 329, n_tau = 339, n_tau_pad = 384, min_period = 10, max_period = 338, cap = 168, n_bins = 601; };
template <> struct YinShape<2> { static constexpr int hop = 128, W = 256, n_fft = 512, R = 4, slots = 4, n_lag = 239, n_tau = 246, n_tau_pad = 256, min_period = 7, max_period = 245, cap = 128, n_bins = 601; };
template <> struct YinShape<3> { static constexpr int hop = 512, W = 1024, n_fft = 2048, R = 11, slots = 11, n_lag = 655, n_tau = 676, n_tau_pad = 704, min_period = 21, max_period = 675, cap = 336, n_bins = 601; };
template <int SH>
inline bool yin_shape_is(const F0Params& fp) {
  typedef YinShape<SH> Y;
  return fp.hop == Y::hop && fp.W == Y::W && fp.n_fft == Y::n_fft && fp.R == Y::R && fp.slots == Y::slots && fp.n_lag == Y::n_lag &&
         fp.n_tau == Y::n_tau && fp.n_tau_pad == Y::n_tau_pad && fp.min_period == Y::min_period && fp.max_period == Y::max_period &&
         fp.cap == Y::cap && fp.n_bins == Y::n_bins;
}

struct VitLds { size_t v, olp, lt, red, edge, total; };
__host__ __device__ inline VitLds vit_lds(int n_bins, int band_) {
  const size_t S = 2 * (size_t)n_bins, width = 2 * (size_t)band_ + 1;
  VitLds L;
  L.v = 0;                                   // two value columns of 2 (n_bins + 2 band) + 4 band doubles
  L.olp = 2 * (S + 8 * band_);               // 3 n_bins doubles
  L.lt = L.olp + 3 * n_bins;                 // width * width doubles: the `stay` rows (k_f0_backtrack holds both tables)
  L.red = L.lt + width * width;              // 32 doubles + 32 ints (16 doubles): two sets of per-wave partials
  L.edge = L.red + 48;                       // per wave 4 x 2 band doubles (its best edge-class move per range-end target); 2 counters
  L.total = (L.edge + (size_t)(kVitThreads / 64) * 8 * band_ + 2) * sizeof(double);
  return L;
}
inline size_t f0_viterbi_lds_bytes(const F0Params& fp) { return vit_lds(fp.n_bins, fp.band).total; }

// depth of k_f0_backtrack's ring: the window of +- (D - 1) band bins around the bin just decided must fit kBtWin
__host__ __device__ inline int f0_bt_depth(int band) { return 2 * band * 5 + 2 <= kBtWin ? 6 : 5; }
// also requires 2 band + 1 <= 64 (a lane per source of the band)
inline size_t f0_backtrack_lds_bytes(const F0Params& fp) {
  const size_t width = 2 * (size_t)fp.band + 1;
  return (2 * width * width + 2 + (size_t)kBtWaves * (f0_bt_depth(fp.band) + 1) * 2 * kBtWin) * sizeof(double);
}

// The instantiation of each of the four kernels a configuration runs.
struct F0Dispatch {
  int32_t energy_lpw;          // 0: k_f0_energy; otherwise k_f0_energy2<LPW> (lanes per wave that carry a frame)
  int32_t epb;                 // frames per workgroup of that kernel: F0Params::epb, or kEnergyWaves * LPW
  int32_t yin_n, yin_fpb, yin_sh;   // k_f0_yin<N, N, FPB, SH>
  int32_t vit_nbt, vit_bandt;  // k_f0_viterbi<0, NBT, BANDT>; 0 / 0: n_bins and band from the parameters
  int32_t vit_tpt;             // targets per Viterbi thread: ceil(n_bins / kVitThreads)
  int32_t bt_depth;            // k_f0_backtrack<D>
  int32_t yin_lds;             // dynamic LDS of the k_f0_yin launch, bytes (the compact layout for SH 1)
};
inline F0Dispatch f0_dispatch(const F0Params& fp) {
  F0Dispatch d{};
  // energy: k_f0_energy2 needs W % hop == 0 (afx_f0.hip); 8 lanes per wave, or 4 for the long hops, if that keeps the
  // workgroup's samples within a quarter of the CU's LDS (four workgroups per CU)
  d.energy_lpw = 0; d.epb = fp.epb;
  if (fp.W % fp.hop == 0 && fp.n_tau <= fp.W) {
    for (int lpw = 8; lpw >= 4 && !d.energy_lpw; lpw -= 4)
      if (f0_energy2_lds_bytes(fp, lpw) <= 40 * 1024) { d.energy_lpw = lpw; d.epb = kEnergyWaves * lpw; }
  }
  const int need = fp.R > fp.slots ? fp.R : fp.slots;
  const int fpb = f0_yin_frames_per_block(fp);
  d.yin_lds = (int32_t)f0_yin_lds_bytes(fp);
  if (yin_shape_is<1>(fp) && fpb == 8) {
    d.yin_n = 6; d.yin_fpb = 8; d.yin_sh = 1;
    d.yin_lds = (int32_t)yin_lds_i(fp.hop, fp.n_fft, fp.n_tau_pad, fp.slots, fp.cap, 8, true, true).total;
  } else if (yin_shape_is<2>(fp) && fpb == 16) {
    d.yin_n = 4; d.yin_fpb = 16; d.yin_sh = 2;
  } else if (yin_shape_is<3>(fp) && fpb == 16) {
    d.yin_n = 11; d.yin_fpb = 16; d.yin_sh = 3;
  } else {
    d.yin_n = need <= 4 ? 4 : need <= 6 ? 6 : need <= 8 ? 8 : need <= 11 ? 11 : 16;
    d.yin_fpb = need <= 6 ? fpb : 16;
    d.yin_sh = 0;
  }
  // n_bins 601 is fmin / fmax of the reference; band 25 at hop / sr = 256 / 22050 and 512 / 44100, band 15 at 128 / 16000
  if (fp.n_bins == 601 && (fp.band == 25 || fp.band == 15)) { d.vit_nbt = 601; d.vit_bandt = fp.band; }
  d.vit_tpt = (fp.n_bins + kVitThreads - 1) / kVitThreads;
  d.bt_depth = f0_bt_depth(fp.band);
  return d;
}
// build_f0_tables, then the limits of the kernels (LDS per workgroup, the 64 lanes of k_f0_backtrack), then the dispatch:
// false + `why` for a configuration extract_f0 refuses.  afx_f0_batch and afx_f0_dispatch both decide here.
bool f0_plan(int sr, int n_fft, int hop, double fmin, double fmax, HostF0Tables& t, F0Dispatch& d, std::string& why);

// per-frame candidate record sizes (device workspace)
inline size_t f0_cand_bins_bytes(const F0Params& fp, int64_t frames) { return (size_t)frames * fp.cap * sizeof(int16_t); }
inline size_t f0_cand_prob_bytes(const F0Params& fp, int64_t frames) { return (size_t)frames * fp.cap * sizeof(double); }
// Viterbi value columns kept for back-tracking: 2 n_bins doubles per frame
inline size_t f0_vrows_bytes(const F0Params& fp, int64_t frames) { return (size_t)frames * 2 * fp.n_bins * sizeof(double); }

hipError_t launch_f0_prep(hipStream_t s, const void* samples, const ClipDesc* clips, const ClipInfo* info,
                          float* ysig, int n_clips, int64_t max_len, const KParams& kp);
hipError_t launch_f0_energy(hipStream_t s, const float* ysig, const ClipDesc* clips, const ClipInfo* info,
                            float* energy, int n_clips, int max_tmax, const F0Params& fp);
hipError_t launch_f0_yin(hipStream_t s, const float* ysig, const ClipDesc* clips, const ClipInfo* info,
                         const float* energy, const F0Tables& tb, const F0Params& fp,
                         int32_t* cand_cnt, double* cand_vp, int16_t* cand_bin, double* cand_prob /* nullable: diagnostics */,
                         double* cand_lp, double* cand_lu, int n_clips, int max_tmax);
hipError_t launch_f0_viterbi(hipStream_t s, const ClipDesc* clips, const ClipInfo* info, const F0Tables& tb,
                             const F0Params& fp, const int32_t* cand_cnt,
                             const int16_t* cand_bin, const double* cand_lp, const double* cand_lu,
                             double* vrows, VitBest* vbest,
                             uint16_t* states, double* out_stats, double* out_f0, const int64_t* f0_offsets,
                             int n_clips);

hipError_t launch_zcr(hipStream_t s, const float* ysig, const ClipDesc* clips, const ClipInfo* info, int n_fft, int hop,
                      double* out, const int64_t* out_offsets, int n_clips, int max_tmax);

}  // namespace afx
