// k_frames_mr<FMT>: the fused frame kernel of the frame lengths that are not powers of two (gfx950): n_fft = 400 / hop = 160
// at 16 kHz, the 25 ms / 10 ms speech front end of 04_feature_extraction_experiment/feature_extraction.py:35-41 and
// feature_extraction_for_student.py:33-44, and every other multiple of 16 in [256, 2048] with prime factors 2, 3, 5.
// Same contract as k_frames (afx_frames.hip): one workgroup per 16-frame BlockDesc; the hop-strided sample block is staged
// once (pre-emphasis + trim mask); per frame window -> real FFT -> |X|^2 into PB[bin][17] and the RMS of the unwindowed
// frame; the block-sparse Slaney mel on the matrix pipe (exact-f32 v_mfma_f32_16x16x4_f32) -> 10 log10 -> log-mel tile
// [mel/4][frame][mel%4] (+ clip maximum).  The staging and mel phases are restated here, not shared through a header:
// k_frames' instantiations keep their code objects.
//
// The FFT (afx_mr.h): one wave per frame, N2 = n_fft / 2 complex points in one LDS image per wave, Stockham passes of
// radix 3, 5, 4, 8 walked at run time from a per-workgroup pass table.  A pass is N2 / R butterflies strided over the
// 64 lanes; a lane reads every input of its butterflies, then writes their outputs (LDS operations of one wave complete
// in order, so one image serves both sides of a pass; wave_lds_order() between the two sides, between passes and around
// the split keeps the compiler from moving an access of the image across).  Where 64 does not divide N2 / R (200 = 5 * 5 * 8: 40 and 25
// butterflies) the idle lanes neither read nor write.  Twiddles, window and split factors are the plan's tables, copied
// to LDS once per workgroup.
//
// LDS banks: a complex point is two dwords.  The first pass writes point R j + r from lane j: R is odd (every length
// here has a factor 3 or 5 and mr_schedule puts those first), so 16 consecutive lanes step 2 R dwords and cover the 32
// banks of a ds_write_b64 group exactly once.  Later passes write runs of NS >= 3 consecutive points; two runs that meet
// in one 16-lane group overlap on at most a few banks (2-way), which a ds_write_b64 absorbs (its LDS-array cycles stay
// under its transfer cycles).  Every read of a pass is 64 consecutive points: conflict-free without padding, so the image
// carries none (k_frames pads because its power-of-two first pass would put 16 lanes on two bank pairs).
#include <hip/hip_runtime.h>

#include <cstdlib>

#include "afx_device.h"
#include "afx_mr.h"
#include "afx_wave.h"

namespace afx {

namespace {

constexpr int kPbStride = 17;   // power-spectrum rows: 16 frames + 1 pad (conflict-free column writes)
constexpr int kSchInts = 8;     // pass table: R, NS, butterflies, twiddle step, magic of j / NS, 0, 0, 0

__host__ __device__ inline int round4(int x) { return (x + 3) & ~3; }

struct MrLds { int s, ex, pb, win, tw, post, rb, sch, total; };   // float offsets
__host__ __device__ inline MrLds mr_lds(int n_fft, int hop) {
  const int N2 = n_fft / 2;
  MrLds L;
  L.s = 0;
  L.ex = L.s + round4((kFramesPerBlock - 1) * hop + n_fft);
  L.pb = L.ex + kWaves * N2 * 2;                                  // one complex image per wave
  L.win = L.pb + round4((N2 + 1 + kPbPadRows) * kPbStride);
  L.tw = L.win + n_fft;
  L.post = L.tw + 2 * N2;
  L.rb = L.post + 2 * N2;
  L.sch = L.rb + kMelMaxSlots * 256;
  L.total = L.sch + kMrMaxPasses * kSchInts;
  return L;
}

typedef float f32x4 __attribute__((ext_vector_type(4)));

// The wave's image is read and written in place by all 64 lanes: every read of a phase must be issued before the first
// write of the next, and every write before the next phase's reads.  The hardware does that for one wave (its LDS
// operations complete in issue order); this keeps the compiler to the same order, whatever it can prove about aliasing.
// No instruction is emitted.
__device__ __forceinline__ void wave_lds_order() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// One pass of radix R of one frame by one wave.  FIRST: the inputs are the staged samples times the window (and their
// squares feed the frame's RMS); no twiddles.
template <int R, bool FIRST>
__device__ __forceinline__ void mr_pass(mrc* __restrict__ ex, const float* Sf, const mrc* WT, const mrc* TW,
                                        int NS, int nbf, int step, int magic, int lane, bool hop_even, float& ss) {
  constexpr int MAXB = (1024 / R + 63) / 64;       // butterflies a lane can own (N2 <= 1024)
  mrc x[MAXB][R];
#pragma unroll
  for (int i = 0; i < MAXB; ++i) {
    const int j = lane + 64 * i;
#pragma unroll
    for (int r = 0; r < R; ++r) x[i][r] = mr_mk(0.f, 0.f);
    if (j < nbf) {
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int a = j + r * nbf;
        if constexpr (FIRST) {
          mrc s;
          if (hop_even) s = *reinterpret_cast<const mrc*>(Sf + 2 * a);
          else { s.x = Sf[2 * a]; s.y = Sf[2 * a + 1]; }
          const mrc w = WT[a];
          ss += s.x * s.x; ss += s.y * s.y;
          x[i][r] = mr_mk(s.x * w.x, s.y * w.y);
        } else {
          x[i][r] = ex[a];
        }
      }
    }
  }
  wave_lds_order();                                // all reads of the pass, then its writes
#pragma unroll
  for (int i = 0; i < MAXB; ++i) {
    const int j = lane + 64 * i;
    if (j < nbf) {
      const int q = (int)(((unsigned)j * (unsigned)magic) >> 20);      // j / NS, exact for j < 1024, NS <= 512
      const int jm = j - q * NS;
      mr_butterfly<R>(x[i], TW, jm, step, FIRST);
      mrc* o = ex + (j - jm) * R + jm;
#pragma unroll
      for (int r = 0; r < R; ++r) o[r * NS] = x[i][r];
    }
  }
  wave_lds_order();                                // the next pass (or the split) reads what other lanes wrote
}

}  // namespace

template <int FMT>
__global__ __launch_bounds__(256, 2) void k_frames_mr(const void* __restrict__ samples, ClipInfo* __restrict__ info,
                                                      const BlockDesc* __restrict__ blocks, int nblocks, DevTables tb,
                                                      KParams kp, float* __restrict__ logmel, float* __restrict__ rms_rows) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int n_fft = kp.n_fft, hop = kp.hop, M = kp.n_mels;
  const int N2 = n_fft / 2, NB = N2 + 1;
  const MrLds L = mr_lds(n_fft, hop);
  float* const S_ = smem + L.s;
  float* const PB = smem + L.pb;
  mrc* const WT = reinterpret_cast<mrc*>(smem + L.win);
  mrc* const TW = reinterpret_cast<mrc*>(smem + L.tw);
  mrc* const PT = reinterpret_cast<mrc*>(smem + L.post);
  float* const RB = smem + L.rb;
  int* const SCH = reinterpret_cast<int*>(smem + L.sch);

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  mrc* const EX = reinterpret_cast<mrc*>(smem + L.ex) + wave * N2;

  // ---- once per workgroup: pad rows of PB, the tables, the pass table
  for (int i = tid; i < kPbPadRows * kPbStride; i += 256) PB[NB * kPbStride + i] = 0.f;
  {
    const mrc* w2 = reinterpret_cast<const mrc*>(tb.window);
    const mrc* t2 = reinterpret_cast<const mrc*>(tb.tw);
    const mrc* p2 = reinterpret_cast<const mrc*>(tb.post);
    for (int i = tid; i < N2; i += 256) { WT[i] = w2[i]; TW[i] = t2[i]; PT[i] = p2[i]; }
  }
  if (tid == 0) {
    const MrSchedule sc = mr_schedule(N2);
    int NS = 1;
#pragma unroll
    for (int p = 0; p < kMrMaxPasses; ++p) {
      const int R = p < sc.n ? sc.radix(p) : 0;
      int* e = SCH + p * kSchInts;
      e[0] = R; e[1] = NS;
      e[2] = R ? N2 / R : 0;
      e[3] = R ? N2 / (NS * R) : 0;
      e[4] = ((1 << 20) + NS - 1) / NS;
      if (R) NS *= R;
    }
  }
  // mel: the per-lane triangle coefficients of this wave's first work items (all of them when n_mels <= 128) stay in
  // registers; the items' wave-uniform metadata is re-read per block through the scalar cache (held across the FFT phase
  // it would push the kernel past its scalar registers)
  const int wv = __builtin_amdgcn_readfirstlane(wave);
  const int f16k = lane & 15;
  const int mel_cnt = tb.mel_item_cnt[0] * (wv == 0) + tb.mel_item_cnt[1] * (wv == 1) + tb.mel_item_cnt[2] * (wv == 2) +
                      tb.mel_item_cnt[3] * (wv == 3);
  float4 mi_cf[kMelRegItems];
  float mi_ko[kMelRegItems];
#pragma unroll
  for (int i = 0; i < kMelRegItems; ++i) {
    mi_cf[i] = make_float4(0.f, 0.f, 0.f, 0.f); mi_ko[i] = 0.f;
    if (i < mel_cnt) {
      const int g = tb.mel_items[(wv * kMelMaxItems + i) * 2].x;
      mi_cf[i] = tb.mel_coef[g * 16 + f16k];
      mi_ko[i] = tb.mel_koff[g * 16 + f16k];
    }
  }

  const bool pre = (kp.flags & AFX_FLAG_PREEMPH) != 0;
  const float b1 = kp.preemph_b1;
  const int slen = (kFramesPerBlock - 1) * hop + n_fft;
  const bool hop_even = (hop & 1) == 0;
  __syncthreads();

  for (int b = blockIdx.x; b < nblocks; b += gridDim.x) {
    const BlockDesc bd = blocks[b];
    if (!bd.active) continue;                       // uniform: the whole workgroup skips the block's barriers

    // ---- stage the block: samples gs + j (zeros outside the clip), pre-emphasis as lfilter does it (zi = 2 y0 - y1 on
    // the clip's sample 0), trim mask -- once per sample
    {
      const int lo = bd.have_lo, hi = bd.have_hi - 1;              // hi >= lo: active clips have >= 2 samples
      const unsigned span = (unsigned)(bd.keep_hi - bd.keep_lo);
      auto at = [&](int jj) {
        const int jc = jj < lo ? lo : (jj > hi ? hi : jj);
        const float v = ld_raw<FMT>(samples, bd.sample_base + jc);
        return (jj == jc) ? v : 0.f;
      };
      for (int j = tid; j < slen; j += 256) {
        const float y = at(j);
        float v = y;
        if (pre) {
          v = preemph1(y, at(j - 1), b1);
          if (j == lo) v = preemph0(ld_raw<FMT>(samples, bd.clip_off), ld_raw<FMT>(samples, bd.clip_off + 1));
        }
        S_[j] = ((unsigned)(j - bd.keep_lo) < span) ? v : 0.f;
      }
    }
    __syncthreads();

    // ---- per frame (one wave each, four in turn): window -> N2-point complex FFT -> split -> |X|^2, and the RMS
#pragma unroll 1
    for (int it = 0; it < kFramesPerBlock / kWaves; ++it) {
      const int fl = wave * (kFramesPerBlock / kWaves) + it;
      const float* Sf = S_ + fl * hop;
      float ss = 0.f;
#pragma unroll 1
      for (int p = 0; p < kMrMaxPasses; ++p) {
        auto sg = [](int v) { return __builtin_amdgcn_readfirstlane(v); };
        const int* e = SCH + p * kSchInts;
        const int R = sg(e[0]);
        if (R == 0) break;
        const int NS = sg(e[1]), nbf = sg(e[2]), step = sg(e[3]), magic = sg(e[4]);
        if (p == 0) {
          switch (R) {
            case 3: mr_pass<3, true>(EX, Sf, WT, TW, NS, nbf, step, magic, lane, hop_even, ss); break;
            case 5: mr_pass<5, true>(EX, Sf, WT, TW, NS, nbf, step, magic, lane, hop_even, ss); break;
            case 4: mr_pass<4, true>(EX, Sf, WT, TW, NS, nbf, step, magic, lane, hop_even, ss); break;
            default: mr_pass<8, true>(EX, Sf, WT, TW, NS, nbf, step, magic, lane, hop_even, ss); break;
          }
        } else {
          switch (R) {
            case 3: mr_pass<3, false>(EX, Sf, WT, TW, NS, nbf, step, magic, lane, hop_even, ss); break;
            case 5: mr_pass<5, false>(EX, Sf, WT, TW, NS, nbf, step, magic, lane, hop_even, ss); break;
            case 4: mr_pass<4, false>(EX, Sf, WT, TW, NS, nbf, step, magic, lane, hop_even, ss); break;
            default: mr_pass<8, false>(EX, Sf, WT, TW, NS, nbf, step, magic, lane, hop_even, ss); break;
          }
        }
      }
      ss = wave_sum(ss);
      if (lane == 0 && bd.t0 + fl < bd.T) rms_rows[bd.frame_slot + fl] = sqrtf(ss / (float)n_fft);

      // real-FFT split: X[k] from Z[k] and Z[N2 - k]; EX holds Z in natural order
      float* const pcol = PB + fl;
#pragma unroll 2
      for (int k = lane; k < N2; k += 64) {
        const mrc z = EX[k], m = EX[k ? N2 - k : 0];
        const mrc X2 = mr_split2(z, m, PT[k]);
        pcol[k * kPbStride] = 0.25f * (X2.x * X2.x + X2.y * X2.y);
        if (k == 0) { const float ny = z.x - z.y; pcol[N2 * kPbStride] = ny * ny; }
      }
      wave_lds_order();                            // the next frame's first pass overwrites the image the split read
    }
    __syncthreads();

    // ---- mel filterbank + dB on the matrix pipe: D[16 filters][16 frames] += A[16x4] * B[4 bins x 16 frames] over the
    // non-zero 16x4 blocks of librosa.filters.mel (MelBlocks, afx_internal.h); the A operand is evaluated per lane.  A
    // group with no bin under any of its filters has no blocks: its rows are 10 log10(amin), and nothing is read.
    const int f16 = lane & 15, q4 = lane >> 4;
    const bool valid = (bd.t0 + f16) < bd.T;
    float lmax = -INFINITY;
    float* tile = logmel + bd.frame_slot * (int64_t)M;
    auto mel_item = [&](int kmin, int b0, int nb, const float4 cf, const float ko) -> f32x4 {
      const float* p0 = PB + (kmin + 4 * b0 + q4) * kPbStride + f16;
      const float* const pmax = PB + (NB + kPbPadRows - 1) * kPbStride + f16;    // a zero pad row
      float kf = (float)(q4 + 4 * b0) + ko;                       // k - kc of this lane's bin, exact
      f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
      for (int bk = 0; bk < nb; bk += 8) {
        float pb[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const float* p = p0 + i * 4 * kPbStride;
          pb[i] = *(p < pmax ? p : pmax);
        }
        p0 += 8 * 4 * kPbStride;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const float lo = fmaf(cf.y, kf, cf.x), hi = fmaf(cf.w, kf, cf.z);
          float w = __builtin_amdgcn_fmed3f(0.f, lo, hi);           // max(0, min(lo, hi))
          w = (bk + i < nb) ? w : 0.f;                               // the next part of a split group owns those bins
          if (i & 1) acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(w, pb[i], acc1, 0, 0, 0);
          else acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(w, pb[i], acc0, 0, 0, 0);
          kf += 4.0f;
        }
      }
      return acc0 + acc1;
    };
    auto mel_finish = [&](const f32x4 acc, int g) {
      float lv[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        // 10*log10(max(amin, mel)); v_log_f32 is log2
        lv[r] = 3.01029995663981195f * __builtin_amdgcn_logf(fmaxf(kp.amin, acc[r]));
        if (valid && g * 16 + q4 * 4 + r < M) lmax = fmaxf(lmax, lv[r]);
      }
      // tile layout [mel/4][frame][mel%4]: this lane's four filters are one 16-byte store (n_mels is a multiple of 4)
      const int m0 = g * 16 + q4 * 4;
      if (valid && m0 < M) *reinterpret_cast<float4*>(tile + (m0 >> 2) * 64 + f16 * 4) = make_float4(lv[0], lv[1], lv[2], lv[3]);
    };
    int wb = wv;                                 // opaque per block: keeps the item records out of the loop-invariant set
    asm volatile("" : "+s"(wb));
    const int4* const items = tb.mel_items + wb * kMelMaxItems * 2;
    f32x4 held[kMelRegItems];
#pragma unroll
    for (int i = 0; i < kMelRegItems; ++i) {
      held[i] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (i < mel_cnt) {
        const int4 ia = items[2 * i], ib = items[2 * i + 1];       // (group, b0, nb, role), (slot, nslots, -, -)
        held[i] = mel_item(tb.mel_grp[ia.x].x, ia.y, ia.z, mi_cf[i], mi_ko[i]);
        if (ia.w == 0) mel_finish(held[i], ia.x);
        else if (ia.w == 1) *reinterpret_cast<f32x4*>(RB + ib.x * 256 + lane * 4) = held[i];
      }
    }
    for (int i = kMelRegItems; i < mel_cnt; ++i) {            // n_mels > 128: whole groups, tables re-read
      const int4 ia = items[2 * i];
      const f32x4 acc = mel_item(tb.mel_grp[ia.x].x, ia.y, ia.z, tb.mel_coef[ia.x * 16 + f16], tb.mel_koff[ia.x * 16 + f16]);
      mel_finish(acc, ia.x);
    }
    if (tb.mel_n_slots > 0) {                                    // uniform for the whole grid
      __syncthreads();
#pragma unroll
      for (int i = 0; i < kMelRegItems; ++i) {
        if (i < mel_cnt) {
          const int4 ia = items[2 * i], ib = items[2 * i + 1];
          if (ia.w == 2) {
            f32x4 acc = held[i];
            for (int sl = 0; sl < ib.y; ++sl)
              acc += *reinterpret_cast<const f32x4*>(RB + (ib.x + sl) * 256 + lane * 4);
            mel_finish(acc, ia.x);
          }
        }
      }
    }
    const float mx = wave_max(lmax);
    if (lane == 0 && mx > -INFINITY) atomicMax(&info[bd.clip].lmax_ord, f2ord(mx));
    // no barrier here: the next staging writes only S_ (dead since the barrier behind the FFT phase), PB is rewritten
    // behind the next staging barrier, and a partial-sum slot behind two.
  }
}

bool frames_mr_shape(int n_fft) { return mr_supported(n_fft) && (n_fft & (n_fft - 1)) != 0; }

size_t frames_mr_lds_bytes(int n_fft, int hop) {
  if (!frames_mr_shape(n_fft) || hop <= 0) return 0;
  const int64_t s = (int64_t)(kFramesPerBlock - 1) * hop + n_fft;      // a hop no LDS could hold must not wrap the int layout
  if (s > (int64_t)1 << 20) return (size_t)1 << 30;
  return (size_t)mr_lds(n_fft, hop).total * sizeof(float);
}

hipError_t launch_frames_mr(hipStream_t s, const void* samples, ClipInfo* info, const BlockDesc* blocks, int nblocks,
                            const DevTables& tb, const KParams& kp, float* logmel, float* rms_rows, int grid) {
  const size_t lds = frames_mr_lds_bytes(kp.n_fft, kp.hop);
  if (lds == 0 || lds > 160 * 1024) return hipErrorInvalidValue;
  if (kp.fmt == AFX_FMT_S16) {
    const hipError_t e = allow_lds_once<k_frames_mr<AFX_FMT_S16>>();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((k_frames_mr<AFX_FMT_S16>), dim3(grid), dim3(256), lds, s, samples, info, blocks, nblocks, tb, kp,
                       logmel, rms_rows);
  } else {
    const hipError_t e = allow_lds_once<k_frames_mr<AFX_FMT_F32>>();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((k_frames_mr<AFX_FMT_F32>), dim3(grid), dim3(256), lds, s, samples, info, blocks, nblocks, tb, kp,
                       logmel, rms_rows);
  }
  return hipGetLastError();
}

}  // namespace afx
