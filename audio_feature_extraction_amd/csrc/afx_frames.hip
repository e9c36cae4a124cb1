// k_frames<NFFT, STAMP>: the generic fused frame kernel of libafx.so (gfx950), n_fft 256 .. 2048 at any hop
// (reference call sites: audio_feature_extraction_toolkit/core/feature_extractor.py:127, 164).  One workgroup per
// 16-frame block: staging of the hop-strided sample block (pre-emphasis + trim mask) -> periodic window -> real FFT
// (N/2-point complex Stockham in LDS: FC / Pass / Sched below) -> |X|^2 -> sparse Slaney mel on the matrix pipe
// (exact-f32 v_mfma_f32_16x16x4_f32, block-sparse filterbank) -> 10*log10 -> log-mel tile (+ clip max), and the RMS
// of the same staged frame.  The shapes with a wave-level kernel (afx_frames3*.hip) do not come here.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <type_traits>

#include "afx_device.h"
#include "afx_devenv.h"
#include "afx_wave.h"

namespace afx {

#define AFX_CBARRIER() asm volatile("" ::: "memory")
// Workgroup barrier that orders LDS only.  __syncthreads() also drains vmcnt, which would wait for
// the sample prefetch (and the log-mel stores) at every phase boundary.
#define AFX_LDS_BARRIER()                                   \
  do {                                                      \
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      \
    __builtin_amdgcn_s_barrier();                           \
    asm volatile("" ::: "memory");                          \
  } while (0)

// ---------------------------------------------------------------------------
// k_frames: the fused per-frame kernel
// ---------------------------------------------------------------------------
template <int NFFT>
struct FC {
  static constexpr int N2 = NFFT / 2;              // complex points
  static constexpr int NB = N2 + 1;                // rfft bins
  static constexpr int LPF = (N2 / 8 >= 64) ? 64 : N2 / 8;   // lanes per frame
  static constexpr int P = N2 / LPF;               // complex points per lane (8 or 16)
  static constexpr int FPW = 64 / LPF;             // frames a wave transforms at once
  static constexpr int EXN = N2 + (N2 >> 3);       // padded complex slots of one exchange buffer
  static constexpr int ITERS = kFramesPerBlock / (kWaves * FPW);
};

__host__ __device__ inline int round4(int x) { return (x + 3) & ~3; }

constexpr int kPbStride = 17;   // power-spectrum rows: 16 frames + 1 pad (conflict-free column writes)

// n_fft = 1024 (the headline configuration) runs a hand-scheduled 8x8x8 core: XOR-swizzled
// exchange image without padding, window / split twiddles in LDS, two frames in flight per wave.
__host__ __device__ inline bool fast1024(int n_fft) { return n_fft == 1024; }

struct LdsLayout { int s, ex, pb, tab, rb, total; };   // float offsets
__host__ __device__ inline LdsLayout lds_layout(int n_fft, int hop) {
  const int N2 = n_fft / 2;
  const int lpf = (N2 / 8 >= 64) ? 64 : N2 / 8;
  const int fpw = 64 / lpf;
  const int exn = fast1024(n_fft) ? N2 : N2 + (N2 >> 3);
  LdsLayout L;
  L.s = 0;
  L.ex = L.s + round4((kFramesPerBlock - 1) * hop + n_fft);
  L.pb = L.ex + kWaves * fpw * exn * 2;
  L.tab = L.pb + round4((N2 + 1 + kPbPadRows) * kPbStride);
  L.rb = L.tab + (fast1024(n_fft) ? 4 * N2 : 0);         // window[N2] float2 + post[N2] float2
  L.total = L.rb + kMelMaxSlots * 256 + (fast1024(n_fft) ? 128 : 0);   // mel partial sums; pass-2 twiddles W64^(c*r), 8x8 float2
  return L;
}

size_t frames_lds_bytes(int n_fft, int hop) {
  if (n_fft != 256 && n_fft != 512 && n_fft != 1024 && n_fft != 2048) return 0;
  return (size_t)lds_layout(n_fft, hop).total * sizeof(float);
}

__device__ __forceinline__ float2 cmul(float2 a, float2 b) {
  return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}
__device__ __forceinline__ float2 cadd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 csub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ float2 mul_mi(float2 a) { return make_float2(a.y, -a.x); }   // a * (-i)

__device__ __forceinline__ void dft4(float2& x0, float2& x1, float2& x2, float2& x3) {
  const float2 a = cadd(x0, x2), b = csub(x0, x2), c = cadd(x1, x3), d = mul_mi(csub(x1, x3));
  x0 = cadd(a, c); x1 = cadd(b, d); x2 = csub(a, c); x3 = csub(b, d);
}

template <int R> __device__ __forceinline__ void dft(float2* x);
template <> __device__ __forceinline__ void dft<4>(float2* x) { dft4(x[0], x[1], x[2], x[3]); }
template <> __device__ __forceinline__ void dft<8>(float2* x) {
  float2 e0 = x[0], e1 = x[2], e2 = x[4], e3 = x[6];
  float2 o0 = x[1], o1 = x[3], o2 = x[5], o3 = x[7];
  dft4(e0, e1, e2, e3);
  dft4(o0, o1, o2, o3);
  const float h = 0.70710678118654752440f;
  o1 = make_float2((o1.x + o1.y) * h, (o1.y - o1.x) * h);      // * W8^1
  o2 = mul_mi(o2);                                             // * W8^2
  o3 = make_float2((o3.y - o3.x) * h, (-o3.x - o3.y) * h);     // * W8^3
  x[0] = cadd(e0, o0); x[1] = cadd(e1, o1); x[2] = cadd(e2, o2); x[3] = cadd(e3, o3);
  x[4] = csub(e0, o0); x[5] = csub(e1, o1); x[6] = csub(e2, o2); x[7] = csub(e3, o3);
}

__device__ __forceinline__ int expad(int a) { return a + (a >> 3); }

// One Stockham autosort pass of radix R with NS = product of earlier radices.
// A lane owns the points a_u = lif + LPF*u (u < P) in every pass; butterfly i of
// the lane takes u = i + r*(P/R).  Outputs go to the exchange buffer at
// expand(j) + r*NS; the last pass lands on the lane's own slots.
template <int N2, int LPF, int P, int R, int NS>
struct Pass {
  static constexpr int NBF = P / R;
  static constexpr int NTW = (NS > 1) ? NBF * (R - 1) : 0;
  static constexpr int STEP = N2 / (NS * R);
  static constexpr bool LAST = (NS * R == N2);

  __device__ static __forceinline__ void load_tw(const float2* __restrict__ tab, int lif, float2* tw) {
    if constexpr (NS > 1) {
#pragma unroll
      for (int i = 0; i < NBF; ++i) {
        const int jm = (lif + LPF * i) & (NS - 1);
#pragma unroll
        for (int r = 1; r < R; ++r) tw[i * (R - 1) + r - 1] = tab[jm * r * STEP];
      }
    }
  }

  __device__ static __forceinline__ void run(float2* v, const float2* tw, float2* ex, int lif) {
#pragma unroll
    for (int i = 0; i < NBF; ++i) {
      float2 x[R];
#pragma unroll
      for (int r = 0; r < R; ++r) x[r] = v[i + r * NBF];
      if constexpr (NS > 1) {
#pragma unroll
        for (int r = 1; r < R; ++r) x[r] = cmul(x[r], tw[i * (R - 1) + r - 1]);
      }
      dft<R>(x);
      const int j = lif + LPF * i;
      const int j0 = (j & ~(NS - 1)) * R + (j & (NS - 1));
#pragma unroll
      for (int r = 0; r < R; ++r) {
        ex[expad(j0 + r * NS)] = x[r];
        if constexpr (LAST) v[i + r * NBF] = x[r];
      }
    }
    AFX_CBARRIER();
    if constexpr (!LAST) {
#pragma unroll
      for (int u = 0; u < P; ++u) v[u] = ex[expad(lif + LPF * u)];
      AFX_CBARRIER();
    }
  }
};

// radix schedules
template <int NFFT> struct Sched;
template <> struct Sched<256>  { using C = FC<256>;  using P1 = Pass<C::N2, C::LPF, C::P, 8, 1>; using P2 = Pass<C::N2, C::LPF, C::P, 4, 8>;  using P3 = Pass<C::N2, C::LPF, C::P, 4, 32>;  using P4 = void; };
template <> struct Sched<512>  { using C = FC<512>;  using P1 = Pass<C::N2, C::LPF, C::P, 8, 1>; using P2 = Pass<C::N2, C::LPF, C::P, 8, 8>;  using P3 = Pass<C::N2, C::LPF, C::P, 4, 64>;  using P4 = void; };
template <> struct Sched<1024> { using C = FC<1024>; using P1 = Pass<C::N2, C::LPF, C::P, 8, 1>; using P2 = Pass<C::N2, C::LPF, C::P, 8, 8>;  using P3 = Pass<C::N2, C::LPF, C::P, 8, 64>;  using P4 = void; };
template <> struct Sched<2048> { using C = FC<2048>; using P1 = Pass<C::N2, C::LPF, C::P, 8, 1>; using P2 = Pass<C::N2, C::LPF, C::P, 8, 8>;  using P3 = Pass<C::N2, C::LPF, C::P, 4, 64>;  using P4 = Pass<C::N2, C::LPF, C::P, 4, 256>; };

template <typename PX> struct NTW { static constexpr int v = PX::NTW; };
template <> struct NTW<void> { static constexpr int v = 0; };

// Raw samples of one staged quad: the 4 samples (bit pattern of the vector load: float4, or 4 x int16
// in .x/.y) and the sample before them.  Kept as native vector registers: a struct of five floats made
// hipcc merge the two loads into an unaligned dwordx4 plus a dword and then shuffle -- and wait -- per quad.
struct RawQuad { float4 q; float prev; };

struct BlkCtx {          // uniform per workgroup; one BlockDesc resolved into scalars
  int64_t sample_base, frame_slot, clip_off;
  int keep_lo, keep_hi, have_lo, have_hi;
  int clip, t0, T;
  bool active, interior;
};

// staged index j -> raw samples j-1 .. j+3 of the block (zeros outside the clip).
// Branch-free on purpose: a per-lane "load or keep" branch makes hipcc wait vmcnt(0) inside every
// branch, which serialises the prefetch.  `interior` is uniform per block: every staged sample and its
// predecessor exist and the quads are 16-byte (F32) / 8-byte (S16) aligned -> one plain vector load per
// quad; the predecessor comes from the neighbouring lane at staging time, so only the wave's first lane
// needs it from memory: all lanes load that one (wave-uniform) address.  Edge blocks take clamped
// scalar loads + selects and carry a per-lane predecessor.
template <bool INTERIOR, int FMT>
__device__ __forceinline__ RawQuad load_raw(const void* __restrict__ samples, const BlkCtx& c, int j, int jwave) {
  RawQuad r;
  if constexpr (INTERIOR) {
    if constexpr (FMT == AFX_FMT_F32) {
      const float* base = (const float*)samples + c.sample_base;
      r.q = *reinterpret_cast<const float4*>(base + j);
      r.prev = base[jwave - 1];
    } else {
      const int16_t* base = (const int16_t*)samples + c.sample_base;
      const int2 q = *reinterpret_cast<const int2*>(base + j);
      r.q = make_float4(__int_as_float(q.x), __int_as_float(q.y), 0.f, 0.f);
      r.prev = (float)base[jwave - 1] * (1.0f / 32768.0f);
    }
  } else {
    const int lo = c.have_lo, hi = c.have_hi - 1;          // hi >= lo: clips have >= 2 samples
    auto at = [&](int jj) {
      const int jc = jj < lo ? lo : (jj > hi ? hi : jj);
      const float v = ld_sample(samples, FMT, c.sample_base + jc);
      return (jj == jc) ? v : 0.f;
    };
    r.prev = at(j - 1);
    r.q = make_float4(at(j), at(j + 1), at(j + 2), at(j + 3));
  }
  return r;
}

// pre-emphasis (as lfilter does it) + trim mask of one quad -> 4 staged samples
template <bool INTERIOR, int FMT>
__device__ __forceinline__ float4 stage_quad(const RawQuad& r, const void* __restrict__ samples,
                                             const BlkCtx& c, int j, bool pre, float b1) {
  float y0, y1, y2, y3, prev;
  if constexpr (INTERIOR && FMT == AFX_FMT_S16) {
    const int a = __float_as_int(r.q.x), b = __float_as_int(r.q.y);
    const float sc = 1.0f / 32768.0f;
    y0 = (float)(short)(a & 0xffff) * sc; y1 = (float)(short)(a >> 16) * sc;
    y2 = (float)(short)(b & 0xffff) * sc; y3 = (float)(short)(b >> 16) * sc;
  } else { y0 = r.q.x; y1 = r.q.y; y2 = r.q.z; y3 = r.q.w; }
  if constexpr (INTERIOR) {
    // predecessor = previous lane's last sample (DPP wave_shr:1); lane 0 keeps the loaded one
    prev = __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(r.prev), __float_as_int(y3), 0x138, 0xf, 0xf, false));
  } else prev = r.prev;
  float v0 = y0, v1 = y1, v2 = y2, v3 = y3;
  if (pre) {
    v0 = preemph1(y0, prev, b1); v1 = preemph1(y1, y0, b1);
    v2 = preemph1(y2, y1, b1); v3 = preemph1(y3, y2, b1);
    if constexpr (!INTERIOR) {            // only edge blocks can hold the clip's sample 0
      const int e0 = c.have_lo - j;
      if (e0 >= 0 && e0 < 4) {            // librosa's zi = 2*y[0] - y[1]
        const float z = preemph0(ld_sample(samples, FMT, c.clip_off), ld_sample(samples, FMT, c.clip_off + 1));
        if (e0 == 0) v0 = z; else if (e0 == 1) v1 = z; else if (e0 == 2) v2 = z; else v3 = z;
      }
    }
  }
  const unsigned span = (unsigned)(c.keep_hi - c.keep_lo), d = (unsigned)(j - c.keep_lo);
  float4 o;
  o.x = (d < span) ? v0 : 0.f;
  o.y = (d + 1u < span) ? v1 : 0.f;
  o.z = (d + 2u < span) ? v2 : 0.f;
  o.w = (d + 3u < span) ? v3 : 0.f;
  return o;
}

typedef float f32x4 __attribute__((ext_vector_type(4)));

// Power-spectrum buffer PB[bin][17]: frame f of bin k at k*17 + f.  The per-frame column
// write (64 consecutive bins, fixed f) walks banks in steps of 17 -> conflict-free; the
// mel stage reads 4 consecutive bins x 16 frames per wave -> one 2-way overlap at most.

// STAMP = true is a separate diagnostic instantiation (AFX_DEBUG_STAMPS): lane 0 of every wave sums
// s_memtime deltas per phase into `stamps`; the production kernel carries none of it.
enum { ST_STAGE = 0, ST_BAR1, ST_FFT, ST_PREFETCH, ST_BAR2, ST_MEL, ST_BAR3, ST_MELFIN, ST_X0, ST_X1, ST_X2, ST_X3, ST_COUNT };

template <int NFFT, bool STAMP>
__global__ __launch_bounds__(256, (NFFT >= 2048 ? 1 : 2)) void k_frames(const void* __restrict__ samples,
                                                   ClipInfo* __restrict__ info,
                                                   const BlockDesc* __restrict__ blocks, int nblocks,
                                                   DevTables tb, KParams kp,
                                                   float* __restrict__ logmel,
                                                   float* __restrict__ rms_rows,
                                                   unsigned long long* __restrict__ stamps) {
  using C = FC<NFFT>;
  unsigned long long st_sum[ST_COUNT] = {}, st_prev = 0;
  auto stamp = [&](int ph) {
    if constexpr (STAMP) {
      __builtin_amdgcn_sched_barrier(0);
      const unsigned long long t = __builtin_amdgcn_s_memtime();
      __builtin_amdgcn_s_waitcnt(0xC07F);          // lgkmcnt(0) only
      __builtin_amdgcn_sched_barrier(0);
      if (ph >= 0) st_sum[ph] += t - st_prev;
      st_prev = t;
    }
  };
  using S = Sched<NFFT>;
  constexpr int N2 = C::N2, NB = C::NB, LPF = C::LPF, P = C::P, FPW = C::FPW;
  constexpr int MAXCH = (NFFT * 5 + 1023) / 1024;    // 1024-sample chunks a thread prefetches (hop <= n_fft/4)
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int hop = kp.hop, M = kp.n_mels;
  const LdsLayout L = lds_layout(NFFT, hop);
  float* const S_ = smem + L.s;
  float* const PB = smem + L.pb;

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int lif = lane % LPF, fsub = lane / LPF;
  constexpr bool FAST = (NFFT == 1024);
  constexpr int EXSTRIDE = FAST ? N2 : C::EXN;
  float2* const EX = reinterpret_cast<float2*>(smem + L.ex) + (wave * FPW + fsub) * EXSTRIDE;
  float2* const WT = reinterpret_cast<float2*>(smem + L.tab);          // FAST only
  float2* const PT = WT + N2;
  float2* const T2 = reinterpret_cast<float2*>(smem + L.rb + kMelMaxSlots * 256);   // FAST only

  // ---- once per workgroup: zero the pad rows of PB; per-lane tables -> registers (or LDS)
  for (int i = tid; i < kPbPadRows * kPbStride; i += 256) PB[NB * kPbStride + i] = 0.f;
  float2 wreg[FAST ? 1 : P], preg[FAST ? 1 : P];
  int maddr[FAST ? 1 : P];            // exchange-buffer slot of the mirror bin Z[N2 - k] (generic path)
  {
    const float2* w2 = reinterpret_cast<const float2*>(tb.window);
    const float2* p2 = reinterpret_cast<const float2*>(tb.post);
    if constexpr (FAST) {
      // window pre-scaled by 1/2 (exact): the split below then yields X, not 2X, and |X|^2 needs no 0.25
      for (int i = tid; i < N2; i += 256) { WT[i] = make_float2(0.5f * w2[i].x, 0.5f * w2[i].y); PT[i] = p2[i]; }
      // pass-2 twiddles W_64^(c*r), c = lane & 7: 64 values, read per frame pair instead of 14 registers per lane
      if (tid < 64) T2[tid] = reinterpret_cast<const float2*>(tb.tw)[(tid >> 3) * (tid & 7) * (N2 / 64)];   // [r*8 + c], symmetric in (r, c)
    }
    if constexpr (!FAST) {
#pragma unroll
      for (int u = 0; u < P; ++u) {
        const int k = lif + LPF * u;
        wreg[u] = w2[k]; preg[u] = p2[k]; maddr[u] = expad((N2 - k) & (N2 - 1));
      }
    }
  }
  // FAST: slot swizzle sw(a) = a ^ ((a>>3)&7) ^ (((a>>6)&1)<<3) makes every exchange access of the
  // 8x8x8 schedule bank-conflict-free; per lane it collapses to four bases:
  //   pass-1 write 8j+r -> A1 ^ r;  pass-2 write -> A2 ^ 9r;  read / last write j+64r -> (r odd ? B1 : B0) + 64r
  const int swA1 = (8 * lane) ^ (lane & 7) ^ (((lane >> 3) & 1) << 3);
  const int swB0 = lane ^ ((lane >> 3) & 7), swB1 = swB0 ^ 8;
  const int swA2 = 64 * (lane >> 3) + 8 * ((lane >> 3) & 1) + (lane & 7);
  constexpr int NT2 = NTW<typename S::P2>::v, NT3 = NTW<typename S::P3>::v, NT4 = NTW<typename S::P4>::v;
  float2 tw2[NT2 > 0 ? NT2 : 1], tw3[NT3 > 0 ? NT3 : 1], tw4[NT4 > 0 ? NT4 : 1];
  {
    const float2* t2 = reinterpret_cast<const float2*>(tb.tw);
    if constexpr (!FAST) S::P2::load_tw(t2, lif, tw2);
    S::P3::load_tw(t2, lif, tw3);
    if constexpr (NT4 > 0) S::P4::load_tw(t2, lif, tw4);
  }
  // mel: this wave's first work items (all of them when n_mels <= 128) stay in registers
  const int f16k = lane & 15;
  float* const RB = smem + L.rb;
  const int mel_cnt = __builtin_amdgcn_readfirstlane(
      tb.mel_item_cnt[0] * (wave == 0) + tb.mel_item_cnt[1] * (wave == 1) +
      tb.mel_item_cnt[2] * (wave == 2) + tb.mel_item_cnt[3] * (wave == 3));
  int4 mi_a[kMelRegItems], mi_b[kMelRegItems];       // (group, b0, nb, role), (slot, nslots, kmin, -)
  float4 mi_cf[kMelRegItems];
  float mi_ko[kMelRegItems];
#pragma unroll
  for (int i = 0; i < kMelRegItems; ++i) {
    mi_a[i] = make_int4(0, 0, 0, 0); mi_b[i] = make_int4(0, 0, 0, 0);
    mi_cf[i] = make_float4(0.f, 0.f, 0.f, 0.f); mi_ko[i] = 0.f;
    if (i < mel_cnt) {
      // wave-uniform metadata -> SGPRs (the compiler cannot see that tid >> 6 is uniform)
      auto sg = [](int v) { return __builtin_amdgcn_readfirstlane(v); };
      const int4 a = tb.mel_items[(wave * kMelMaxItems + i) * 2], bb = tb.mel_items[(wave * kMelMaxItems + i) * 2 + 1];
      mi_a[i] = make_int4(sg(a.x), sg(a.y), sg(a.z), sg(a.w));
      mi_b[i] = make_int4(sg(bb.x), sg(bb.y), sg(tb.mel_grp[a.x].x), 0);
      mi_cf[i] = tb.mel_coef[mi_a[i].x * 16 + f16k];
      mi_ko[i] = tb.mel_koff[mi_a[i].x * 16 + f16k];
    }
  }

  const bool pre = (kp.flags & AFX_FLAG_PREEMPH) != 0;
  const float b1 = kp.preemph_b1;
  const int fmt = kp.fmt;
  const int slen = (kFramesPerBlock - 1) * hop + NFFT;
  const bool hop_even = (hop & 1) == 0;

  // A block's 64-byte descriptor is fetched as one dword per lane (VMEM, so that it does not
  // share a wait counter with the LDS traffic) two blocks ahead and resolved with readlanes.
  auto fetch_desc = [&](int b) -> int {
    const int bb = b < nblocks ? b : nblocks - 1;
    return reinterpret_cast<const int*>(blocks + bb)[lane & 15];
  };
  auto resolve = [&](int w, int b) -> BlkCtx {
    BlkCtx c;
    auto rl = [&](int i) { return __builtin_amdgcn_readlane(w, i); };
    auto rl64 = [&](int i) { return (int64_t)(((uint64_t)(uint32_t)rl(i + 1) << 32) | (uint32_t)rl(i)); };
    c.sample_base = rl64(0); c.frame_slot = rl64(2); c.clip_off = rl64(4);
    c.keep_lo = rl(6); c.keep_hi = rl(7); c.have_lo = rl(8); c.have_hi = rl(9);
    c.clip = rl(10); c.t0 = rl(11); c.T = rl(12);
    c.active = (b < nblocks) && rl(13) != 0;
    c.interior = ((c.sample_base & 3) == 0) && ((slen & 3) == 0) && c.have_lo <= -1 && c.have_hi >= slen;
    return c;
  };

  // Log-mel values of the block just finished wait in registers and are stored one iteration later,
  // right after the staging wait: vmcnt retires in order and counts stores, so stores issued after the
  // sample prefetch would be drained (1-2 us) by the wait for those samples at the top of the loop.
  float lmh[kMelRegItems][4];
  bool pend = false;
  float pend_lmax = -INFINITY;
  int64_t pend_slot = 0;
  int pend_t0 = 0, pend_T = 0, pend_clip = 0;
  auto flush_logmel = [&]() {
    if (!pend) return;
    pend = false;
    int lane_f = lane;
    asm volatile("" : "+v"(lane_f));
    const int f16 = lane_f & 15, q4 = lane_f >> 4;
    const bool valid = (pend_t0 + f16) < pend_T;
    float* tile = logmel + pend_slot * (int64_t)M;
    if (!(kp.flags & 0x800)) {
#pragma unroll
      for (int i = 0; i < kMelRegItems; ++i) {
        if (i < mel_cnt && mi_a[i].w != 1) {
// tile layout [mel/4][frame][mel%4]: this lane's four filters are one 16-byte store
          const int m0 = mi_a[i].x * 16 + q4 * 4;
          if (valid && m0 < M)
            *reinterpret_cast<float4*>(tile + (m0 >> 2) * 64 + f16 * 4) = make_float4(lmh[i][0], lmh[i][1], lmh[i][2], lmh[i][3]);
        }
      }
      const float mx = wave_max(pend_lmax);
      if (lane_f == 0 && mx > -INFINITY) atomicMax(&info[pend_clip].lmax_ord, f2ord(mx));
    }
  };

  // experiment (AFX_DEBUG_SKIP bits 0x1000 / 0x2000): start half of the workgroups ~half a block late so
  // that co-resident workgroups sit in complementary phases (FFT = VALU+LDS, mel = matrix pipe)
  if (((kp.flags & 0x1000) && blockIdx.x >= gridDim.x / 2) || ((kp.flags & 0x2000) && (blockIdx.x & 1))) {
    for (int i = 0; i < 2; ++i) __builtin_amdgcn_s_sleep(127);
  }

  RawQuad pf[MAXCH];
  BlkCtx cur = resolve(fetch_desc(blockIdx.x), blockIdx.x);
  int dnext = fetch_desc(blockIdx.x + gridDim.x);
  // chunk c of a thread covers staged samples j = 4*tid + 1024*c .. +3; indices past the block are
  // clamped (loaded, never stored) so that no load sits under a per-lane branch
  const int jlast = ((slen + 3) & ~3) - 4;
  const int jwave0 = (tid & ~63) * 4;          // staged index of this wave's first lane in chunk 0
  auto prefetch = [&](const BlkCtx& bc) {
#define AFX_PF_LOOP(INTERIOR, FMT)                                                                  \
    _Pragma("unroll") for (int c = 0; c < MAXCH; ++c) {                                             \
      const int j = tid * 4 + c * 1024, jw = jwave0 + c * 1024;                                     \
      pf[c] = load_raw<INTERIOR, FMT>(samples, bc, j < jlast ? j : jlast, jw < jlast ? jw : jlast); \
    }
    if (fmt == AFX_FMT_F32) {
      if (bc.interior) { AFX_PF_LOOP(true, AFX_FMT_F32) } else { AFX_PF_LOOP(false, AFX_FMT_F32) }
    } else {
      if (bc.interior) { AFX_PF_LOOP(true, AFX_FMT_S16) } else { AFX_PF_LOOP(false, AFX_FMT_S16) }
    }
#undef AFX_PF_LOOP
  };
  auto stage_all = [&](const BlkCtx& bc) {
#define AFX_ST_LOOP(INTERIOR, FMT)                                                                  \
    _Pragma("unroll") for (int c = 0; c < MAXCH; ++c) {                                             \
      const int j = tid * 4 + c * 1024;                                                             \
      const float4 o = stage_quad<INTERIOR, FMT>(pf[c], samples, bc, j < jlast ? j : jlast, pre, b1); \
      if (j < slen) *reinterpret_cast<float4*>(S_ + j) = o;                                         \
    }                                                                                               \
    for (int j = tid * 4 + MAXCH * 1024; j < slen; j += 1024)  /* hop > n_fft/4: not prefetched */   \
      *reinterpret_cast<float4*>(S_ + j) = stage_quad<false, FMT>(load_raw<false, FMT>(samples, bc, j, j), samples, bc, j, pre, b1);
    if (fmt == AFX_FMT_F32) {
      if (bc.interior) { AFX_ST_LOOP(true, AFX_FMT_F32) } else { AFX_ST_LOOP(false, AFX_FMT_F32) }
    } else {
      if (bc.interior) { AFX_ST_LOOP(true, AFX_FMT_S16) } else { AFX_ST_LOOP(false, AFX_FMT_S16) }
    }
#undef AFX_ST_LOOP
  };
  if (cur.active && !(kp.flags & 0x100)) prefetch(cur);
  AFX_LDS_BARRIER();

  for (int b = blockIdx.x; b < nblocks; b += gridDim.x) {
    stamp(-1);
    // ---- stage block b from the prefetched registers: pre-emphasis + trim mask, once per sample
    // (0x100/0x200/0x400: timing-only ablation switches (AFX_DEBUG_SKIP), results invalid)
    if (cur.active && !(kp.flags & 0x100)) stage_all(cur);
    flush_logmel();
    stamp(ST_STAGE);
    AFX_LDS_BARRIER();
    stamp(ST_BAR1);

    const BlkCtx nxt = resolve(dnext, b + gridDim.x);
    dnext = fetch_desc(b + 2 * gridDim.x);

    // ---- per frame: window -> rFFT -> power spectrum (+ RMS of the unwindowed frame)
    if (cur.active && !(kp.flags & 0x200)) {
      if constexpr (FAST) {
        // two frames (A, B) in flight per wave; they take turns on the wave's single exchange image,
        // so each one's LDS round trip hides under the other's butterflies
#pragma unroll 1
        for (int pr = 0; pr < 2; ++pr) {
          const int flA = wave * 4 + 2 * pr;
          int a1 = swA1, a2 = swA2;              // opaque per iteration: keeps LICM from parking the 16
          asm volatile("" : "+v"(a1), "+v"(a2)); // XOR-ed exchange addresses in registers for the whole kernel
          const float* SA = S_ + flA * hop;
          const float* SB = SA + hop;
          float2 vA[8], vB[8];
          float ssA = 0.f, ssB = 0.f;
          {
            float2 xa[8], xb[8], ww[8];
            if (hop_even) {
#pragma unroll
              for (int u = 0; u < 8; ++u) {
                xa[u] = *reinterpret_cast<const float2*>(SA + 2 * (lane + 64 * u));
                xb[u] = *reinterpret_cast<const float2*>(SB + 2 * (lane + 64 * u));
              }
            } else {
#pragma unroll
              for (int u = 0; u < 8; ++u) {
                const int a = 2 * (lane + 64 * u);
                xa[u].x = SA[a]; xa[u].y = SA[a + 1]; xb[u].x = SB[a]; xb[u].y = SB[a + 1];
              }
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) ww[u] = WT[lane + 64 * u];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
              ssA += xa[u].x * xa[u].x; ssA += xa[u].y * xa[u].y;
              ssB += xb[u].x * xb[u].x; ssB += xb[u].y * xb[u].y;
              vA[u] = make_float2(xa[u].x * ww[u].x, xa[u].y * ww[u].y);
              vB[u] = make_float2(xb[u].x * ww[u].x, xb[u].y * ww[u].y);
            }
          }
          ssA = wave_sum(ssA); ssB = wave_sum(ssB);
          if (lane == 0) {
            if (cur.t0 + flA < cur.T) rms_rows[cur.frame_slot + flA] = sqrtf(ssA / (float)NFFT);
            if (cur.t0 + flA + 1 < cur.T) rms_rows[cur.frame_slot + flA + 1] = sqrtf(ssB / (float)NFFT);
          }
          // pass 1 (radix 8, no twiddles) + exchange
          dft<8>(vA); dft<8>(vB);
#pragma unroll
          for (int r = 0; r < 8; ++r) EX[a1 ^ r] = vA[r];
          AFX_CBARRIER();
#pragma unroll
          for (int r = 0; r < 8; ++r) vA[r] = EX[((r & 1) ? swB1 : swB0) + 64 * r];
          AFX_CBARRIER();
#pragma unroll
          for (int r = 0; r < 8; ++r) EX[a1 ^ r] = vB[r];
          AFX_CBARRIER();
#pragma unroll
          for (int r = 0; r < 8; ++r) vB[r] = EX[((r & 1) ? swB1 : swB0) + 64 * r];
          AFX_CBARRIER();
          // pass 2
          float2 t2v[8];
#pragma unroll
          for (int r = 1; r < 8; ++r) t2v[r] = T2[r * 8 + (lane & 7)];
#pragma unroll
          for (int r = 1; r < 8; ++r) vA[r] = cmul(vA[r], t2v[r]);
          dft<8>(vA);
#pragma unroll
          for (int r = 0; r < 8; ++r) EX[a2 ^ (9 * r)] = vA[r];
          AFX_CBARRIER();
#pragma unroll
          for (int r = 0; r < 8; ++r) vA[r] = EX[((r & 1) ? swB1 : swB0) + 64 * r];
          AFX_CBARRIER();
#pragma unroll
          for (int r = 1; r < 8; ++r) vB[r] = cmul(vB[r], t2v[r]);
          dft<8>(vB);
#pragma unroll
          for (int r = 0; r < 8; ++r) EX[a2 ^ (9 * r)] = vB[r];
          AFX_CBARRIER();
#pragma unroll
          for (int r = 0; r < 8; ++r) vB[r] = EX[((r & 1) ? swB1 : swB0) + 64 * r];
          AFX_CBARRIER();
          // pass 3: outputs land on the lane's own bins k = lane + 64 r; publish them for the mirror
          // reads Z[N2-k]; then the real-FFT split and the power spectrum.  B's pass 3 runs under A's
          // mirror-read latency.
          float* const pcol = PB + lane * kPbStride + flA;
          float2 pw[8];             // split twiddles; read once for both frames (LDS reads must not
#pragma unroll                  // sit between the PB stores: the compiler would serialise them)
          for (int u = 0; u < 8; ++u) pw[u] = PT[lane + 64 * u];
          auto split_store = [&](const float2 (&v)[8], const float2 (&m)[8], int col) {
            float pv[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
              const float2 w = pw[u];
              const float2 z = v[u], mm = m[u];
              const float e2r = z.x + mm.x, e2i = z.y - mm.y, o2r = z.y + mm.y, o2i = mm.x - z.x;
              const float xr = e2r + w.x * o2r - w.y * o2i, xi = e2i + w.x * o2i + w.y * o2r;
              pv[u] = xr * xr + xi * xi;
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) pcol[64 * u * kPbStride + col] = pv[u];
            if (lane == 0) { const float ny = 2.0f * (v[0].x - v[0].y); pcol[N2 * kPbStride + col] = ny * ny; }
          };
          const int msrc = ((64 - lane) & 63) << 2;           // ds_bpermute byte address of the mirror lane
          auto mirror = [&](const float2 (&v)[8], float2 (&m)[8]) {
            // Z[N2 - k] for k = lane + 64u sits in lane 64 - lane, register 7 - u: a crossbar permute,
            // no LDS image needed.  Lane 0 mirrors onto itself one register up ((8 - u) & 7).
#pragma unroll
            for (int u = 0; u < 8; ++u) {
              m[u].x = __int_as_float(__builtin_amdgcn_ds_bpermute(msrc, __float_as_int(v[7 - u].x)));
              m[u].y = __int_as_float(__builtin_amdgcn_ds_bpermute(msrc, __float_as_int(v[7 - u].y)));
            }
            if (lane == 0) {
#pragma unroll
              for (int u = 0; u < 8; ++u) m[u] = v[(8 - u) & 7];
            }
          };
          {
            float2 mA[8];
#pragma unroll
            for (int r = 1; r < 8; ++r) vA[r] = cmul(vA[r], tw3[r - 1]);
            dft<8>(vA);
            mirror(vA, mA);
#pragma unroll
            for (int r = 1; r < 8; ++r) vB[r] = cmul(vB[r], tw3[r - 1]);
            dft<8>(vB);
            split_store(vA, mA, 0);
          }
          {
            float2 mB[8];
            mirror(vB, mB);
            split_store(vB, mB, 1);
          }
          AFX_CBARRIER();
        }
      } else {
#pragma unroll 1
      for (int it = 0; it < C::ITERS; ++it) {
        const int fl = (wave * C::ITERS + it) * FPW + fsub;      // frame within the block
        const float* Sf = S_ + fl * hop;
        float2 v[P];
        float ss = 0.f;
#pragma unroll
        for (int u = 0; u < P; ++u) {
          const int a = lif + LPF * u;
          float2 x;
          if (hop_even) x = *reinterpret_cast<const float2*>(Sf + 2 * a);
          else { x.x = Sf[2 * a]; x.y = Sf[2 * a + 1]; }
          ss += x.x * x.x; ss += x.y * x.y;
          v[u] = make_float2(x.x * wreg[u].x, x.y * wreg[u].y);
        }
        if constexpr (LPF == 64) ss = wave_sum(ss);
        else {
#pragma unroll
          for (int o = LPF / 2; o >= 1; o >>= 1) ss += __shfl_xor(ss, o);
        }
        if (lif == 0 && cur.t0 + fl < cur.T) rms_rows[cur.frame_slot + fl] = sqrtf(ss / (float)NFFT);

        S::P1::run(v, nullptr, EX, lif);
        S::P2::run(v, tw2, EX, lif);
        S::P3::run(v, tw3, EX, lif);
        if constexpr (NT4 > 0) S::P4::run(v, tw4, EX, lif);

        // real-FFT split: X[k] from Z[k] and Z[N2-k]; EX now holds Z in natural order
        float* const pcol = PB + lif * kPbStride + fl;
#pragma unroll
        for (int u = 0; u < P; ++u) {
          const float2 z = v[u];
          const float2 m = EX[maddr[u]];
          const float e2r = z.x + m.x, e2i = z.y - m.y;
          const float o2r = z.y + m.y, o2i = m.x - z.x;
          const float2 w = preg[u];
          const float xr = e2r + w.x * o2r - w.y * o2i;
          const float xi = e2i + w.x * o2i + w.y * o2r;
          pcol[LPF * u * kPbStride] = 0.25f * (xr * xr + xi * xi);
          if (u == 0 && lif == 0) { const float ny = z.x - z.y; pcol[N2 * kPbStride] = ny * ny; }
        }
        AFX_CBARRIER();
      }
      }
    }
    // ---- issue the next block's sample loads; they land under the mel phase (issued here rather
    // than before the FFT so that the raw quads are not live across the register-hungry FFT phase)
    stamp(ST_FFT);
    if (nxt.active && !(kp.flags & 0x100)) prefetch(nxt);
    stamp(ST_PREFETCH);
    AFX_LDS_BARRIER();
    stamp(ST_BAR2);

    // ---- mel filterbank + dB on the matrix pipe: D[16 filters][16 frames] += A[16x4] * B[4 bins x 16 frames]
    // (exact f32 MFMA over the non-zero 16x4 blocks of librosa.filters.mel; the A operand -- the
    // filter triangles -- is evaluated per lane, see MelBlocks in afx_internal.h).  The block ranges are
    // cut into work items balanced over the 4 waves; a split group's partial sums meet in an LDS slot.
    const bool mel_on = cur.active && !(kp.flags & 0x400);
    // lane index made opaque per block: otherwise LICM hoists every lane-derived address of this phase
    // out of the block loop and they sit in registers through the (register-bound) FFT phase
    int lane_m = lane;
    asm volatile("" : "+v"(lane_m));
    const int f16 = lane_m & 15, q4 = lane_m >> 4;
    const bool valid = (cur.t0 + f16) < cur.T;
    float lmax = -INFINITY;
    float* tile = logmel + cur.frame_slot * (int64_t)M;
    auto mel_item = [&](int kmin, int b0, int nb, const float4 cf, const float ko) -> f32x4 {
      const float* p0 = PB + (kmin + 4 * b0 + q4) * kPbStride + f16;
      const float* const pmax = PB + (NB + kPbPadRows - 1) * kPbStride + f16;    // a zero pad row
      float kf = (float)(q4 + 4 * b0) + ko;                       // k - kc of this lane's bin, exact
      f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
      // 8 blocks (32 bins) per step: the 8 B-operand reads are issued together and two accumulators
      // alternate, so neither the LDS latency nor the MFMA dependency serialises the chain.  Blocks
      // past the item's range get zero weight (and rows past the Nyquist bin are the zero pad rows).
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
    // dst == nullptr: store the tile rows now (table-driven items); otherwise park the four values in
    // registers -- their global stores are issued next iteration, after the staging wait (see lmh)
    auto mel_finish = [&](const f32x4 acc, int g, float* dst) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = g * 16 + q4 * 4 + r;
        // 10*log10(max(amin, mel)); v_log_f32 is log2
        const float Lv = 3.01029995663981195f * __builtin_amdgcn_logf(fmaxf(kp.amin, acc[r]));
        if (dst) dst[r] = Lv;
        if (valid && m < M) {
          if (!dst && !(kp.flags & 0x800)) tile[(m >> 2) * 64 + f16 * 4 + (m & 3)] = Lv;
          lmax = fmaxf(lmax, Lv);
        }
      }
    };
    f32x4 held[kMelRegItems];
    if (mel_on) {
#pragma unroll
      for (int i = 0; i < kMelRegItems; ++i) {
        if (i < mel_cnt) {
          held[i] = mel_item(mi_b[i].z, mi_a[i].y, mi_a[i].z, mi_cf[i], mi_ko[i]);
          if (mi_a[i].w == 0) mel_finish(held[i], mi_a[i].x, lmh[i]);
          else if (mi_a[i].w == 1) *reinterpret_cast<f32x4*>(RB + mi_b[i].x * 256 + lane_m * 4) = held[i];
        }
      }
      for (int i = kMelRegItems; i < mel_cnt; ++i) {            // n_mels > 128: whole groups, tables re-read
        const int4 ia = tb.mel_items[(wave * kMelMaxItems + i) * 2];
        const f32x4 acc = mel_item(tb.mel_grp[ia.x].x, ia.y, ia.z, tb.mel_coef[ia.x * 16 + f16], tb.mel_koff[ia.x * 16 + f16]);
        mel_finish(acc, ia.x, nullptr);
      }
    }
    stamp(ST_MEL);
    if (tb.mel_n_slots > 0) {                                    // uniform for the whole grid
      AFX_LDS_BARRIER();
      stamp(ST_BAR3);
      if (mel_on) {
#pragma unroll
        for (int i = 0; i < kMelRegItems; ++i) {
          if (i < mel_cnt && mi_a[i].w == 2) {
            f32x4 acc = held[i];
            for (int sl = 0; sl < mi_b[i].y; ++sl)
              acc += *reinterpret_cast<const f32x4*>(RB + (mi_b[i].x + sl) * 256 + lane_m * 4);
            mel_finish(acc, mi_a[i].x, lmh[i]);
          }
        }
      }
    }
    stamp(ST_MELFIN);
    if (mel_on) {
      pend = true;
      pend_lmax = lmax; pend_slot = cur.frame_slot; pend_t0 = cur.t0; pend_T = cur.T; pend_clip = cur.clip;
    }
    // no barrier here: the next staging writes only S_ (dead since the barrier above) and PB is
    // rewritten only after the next iteration's first barrier.
    cur = nxt;
  }
  if constexpr (STAMP) { if (lane == 0) for (int i = 0; i < ST_COUNT; ++i) stamps[((size_t)blockIdx.x * kWaves + wave) * ST_COUNT + i] = st_sum[i]; }
  flush_logmel();
}

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------
template <int NFFT>
static hipError_t launch_frames_t(hipStream_t s, const void* samples, ClipInfo* info,
                                  const BlockDesc* blocks, int nblocks, const DevTables& tb, const KParams& kp,
                                  float* logmel, float* rms_rows, int grid, unsigned long long* stamps) {
  const size_t lds = frames_lds_bytes(NFFT, kp.hop);
  const hipError_t e = stamps ? allow_lds_once<k_frames<NFFT, true>>() : allow_lds_once<k_frames<NFFT, false>>();
  if (e != hipSuccess) return e;
  if (stamps)
    hipLaunchKernelGGL((k_frames<NFFT, true>), dim3(grid), dim3(256), lds, s, samples, info, blocks, nblocks,
                       tb, kp, logmel, rms_rows, stamps);
  else
    hipLaunchKernelGGL((k_frames<NFFT, false>), dim3(grid), dim3(256), lds, s, samples, info, blocks, nblocks,
                       tb, kp, logmel, rms_rows, stamps);
  return hipGetLastError();
}

hipError_t launch_frames(hipStream_t s, const void* samples, ClipInfo* info,
                         const BlockDesc* blocks, int nblocks, const DevTables& tb, const KParams& kp,
                         float* logmel, float* rms_rows, int grid, unsigned long long* stamps) {
  switch (kp.n_fft) {
    case 256:  return launch_frames_t<256>(s, samples, info, blocks, nblocks, tb, kp, logmel, rms_rows, grid, stamps);
    case 512:  return launch_frames_t<512>(s, samples, info, blocks, nblocks, tb, kp, logmel, rms_rows, grid, stamps);
    case 1024: return launch_frames_t<1024>(s, samples, info, blocks, nblocks, tb, kp, logmel, rms_rows, grid, stamps);
    case 2048: return launch_frames_t<2048>(s, samples, info, blocks, nblocks, tb, kp, logmel, rms_rows, grid, stamps);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace afx
