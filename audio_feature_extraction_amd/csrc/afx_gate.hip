// Spectral-gating noise reduction (noisereduce's reduce_noise) on scipy's STFT grid, n_fft 1024 / hop 256 or 2048 / 512.
// A clip's frames are coupled through whole-clip statistics (stationary) or a recurrence along time (non-stationary) and
// through the smoothing of the mask, so the work is cut at those points:
//   k_gate_frames<.., false>  one wave per unit (a 2048 frame, or two 1024 frames packed into one complex transform):
//                             window, FFT, |X| as a float32 row of the grid's plane
//   k_gate_stats              stationary, one lane per (clip, bin): the noise rows' maximum, mean and std in dB, the signal
//                             rows' maximum, in float64 and in the order of t
//   k_gate_hard               stationary: the decision of every (frame, bin) of the signal grid, one bit each
//   k_gate_recur              non-stationary, one lane per (clip, bin): filtfilt along t in float64, the sigmoid in place
//   k_gate_smooth             one workgroup per frame: +- n_t frames into LDS, then +- n_f bins, float64
//   k_gate_frames<.., true>   the FFT again (a stored spectrum would cost 8 bytes per bin and frame each way, more than the
//                             transform in LDS), x mask, the inverse, x window, as the rows k_gate_ola reads
//   k_gate_ola                overlap-add as a gather in increasing frame order, / the overlap-added window^2
// No atomics; every sum runs in one fixed order, and a clip reads nothing of another.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "afx.h"
#include "afx_gate.h"
#include "afx_hpss_dev.h"

namespace afx {

namespace {

constexpr double kGateEps = 0x1p-52;

__device__ __forceinline__ float gt_abs(v2 x) {
#pragma clang fp contract(off)
  const float a = x.x * x.x;
  const float b = x.y * x.y;
  return sqrtf(a + b);
}

__device__ __forceinline__ float gt_sample(const float* __restrict__ y, const GateGrid& g, int64_t i, bool zero) {
  return (!zero && i >= 0 && i < g.len) ? y[g.y_off + i] : 0.f;
}

__device__ __forceinline__ double gt_db(float a) { return 20.0 * log10((double)a + kGateEps); }

}  // namespace

// APPLY false: out is the magnitude plane (mask unused); true: out is the time-domain rows, mask the smoothed mask plane
template <int NFFT, bool APPLY>
__global__ __launch_bounds__(256) void k_gate_frames(const float* __restrict__ y, const GateGrid* __restrict__ grids,
                                                     const uint32_t* __restrict__ bad, int n, int64_t n_units, GateTabs tb,
                                                     const float* __restrict__ mask, float* __restrict__ out) {
  constexpr int HOP = NFFT / 4, PITCH = gate_pitch(NFFT);
  __shared__ v2 lds[4][1024];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t u = (int64_t)blockIdx.x * 4 + wave;
  const bool live = u < n_units;
  const int64_t uu = live ? u : n_units - 1;
  const int gi = hp_find(n, uu, [&](int i) { return grids[i].unit_base; });
  const GateGrid g = grids[gi];
  const bool zero = !live || (bad[g.clip] | bad[n + g.clip]) != 0;
  v2* buf = lds[wave];
  const v2* W1 = (const v2*)tb.w1024;

  if constexpr (NFFT == 2048) {
    const int t = g.ta + (int)(uu - g.unit_base);
    const int64_t s0 = (int64_t)t * HOP - NFFT / 2 - g.shift;
#pragma unroll 4
    for (int q = 0; q < 16; ++q) {
      const int m = lane + 64 * q;
      buf[m] = v2{tb.window[2 * m] * gt_sample(y, g, s0 + 2 * m, zero), tb.window[2 * m + 1] * gt_sample(y, g, s0 + 2 * m + 1, zero)};
    }
    hp_fft1024(buf, W1, lane);
    const v2* W = (const v2*)tb.w2048;
    if constexpr (!APPLY) {
      float* row = out + (g.row_base + t) * PITCH;
      const float sc = 2.0f / NFFT;                              // 1 / sum(window)
#pragma unroll 4
      for (int q = 0; q < 8; ++q) {
        const int k = lane + 64 * q;
        const v2 zk = buf[k], zn = buf[(1024 - k) & 1023];
        const v2 xk = hp_split(zk, zn, W[k]);
        const v2 xn = k ? hp_split(zn, zk, W[(1024 - k) & 1023]) : v2{zk.x - zk.y, 0.f};
        if (live) { row[k] = gt_abs(xk) * sc; row[1024 - k] = gt_abs(xn) * sc; }
      }
      if (lane == 0 && live) {
        const v2 zm = buf[512];
        row[512] = gt_abs(hp_split(zm, zm, W[512])) * sc;
      }
    } else {
      // split, mask and merge of the pair (k, 1024 - k) in place, as k_dn_frames does
      const float* M = mask + (g.row_base + t) * PITCH;
#pragma unroll 4
      for (int q = 0; q < 8; ++q) {
        const int k = lane + 64 * q;
        const v2 zk = buf[k], zn = buf[(1024 - k) & 1023];
        const v2 xk = hp_split(zk, zn, W[k]);
        const v2 xn = k ? hp_split(zn, zk, W[(1024 - k) & 1023]) : v2{zk.x - zk.y, 0.f};
        v2 yk = xk * M[k], yn = xn * M[1024 - k];
        if (k == 0) { yk.y = 0.f; yn.y = 0.f; }
        buf[k] = hp_merge(yk, yn, W[k]);
        if (k) buf[1024 - k] = hp_merge(yn, yk, W[(1024 - k) & 1023]);
      }
      if (lane == 0) {
        const v2 zm = buf[512];
        const v2 ym = hp_split(zm, zm, W[512]) * M[512];
        buf[512] = hp_merge(ym, ym, W[512]);
      }
      hp_fft1024(buf, W1, lane);
      if (!live) return;
      const float sc = 1.0f / 2048.0f;
      v2* row = (v2*)(out + (g.arow_base + (t - g.ta)) * NFFT);
#pragma unroll 4
      for (int q = 0; q < 16; ++q) {
        const int m = lane + 64 * q;
        const v2 z = buf[m];
        row[m] = v2{tb.window[2 * m] * (z.x * sc), tb.window[2 * m + 1] * (-z.y * sc)};
      }
    }
  } else {
    // two real frames a, b as z = a + i b: A[k] = (Z[k] + conj Z[N - k]) / 2, B[k] = (Z[k] - conj Z[N - k]) / 2i
    const int ta = g.ta + 2 * (int)(uu - g.unit_base), tbq = ta + 1;
    const bool has_b = tbq < g.ta + g.na;
    const int64_t sa = (int64_t)ta * HOP - NFFT / 2 - g.shift, sb = sa + HOP;
#pragma unroll 4
    for (int q = 0; q < 16; ++q) {
      const int m = lane + 64 * q;
      const float w = tb.window[m];
      buf[m] = v2{w * gt_sample(y, g, sa + m, zero), w * gt_sample(y, g, sb + m, zero || !has_b)};
    }
    hp_fft1024(buf, W1, lane);
    const int64_t ra = g.row_base + ta, rb = has_b ? ra + 1 : ra;   // the second row is never touched without a frame b
    if constexpr (!APPLY) {
      float* rowa = out + ra * PITCH;
      float* rowb = out + rb * PITCH;
      const float sc = 2.0f / NFFT;
#pragma unroll 4
      for (int q = 0; q < 8; ++q) {
        const int k = lane + 64 * q;
        const v2 zk = buf[k], zn = buf[(1024 - k) & 1023];
        const v2 A = v2{zk.x + zn.x, zk.y - zn.y} * 0.5f;
        const v2 B = v2{zk.y + zn.y, zn.x - zk.x} * 0.5f;
        if (live) {
          rowa[k] = gt_abs(A) * sc;
          if (has_b) rowb[k] = gt_abs(B) * sc;
        }
      }
      if (lane == 0 && live) {
        const v2 z = buf[512];
        rowa[512] = fabsf(z.x) * sc;
        if (has_b) rowb[512] = fabsf(z.y) * sc;
      }
    } else {
      const float* Ma = mask + ra * PITCH;
      const float* Mb = mask + rb * PITCH;
      // Y = Ya + i Yb with both extended Hermitian; buf takes conj Y, whose forward FFT is the conjugate of N times the inverse
#pragma unroll 4
      for (int q = 0; q < 8; ++q) {
        const int k = lane + 64 * q;
        const v2 zk = buf[k], zn = buf[(1024 - k) & 1023];
        const v2 A = v2{zk.x + zn.x, zk.y - zn.y} * 0.5f;
        const v2 B = v2{zk.y + zn.y, zn.x - zk.x} * 0.5f;
        const v2 Ya = A * Ma[k];
        const v2 Yb = has_b ? B * Mb[k] : v2{0.f, 0.f};
        buf[k] = v2{Ya.x - Yb.y, -(Ya.y + Yb.x)};
        if (k) buf[1024 - k] = v2{Ya.x + Yb.y, Ya.y - Yb.x};
      }
      if (lane == 0) {
        const v2 z = buf[512];
        const float ya = z.x * Ma[512];
        const float yb = has_b ? z.y * Mb[512] : 0.f;
        buf[512] = v2{ya, -yb};
      }
      hp_fft1024(buf, W1, lane);
      if (!live) return;
      const float sc = 1.0f / 1024.0f;
      float* rowa = out + (g.arow_base + (ta - g.ta)) * NFFT;
      float* rowb = rowa + (has_b ? NFFT : 0);
#pragma unroll 4
      for (int q = 0; q < 16; ++q) {
        const int m = lane + 64 * q;
        const v2 z = buf[m];
        const float w = tb.window[m];
        const float vb = w * (-z.y * sc);
        rowa[m] = w * (z.x * sc);
        if (has_b) rowb[m] = vb;
      }
    }
  }
}

template <int NFFT>
__global__ __launch_bounds__(256) void k_gate_stats(const GateGrid* __restrict__ sig, const GateGrid* __restrict__ noise,
                                                    const float* __restrict__ mag, const float* __restrict__ nmag, double n_std,
                                                    double* __restrict__ thr, double* __restrict__ amp) {
#pragma clang fp contract(off)
  constexpr int BINS = gate_bins(NFFT), PITCH = gate_pitch(NFFT);
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= BINS) return;
  const GateGrid gs = sig[blockIdx.y], gn = noise[blockIdx.y];
  const float* N = nmag + gn.row_base * PITCH + b;
  float amax = 0.f;
  for (int t = 0; t < gn.T; ++t) amax = fmaxf(amax, N[(int64_t)t * PITCH]);
  const double floor_n = gt_db(amax) - 80.0;
  double sum = 0.0;
  for (int t = 0; t < gn.T; ++t) sum += fmax(gt_db(N[(int64_t)t * PITCH]), floor_n);
  const double mean = sum / (double)gn.T;
  double sq = 0.0;
  for (int t = 0; t < gn.T; ++t) {
    const double e = fmax(gt_db(N[(int64_t)t * PITCH]), floor_n) - mean;
    sq += e * e;
  }
  const double th = mean + n_std * sqrt(sq / (double)gn.T);
  const float* S = mag + gs.row_base * PITCH + b;
  float smax = 0.f;
  for (int t = 0; t < gs.T; ++t) smax = fmaxf(smax, S[(int64_t)t * PITCH]);
  const double floor_s = gt_db(smax) - 80.0;
  thr[(int64_t)blockIdx.y * PITCH + b] = th;
  // db(|X|) floored at floor_s exceeds th where |X| + eps exceeds 10^(th / 20), or everywhere when the floor itself does
  amp[(int64_t)blockIdx.y * PITCH + b] = floor_s > th ? -1.0 : pow(10.0, th / 20.0);
}

template <int NFFT>
__global__ __launch_bounds__(256) void k_gate_hard(const GateGrid* __restrict__ sig, int n, const float* __restrict__ mag,
                                                   const double* __restrict__ amp, uint32_t* __restrict__ bits) {
  constexpr int BINS = gate_bins(NFFT), PITCH = gate_pitch(NFFT), WORDS = gate_words(NFFT);
  const int64_t r = blockIdx.x;
  const int ci = hp_find(n, r, [&](int i) { return sig[i].row_base; });
  const float* row = mag + r * PITCH;
  const double* a = amp + (int64_t)ci * PITCH;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int j = 0; j < (BINS + 255) / 256; ++j) {                 // block-uniform
    const int b = j * 256 + (int)threadIdx.x;
    const bool on = b < BINS && (double)row[b < BINS ? b : 0] + kGateEps > a[b < BINS ? b : 0];
    const unsigned long long m = __ballot(on);
    const int wi = 8 * j + 2 * wave;
    if (lane == 0) {
      if (wi < WORDS) bits[r * WORDS + wi] = (uint32_t)m;
      if (wi + 1 < WORDS) bits[r * WORDS + wi + 1] = (uint32_t)(m >> 32);
    }
  }
}

template <int NFFT>
__global__ __launch_bounds__(256) void k_gate_recur(const GateGrid* __restrict__ sig, double beta, double n_mult, double slope,
                                                    float* __restrict__ mag, double* __restrict__ fwd) {
#pragma clang fp contract(off)
  constexpr int BINS = gate_bins(NFFT), PITCH = gate_pitch(NFFT);
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= BINS) return;
  const GateGrid g = sig[blockIdx.y];
  float* A = mag + g.row_base * PITCH + b;
  double* F = fwd + g.row_base * PITCH + b;
  const double a1 = beta - 1.0, zi = 1.0 - beta;                 // scipy.signal.lfilter_zi([beta], [1, beta - 1])
  double z = zi * (double)A[0], yv = 0.0;
#pragma unroll 8
  for (int t = 0; t < g.T; ++t) {
    yv = beta * (double)A[(int64_t)t * PITCH] + z;
    F[(int64_t)t * PITCH] = yv;
    z = -a1 * yv;
  }
  z = zi * yv;
#pragma unroll 8
  for (int t = g.T - 1; t >= 0; --t) {
    const double s = beta * F[(int64_t)t * PITCH] + z;
    z = -a1 * s;
    const double a = (double)A[(int64_t)t * PITCH];
    const double m = s == 0.0 ? 0.0 : 1.0 / (1.0 + exp(-((a - s) / s - n_mult) * slope));
    A[(int64_t)t * PITCH] = (float)m;
  }
}

template <int NFFT, bool BITS>
__global__ __launch_bounds__(256) void k_gate_smooth(const GateGrid* __restrict__ sig, int n, const uint32_t* __restrict__ bits,
                                                     const float* __restrict__ plane, int n_f, int n_t, double p, GateTabs tb,
                                                     float* __restrict__ mask) {
#pragma clang fp contract(off)
  constexpr int BINS = gate_bins(NFFT), PITCH = gate_pitch(NFFT), WORDS = gate_words(NFFT);
  __shared__ double u[BINS + 2 * kGateMaxNf];
  const int64_t r = blockIdx.x;
  const int ci = hp_find(n, r, [&](int i) { return sig[i].row_base; });
  const GateGrid g = sig[ci];
  const int t = (int)(r - g.row_base);
  const double q = 1.0 - p;
  for (int i = threadIdx.x; i < BINS + 2 * n_f; i += 256) {
    const int b = i - n_f;
    double acc = 0.0;
    if (b >= 0 && b < BINS) {
      for (int dt = -n_t; dt <= n_t; ++dt) {
        const int tt = t + dt;
        if (tt < 0 || tt >= g.T) continue;
        double v;
        if constexpr (BITS) v = (double)((bits[(r + dt) * WORDS + (b >> 5)] >> (b & 31)) & 1u) * p + q;
        else v = (double)plane[(r + dt) * PITCH + b];
        acc += tb.vt[dt + n_t] * v;
      }
    }
    u[i] = acc;
  }
  __syncthreads();
  for (int b = threadIdx.x; b < BINS; b += 256) {
    double acc = 0.0;
    for (int df = 0; df <= 2 * n_f; ++df) acc += tb.vf[df] * u[b + df];
    mask[r * PITCH + b] = (float)(BITS ? acc : acc * p + q);
  }
}

template <int NFFT>
__global__ __launch_bounds__(256) void k_gate_ola(const float* __restrict__ rows, const GateGrid* __restrict__ sig,
                                                  const uint32_t* __restrict__ bad, int n, GateTabs tb, float* __restrict__ out) {
#pragma clang fp contract(off)
  constexpr int HOP = NFFT / 4;
  const GateGrid g = sig[blockIdx.y];
  const bool dead = (bad[g.clip] | bad[n + g.clip]) != 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int64_t s = (int64_t)blockIdx.x * 1024 + k * 256 + threadIdx.x;
    if (s >= g.len) break;
    const int64_t c = s + g.shift;
    float acc = 0.f, nrm = 0.f;
    if (!dead && c < (int64_t)(g.T - 1) * HOP) {
      const int64_t tlo = c - NFFT / 2 + 1 <= 0 ? 0 : (c - NFFT / 2 + HOP) / HOP;
      const int64_t thi = std::min<int64_t>((c + NFFT / 2) / HOP, g.T - 1);
      for (int64_t t = tlo; t <= thi; ++t) {                     // every such frame reaches the clip: ta <= t < ta + na
        const int j = (int)(c - t * HOP + NFFT / 2);
        acc += rows[(g.arow_base + (t - g.ta)) * NFFT + j];
        const float w = tb.window[j];
        nrm += w * w;
      }
    }
    out[g.out_off + s] = nrm > 1e-10f ? acc / nrm : acc;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
hipError_t launch_gate_mag(hipStream_t s, int n_fft, const float* y, const GateGrid* grids, const uint32_t* bad, int n,
                           int64_t n_units, GateTabs tb, float* plane) {
  if (n_units <= 0) return hipSuccess;
  const dim3 grid((unsigned)((n_units + 3) / 4));
  { if (n_fft == 1024) hipLaunchKernelGGL((k_gate_frames<1024, false>), grid, dim3(256), 0, s, y, grids, bad, n, n_units, tb, (const float*)nullptr, plane);
      else hipLaunchKernelGGL((k_gate_frames<2048, false>), grid, dim3(256), 0, s, y, grids, bad, n, n_units, tb, (const float*)nullptr, plane); }
  return hipGetLastError();
}

hipError_t launch_gate_stats(hipStream_t s, int n_fft, const GateGrid* sig, const GateGrid* noise, int n, const float* mag,
                             const float* nmag, double n_std, double* thr, double* amp) {
  const dim3 grid((unsigned)((gate_bins(n_fft) + 255) / 256), (unsigned)n);
  { if (n_fft == 1024) hipLaunchKernelGGL(k_gate_stats<1024>, grid, dim3(256), 0, s, sig, noise, mag, nmag, n_std, thr, amp);
      else hipLaunchKernelGGL(k_gate_stats<2048>, grid, dim3(256), 0, s, sig, noise, mag, nmag, n_std, thr, amp); }
  return hipGetLastError();
}

hipError_t launch_gate_hard(hipStream_t s, int n_fft, const GateGrid* sig, int n, int64_t n_rows, const float* mag,
                            const double* amp, uint32_t* bits) {
  const dim3 grid((unsigned)n_rows);
  { if (n_fft == 1024) hipLaunchKernelGGL(k_gate_hard<1024>, grid, dim3(256), 0, s, sig, n, mag, amp, bits);
      else hipLaunchKernelGGL(k_gate_hard<2048>, grid, dim3(256), 0, s, sig, n, mag, amp, bits); }
  return hipGetLastError();
}

hipError_t launch_gate_recur(hipStream_t s, int n_fft, const GateGrid* sig, int n, double beta, double n_mult, double slope,
                             float* mag, double* fwd) {
  const dim3 grid((unsigned)((gate_bins(n_fft) + 255) / 256), (unsigned)n);
  { if (n_fft == 1024) hipLaunchKernelGGL(k_gate_recur<1024>, grid, dim3(256), 0, s, sig, beta, n_mult, slope, mag, fwd);
      else hipLaunchKernelGGL(k_gate_recur<2048>, grid, dim3(256), 0, s, sig, beta, n_mult, slope, mag, fwd); }
  return hipGetLastError();
}

hipError_t launch_gate_smooth(hipStream_t s, int n_fft, const GateGrid* sig, int n, int64_t n_rows, const uint32_t* bits,
                              const float* plane, int n_f, int n_t, double p, GateTabs tb, float* mask) {
  const dim3 grid((unsigned)n_rows);
  if (bits)
    { if (n_fft == 1024) hipLaunchKernelGGL((k_gate_smooth<1024, true>), grid, dim3(256), 0, s, sig, n, bits, plane, n_f, n_t, p, tb, mask);
      else hipLaunchKernelGGL((k_gate_smooth<2048, true>), grid, dim3(256), 0, s, sig, n, bits, plane, n_f, n_t, p, tb, mask); }
  else
    { if (n_fft == 1024) hipLaunchKernelGGL((k_gate_smooth<1024, false>), grid, dim3(256), 0, s, sig, n, bits, plane, n_f, n_t, p, tb, mask);
      else hipLaunchKernelGGL((k_gate_smooth<2048, false>), grid, dim3(256), 0, s, sig, n, bits, plane, n_f, n_t, p, tb, mask); }
  return hipGetLastError();
}

hipError_t launch_gate_apply(hipStream_t s, int n_fft, const float* y, const GateGrid* sig, const uint32_t* bad, int n,
                             int64_t n_units, GateTabs tb, const float* mask, float* rows) {
  if (n_units <= 0) return hipSuccess;
  const dim3 grid((unsigned)((n_units + 3) / 4));
  { if (n_fft == 1024) hipLaunchKernelGGL((k_gate_frames<1024, true>), grid, dim3(256), 0, s, y, sig, bad, n, n_units, tb, mask, rows);
      else hipLaunchKernelGGL((k_gate_frames<2048, true>), grid, dim3(256), 0, s, y, sig, bad, n, n_units, tb, mask, rows); }
  return hipGetLastError();
}

hipError_t launch_gate_ola(hipStream_t s, int n_fft, const float* rows, const GateGrid* sig, const uint32_t* bad, int n,
                           int64_t max_len, GateTabs tb, float* out) {
  const dim3 grid((unsigned)std::max<int64_t>((max_len + 1023) / 1024, 1), (unsigned)n);
  { if (n_fft == 1024) hipLaunchKernelGGL(k_gate_ola<1024>, grid, dim3(256), 0, s, rows, sig, bad, n, tb, out);
      else hipLaunchKernelGGL(k_gate_ola<2048>, grid, dim3(256), 0, s, rows, sig, bad, n, tb, out); }
  return hipGetLastError();
}

}  // namespace afx
