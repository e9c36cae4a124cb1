// microbenchmark: LDS-pipe cost per wave-instruction of the ops the FFT exchange uses (gfx950), at 4, 8 and 16 waves per
// CU, and the issue cost of the lane swaps that take half of exchange 2 off that pipe (v_permlane16_swap / v_permlane32_swap),
// run beside packed FMAs as issue_mix.hip runs the LDS instructions.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <vector>
template <int OP>
__global__ void k(unsigned long long* out, float* sink, int iters) {
  __shared__ __attribute__((aligned(16))) float lds[8 * 1024 * 4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float* base = lds + wave * (blockDim.x > 512 ? 2048 : 4096);      // a wave touches 1024 floats; 16 waves share the 128 KB
  float2 v2 = make_float2(lane, lane * 2.f); float4 v4 = make_float4(lane, 1, 2, 3); float v1 = lane;
  float acc = 0.f;
  for (int i = lane; i < 2048; i += 64) base[i] = i;
  __syncthreads();
  unsigned long long t0 = __builtin_amdgcn_s_memtime();
  __builtin_amdgcn_s_waitcnt(0xC07F);
  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      if (OP == 0) reinterpret_cast<float2*>(base)[lane + 64 * (u & 7)] = v2;                       // ds_write_b64
      if (OP == 1) { float2 t = reinterpret_cast<float2*>(base)[lane + 64 * (u & 7)]; acc += t.x + t.y; } // ds_read_b64
      if (OP == 2) base[lane + 64 * u] = v1;                                                            // ds_write_b32
      if (OP == 3) acc += base[lane + 64 * u];                                                          // ds_read_b32
      if (OP == 4) acc += __int_as_float(__builtin_amdgcn_ds_bpermute(((63 - lane) << 2), __float_as_int(v1 + u))); // bpermute
      if (OP == 5) reinterpret_cast<float4*>(base)[lane + 64 * (u & 3)] = v4;                       // ds_write_b128
      if (OP == 6) { float4 t = reinterpret_cast<float4*>(base)[lane + 64 * (u & 3)]; acc += t.x + t.w; }  // ds_read_b128
    }
    asm volatile("" ::: "memory");
  }
  unsigned long long t1 = __builtin_amdgcn_s_memtime();
  __builtin_amdgcn_s_waitcnt(0xC07F);
  if (lane == 0) out[blockIdx.x * (blockDim.x / 64) + wave] = t1 - t0;
  sink[blockIdx.x * blockDim.x + threadIdx.x] = acc + v2.x + v4.x;
}
template <int OP> void run(const char* name, int waves) {
  const int iters = 1000, blocks = 256;
  unsigned long long* d; float* s;
  hipMalloc(&d, blocks * waves * 8); hipMalloc(&s, blocks * waves * 64 * 4);
  for (int rep = 0; rep < 2; ++rep) hipLaunchKernelGGL(k<OP>, dim3(blocks), dim3(64 * waves), 0, 0, d, s, iters);
  hipDeviceSynchronize();
  std::vector<unsigned long long> h(blocks * waves); hipMemcpy(h.data(), d, blocks * waves * 8, hipMemcpyDeviceToHost);
  double sum = 0; for (int i = 0; i < blocks * waves; ++i) sum += h[i];
  const double per_wave = sum / (blocks * waves) / (iters * 16.0);
  printf("%-16s waves/CU=%d  cycles per instr per wave = %6.1f  => LDS pipe cycles per instr = %5.1f\n", name, waves, per_wave, per_wave / waves);
  hipFree(d); hipFree(s);
}
// 8 v_pk_fma_f32 per iteration plus N16 v_permlane16_swap and N32 v_permlane32_swap on four independent register pairs
typedef float f2 __attribute__((ext_vector_type(2)));
template <int N16, int N32>
__global__ void ksw(unsigned long long* out, float* sink, int iters, float seed) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  f2 a[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) a[i] = f2{seed * (lane + i + 1), seed * (lane + 2 * i + 1)};
  const f2 c = f2{seed * 0.5f, seed * 0.25f};
  unsigned x[4], y[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) { x[i] = lane * 4 + i; y[i] = lane * 8 + i; }
  const unsigned long long t0 = __builtin_amdgcn_s_memtime();
  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      asm volatile("v_pk_fma_f32 %0, %0, %1, %1" : "+v"(a[u]) : "v"(c));
      if (u < N16) { const auto r = __builtin_amdgcn_permlane16_swap(x[u & 3], y[u & 3], false, false); x[u & 3] = r[0]; y[u & 3] = r[1]; }
      if (u < N32) { const auto r = __builtin_amdgcn_permlane32_swap(x[(u + 2) & 3], y[(u + 2) & 3], false, false); x[(u + 2) & 3] = r[0]; y[(u + 2) & 3] = r[1]; }
    }
    asm volatile("" : "+v"(x[0]), "+v"(x[1]), "+v"(x[2]), "+v"(x[3]), "+v"(y[0]), "+v"(y[1]), "+v"(y[2]), "+v"(y[3]));
  }
  const unsigned long long t1 = __builtin_amdgcn_s_memtime();
  if (lane == 0) out[blockIdx.x * (blockDim.x / 64) + wave] = t1 - t0;
  float s = 0.f;
  for (int i = 0; i < 8; ++i) s += a[i].x + a[i].y;
  for (int i = 0; i < 4; ++i) s += (float)(x[i] ^ y[i]);
  sink[blockIdx.x * blockDim.x + threadIdx.x] = s;
}
template <int N16, int N32> void run_sw(int waves) {
  const int iters = 2000, blocks = 256;
  unsigned long long* d; float* s;
  hipMalloc(&d, blocks * waves * 8); hipMalloc(&s, blocks * waves * 64 * 4);
  for (int rep = 0; rep < 2; ++rep) hipLaunchKernelGGL((ksw<N16, N32>), dim3(blocks), dim3(64 * waves), 0, 0, d, s, iters, 1e-3f);
  hipDeviceSynchronize();
  std::vector<unsigned long long> h(blocks * waves); hipMemcpy(h.data(), d, blocks * waves * 8, hipMemcpyDeviceToHost);
  double st = 0; for (auto v : h) st += v;
  const double per_iter = st / (blocks * waves) / iters;
  printf("waves/SIMD=%d  8 pk_fma + %d permlane16_swap + %d permlane32_swap: %7.1f cycles per iteration per wave = %5.1f per SIMD\n",
         waves / 4, N16, N32, per_iter, per_iter / (waves / 4.0));
  hipFree(d); hipFree(s);
}
int main() {
  run<0>("ds_write_b64", 8); run<1>("ds_read_b64", 8); run<2>("ds_write_b32", 8); run<3>("ds_read_b32", 8);
  run<4>("ds_bpermute_b32", 8); run<5>("ds_write_b128", 8); run<6>("ds_read_b128", 8);
  run<0>("ds_write_b64", 4); run<1>("ds_read_b64", 4); run<4>("ds_bpermute_b32", 4);
  run<0>("ds_write_b64", 16); run<1>("ds_read_b64", 16); run<4>("ds_bpermute_b32", 16); run<5>("ds_write_b128", 16); run<6>("ds_read_b128", 16);
  printf("\n");
  for (int w : {4, 8, 12, 16}) {
    run_sw<0, 0>(w); run_sw<4, 0>(w); run_sw<0, 4>(w); run_sw<8, 0>(w); run_sw<0, 8>(w); run_sw<4, 4>(w);
    printf("\n");
  }
  return 0;
}
