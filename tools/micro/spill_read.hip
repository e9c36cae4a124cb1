// microbenchmark: the rate at which the chip reads the log-mel spill in exactly k_tail's fetch shape, with no arithmetic
// behind it (gfx950) -- the roof k_tail is held against.
//   1000 "clips" of 54 tiles; a tile is 16 rows x 512 bytes = 8 KB of contiguous memory, fetched as eight 1 KB
//   global_load_lds_dwordx4 pieces with k_tail's source swizzle into the wave's one 8 KB LDS slot; a workgroup of four waves
//   walks clips blockIdx.x, + gridDim.x, ..., wave w takes tiles w, w + 4, ... and waits for a tile before it asks for the
//   next (one tile in flight per wave, as k_tail's one-slot form keeps it).
//   8 waves per CU (two workgroups, k_tail's 4 x 2 ring form) and 16 (four workgroups, the one-slot form); default cache
//   policy and nt (aux = 2).  Prints TB/s for each of the four cases: best and median of 20 launches.
// build: hipcc --offload-arch=gfx950 -O3 -o spill_read spill_read.hip
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <vector>

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

constexpr int kClips = 1000, kTiles = 54, kTileFloats = 2048;

template <int AUX>
__global__ __launch_bounds__(256) void k_read(const float* __restrict__ spill, float* __restrict__ sink, int n_clips) {
  extern __shared__ float smem[];                           // [wave][2048]; the rest of the allocation only sets the occupancy
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  float* const slot = smem + wave * kTileFloats;
  for (int clip = blockIdx.x; clip < n_clips; clip += gridDim.x) {
    const float* const rows = spill + (size_t)clip * kTiles * kTileFloats;
    for (int tile = wave; tile < kTiles; tile += 4) {
      const float* tb = rows + tile * kTileFloats;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const unsigned fr = 2 * i + (lane >> 5), j = (lane & 31) ^ fr;
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(tb + (fr * 128u + j * 4u)),
                                         (__attribute__((address_space(3))) void*)(slot + i * 256), 16, 0, AUX);
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
  }
  if (sink) sink[blockIdx.x * 256 + threadIdx.x] = slot[lane];      // never taken: keeps the slot observable
}

template <int AUX>
static int run(const char* name, const float* d, int n_cu, int wg_per_cu) {
  // LDS per workgroup chosen so that exactly wg_per_cu fit the CU's 160 KB
  const size_t lds = wg_per_cu == 2 ? 72 * 1024 : 36 * 1024;
  CK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_read<AUX>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  const int grid = std::min(kClips, n_cu * wg_per_cu);
  hipEvent_t a, b;
  CK(hipEventCreate(&a)); CK(hipEventCreate(&b));
  std::vector<float> ms;
  for (int rep = 0; rep < 23; ++rep) {
    CK(hipEventRecord(a, 0));
    hipLaunchKernelGGL(k_read<AUX>, dim3(grid), dim3(256), lds, 0, d, (float*)nullptr, kClips);
    CK(hipEventRecord(b, 0));
    CK(hipEventSynchronize(b));
    float t = 0.f;
    CK(hipEventElapsedTime(&t, a, b));
    if (rep >= 3) ms.push_back(t);
  }
  CK(hipGetLastError());
  std::sort(ms.begin(), ms.end());
  const double bytes = (double)kClips * kTiles * kTileFloats * 4;
  printf("%-8s %2d waves/CU (%4d workgroups)  best %7.1f us = %5.2f TB/s   median %7.1f us = %5.2f TB/s\n", name, 4 * wg_per_cu, grid,
         ms.front() * 1e3, bytes / (ms.front() * 1e-3) * 1e-12, ms[ms.size() / 2] * 1e3, bytes / (ms[ms.size() / 2] * 1e-3) * 1e-12);
  CK(hipEventDestroy(a)); CK(hipEventDestroy(b));
  return 0;
}

int main() {
  hipDeviceProp_t prop;
  CK(hipGetDeviceProperties(&prop, 0));
  const int n_cu = prop.multiProcessorCount;
  const size_t bytes = (size_t)kClips * kTiles * kTileFloats * 4;
  float* d = nullptr;
  CK(hipMalloc(&d, bytes));
  CK(hipMemset(d, 0, bytes));
  CK(hipDeviceSynchronize());
  printf("%s, %d CUs; %.1f MB per launch as %d x %d tiles of 8 KB (eight 1 KB LDS-DMA pieces), one slot per wave, no compute\n",
         prop.gcnArchName, n_cu, bytes * 1e-6, kClips, kTiles);
  if (run<0>("default", d, n_cu, 2) || run<0>("default", d, n_cu, 4) || run<2>("nt", d, n_cu, 2) || run<2>("nt", d, n_cu, 4)) return 1;
  CK(hipFree(d));
  return 0;
}
