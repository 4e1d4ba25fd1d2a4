// Placement probe for the XCD-striped PageRank sweep (experiment tooling).
//
// Each block reads the id of the XCD it runs on (a register read:
// HW_REG_XCC_ID, bits 3:0) and stores it with an ordinary store. Launched
// with the striped sweep's geometry (256-thread blocks, a grid that is
// resident at once), it reports for how many blocks b the XCD equals the XCD
// of block b % 8 — the observed round-robin dispatch that the sweep's L2
// affinity rests on (for speed only: its results do not depend on it).
//
// usage: xcc_probe [grid = 1792] [repeats = 5]
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHECK(e)                                                         \
  do {                                                                   \
    hipError_t _e = (e);                                                 \
    if (_e != hipSuccess) {                                              \
      std::fprintf(stderr, "%s: %s\n", #e, hipGetErrorString(_e));       \
      return 1;                                                          \
    }                                                                    \
  } while (0)

__global__ void __launch_bounds__(256) k_probe(int n, int *xcc) {
  unsigned v;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(v));
  if (threadIdx.x == 0 && (int)blockIdx.x < n) xcc[blockIdx.x] = (int)(v & 0xf);
}

int main(int argc, char **argv) {
  const int grid = argc > 1 ? std::atoi(argv[1]) : 1792;
  const int repeats = argc > 2 ? std::atoi(argv[2]) : 5;
  if (grid < 8 || grid > (1 << 20)) return 2;
  int *d = nullptr;
  CHECK(hipMalloc(&d, grid * sizeof(int)));
  std::vector<int> h(grid);
  for (int r = 0; r < repeats; ++r) {
    CHECK(hipMemset(d, 0xff, grid * sizeof(int)));
    hipLaunchKernelGGL(k_probe, dim3(grid), dim3(256), 0, 0, grid, d);
    CHECK(hipDeviceSynchronize());
    CHECK(hipMemcpy(h.data(), d, grid * sizeof(int), hipMemcpyDeviceToHost));
    int same = 0, per_xcc[16] = {0};
    for (int b = 0; b < grid; ++b) {
      same += h[b] == h[b % 8];
      if (h[b] >= 0 && h[b] < 16) ++per_xcc[h[b]];
    }
    std::printf("launch %d: grid %d, xcc(b) == xcc(b %% 8) for %d blocks (%.1f%%); "
                "xcc of blocks 0..7:", r, grid, same, 100.0 * same / grid);
    for (int b = 0; b < 8; ++b) std::printf(" %d", h[b]);
    std::printf("; blocks per xcc:");
    for (int x = 0; x < 8; ++x) std::printf(" %d", per_xcc[x]);
    std::printf("\n");
  }
  CHECK(hipFree(d));
  return 0;
}
