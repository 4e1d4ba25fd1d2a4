// Gather-bandwidth microbenchmark for MI355X (experiment tooling).
//
// Measures the chip's achievable rate for the PageRank sweep's exact access
// shape — random 4-B gathers from an N-byte f32 table driven by a streamed
// index array — as a function of table size (4 MB..1 GB) and gathers in
// flight per lane. This bounds what ANY vertex ordering can achieve and
// decides whether the sweep is traffic-bound or issue/latency-bound
// (DESIGN.md round-2 item 1).
//
// `lds` mode: a fraction f of the indices falls into the first K table entries,
// which every block copies into LDS first and serves from there (the hot
// prefix of the XCD-striped sweep, profiles/lds_hot_prefix.md). Two forms of
// the two-path gather are timed: the ternary, which compiles to one flat load
// whose address is the LDS or the global one, and both loads unconditional
// with a select (LDS lanes re-read table[0]).
//
// The mode takes the block width and the resident blocks per CU as well: the
// same waves per CU in fewer, wider blocks share a larger table
// (profiles/lds_wide_blocks.md). It prints f = 0 (what the geometry alone
// costs) and the given share.
//
// Build: hipcc --offload-arch=gfx950 -O3 gatherbench.hip -o gatherbench
// Run:   ./gatherbench [table_mb...]
//        ./gatherbench lds [K floats, default 5632]
//        ./gatherbench lds K <256|512|768|896|1024> <blocks per CU> <f>
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#define TRY(x)                                                   \
  do {                                                           \
    hipError_t e = (x);                                          \
    if (e != hipSuccess) {                                       \
      fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__,          \
              hipGetErrorString(e));                             \
      exit(1);                                                   \
    }                                                            \
  } while (0)

constexpr int kBlock = 256;

__global__ void k_fill_idx(int64_t n, uint32_t mask, uint64_t seed, int32_t *idx) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    uint64_t x = seed + (uint64_t)i * 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    x ^= x >> 31;
    idx[i] = (int32_t)((uint32_t)x & mask);
  }
}

// Like k_fill_idx, but a share `hot` (of 2^32) of the indices is uniform in
// [0, k) instead.
__global__ void k_fill_idx_hot(int64_t n, uint32_t mask, uint32_t k, uint32_t hot,
                               uint64_t seed, int32_t *idx) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    uint64_t x = seed + (uint64_t)i * 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    x ^= x >> 31;
    const uint32_t lo = (uint32_t)x, hi = (uint32_t)(x >> 32);
    idx[i] = (int32_t)(hi < hot ? lo % k : lo & mask);
  }
}

// The two-path gather: entries below k from LDS, the rest from the table.
// FORM 0: table only, 1: ternary (one flat load), 2: both loads + select.
template <int FORM>
__device__ inline float lds_or_table(const float *lds, const float *table, uint32_t k,
                                     int32_t c) {
  const bool in = (uint32_t)c < k;
  if constexpr (FORM == 0) {
    return table[c];
  } else if constexpr (FORM == 1) {
    // hipcc selects the address and issues one flat_load_dword (it does the
    // same for a branch around the global load).
    return in ? lds[c] : table[c];
  } else {
    const float a = lds[in ? c : 0];
    const float b = table[in ? 0 : c];
    return in ? a : b;
  }
}

template <int FORM, int THREADS>
__global__ void __launch_bounds__(THREADS) k_gather_lds(int64_t n, const int32_t *idx,
                                                        const float *table, uint32_t k,
                                                        double *out) {
  extern __shared__ float hot_lds[];
  for (uint32_t i = threadIdx.x; i < k; i += THREADS) hot_lds[i] = table[i];
  __syncthreads();
  typedef int v4i __attribute__((ext_vector_type(4)));
  const v4i *idx4 = reinterpret_cast<const v4i *>(idx);
  const int64_t n4 = n / 4;
  double acc = 0.0;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i + stride < n4;
       i += 2 * stride) {
    const v4i c0 = __builtin_nontemporal_load(idx4 + i);
    const v4i c1 = __builtin_nontemporal_load(idx4 + i + stride);
    const float g0 = lds_or_table<FORM>(hot_lds, table, k, c0.x);
    const float g1 = lds_or_table<FORM>(hot_lds, table, k, c0.y);
    const float g2 = lds_or_table<FORM>(hot_lds, table, k, c0.z);
    const float g3 = lds_or_table<FORM>(hot_lds, table, k, c0.w);
    const float g4 = lds_or_table<FORM>(hot_lds, table, k, c1.x);
    const float g5 = lds_or_table<FORM>(hot_lds, table, k, c1.y);
    const float g6 = lds_or_table<FORM>(hot_lds, table, k, c1.z);
    const float g7 = lds_or_table<FORM>(hot_lds, table, k, c1.w);
    acc += (double)g0;
    acc += (double)g1;
    acc += (double)g2;
    acc += (double)g3;
    acc += (double)g4;
    acc += (double)g5;
    acc += (double)g6;
    acc += (double)g7;
  }
  __shared__ double red[THREADS / 64];
  for (int o = 32; o; o >>= 1) acc += __shfl_down(acc, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int i = 0; i < THREADS / 64; ++i) s += red[i];
    atomicAdd(out, s);
  }
}

template <int FORM, int THREADS>
double run_lds(int64_t n_idx, const int32_t *d_idx, const float *d_table, uint32_t k,
               double *d_out, int grid) {
  hipEvent_t e0, e1;
  TRY(hipEventCreate(&e0));
  TRY(hipEventCreate(&e1));
  const size_t lds = (size_t)(k ? k : 1) * 4;
  // Past the default per-block limit the kernel has to be told.
  TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k_gather_lds<FORM, THREADS>),
                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL((k_gather_lds<FORM, THREADS>), dim3(grid), dim3(THREADS), lds, 0, n_idx,
                     d_idx, d_table, k, d_out);
  TRY(hipGetLastError());
  TRY(hipDeviceSynchronize());
  TRY(hipEventRecord(e0));
  for (int r = 0; r < 5; ++r)
    hipLaunchKernelGGL((k_gather_lds<FORM, THREADS>), dim3(grid), dim3(THREADS), lds, 0, n_idx,
                       d_idx, d_table, k, d_out);
  TRY(hipEventRecord(e1));
  TRY(hipEventSynchronize(e1));
  float ms = 0;
  TRY(hipEventElapsedTime(&ms, e0, e1));
  TRY(hipEventDestroy(e0));
  TRY(hipEventDestroy(e1));
  return ms / 5.0;
}

// A share f of the gathers served from a k-float LDS prefix, the rest from a
// 4 MB (L2-resident) table; unroll 8, a grid of per_cu blocks of THREADS per
// CU, which the occupancy query must confirm resident. share < 0: the f
// series {0, 0.25, 0.4} of profiles/lds_hot_prefix.md.
template <int THREADS>
int lds_mode(uint32_t k, int per_cu, double share) {
  const int64_t n_idx = 1ll << 30;
  const uint32_t mask = (4u << 20) / 4 - 1;
  int32_t *d_idx = nullptr;
  double *d_out = nullptr;
  float *d_table = nullptr;
  TRY(hipMalloc(&d_idx, n_idx * 4));
  TRY(hipMalloc(&d_out, 8));
  TRY(hipMalloc(&d_table, (size_t)(mask + 1) * 4));
  TRY(hipMemset(d_table, 0x3f, (size_t)(mask + 1) * 4));
  int cus = 0, block_lds = 0, resident = 0;
  TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, 0));
  TRY(hipDeviceGetAttribute(&block_lds, hipDeviceAttributeMaxSharedMemoryPerBlock, 0));
  TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k_gather_lds<1, THREADS>),
                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)(k ? k : 1) * 4));
  TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&resident, k_gather_lds<1, THREADS>, THREADS,
                                                   (size_t)(k ? k : 1) * 4));
  const int grid = per_cu * cus;
  printf("lds mode: K=%u floats, %d threads x %d blocks per CU (occupancy query: %d; "
         "per-block LDS attribute %d B), 4 MB table, unroll 8, grid %d\n",
         k, THREADS, per_cu, resident, block_lds, grid);
  printf("%6s %10s %10s %12s\n", "f", "form", "ms", "Ggather/s");
  const char *names[3] = {"table", "flat", "select"};
  std::vector<double> fs = {0.0, 0.25, 0.4};
  if (share >= 0.0) fs = {0.0, share};
  for (double f : fs) {
    const uint32_t hot = (uint32_t)(f * 4294967296.0);
    hipLaunchKernelGGL(k_fill_idx_hot, dim3(4096), dim3(kBlock), 0, 0, n_idx, mask, k, hot,
                       1ull, d_idx);
    TRY(hipDeviceSynchronize());
    const double ms[3] = {run_lds<0, THREADS>(n_idx, d_idx, d_table, k, d_out, grid),
                          run_lds<1, THREADS>(n_idx, d_idx, d_table, k, d_out, grid),
                          run_lds<2, THREADS>(n_idx, d_idx, d_table, k, d_out, grid)};
    for (int m = 0; m < 3; ++m)
      printf("%6.2f %10s %10.3f %12.2f\n", f, names[m], ms[m], (double)n_idx / (ms[m] * 1e6));
    fflush(stdout);
  }
  TRY(hipFree(d_table));
  TRY(hipFree(d_idx));
  TRY(hipFree(d_out));
  return 0;
}

int lds_mode_for(int threads, uint32_t k, int per_cu, double share) {
  switch (threads) {
    case 256: return lds_mode<256>(k, per_cu, share);
    case 512: return lds_mode<512>(k, per_cu, share);
    case 768: return lds_mode<768>(k, per_cu, share);
    case 896: return lds_mode<896>(k, per_cu, share);
    case 1024: return lds_mode<1024>(k, per_cu, share);
    default: fprintf(stderr, "block width %d is not built\n", threads); return 2;
  }
}

// The sweep's wide-row shape: int4 nontemporal index loads + G independent
// gathers per lane in flight, f64 accumulation.
template <int UNROLL>
__global__ void __launch_bounds__(kBlock) k_gather(int64_t n, const int32_t *idx,
                                                   const float *table, double *out) {
  typedef int v4i __attribute__((ext_vector_type(4)));
  const v4i *idx4 = reinterpret_cast<const v4i *>(idx);
  const int64_t n4 = n / 4;
  double acc = 0.0;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  for (; i + (UNROLL - 1) * stride < n4; i += UNROLL * stride) {
    float g[4 * UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const v4i c = __builtin_nontemporal_load(idx4 + i + u * stride);
      g[4 * u + 0] = table[c.x];
      g[4 * u + 1] = table[c.y];
      g[4 * u + 2] = table[c.z];
      g[4 * u + 3] = table[c.w];
    }
#pragma unroll
    for (int k = 0; k < 4 * UNROLL; ++k) acc += (double)g[k];
  }
  for (; i < n4; i += stride) {
    const v4i c = __builtin_nontemporal_load(idx4 + i);
    acc += (double)table[c.x] + (double)table[c.y] + (double)table[c.z] +
           (double)table[c.w];
  }
  __shared__ double red[kBlock / 64];
  for (int o = 32; o; o >>= 1) acc += __shfl_down(acc, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) atomicAdd(out, red[0] + red[1] + red[2] + red[3]);
}

template <int UNROLL>
double run_one(int64_t n_idx, const int32_t *d_idx, const float *d_table, double *d_out,
               int grid) {
  hipEvent_t e0, e1;
  TRY(hipEventCreate(&e0));
  TRY(hipEventCreate(&e1));
  // warmup
  hipLaunchKernelGGL((k_gather<UNROLL>), dim3(grid), dim3(kBlock), 0, 0, n_idx, d_idx,
                     d_table, d_out);
  TRY(hipDeviceSynchronize());
  TRY(hipEventRecord(e0));
  for (int r = 0; r < 5; ++r)
    hipLaunchKernelGGL((k_gather<UNROLL>), dim3(grid), dim3(kBlock), 0, 0, n_idx, d_idx,
                       d_table, d_out);
  TRY(hipEventRecord(e1));
  TRY(hipEventSynchronize(e1));
  float ms = 0;
  TRY(hipEventElapsedTime(&ms, e0, e1));
  TRY(hipEventDestroy(e0));
  TRY(hipEventDestroy(e1));
  return ms / 5.0;
}

int main(int argc, char **argv) {
  if (argc > 1 && std::string(argv[1]) == "lds")
    return lds_mode_for(argc > 3 ? atoi(argv[3]) : 256, argc > 2 ? (uint32_t)atol(argv[2]) : 5632u,
                        argc > 4 ? atoi(argv[4]) : 7, argc > 5 ? atof(argv[5]) : -1.0);
  const int64_t n_idx = 1ll << 30;  // 1Gi gathers per pass (the RMAT-26 edge count)
  int32_t *d_idx = nullptr;
  double *d_out = nullptr;
  TRY(hipMalloc(&d_idx, n_idx * 4));
  TRY(hipMalloc(&d_out, 8));
  std::vector<long> sizes = {4, 16, 32, 64, 108, 128, 256, 512, 1024};
  if (argc > 1) {
    sizes.clear();
    for (int a = 1; a < argc; ++a) sizes.push_back(atol(argv[a]));
  }
  printf("gathers=%lld per pass; effective bytes/gather = 4 (idx) + 4 (val)\n",
         (long long)n_idx);
  printf("%8s %6s %6s %10s %12s %12s\n", "table_mb", "unroll", "grid", "ms",
         "Ggather/s", "eff_GB/s");
  for (long mb : sizes) {
    // table sizes are powers of two for masking; 108 -> 128-mask truncated
    uint32_t entries = (uint32_t)((mb << 20) / 4);
    uint32_t mask = 1;
    while ((mask << 1) <= entries) mask <<= 1;
    mask -= 1;  // gathers within the largest pow2 <= size
    float *d_table = nullptr;
    TRY(hipMalloc(&d_table, (size_t)(mask + 1) * 4));
    TRY(hipMemset(d_table, 0x3f, (size_t)(mask + 1) * 4));
    hipLaunchKernelGGL(k_fill_idx, dim3(4096), dim3(kBlock), 0, 0, n_idx, mask, 1ull,
                       d_idx);
    TRY(hipDeviceSynchronize());
    for (int grid : {8192}) {
      double ms2 = run_one<2>(n_idx, d_idx, d_table, d_out, grid);
      double ms4 = run_one<4>(n_idx, d_idx, d_table, d_out, grid);
      double ms8 = run_one<8>(n_idx, d_idx, d_table, d_out, grid);
      for (auto [u, ms] : {std::pair<int, double>{2, ms2}, {4, ms4}, {8, ms8}}) {
        const double gps = (double)n_idx / (ms * 1e6);
        printf("%8ld %6d %6d %10.3f %12.2f %12.1f\n", mb, u, grid, ms, gps, gps * 8);
      }
    }
    TRY(hipFree(d_table));
  }
  TRY(hipFree(d_idx));
  TRY(hipFree(d_out));
  return 0;
}
