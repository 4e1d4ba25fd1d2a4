// Shared launch / device scaffold for the .hip translation units: grid
// sizing, the four-section degree-binned sweep (mgx_bins), row and block
// reductions, the wide-row column gather, element-wise one-liners and the
// rocPRIM temp-storage call. Algorithm files keep only what they compute.
// Include from .hip files only.
#ifndef MGX_DEVICE_H
#define MGX_DEVICE_H

#include <type_traits>

#include "mgx_internal.h"

constexpr int kBlock = 256;

// Blocks of kBlock threads for a grid-stride loop over `work` items.
inline int64_t grid_for(int64_t work, int64_t cap = 4096) {
  int64_t g = (work + kBlock - 1) / kBlock;
  if (g < 1) g = 1;
  return g > cap ? cap : g;
}

// ---- bin sections ----------------------------------------------------------
// One launch covers all four degree bins: section `sec` owns blocks
// [goff[sec], goff[sec] + grid[sec]) and the rows rows[off[sec] .. +n[sec]).
struct mgx_bin_sections {
  const int32_t *rows;
  int64_t n[4], off[4], goff[4], grid[4];
};

// Fill the sections from a bin list; returns the total grid (0 = no launch).
inline int64_t mgx_fill_sections(const mgx_bins &bins, mgx_bin_sections *s) {
  s->rows = bins.rows;
  int64_t off = 0, goff = 0;
  for (int b = 0; b < 4; ++b) {
    s->n[b] = bins.count[b];
    s->off[b] = off;
    off += s->n[b];
    s->goff[b] = goff;
    s->grid[b] = bins.grid[b];
    goff += s->grid[b];
  }
  return goff;
}

// Block index b of the launch -> (section, block within the section).
__device__ inline int bin_section(const int64_t (&goff)[4], int64_t b, int64_t *block_in_sec) {
  int sec = 3;
  if (b < goff[1]) sec = 0;
  else if (b < goff[2]) sec = 1;
  else if (b < goff[3]) sec = 2;
  *block_in_sec = b - goff[sec];
  return sec;
}

// blockIdx.x -> (section, block within the section).
__device__ inline int bin_section(const int64_t (&goff)[4], int64_t *block_in_sec) {
  return bin_section(goff, (int64_t)blockIdx.x, block_in_sec);
}

// Call f(lanes, sec, block_in_sec) for the section of block index b, where
// decltype(lanes)::value is the section's lanes per row (4/16/64/256).
template <typename F>
__device__ inline void for_bin_section(const int64_t (&goff)[4], int64_t b, F &&f) {
  int64_t bis;
  switch (bin_section(goff, b, &bis)) {
    case 0: f(std::integral_constant<int, 4>{}, 0, bis); break;
    case 1: f(std::integral_constant<int, 16>{}, 1, bis); break;
    case 2: f(std::integral_constant<int, 64>{}, 2, bis); break;
    default: f(std::integral_constant<int, 256>{}, 3, bis); break;
  }
}

// The same for this block's own index.
template <typename F>
__device__ inline void for_bin_section(const int64_t (&goff)[4], F &&f) {
  for_bin_section(goff, (int64_t)blockIdx.x, static_cast<F &&>(f));
}

// Grid-stride over the rows of section `sec`, THREADS/LANES rows per block per
// step, for block `block` of `nblocks`. Every thread of the block takes every
// step: step(rowp, live, sub), where *rowp is this thread's row if live (the
// groups past the end of the last step are not) and sub its lane within the
// LANES sharing the row.
template <int LANES, int THREADS = kBlock, typename Step>
__device__ inline void for_row_steps(const int32_t *rows_list, int64_t nrows, int64_t block,
                                     int64_t nblocks, Step &&step) {
  static_assert(THREADS % LANES == 0, "whole rows per block");
  constexpr int RPB = THREADS / LANES;
  const int sub = threadIdx.x % LANES;
  for (int64_t base = block * RPB; base < nrows; base += nblocks * RPB) {
    const int64_t ri = base + threadIdx.x / LANES;
    step(rows_list + ri, ri < nrows, sub);
  }
}

// The same over section `sec` as block `block_in_sec` of the section's grid.
template <int LANES, int THREADS = kBlock, typename Step>
__device__ inline void for_bin_row_steps(const mgx_bin_sections &S, int sec,
                                         int64_t block_in_sec, Step &&step) {
  for_row_steps<LANES, THREADS>(S.rows + S.off[sec], S.n[sec], block_in_sec, S.grid[sec],
                                static_cast<Step &&>(step));
}

// f(row, sub) for every row of the section, by each of the row's LANES lanes.
template <int LANES, typename F>
__device__ inline void for_bin_rows(const mgx_bin_sections &S, int sec, int64_t block_in_sec,
                                    F &&f) {
  for_bin_row_steps<LANES>(S, sec, block_in_sec, [&](const int32_t *rowp, bool live, int sub) {
    if (live) f(*rowp, sub);
  });
}

// Reduce v over the LANES lanes of a row; the result is valid in the row's
// lane 0. Sub-wave rows: shuffle tree of width LANES. 256 lanes: wave tree,
// one LDS slot per wave, the row's thread 0 combines its four slots left to
// right; a block of THREADS > 256 is THREADS / 256 such teams of four waves,
// each with its own slots. The 256-lane caller must __syncthreads() before
// its next row_reduce (the slots are reused).
template <int LANES, int THREADS = kBlock, typename T, typename Op>
__device__ inline T row_reduce(T v, Op op) {
  if constexpr (LANES <= 64) {
    for (int o = LANES / 2; o; o >>= 1) v = op(v, __shfl_down(v, o, LANES));
  } else {
    static_assert(LANES == 256, "a row takes a sub-wave group or four waves");
    __shared__ T red[THREADS / 64];
    for (int o = 32; o; o >>= 1) v = op(v, __shfl_down(v, o, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    if constexpr (THREADS == LANES) {
      if (threadIdx.x == 0) v = op(op(op(red[0], red[1]), red[2]), red[3]);
    } else {
      const int w = threadIdx.x >> 6;  // this team's first slot, in its thread 0
      if (threadIdx.x % LANES == 0) v = op(op(op(red[w], red[w + 1]), red[w + 2]), red[w + 3]);
    }
  }
  return v;
}

// The gather-reduce-write sweep over a row list: each lane of a row computes
// gather(row, sub), the row's lanes are combined with op (idle groups
// contribute `identity`), and the row's lane 0 calls finish(row, value).
template <int LANES, int THREADS = kBlock, typename T, typename Op, typename Gather,
          typename Finish>
__device__ inline void reduce_rows(const int32_t *rows_list, int64_t nrows, int64_t block,
                                   int64_t nblocks, T identity, Op op, Gather &&gather,
                                   Finish &&finish) {
  for_row_steps<LANES, THREADS>(
      rows_list, nrows, block, nblocks, [&](const int32_t *rowp, bool live, int sub) {
        T v = identity;
        int32_t row = -1;
        if (live) {
          row = *rowp;
          v = gather(row, sub);
        }
        v = row_reduce<LANES, THREADS>(v, op);
        if (sub == 0 && row >= 0) finish(row, v);
        if constexpr (LANES > 64) __syncthreads();  // row_reduce's slots are reused
      });
}

// The same over section `sec` as block `block_in_sec` of the section's grid.
template <int LANES, int THREADS = kBlock, typename T, typename Op, typename Gather,
          typename Finish>
__device__ inline void reduce_bin_rows(const mgx_bin_sections &S, int sec,
                                       int64_t block_in_sec, T identity, Op op,
                                       Gather &&gather, Finish &&finish) {
  reduce_rows<LANES, THREADS>(S.rows + S.off[sec], S.n[sec], block_in_sec, S.grid[sec],
                              identity, op, static_cast<Gather &&>(gather),
                              static_cast<Finish &&>(finish));
}

// f(c) for every column of CSR range [s, e) owned by lane `sub` of LANES.
// Wide rows: scalar head to 16-byte alignment, int4 nontemporal column loads
// (the col stream is read once: keep it out of L1), scalar tail.
template <int LANES, typename F>
__device__ inline void row_gather(const int32_t *col, uint32_t s, uint32_t e, int sub, F &&f) {
  if constexpr (LANES >= 64) {
    uint32_t s_al = (s + 3u) & ~3u;
    if (s_al > e) s_al = e;
    for (uint32_t j = s + sub; j < s_al; j += LANES) f(col[j]);
    const uint32_t nvec = (e - s_al) / 4;
    typedef int v4i __attribute__((ext_vector_type(4)));
    const v4i *col4 = reinterpret_cast<const v4i *>(col + s_al);
    for (uint32_t c = sub; c < nvec; c += LANES) {
      const v4i cc = __builtin_nontemporal_load(col4 + c);
      f(cc.x);
      f(cc.y);
      f(cc.z);
      f(cc.w);
    }
    for (uint32_t j = s_al + nvec * 4 + sub; j < e; j += LANES) f(col[j]);
  } else {
    for (uint32_t j = s + sub; j < e; j += LANES) f(__builtin_nontemporal_load(col + j));
  }
}

// Reduce v over a THREADS-thread block (wave tree, one LDS slot per wave,
// thread 0 folds identity, slot 0, 1, ... left to right) and hand the block's
// value to atomic(), once per block.
template <int THREADS = kBlock, typename T, typename Op, typename Atomic>
__device__ inline void block_reduce_atomic(T v, T identity, Op op, Atomic atomic) {
  static_assert(THREADS % 64 == 0, "whole waves");
  __shared__ T red[THREADS / 64];
  for (int o = 32; o; o >>= 1) v = op(v, __shfl_down(v, o, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    T s = identity;
    for (int i = 0; i < THREADS / 64; ++i) s = op(s, red[i]);
    atomic(s);
  }
}

struct mgx_op_add {
  template <typename T>
  __device__ T operator()(T a, T b) const { return a + b; }
};
struct mgx_op_min {
  template <typename T>
  __device__ T operator()(T a, T b) const { return min(a, b); }
};
struct mgx_op_max {
  template <typename T>
  __device__ T operator()(T a, T b) const { return max(a, b); }
};

// ---- element-wise kernels ----------------------------------------------------
template <typename T>
__global__ void mgx_k_iota(int64_t n, T *p) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    p[i] = (T)i;
}

template <typename T>
__global__ void mgx_k_fill(int64_t n, T v, T *p) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    p[i] = v;
}

template <typename From, typename To>
__global__ void mgx_k_widen(int64_t n, const From *in, To *out) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    out[i] = (To)in[i];
}

// ---- rocPRIM temp storage ----------------------------------------------------
// call(tmp, bytes) -> hipError_t wraps one rocPRIM primitive: run it with
// tmp = nullptr to size the temp storage, reserve that from the context
// workspace, run it for real.
template <typename Call>
inline mgx_status mgx_with_temp(mgx_context *ctx, const char *what, Call &&call) {
  size_t bytes = 0;
  hipError_t err = call(nullptr, bytes);
  if (err == hipSuccess) {
    void *tmp = nullptr;
    MGX_TRY(ctx->reserve(bytes, &tmp));
    err = call(tmp, bytes);
  }
  if (err != hipSuccess) {
    mgx_set_error("%s failed: %s", what, hipGetErrorString(err));
    return MGX_ERR_HIP;
  }
  return MGX_OK;
}

#endif  // MGX_DEVICE_H
