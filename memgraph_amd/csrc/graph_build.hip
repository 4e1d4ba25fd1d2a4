// Device-side graph construction for gfx950: deterministic edge-stream
// generation, COO -> CSR (histogram + exclusive scan + scatter), and
// degree-bin work lists for the fused sweep kernels.
//
// Replaces (MI355X-native, from scratch) the host-side layouts built by
// pagerank_alg::PageRankGraph (reference algorithm/pagerank.cpp:166-182) and
// GetGrappoloSuitableGraph (reference louvain.cpp:158-233; sym-CSR, every
// edge stored twice) with int32 indices / fp32 weights in HBM.

#include <cstring>

#include <rocprim/rocprim.hpp>

#include "../../include/mgx_graphgen.h"
#include "mgx_device.h"
#include "mgx_xcd_deal.h"
#include "mgx_xcd_stream.h"

namespace {

__global__ void k_rmat(int64_t n_edges, int scale, uint64_t mixed_seed,
                       mgx_rmat_thresholds t, int32_t *src, int32_t *dst) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n_edges;
       i += (int64_t)gridDim.x * blockDim.x) {
    uint64_t s, d;
    mgx_rmat_edge(mixed_seed, (uint64_t)i, scale, t, &s, &d);
    src[i] = (int32_t)s;
    dst[i] = (int32_t)d;
  }
}

__global__ void k_uniform(int64_t n_edges, uint64_t mixed_seed, uint64_t n_vertices,
                          int32_t *src, int32_t *dst) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n_edges;
       i += (int64_t)gridDim.x * blockDim.x) {
    uint64_t s, d;
    mgx_uniform_edge(mixed_seed, (uint64_t)i, n_vertices, &s, &d);
    src[i] = (int32_t)s;
    dst[i] = (int32_t)d;
  }
}

__global__ void k_weights(int64_t n_edges, uint64_t mixed_seed, float *w) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n_edges;
       i += (int64_t)gridDim.x * blockDim.x) {
    w[i] = (float)mgx_edge_weight(mixed_seed, (uint64_t)i);
  }
}

__global__ void k_hist(int64_t n_edges, const int32_t *idx, uint32_t *counts) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n_edges;
       i += (int64_t)gridDim.x * blockDim.x)
    atomicAdd(&counts[idx[i]], 1u);
}

__global__ void k_hist2(int64_t n_edges, const int32_t *a, const int32_t *b,
                        uint32_t *counts) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n_edges;
       i += (int64_t)gridDim.x * blockDim.x) {
    atomicAdd(&counts[a[i]], 1u);
    atomicAdd(&counts[b[i]], 1u);
  }
}

__global__ void k_hist_ranged(int64_t n_edges, const int32_t *idx, int32_t lo, int32_t hi,
                              uint32_t *counts /* [hi-lo] */) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n_edges;
       i += (int64_t)gridDim.x * blockDim.x) {
    int32_t v = idx[i];
    if (v >= lo && v < hi) atomicAdd(&counts[v - lo], 1u);
  }
}

__global__ void k_inv_outdeg(int64_t n, const uint32_t *deg, float *inv) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    inv[i] = deg[i] ? 1.0f / (float)deg[i] : 0.0f;
}

__global__ void k_bin_keys(int64_t rows, const uint32_t *lo, const uint32_t *hi,
                           int include_zero, uint32_t *keys, uint32_t *vals) {
  for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < rows;
       r += (int64_t)gridDim.x * blockDim.x) {
    const uint32_t deg = hi[r] - lo[r];
    // 0 = zero-degree rows (a section of their own in front of bin0),
    // 1..4 = the four bins, 5 = dropped (sorts last).
    uint32_t k = deg < 8 ? 1u : deg < 64 ? 2u : deg < 1024 ? 3u : 4u;
    if (deg == 0) k = include_zero ? 0u : 5u;
    keys[r] = k;
    vals[r] = (uint32_t)r;
  }
}

__global__ void k_count_bins(int64_t rows, const uint32_t *keys, uint32_t *counts6) {
  // Per-block LDS aggregation first: a naive global histogram measured
  // 706 ms at RMAT-26 (atomic hotspot); this form is ~ms. Key 0 counts the
  // kept zero-degree rows, key 5 the dropped ones.
  __shared__ uint32_t local[6];
  if (threadIdx.x < 6) local[threadIdx.x] = 0;
  __syncthreads();
  for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < rows;
       r += (int64_t)gridDim.x * blockDim.x)
    atomicAdd(&local[keys[r]], 1u);
  __syncthreads();
  if (threadIdx.x < 6 && local[threadIdx.x]) atomicAdd(&counts6[threadIdx.x], local[threadIdx.x]);
}

__global__ void k_pack_pairs(int64_t n_edges, const int32_t *src, const int32_t *dst,
                             const int32_t *perm, uint64_t *keys) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n_edges;
       i += (int64_t)gridDim.x * blockDim.x) {
    const uint32_t d = perm ? (uint32_t)perm[dst[i]] : (uint32_t)dst[i];
    const uint32_t sr = perm ? (uint32_t)perm[src[i]] : (uint32_t)src[i];
    keys[i] = ((uint64_t)d << 32) | sr;
  }
}

__global__ void k_invert_perm(int64_t n, const int32_t *order, int32_t *perm) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    perm[order[i]] = (int32_t)i;
}

__global__ void k_gather_u32(int64_t n, const uint32_t *in, const int32_t *order,
                             uint32_t *out) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    out[i] = in[order[i]];
}

__global__ void k_hist_perm(int64_t n_edges, const int32_t *idx, const int32_t *perm,
                            uint32_t *counts) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n_edges;
       i += (int64_t)gridDim.x * blockDim.x)
    atomicAdd(&counts[perm[idx[i]]], 1u);
}

__global__ void k_pack_pairs_ranged(int64_t n_edges, const int32_t *src, const int32_t *dst,
                                    int32_t lo, int32_t hi, uint64_t *keys) {
  // Out-of-range edges get the max key: they sort last and are trimmed.
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n_edges;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int32_t d = dst[i];
    keys[i] = (d >= lo && d < hi)
                  ? ((uint64_t)(uint32_t)(d - lo) << 32) | (uint32_t)src[i]
                  : ~0ull;
  }
}

__global__ void k_unpack_cols(int64_t n, const uint64_t *keys, int32_t *col) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    col[i] = (int32_t)(uint32_t)keys[i];
}

// Build a sorted in-CSR column array: cols within each row in ascending
// order (gather locality: adjacent cols share cache lines — the measured
// unsorted-scatter build over-fetched 3x algorithmic bytes in the sweep).
mgx_status build_sorted_cols(mgx_context *ctx, const int32_t *d_src, const int32_t *d_dst,
                             const int32_t *perm, int64_t n_edges, int64_t key_rows,
                             bool ranged, int32_t lo, int32_t hi, int32_t *col,
                             int64_t col_count) {
  if (n_edges == 0) return MGX_OK;
  mgx_scope bufs(ctx);
  uint64_t *keys = nullptr, *keys_out = nullptr;
  MGX_TRY(bufs.alloc(&keys, n_edges));
  MGX_TRY(bufs.alloc(&keys_out, n_edges));
  if (ranged) {
    hipLaunchKernelGGL(k_pack_pairs_ranged, dim3(grid_for(n_edges)), dim3(kBlock), 0,
                       ctx->stream, n_edges, d_src, d_dst, lo, hi, keys);
  } else {
    hipLaunchKernelGGL(k_pack_pairs, dim3(grid_for(n_edges)), dim3(kBlock), 0, ctx->stream,
                       n_edges, d_src, d_dst, perm, keys);
  }
  int end_bit = 33;
  while ((1ll << (end_bit - 32)) < key_rows + 1) ++end_bit;
  if (ranged) end_bit = 64;  // the ~0 sentinel must sort last
  MGX_TRY(mgx_with_temp(ctx, "edge key sort", [&](void *tmp, size_t &bytes) {
    return rocprim::radix_sort_keys(tmp, bytes, keys, keys_out, n_edges, 0, end_bit,
                                    ctx->stream);
  }));
  hipLaunchKernelGGL(k_unpack_cols, dim3(grid_for(col_count)), dim3(kBlock), 0, ctx->stream,
                     col_count, keys_out, col);
  return MGX_OK;
}

// Weighted variant of build_sorted_cols (identity layout only): carries the
// fp32 edge weight through the (dst<<32|src) sort so in_w[j] matches
// in_col[j]. Keys sort on the full 64 bits so weight order is deterministic
// (ties between parallel edges keep ascending weight-payload order — the
// weights of parallel edges are interchangeable for every consumer anyway).
mgx_status build_sorted_cols_w(mgx_context *ctx, const int32_t *d_src,
                               const int32_t *d_dst, const float *d_w, int64_t n_edges,
                               int64_t key_rows, int32_t *col, float *out_w) {
  if (n_edges == 0) return MGX_OK;
  mgx_scope bufs(ctx);
  uint64_t *keys = nullptr, *keys_out = nullptr;
  float *vals_out = nullptr;
  MGX_TRY(bufs.alloc(&keys, n_edges));
  MGX_TRY(bufs.alloc(&keys_out, n_edges));
  MGX_TRY(bufs.alloc(&vals_out, n_edges));
  hipLaunchKernelGGL(k_pack_pairs, dim3(grid_for(n_edges)), dim3(kBlock), 0, ctx->stream,
                     n_edges, d_src, d_dst, (const int32_t *)nullptr, keys);
  int end_bit = 33;
  while ((1ll << (end_bit - 32)) < key_rows + 1) ++end_bit;
  MGX_TRY(mgx_with_temp(ctx, "weighted edge sort", [&](void *tmp, size_t &bytes) {
    return rocprim::radix_sort_pairs(tmp, bytes, keys, keys_out, (const float *)d_w,
                                     vals_out, n_edges, 0, end_bit, ctx->stream);
  }));
  hipLaunchKernelGGL(k_unpack_cols, dim3(grid_for(n_edges)), dim3(kBlock), 0, ctx->stream,
                     n_edges, keys_out, col);
  MGX_HIP_TRY(hipMemcpyAsync(out_w, vals_out, n_edges * sizeof(float),
                             hipMemcpyDeviceToDevice, ctx->stream));
  return MGX_OK;
}

__global__ void k_pack_sym(int64_t n_edges, const int32_t *src, const int32_t *dst,
                           const float *w, uint64_t *keys, float *vals) {
  // Each input edge twice: (s->d) and (d->s), the GetGrappoloSuitableGraph
  // layout (louvain.cpp:176-233), as sortable (row<<32|col) keys.
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n_edges;
       i += (int64_t)gridDim.x * blockDim.x) {
    const uint32_t a = (uint32_t)src[i], b = (uint32_t)dst[i];
    const float wi = w ? w[i] : 1.0f;
    keys[2 * i] = ((uint64_t)a << 32) | b;
    keys[2 * i + 1] = ((uint64_t)b << 32) | a;
    if (vals) {
      vals[2 * i] = wi;
      vals[2 * i + 1] = wi;
    }
  }
}

// Sorted symmetric CSR (cols ascending within each row) via pair sort.
mgx_status build_sorted_sym(mgx_context *ctx, const int32_t *d_src, const int32_t *d_dst,
                            const float *d_w, int64_t n_edges, int64_t n_vertices,
                            int32_t *col, float *out_w) {
  if (n_edges == 0) return MGX_OK;
  const int64_t n2 = 2 * n_edges;
  mgx_scope bufs(ctx);
  uint64_t *keys = nullptr, *keys_out = nullptr;
  float *vals = nullptr, *vals_out = nullptr;
  MGX_TRY(bufs.alloc(&keys, n2));
  MGX_TRY(bufs.alloc(&keys_out, n2));
  if (out_w) {
    MGX_TRY(bufs.alloc(&vals, n2));
    MGX_TRY(bufs.alloc(&vals_out, n2));
  }
  hipLaunchKernelGGL(k_pack_sym, dim3(grid_for(n_edges)), dim3(kBlock), 0, ctx->stream,
                     n_edges, d_src, d_dst, d_w, keys, vals);
  int end_bit = 33;
  while ((1ll << (end_bit - 32)) < n_vertices + 1) ++end_bit;
  MGX_TRY(mgx_with_temp(ctx, "symmetric edge sort", [&](void *tmp, size_t &bytes) {
    if (out_w)
      return rocprim::radix_sort_pairs(tmp, bytes, keys, keys_out, vals, vals_out, n2, 0,
                                       end_bit, ctx->stream);
    return rocprim::radix_sort_keys(tmp, bytes, keys, keys_out, n2, 0, end_bit, ctx->stream);
  }));
  hipLaunchKernelGGL(k_unpack_cols, dim3(grid_for(n2)), dim3(kBlock), 0, ctx->stream, n2,
                     keys_out, col);
  if (out_w) {
    MGX_HIP_TRY(hipMemcpyAsync(out_w, vals_out, n2 * sizeof(float),
                               hipMemcpyDeviceToDevice, ctx->stream));
  }
  return MGX_OK;
}

__global__ void k_i64_to_i32(int64_t n, const int64_t *in, int32_t *out) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    out[i] = (int32_t)in[i];
}

__global__ void k_f64_to_f32(int64_t n, const double *in, float *out) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    out[i] = (float)in[i];
}

// Exclusive scan of u32 counts[n] -> row_ptr[n+1] (row_ptr[n] = total).
mgx_status scan_counts(mgx_context *ctx, const uint32_t *counts, int64_t n,
                       uint32_t *row_ptr) {
  // counts has n entries (reading one past would be invalid): scan n entries
  // into row_ptr[0..n) and set the total separately.
  MGX_TRY(mgx_with_temp(ctx, "row_ptr scan", [&](void *tmp, size_t &bytes) {
    return rocprim::exclusive_scan(tmp, bytes, counts, row_ptr, 0u, n,
                                   rocprim::plus<uint32_t>(), ctx->stream);
  }));
  // row_ptr[n] = row_ptr[n-1] + counts[n-1]
  uint32_t last_off = 0, last_cnt = 0;
  if (n > 0) {
    MGX_HIP_TRY(hipMemcpyAsync(&last_off, row_ptr + n - 1, 4, hipMemcpyDeviceToHost,
                               ctx->stream));
    MGX_HIP_TRY(hipMemcpyAsync(&last_cnt, counts + n - 1, 4, hipMemcpyDeviceToHost,
                               ctx->stream));
    MGX_HIP_TRY(hipStreamSynchronize(ctx->stream));
  }
  const uint32_t total = last_off + last_cnt;
  MGX_HIP_TRY(hipMemcpyAsync(row_ptr + n, &total, 4, hipMemcpyHostToDevice, ctx->stream));
  MGX_HIP_TRY(hipStreamSynchronize(ctx->stream));
  return MGX_OK;
}

}  // namespace

mgx_status mgx_gen_rmat_device(mgx_context *ctx, int scale, int64_t n_edges, uint64_t seed,
                               double a, double b, double c, int32_t *d_src, int32_t *d_dst) {
  const uint64_t ms = mgx_seed_mix(seed);
  const mgx_rmat_thresholds t = mgx_rmat_make_thresholds(a, b, c);
  hipLaunchKernelGGL(k_rmat, dim3(grid_for(n_edges)), dim3(kBlock), 0, ctx->stream, n_edges,
                     scale, ms, t, d_src, d_dst);
  MGX_HIP_TRY(hipGetLastError());
  return MGX_OK;
}

mgx_status mgx_gen_uniform_device(mgx_context *ctx, int64_t n_vertices, int64_t n_edges,
                                  uint64_t seed, int32_t *d_src, int32_t *d_dst) {
  const uint64_t ms = mgx_seed_mix(seed);
  hipLaunchKernelGGL(k_uniform, dim3(grid_for(n_edges)), dim3(kBlock), 0, ctx->stream,
                     n_edges, ms, (uint64_t)n_vertices, d_src, d_dst);
  MGX_HIP_TRY(hipGetLastError());
  return MGX_OK;
}

mgx_status mgx_gen_weights_device(mgx_context *ctx, int64_t n_edges, uint64_t seed,
                                  float *d_w) {
  const uint64_t ms = mgx_seed_mix(seed);
  hipLaunchKernelGGL(k_weights, dim3(grid_for(n_edges)), dim3(kBlock), 0, ctx->stream,
                     n_edges, ms, d_w);
  MGX_HIP_TRY(hipGetLastError());
  return MGX_OK;
}

mgx_status mgx_build_bins_range(mgx_scope &own, const uint32_t *lo, const uint32_t *hi,
                                int64_t rows, bool include_zero, mgx_bins *bins) {
  mgx_context *ctx = own.ctx;
  bins->rows = nullptr;
  if (rows == 0) return MGX_OK;
  int32_t *list = nullptr;
  MGX_TRY(own.alloc_plain(&list, rows));
  mgx_scope bufs(ctx);
  uint32_t *keys = nullptr, *keys_out = nullptr, *vals = nullptr;
  MGX_TRY(bufs.alloc_plain(&keys, rows));
  MGX_TRY(bufs.alloc_plain(&keys_out, rows));
  MGX_TRY(bufs.alloc_plain(&vals, rows));
  uint32_t *counts6 = nullptr;
  MGX_TRY(bufs.alloc_plain(&counts6, 6));
  MGX_HIP_TRY(hipMemsetAsync(counts6, 0, 24, ctx->stream));

  hipLaunchKernelGGL(k_bin_keys, dim3(grid_for(rows)), dim3(kBlock), 0, ctx->stream, rows,
                     lo, hi, include_zero ? 1 : 0, keys, vals);
  hipLaunchKernelGGL(k_count_bins, dim3(grid_for(rows)), dim3(kBlock), 0, ctx->stream, rows,
                     keys, counts6);

  // Stable 3-bit radix sort: within a bin, rows stay in ascending id order,
  // the zero-degree rows (key 0) ahead of bin0's others; key 5 (dropped rows)
  // lands past the used prefix.
  MGX_TRY(mgx_with_temp(ctx, "degree-bin sort", [&](void *tmp, size_t &bytes) {
    return rocprim::radix_sort_pairs(tmp, bytes, keys, keys_out, vals,
                                     (uint32_t *)list, rows, 0, 3, ctx->stream);
  }));

  uint32_t h_counts[6] = {0, 0, 0, 0, 0, 0};
  MGX_HIP_TRY(hipMemcpyAsync(h_counts, counts6, 24, hipMemcpyDeviceToHost, ctx->stream));
  MGX_HIP_TRY(hipStreamSynchronize(ctx->stream));
  // Consumers see bin0 as before: the zero-degree rows and the rows of
  // degree 1..7 from offset 0.
  bins->n_zero = h_counts[0];
  bins->count[0] = (int64_t)h_counts[0] + h_counts[1];
  for (int b = 1; b < 4; ++b) bins->count[b] = h_counts[b + 1];
  for (int b = 0; b < 4; ++b) bins->grid[b] = mgx_bin_grid(b, bins->count[b]);
  bins->rows = list;
  return MGX_OK;
}

mgx_status mgx_build_bins_range(mgx_context *ctx, const uint32_t *lo, const uint32_t *hi,
                                int64_t rows, bool include_zero, mgx_bins *bins) {
  mgx_scope own(ctx);
  MGX_TRY(mgx_build_bins_range(own, lo, hi, rows, include_zero, bins));
  (void)own.give_up(bins->rows);
  return MGX_OK;
}

mgx_status mgx_build_bins(mgx_context *ctx, const uint32_t *row_ptr, int64_t rows,
                          mgx_bins *bins) {
  return mgx_build_bins_range(ctx, row_ptr, row_ptr + 1, rows, /*include_zero=*/true,
                              bins);
}

namespace {
// Binary-search the sorted cols of each row for the stripe boundary value.
__global__ void k_stripe_search(int64_t rows, const uint32_t *row_ptr, const int32_t *col,
                                int32_t boundary, uint32_t *out) {
  for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < rows;
       r += (int64_t)gridDim.x * blockDim.x) {
    uint32_t lo = row_ptr[r], hi = row_ptr[r + 1];
    while (lo < hi) {
      uint32_t mid = (lo + hi) / 2;
      if (col[mid] < boundary) lo = mid + 1;
      else hi = mid;
    }
    out[r] = lo;
  }
}

// The 9 XCD-stripe boundaries of every heavy row: out[x*nH + slot] is the
// first col of row H[slot] whose source id is >= off[x] (off[0] = 0 and
// off[8] = V give the row's own start and end).
__global__ void k_xcd_search(int64_t nH, const int32_t *H, const uint32_t *row_ptr,
                             const int32_t *col, int64_t V, uint32_t *out) {
  for (int64_t s = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; s < nH;
       s += (int64_t)gridDim.x * blockDim.x) {
    const int32_t r = H[s];
    const uint32_t end = row_ptr[r + 1];
    uint32_t lo = row_ptr[r];
    out[s] = lo;
    for (int x = 1; x < kXcdStripes; ++x) {
      const int32_t boundary = (int32_t)mgx_xcd_stripe_off(V, x);
      uint32_t hi = end;  // boundaries ascend: resume from the previous one
      while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (col[mid] < boundary) lo = mid + 1;
        else hi = mid;
      }
      out[(size_t)x * nH + s] = lo;
    }
    out[(size_t)kXcdStripes * nH + s] = end;
  }
}

// Deal the hot-first sort to the 8 XCD stripes: position p -> id
// mgx_xcd_deal(p, V), for the order map and the permuted out-degrees alike.
__global__ void k_xcd_deal(int64_t n, const int32_t *order_sorted, const uint32_t *deg_sorted,
                           int32_t *order, uint32_t *deg) {
  for (int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; p < n;
       p += (int64_t)gridDim.x * blockDim.x) {
    const int64_t id = mgx_xcd_deal(p, n);
    order[id] = order_sorted[p];
    deg[id] = deg_sorted[p];
  }
}

// The 32 (stripe, section) lists of the striped launch in the order it reads
// them: list k = x * 4 + (3 - sec). Segment i of list k is item first + i of
// the stream build's allotment and offset arrays.
struct xcd_stream_lists {
  const int32_t *rows[kXcdStripes * 4];
  int64_t n[kXcdStripes * 4];
  int64_t first[kXcdStripes * 4 + 1];
  uint32_t base[kXcdStripes];  // first int of the stripe's window (fill pass)
};

// allot[item] = ints allotted to the item's segment (mgx_xcd_stream.h).
__global__ void k_xcd_stream_allot(xcd_stream_lists L, const uint32_t *xptr, int64_t nH,
                                   uint32_t *allot) {
  for (int k = 0; k < kXcdStripes * 4; ++k) {
    const int x = k / 4, sec = 3 - k % 4;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < L.n[k];
         i += (int64_t)gridDim.x * blockDim.x) {
      const int32_t slot = L.rows[k][i];
      const uint32_t lo = xptr[(size_t)x * nH + slot];
      const uint32_t hi = xptr[(size_t)(x + 1) * nH + slot];
      allot[L.first[k] + i] = mgx_xcd_seg_allot(lo, hi - lo, mgx_xcd_seg_aligned(sec));
    }
  }
}

// Copy every segment to its place in the stream, zero the padding of its
// allotment and record its bounds. rel[item] is the start of the item's
// allotment within its stripe's window. A segment is copied by as many lanes
// as the sweep gives it.
__global__ void __launch_bounds__(kBlock)
k_xcd_stream_fill(xcd_stream_lists L, const uint32_t *xptr, int64_t nH, const int32_t *col,
                  const uint32_t *rel, int32_t *scol, uint32_t *slo, uint32_t *shi) {
  for (int x = 0; x < kXcdStripes; ++x) {
    auto section = [&](auto lanes, int sec) {
      constexpr int LANES = decltype(lanes)::value;
      const int k = x * 4 + (3 - sec);
      const bool aligned = mgx_xcd_seg_aligned(sec);
      for_row_steps<LANES>(
          L.rows[k], L.n[k], blockIdx.x, gridDim.x, [&](const int32_t *rowp, bool live, int sub) {
            if (!live) return;
            const int32_t slot = *rowp;
            const int64_t item = L.first[k] + (rowp - L.rows[k]);
            const uint32_t lo = xptr[(size_t)x * nH + slot];
            const uint32_t len = xptr[(size_t)(x + 1) * nH + slot] - lo;
            const uint32_t pos = L.base[x] + rel[item];
            const uint32_t start = mgx_xcd_seg_start(pos, lo, aligned);
            for (uint32_t j = sub; j < len; j += LANES) scol[start + j] = col[lo + j];
            if (sub == 0) {
              slo[(size_t)x * nH + slot] = start;
              shi[(size_t)x * nH + slot] = start + len;
              const uint32_t end = pos + mgx_xcd_seg_allot(lo, len, aligned);
              for (uint32_t j = pos; j < start; ++j) scol[j] = 0;
              for (uint32_t j = start + len; j < end; ++j) scol[j] = 0;
            }
          });
    };
    section(std::integral_constant<int, 256>{}, 3);
    section(std::integral_constant<int, 64>{}, 2);
    section(std::integral_constant<int, 16>{}, 1);
    section(std::integral_constant<int, 4>{}, 0);
  }
}

// The stripe-major column stream of the striped launch (g->xcd_scol, lever 6).
mgx_status build_xcd_stream(mgx_context *ctx, mgx_graph *g) {
  if (const char *e = getenv("MGX_PR_XCD_STREAM")) {
    if (*e && atoi(e) == 0) return MGX_OK;
  }
  const int64_t nH = g->xcd_nH;
  xcd_stream_lists L = {};
  int64_t items = 0, aligned_items = 0;
  for (int x = 0; x < kXcdStripes; ++x) {
    mgx_bin_sections S;
    (void)mgx_fill_sections(g->xcd_bins[x], &S);
    for (int sec = 3; sec >= 0; --sec) {
      const int k = x * 4 + (3 - sec);
      L.rows[k] = S.rows + S.off[sec];
      L.n[k] = S.n[sec];
      L.first[k] = items;
      items += S.n[sec];
      if (mgx_xcd_seg_aligned(sec)) aligned_items += S.n[sec];
    }
  }
  L.first[kXcdStripes * 4] = items;
  if (items == 0) return MGX_OK;
  // Bounds are uint32. The segments hold at most in_edges ints, an aligned
  // allotment adds at most 6 and a stripe's window at most kXcdStreamAlign - 1:
  // when that bound fits, no offset below can wrap. A graph past it (a stream
  // within a few percent of 2^32 ints) keeps reading in_col.
  const uint64_t most = (uint64_t)g->in_edges + 6ull * (uint64_t)aligned_items +
                        (uint64_t)kXcdStripes * kXcdStreamAlign;
  if (most > 0xFFFFFFFFull) return MGX_OK;

  mgx_scope bufs(ctx);
  uint32_t *allot = nullptr, *rel = nullptr;
  MGX_TRY(bufs.alloc(&allot, items));
  MGX_TRY(bufs.alloc(&rel, items));
  hipLaunchKernelGGL(k_xcd_stream_allot, dim3(grid_for(items)), dim3(kBlock), 0, ctx->stream, L,
                     (const uint32_t *)g->xcd_ptr, nH, allot);
  // One exclusive scan per stripe; a stripe's length is its last offset plus
  // its last allotment.
  uint32_t last_rel[kXcdStripes] = {0}, last_allot[kXcdStripes] = {0};
  for (int x = 0; x < kXcdStripes; ++x) {
    const int64_t first = L.first[x * 4], n = L.first[x * 4 + 4] - first;
    if (n == 0) continue;
    MGX_TRY(mgx_with_temp(ctx, "column stream scan", [&](void *tmp, size_t &bytes) {
      return rocprim::exclusive_scan(tmp, bytes, allot + first, rel + first, 0u, n,
                                     rocprim::plus<uint32_t>(), ctx->stream);
    }));
    MGX_HIP_TRY(hipMemcpyAsync(&last_rel[x], rel + first + n - 1, 4, hipMemcpyDeviceToHost,
                               ctx->stream));
    MGX_HIP_TRY(hipMemcpyAsync(&last_allot[x], allot + first + n - 1, 4, hipMemcpyDeviceToHost,
                               ctx->stream));
  }
  MGX_HIP_TRY(hipStreamSynchronize(ctx->stream));
  uint64_t end[kXcdStripes], total = 0;
  for (int x = 0; x < kXcdStripes; ++x) {
    L.base[x] = (uint32_t)total;
    end[x] = total + last_rel[x] + last_allot[x];
    total = mgx_xcd_stream_round(end[x]);
  }
  if (total > most) {  // cannot be: the scans would contradict the bound above
    mgx_set_error("column stream: %llu ints exceed the bound %llu",
                  (unsigned long long)total, (unsigned long long)most);
    return MGX_ERR_TOO_LARGE;
  }

  MGX_HIP_TRY(mgx_hip_malloc(&g->xcd_scol, (size_t)total * sizeof(int32_t)));
  MGX_HIP_TRY(mgx_hip_malloc(&g->xcd_slo, (size_t)kXcdStripes * nH * sizeof(uint32_t)));
  MGX_HIP_TRY(mgx_hip_malloc(&g->xcd_shi, (size_t)kXcdStripes * nH * sizeof(uint32_t)));
  // Empty segments are in no list: their bounds stay 0 and nothing reads them.
  MGX_HIP_TRY(hipMemsetAsync(g->xcd_slo, 0, (size_t)kXcdStripes * nH * sizeof(uint32_t),
                             ctx->stream));
  MGX_HIP_TRY(hipMemsetAsync(g->xcd_shi, 0, (size_t)kXcdStripes * nH * sizeof(uint32_t),
                             ctx->stream));
  for (int x = 0; x < kXcdStripes; ++x) {  // the gap up to the next window
    const uint64_t next = mgx_xcd_stream_round(end[x]);
    if (next > end[x]) {
      MGX_HIP_TRY(hipMemsetAsync(g->xcd_scol + end[x], 0, (size_t)(next - end[x]) * sizeof(int32_t),
                                 ctx->stream));
    }
  }
  hipLaunchKernelGGL(k_xcd_stream_fill, dim3(grid_for(items, 8192)), dim3(kBlock), 0,
                     ctx->stream, L, (const uint32_t *)g->xcd_ptr, nH,
                     (const int32_t *)g->in_col, (const uint32_t *)rel, g->xcd_scol, g->xcd_slo,
                     g->xcd_shi);
  MGX_HIP_TRY(hipGetLastError());
  MGX_HIP_TRY(hipStreamSynchronize(ctx->stream));
  g->xcd_stream_ints = (int64_t)total;
  return MGX_OK;
}

// Heavy-row stripe view for the XCD-striped PageRank sweep (g->xcd).
mgx_status build_xcd_view(mgx_context *ctx, mgx_graph *g) {
  // Heavy rows are whole sections of bins_in, so the slot -> row list is the
  // tail of bins_in.rows: MGX_PR_XCD_HEAVY_MIN is one of the bin edges.
  int heavy_min = 64;
  if (const char *e = getenv("MGX_PR_XCD_HEAVY_MIN")) {
    const int v = atoi(e);
    if (v == 8 || v == 64 || v == 1024) heavy_min = v;
  }
  const int sec = heavy_min == 8 ? 1 : heavy_min == 64 ? 2 : 3;
  g->xcd_heavy_min = heavy_min;
  g->xcd_heavy_sec = sec;
  int64_t light = 0, nH = 0;
  for (int b = 0; b < 4; ++b) (b < sec ? light : nH) += g->bins_in.count[b];
  g->xcd_nH = nH;
  if (nH == 0) return MGX_OK;
  g->xcd_H = g->bins_in.rows + light;
  MGX_HIP_TRY(mgx_hip_malloc(&g->xcd_ptr, (size_t)(kXcdStripes + 1) * nH * sizeof(uint32_t)));
  hipLaunchKernelGGL(k_xcd_search, dim3(grid_for(nH)), dim3(kBlock), 0, ctx->stream, nH,
                     g->xcd_H, g->in_row_ptr, g->in_col, g->n_vertices, g->xcd_ptr);
  for (int x = 0; x < kXcdStripes; ++x) {
    // Empty segments are dropped: the finish kernel skips them by comparing
    // the two boundaries, so their partial slots are never read.
    MGX_TRY(mgx_build_bins_range(ctx, g->xcd_ptr + (size_t)x * nH,
                                 g->xcd_ptr + (size_t)(x + 1) * nH, nH,
                                 /*include_zero=*/false, &g->xcd_bins[x]));
  }
  // The sweep picks its stripe's sections by block index: keep them on the
  // device rather than in the kernel arguments.
  mgx_bin_sections secs[kXcdStripes];
  for (int x = 0; x < kXcdStripes; ++x) (void)mgx_fill_sections(g->xcd_bins[x], &secs[x]);
  MGX_HIP_TRY(mgx_hip_malloc(&g->xcd_sec, sizeof(secs)));
  MGX_HIP_TRY(hipMemcpyAsync(g->xcd_sec, secs, sizeof(secs), hipMemcpyHostToDevice,
                             ctx->stream));
  MGX_HIP_TRY(hipStreamSynchronize(ctx->stream));
  return build_xcd_stream(ctx, g);
}
}  // namespace

bool mgx_xcd_wanted(int64_t n_vertices) {
  const char *stripes = getenv("MGX_PR_STRIPES");
  if (stripes && atoi(stripes) > 0) return false;  // the sequential stripe path
  const char *e = getenv("MGX_PR_XCD");
  if (e && *e) return atoi(e) != 0;
  // Unset: on from 1.5 * 2^25 vertices. Measured per sweep against the
  // unstriped layout (profiles/xcd_stripes.md): +6% at 2^22, +3% at 2^23,
  // -0.7% at 2^24, -2% at 2^25, -12% at 2^26. While f32 contrib[V] sits
  // well inside the 256 MiB Infinity Cache an L2 miss is cheap and the
  // partials and two extra launches cost more than they save; the 2% at
  // 2^25 does not repay the ~7 ms the view adds to the build within 20
  // sweeps. The threshold lies between the two measured points, where
  // contrib reaches three quarters of the Infinity Cache.
  return n_vertices >= (int64_t)3 << 24;
}

mgx_status mgx_build_stripes(mgx_context *ctx, mgx_graph *g) {
  // Called while row_end is still the clamped row count (the sharded path
  // re-pads it afterwards), so this is exactly the in-CSR row count.
  const int64_t rows = g->row_end - g->row_begin;
  const int64_t V = g->n_vertices;
  if (g->xcd) {
    // XCD-affine layout: `order` is already dealt to 8 stripes, whose
    // boundaries are the exact prefix sums off[1..7] (not x * width). Only
    // heavy rows are striped, all 8 stripes in one launch; the sequential
    // stripe view below stays off.
    g->n_stripes = 1;
    return build_xcd_view(ctx, g);
  }
  int n_stripes = 1;
  const char *env = getenv("MGX_PR_STRIPES");
  if (env && atoi(env) > 0) {
    n_stripes = atoi(env);
  } else if (g->order == nullptr) {
    // auto (identity layout, e.g. sharded): keep the gathered contrib
    // stripe (f32[V/S]) under ~96 MB so it stays Infinity-Cache-resident.
    const int64_t contrib_bytes = V * 4;
    n_stripes = (int)((contrib_bytes + (96 << 20) - 1) / (96 << 20));
    if (n_stripes < 1) n_stripes = 1;
  } else {
    // Hot-first-permuted layout: the hub prefix already keeps the gather
    // working set cache-resident; stripes only add fp64-partial traffic
    // (measured RMAT-26: S=1 116.3 G edges/s vs S=3 106.0: a few contiguous
    // stripes only move lines from HBM to the Infinity Cache, and the sweep
    // is bound by the fabric line rate per L2 miss, not by HBM). Stay
    // unstriped; the XCD-affine view above is the striping that changes
    // what each L2 holds.
    n_stripes = 1;
  }
  if (n_stripes > 16) n_stripes = 16;
  g->n_stripes = n_stripes;
  if (n_stripes == 1) return MGX_OK;
  g->stripe_width = (V + n_stripes - 1) / n_stripes;

  MGX_HIP_TRY(mgx_hip_malloc(&g->stripe_ptr, (size_t)(n_stripes + 1) * rows * sizeof(uint32_t)));
  // boundaries: sp[0] = row starts, sp[S] = row ends, sp[s] = searchsorted.
  struct CopyK {
    static __global__ void shift(int64_t rows, const uint32_t *row_ptr, uint32_t *lo,
                                 uint32_t *hi) {
      for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < rows;
           r += (int64_t)gridDim.x * blockDim.x) {
        lo[r] = row_ptr[r];
        hi[r] = row_ptr[r + 1];
      }
    }
  };
  hipLaunchKernelGGL(CopyK::shift, dim3(grid_for(rows)), dim3(kBlock), 0, ctx->stream, rows,
                     g->in_row_ptr, g->stripe_ptr, g->stripe_ptr + (size_t)n_stripes * rows);
  for (int sIdx = 1; sIdx < n_stripes; ++sIdx) {
    hipLaunchKernelGGL(k_stripe_search, dim3(grid_for(rows)), dim3(kBlock), 0, ctx->stream,
                       rows, g->in_row_ptr, g->in_col,
                       (int32_t)((int64_t)sIdx * g->stripe_width),
                       g->stripe_ptr + (size_t)sIdx * rows);
  }
  for (int sIdx = 0; sIdx < n_stripes; ++sIdx) {
    const bool include_zero = (sIdx == 0) || (sIdx == n_stripes - 1);
    MGX_TRY(mgx_build_bins_range(ctx, g->stripe_ptr + (size_t)sIdx * rows,
                                 g->stripe_ptr + (size_t)(sIdx + 1) * rows, rows,
                                 include_zero, &g->stripe_bins[sIdx]));
  }
  return MGX_OK;
}

mgx_status mgx_build_from_device_coo(mgx_context *ctx, const int32_t *d_src,
                                     const int32_t *d_dst, const float *d_w,
                                     int64_t n_vertices, int64_t n_edges, uint32_t flags,
                                     mgx_graph *g) {
  const int64_t V = n_vertices, E = n_edges;
  g->n_vertices = V;
  g->n_edges = E;
  g->flags = flags;
  g->row_begin = 0;
  g->row_end = V;
  g->in_edges = E;

  hipEvent_t ev0, ev1;
  MGX_HIP_TRY(hipEventCreate(&ev0));
  MGX_HIP_TRY(hipEventCreate(&ev1));
  MGX_HIP_TRY(hipEventRecord(ev0, ctx->stream));

  mgx_scope bufs(ctx);
  uint32_t *counts = nullptr;
  MGX_TRY(bufs.alloc_plain(&counts, V));

  // out-degree (+ inv) — always needed by PageRank/Katz result paths.
  MGX_HIP_TRY(mgx_hip_malloc(&g->out_degree, (V > 0 ? V : 1) * sizeof(uint32_t)));
  MGX_HIP_TRY(hipMemsetAsync(g->out_degree, 0, V * sizeof(uint32_t), ctx->stream));
  hipLaunchKernelGGL(k_hist, dim3(grid_for(E)), dim3(kBlock), 0, ctx->stream, E, d_src,
                     g->out_degree);
  MGX_HIP_TRY(mgx_hip_malloc(&g->inv_outdeg, (V > 0 ? V : 1) * sizeof(float)));
  hipLaunchKernelGGL(k_inv_outdeg, dim3(grid_for(V)), dim3(kBlock), 0, ctx->stream, V,
                     g->out_degree, g->inv_outdeg);

  if ((flags & MGX_BUILD_IN_CSR) && (flags & MGX_BUILD_NO_PERM)) {
    // Identity layout (online/dynamic paths: row ids must equal scan ids).
    MGX_HIP_TRY(hipMemsetAsync(counts, 0, V * sizeof(uint32_t), ctx->stream));
    hipLaunchKernelGGL(k_hist, dim3(grid_for(E)), dim3(kBlock), 0, ctx->stream, E, d_dst,
                       counts);
    MGX_HIP_TRY(mgx_hip_malloc(&g->in_row_ptr, (V + 1) * sizeof(uint32_t)));
    MGX_TRY(scan_counts(ctx, counts, V, g->in_row_ptr));
    MGX_HIP_TRY(mgx_hip_malloc(&g->in_col, (E > 0 ? E : 1) * sizeof(int32_t)));
    if ((flags & MGX_BUILD_WEIGHTED) && d_w) {
      MGX_HIP_TRY(mgx_hip_malloc(&g->in_w, (E > 0 ? E : 1) * sizeof(float)));
      MGX_TRY(build_sorted_cols_w(ctx, d_src, d_dst, d_w, E, V, g->in_col, g->in_w));
    } else {
      MGX_TRY(build_sorted_cols(ctx, d_src, d_dst, nullptr, E, V, false, 0, 0, g->in_col,
                                E));
    }
    MGX_TRY(mgx_build_bins(ctx, g->in_row_ptr, V, &g->bins_in));
  } else if (flags & MGX_BUILD_IN_CSR) {
    // Hot-first vertex permutation: renumber by descending out-degree
    // (stable, ties by original id) so the most-gathered contrib entries
    // pack into the lowest addresses (L2/L3-resident under power-law skew).
    int32_t *d_perm = nullptr;
    MGX_HIP_TRY(mgx_hip_malloc(&g->order, (V > 0 ? V : 1) * sizeof(int32_t)));
    MGX_TRY(bufs.alloc_plain(&d_perm, V));
    {
      mgx_scope sort_bufs(ctx);
      uint32_t *deg_sorted = nullptr;
      int32_t *iota = nullptr;
      MGX_TRY(sort_bufs.alloc_plain(&deg_sorted, V));
      MGX_TRY(sort_bufs.alloc_plain(&iota, V));
      hipLaunchKernelGGL(mgx_k_iota<int32_t>, dim3(grid_for(V)), dim3(kBlock), 0,
                         ctx->stream, V, iota);
      MGX_TRY(mgx_with_temp(ctx, "hot-first degree sort", [&](void *tmp, size_t &bytes) {
        return rocprim::radix_sort_pairs_desc(tmp, bytes, g->out_degree, deg_sorted, iota,
                                              g->order, V, 0, 32, ctx->stream);
      }));
      g->xcd = mgx_xcd_wanted(V);
      if (g->xcd) {
        // XCD-affine layout: deal the sorted positions to 8 stripes
        // (mgx_xcd_deal.h); iota is free again and holds the sorted order.
        MGX_HIP_TRY(hipMemcpyAsync(iota, g->order, V * sizeof(int32_t),
                                   hipMemcpyDeviceToDevice, ctx->stream));
        hipLaunchKernelGGL(k_xcd_deal, dim3(grid_for(V)), dim3(kBlock), 0, ctx->stream, V,
                           iota, deg_sorted, g->order, g->out_degree);
      } else {
        MGX_HIP_TRY(hipMemcpyAsync(g->out_degree, deg_sorted, V * sizeof(uint32_t),
                                   hipMemcpyDeviceToDevice, ctx->stream));
      }
      // out_degree / inv_outdeg are now in the permuted space.
      hipLaunchKernelGGL(k_invert_perm, dim3(grid_for(V)), dim3(kBlock), 0, ctx->stream, V,
                         g->order, d_perm);
      hipLaunchKernelGGL(k_inv_outdeg, dim3(grid_for(V)), dim3(kBlock), 0, ctx->stream, V,
                         g->out_degree, g->inv_outdeg);
    }
    MGX_HIP_TRY(hipMemsetAsync(counts, 0, V * sizeof(uint32_t), ctx->stream));
    hipLaunchKernelGGL(k_hist_perm, dim3(grid_for(E)), dim3(kBlock), 0, ctx->stream, E,
                       d_dst, d_perm, counts);
    MGX_HIP_TRY(mgx_hip_malloc(&g->in_row_ptr, (V + 1) * sizeof(uint32_t)));
    MGX_TRY(scan_counts(ctx, counts, V, g->in_row_ptr));
    MGX_HIP_TRY(mgx_hip_malloc(&g->in_col, (E > 0 ? E : 1) * sizeof(int32_t)));
    MGX_TRY(build_sorted_cols(ctx, d_src, d_dst, d_perm, E, V, false, 0, 0, g->in_col, E));
    bufs.release(d_perm);
    MGX_TRY(mgx_build_bins(ctx, g->in_row_ptr, V, &g->bins_in));
    MGX_TRY(mgx_build_stripes(ctx, g));
  }

  if (flags & MGX_BUILD_OUT_CSR) {
    // out-CSR in the ORIGINAL vertex space (Brandes keys results by scan
    // ids and traverses forward edges; no hot-first perm here).
    MGX_HIP_TRY(hipMemsetAsync(counts, 0, V * sizeof(uint32_t), ctx->stream));
    hipLaunchKernelGGL(k_hist, dim3(grid_for(E)), dim3(kBlock), 0, ctx->stream, E, d_src,
                       counts);
    MGX_HIP_TRY(mgx_hip_malloc(&g->out_row_ptr, (V + 1) * sizeof(uint32_t)));
    MGX_TRY(scan_counts(ctx, counts, V, g->out_row_ptr));
    MGX_HIP_TRY(mgx_hip_malloc(&g->out_col, (E > 0 ? E : 1) * sizeof(int32_t)));
    // reuse the sorted-cols builder with (src,dst) swapped: rows = sources
    MGX_TRY(build_sorted_cols(ctx, d_dst, d_src, nullptr, E, V, false, 0, 0, g->out_col,
                              E));
    MGX_TRY(mgx_build_bins(ctx, g->out_row_ptr, V, &g->bins_out));
  }

  if (flags & MGX_BUILD_SYM_CSR) {
    MGX_HIP_TRY(hipMemsetAsync(counts, 0, V * sizeof(uint32_t), ctx->stream));
    hipLaunchKernelGGL(k_hist2, dim3(grid_for(E)), dim3(kBlock), 0, ctx->stream, E, d_src,
                       d_dst, counts);
    MGX_HIP_TRY(mgx_hip_malloc(&g->sym_row_ptr, (V + 1) * sizeof(uint32_t)));
    MGX_TRY(scan_counts(ctx, counts, V, g->sym_row_ptr));
    MGX_HIP_TRY(mgx_hip_malloc(&g->sym_col, (E > 0 ? 2 * E : 1) * sizeof(int32_t)));
    if (flags & MGX_BUILD_WEIGHTED) {
      MGX_HIP_TRY(mgx_hip_malloc(&g->sym_w, (E > 0 ? 2 * E : 1) * sizeof(float)));
    }
    MGX_TRY(build_sorted_sym(ctx, d_src, d_dst, d_w, E, V, g->sym_col, g->sym_w));
    MGX_TRY(mgx_build_bins(ctx, g->sym_row_ptr, V, &g->bins_sym));
  }

  bufs.release(counts);
  MGX_HIP_TRY(hipEventRecord(ev1, ctx->stream));
  MGX_HIP_TRY(hipEventSynchronize(ev1));
  float ms = 0.f;
  MGX_HIP_TRY(hipEventElapsedTime(&ms, ev0, ev1));
  g->build_ms = ms;
  MGX_HIP_TRY(hipEventDestroy(ev0));
  MGX_HIP_TRY(hipEventDestroy(ev1));
  MGX_HIP_TRY(hipGetLastError());
  return MGX_OK;
}

mgx_status mgx_build_sharded_in_csr(mgx_context *ctx, const int32_t *d_src,
                                    const int32_t *d_dst, int64_t n_vertices,
                                    int64_t n_edges, int64_t row_begin, int64_t row_end,
                                    mgx_graph *g) {
  const int64_t V = n_vertices, E = n_edges;
  const int64_t rows = row_end - row_begin;
  g->n_vertices = V;
  g->n_edges = E;
  g->flags = MGX_BUILD_IN_CSR;
  g->row_begin = row_begin;
  g->row_end = row_end;

  hipEvent_t ev0, ev1;
  MGX_HIP_TRY(hipEventCreate(&ev0));
  MGX_HIP_TRY(hipEventCreate(&ev1));
  MGX_HIP_TRY(hipEventRecord(ev0, ctx->stream));

  // Global out-degree (contrib denominators need every source).
  MGX_HIP_TRY(mgx_hip_malloc(&g->out_degree, V * sizeof(uint32_t)));
  MGX_HIP_TRY(hipMemsetAsync(g->out_degree, 0, V * sizeof(uint32_t), ctx->stream));
  hipLaunchKernelGGL(k_hist, dim3(grid_for(E)), dim3(kBlock), 0, ctx->stream, E, d_src,
                     g->out_degree);
  MGX_HIP_TRY(mgx_hip_malloc(&g->inv_outdeg, V * sizeof(float)));
  hipLaunchKernelGGL(k_inv_outdeg, dim3(grid_for(V)), dim3(kBlock), 0, ctx->stream, V,
                     g->out_degree, g->inv_outdeg);

  mgx_scope bufs(ctx);
  uint32_t *counts = nullptr;
  MGX_TRY(bufs.alloc_plain(&counts, rows));
  MGX_HIP_TRY(hipMemsetAsync(counts, 0, rows * sizeof(uint32_t), ctx->stream));
  hipLaunchKernelGGL(k_hist_ranged, dim3(grid_for(E)), dim3(kBlock), 0, ctx->stream, E,
                     d_dst, (int32_t)row_begin, (int32_t)row_end, counts);
  MGX_HIP_TRY(mgx_hip_malloc(&g->in_row_ptr, (rows + 1) * sizeof(uint32_t)));
  MGX_TRY(scan_counts(ctx, counts, rows, g->in_row_ptr));
  uint32_t local_edges = 0;
  MGX_HIP_TRY(hipMemcpyAsync(&local_edges, g->in_row_ptr + rows, 4, hipMemcpyDeviceToHost,
                             ctx->stream));
  MGX_HIP_TRY(hipStreamSynchronize(ctx->stream));
  g->in_edges = local_edges;
  MGX_HIP_TRY(mgx_hip_malloc(&g->in_col, (local_edges > 0 ? local_edges : 1) * sizeof(int32_t)));
  MGX_TRY(build_sorted_cols(ctx, d_src, d_dst, nullptr, E, rows, true, (int32_t)row_begin,
                            (int32_t)row_end, g->in_col, local_edges));
  MGX_TRY(mgx_build_bins(ctx, g->in_row_ptr, rows, &g->bins_in));
  MGX_TRY(mgx_build_stripes(ctx, g));
  bufs.release(counts);

  MGX_HIP_TRY(hipEventRecord(ev1, ctx->stream));
  MGX_HIP_TRY(hipEventSynchronize(ev1));
  float ms = 0.f;
  MGX_HIP_TRY(hipEventElapsedTime(&ms, ev0, ev1));
  g->build_ms = ms;
  MGX_HIP_TRY(hipEventDestroy(ev0));
  MGX_HIP_TRY(hipEventDestroy(ev1));
  MGX_HIP_TRY(hipGetLastError());
  return MGX_OK;
}

// Host COO (int64/double) upload helpers, used by mgx_graph_from_coo. The
// device COO belongs to the caller's scope `own`.
mgx_status mgx_upload_coo(mgx_scope &own, const int64_t *src, const int64_t *dst,
                          const double *weights, int64_t n_edges, int32_t **d_src,
                          int32_t **d_dst, float **d_w) {
  mgx_context *ctx = own.ctx;
  MGX_TRY(own.alloc_plain(d_src, n_edges));
  MGX_TRY(own.alloc_plain(d_dst, n_edges));
  *d_w = nullptr;
  if (weights) MGX_TRY(own.alloc_plain(d_w, n_edges));

  // Chunked staging: int64 -> int32 converted on device.
  const int64_t chunk = 16 << 20;
  mgx_scope stage(ctx);
  int64_t *stage64 = nullptr;
  double *stagef = nullptr;
  const int64_t this_chunk = n_edges < chunk ? n_edges : chunk;
  if (this_chunk > 0) {
    MGX_TRY(stage.alloc_plain(&stage64, this_chunk));
    if (weights) MGX_TRY(stage.alloc_plain(&stagef, this_chunk));
  }
  for (int64_t off = 0; off < n_edges; off += chunk) {
    const int64_t n = (n_edges - off) < chunk ? (n_edges - off) : chunk;
    MGX_HIP_TRY(hipMemcpyAsync(stage64, src + off, n * sizeof(int64_t),
                               hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_i64_to_i32, dim3(grid_for(n)), dim3(kBlock), 0, ctx->stream, n,
                       stage64, *d_src + off);
    MGX_HIP_TRY(hipMemcpyAsync(stage64, dst + off, n * sizeof(int64_t),
                               hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_i64_to_i32, dim3(grid_for(n)), dim3(kBlock), 0, ctx->stream, n,
                       stage64, *d_dst + off);
    if (weights) {
      MGX_HIP_TRY(hipMemcpyAsync(stagef, weights + off, n * sizeof(double),
                                 hipMemcpyHostToDevice, ctx->stream));
      hipLaunchKernelGGL(k_f64_to_f32, dim3(grid_for(n)), dim3(kBlock), 0, ctx->stream, n,
                         stagef, *d_w + off);
    }
    // The next chunk reuses the staging buffer: wait for queued copies.
    MGX_HIP_TRY(hipStreamSynchronize(ctx->stream));
  }
  return MGX_OK;
}

// Test support: device-generate an edge list and download it (int64), so
// tests can check bit-identity with the numpy/C generators.
extern "C" mgx_status mgx_gen_edges_to_host(mgx_context *ctx, int rmat, int scale,
                                            int64_t n_vertices, int64_t n_edges,
                                            uint64_t seed, double a, double b, double c,
                                            int64_t *out_src, int64_t *out_dst) {
  MGX_HIP_TRY(hipSetDevice(ctx->device));
  mgx_scope bufs(ctx);
  int32_t *d_src = nullptr, *d_dst = nullptr;
  int64_t *d_wide = nullptr;
  MGX_TRY(bufs.alloc_plain(&d_src, n_edges));
  MGX_TRY(bufs.alloc_plain(&d_dst, n_edges));
  MGX_TRY(bufs.alloc_plain(&d_wide, n_edges));
  mgx_status s;
  if (rmat) {
    s = mgx_gen_rmat_device(ctx, scale, n_edges, seed, a, b, c, d_src, d_dst);
  } else {
    s = mgx_gen_uniform_device(ctx, n_vertices, n_edges, seed, d_src, d_dst);
  }
  if (s == MGX_OK) {
    hipLaunchKernelGGL((mgx_k_widen<int32_t, int64_t>), dim3(grid_for(n_edges)), dim3(kBlock),
                       0, ctx->stream, n_edges,d_src, d_wide);
    (void)hipMemcpyAsync(out_src, d_wide, n_edges * sizeof(int64_t), hipMemcpyDeviceToHost,
                         ctx->stream);
    (void)hipStreamSynchronize(ctx->stream);
    hipLaunchKernelGGL((mgx_k_widen<int32_t, int64_t>), dim3(grid_for(n_edges)), dim3(kBlock),
                       0, ctx->stream, n_edges,d_dst, d_wide);
    (void)hipMemcpyAsync(out_dst, d_wide, n_edges * sizeof(int64_t), hipMemcpyDeviceToHost,
                         ctx->stream);
    (void)hipStreamSynchronize(ctx->stream);
  }
  return s;
}
