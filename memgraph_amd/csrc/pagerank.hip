// PageRank on gfx950 — replaces pagerank_alg::ParallelIterativePageRank
// (reference algorithm/pagerank.cpp:194-242) with a fused pull-SpMV sweep:
//
//   new_rank[v] = (1-d)/N + d * sum_{u->v} contrib[u],  contrib[u] = rank[u]/outdeg(u)
//
// One kernel launch per iteration covers all degree bins (sub-wave work
// assignment per mgx_bins): f32 ranks/contrib in HBM, f64 accumulation in
// registers, and the same kernel writes new_rank AND new_contrib and folds
// the per-block Linf(delta) into a device scalar — so per-iteration traffic
// is the algorithmic 8 B/edge + ~20 B/vertex (DESIGN.md roofline).
//
// Large permuted graphs take the XCD-affine layout instead (mgx_graph::xcd,
// DESIGN.md "Memory layout levers" item 4): the heavy rows in one launch
// whose blocks each gather from one eighth of contrib, the light rows in the
// fused kernel above, and a finish kernel over the heavy rows. The striped
// launch keeps the hottest sources of its stripe in LDS (lever 5) and reads
// its column ids from a stripe-major copy of the heavy rows' columns (lever
// 6). From a run's third sweep on, the rows of in-degree 0 are left out: both
// ping-pong buffers already hold their values.
//
// Parity bar (tests/test_gpu_pagerank.py): |r_gpu - r_cpu|inf <= 1e-6 vs the
// fp64 oracle after equal iterations, post sum-normalize.

#include <chrono>

#include "mgx_device.h"
#include "mgx_xcd_deal.h"

namespace {

struct PrArgs {
  const uint32_t *row_ptr;
  const int32_t *col;
  mgx_bin_sections bins;
  const float *contrib_old;
  const float *rank_old;
  float *rank_new;
  float *contrib_new;
  const float *inv_outdeg;  // global vertex id
  int64_t row_base;         // sharded: global row = row_base + local row
  float base_term;          // (1-d)/N
  float damping;
  uint32_t *delta_max;      // f32-as-ordered-uint
  // Source-striped sweep (large V): per-stripe row sub-ranges
  // and fp64 row partials. mode: 0 = direct (single launch),
  // 1 = first stripe (partial = acc), 2 = middle (partial += acc),
  // 3 = last stripe (finish from partial + acc).
  const uint32_t *sp_lo;
  const uint32_t *sp_hi;
  double *partial;
  int mode;
};

// How a sweep reads contrib[c]. The plain global gather: the fused sweep and
// the striped launch without an LDS table.
struct PrLoadGlobal {
  static constexpr bool kFlat = false;
  const float *contrib;
  __device__ float operator()(int32_t c) const { return contrib[c]; }
};

// The striped launch with its stripe's hot prefix in LDS (DESIGN.md lever 5):
// hot[0 .. kx) holds contrib[base .. base + kx), the same bits, so a gather
// served from it adds the same value. The select of the two addresses
// compiles to one flat load per gather, no branch.
struct PrLoadHot {
  static constexpr bool kFlat = true;
  const float *contrib;
  const float *hot;
  uint32_t base, kx;
  __device__ float operator()(int32_t c) const {
    const uint32_t r = (uint32_t)c - base;
    return r < kx ? hot[r] : contrib[c];
  }
};

// This lane's share of sum_{u->row} contrib[u] over the row's stripe range;
// load(c) reads contrib[c].
template <int LANES, typename Load>
__device__ inline double pr_row_sum(const PrArgs &A, int32_t row, int sub, Load load) {
  double acc = 0.0;
  const uint32_t s = A.sp_lo[row], e = A.sp_hi[row];
  if constexpr (LANES >= 64) {
    // Wide rows: scalar head to 16-B alignment, then int4 nontemporal
    // column loads (the col stream is read exactly once — keep it out
    // of L1 so the contrib gathers stay cached; G13/nt-weights) with 4
    // independent gathers per lane per iteration for latency hiding.
    uint32_t s_al = (s + 3u) & ~3u;
    if (s_al > e) s_al = e;
    for (uint32_t j = s + sub; j < s_al; j += LANES)
      acc += (double)load(A.col[j]);
    const uint32_t nvec = (e - s_al) / 4;
    typedef int v4i __attribute__((ext_vector_type(4)));
    const v4i *col4 = reinterpret_cast<const v4i *>(A.col + s_al);
    uint32_t c = sub;
    // 2x unrolled: 8 independent gathers in flight per lane.
    for (; c + LANES < nvec; c += 2 * LANES) {
      v4i c0 = __builtin_nontemporal_load(col4 + c);
      v4i c1 = __builtin_nontemporal_load(col4 + c + LANES);
      if constexpr (Load::kFlat) {
        // Flat loads return out of order, so once one is pending the wait
        // for c1 becomes vmcnt(0) and drains the gathers issued before it,
        // four in flight instead of eight. Have both column vectors arrive
        // before the first gather.
        asm volatile("" : "+v"(c0.x), "+v"(c0.y), "+v"(c0.z), "+v"(c0.w), "+v"(c1.x),
                     "+v"(c1.y), "+v"(c1.z), "+v"(c1.w));
      }
      const float g0 = load(c0.x);
      const float g1 = load(c0.y);
      const float g2 = load(c0.z);
      const float g3 = load(c0.w);
      const float g4 = load(c1.x);
      const float g5 = load(c1.y);
      const float g6 = load(c1.z);
      const float g7 = load(c1.w);
      acc += (double)g0;
      acc += (double)g1;
      acc += (double)g2;
      acc += (double)g3;
      acc += (double)g4;
      acc += (double)g5;
      acc += (double)g6;
      acc += (double)g7;
    }
    for (; c < nvec; c += LANES) {
      const v4i cc = __builtin_nontemporal_load(col4 + c);
      acc += (double)load(cc.x);
      acc += (double)load(cc.y);
      acc += (double)load(cc.z);
      acc += (double)load(cc.w);
    }
    for (uint32_t j = s_al + nvec * 4 + sub; j < e; j += LANES)
      acc += (double)load(A.col[j]);
  } else {
    // Short rows: a LANES-wide group reads consecutive cols (16/64-B
    // granules); nt keeps the one-pass col stream out of L1.
    row_gather<LANES>(A.col, s, e, sub,
                      [&](int32_t c) { acc += (double)load(c); });
  }
  return acc;
}

// Row epilogue from the row's fp64 gather sum: new rank, new contrib, and
// this thread's running Linf(new - old) when that is tracked.
__device__ inline void pr_finish_row(const PrArgs &A, int32_t row, double acc, float &maxd) {
  const float newr = (float)((double)A.base_term + (double)A.damping * acc);
  const int64_t gv = A.row_base + row;
  A.rank_new[gv] = newr;
  A.contrib_new[gv] = newr * A.inv_outdeg[gv];
  if (A.delta_max) {  // old-rank read only paid when Linf is tracked
    const float d = fabsf(newr - A.rank_old[gv]);
    if (d > maxd) maxd = d;
  }
}

// Block max of the per-thread Linf -> one atomic per block (guide G12).
__device__ inline void pr_fold_delta(const PrArgs &A, float maxd) {
  block_reduce_atomic(
      maxd, 0.0f, [](float a, float b) { return fmaxf(a, b); },
      [&](float m) { atomicMax(A.delta_max, __float_as_uint(m)); });
}

template <int LANES>
__device__ inline float pr_rows(const PrArgs &A, int sec, int64_t block_in_sec) {
  float maxd = 0.0f;
  reduce_bin_rows<LANES>(
      A.bins, sec, block_in_sec, 0.0, mgx_op_add(),
      [&](int32_t row, int sub) {
        return pr_row_sum<LANES>(A, row, sub, PrLoadGlobal{A.contrib_old});
      },
      [&](int32_t row, double acc) {
        if (A.mode == 1) {
          A.partial[row] = acc;
        } else if (A.mode == 2) {
          A.partial[row] += acc;
        } else {
          if (A.mode == 3) acc += A.partial[row];
          pr_finish_row(A, row, acc, maxd);
        }
      });
  return maxd;
}

__global__ void __launch_bounds__(kBlock) k_pr_sweep(PrArgs A) {
  float maxd = 0.0f;
  for_bin_section(A.bins.goff, [&](auto lanes, int sec, int64_t bis) {
    maxd = pr_rows<decltype(lanes)::value>(A, sec, bis);
  });
  if (A.delta_max) pr_fold_delta(A, maxd);
}

// XCD-striped sweep over the heavy rows (mgx_graph::xcd). Block b gathers
// only from source stripe b & 7 and acts as block b >> 3 of that stripe
// (rows are slots here), so the blocks that share an XCD — b and b + 8 under
// the observed round-robin dispatch — share one eighth of contrib and the
// eight L2s hold eight different slices. The grid is resident at once and
// each block strides over the rows of the stripe's four bin sections in turn,
// the 256-lane section (the longest segments) first, so that placement does
// not depend on redispatch order. A block of THREADS threads takes
// THREADS / LANES segments per step; a segment's lanes, their share of the
// columns and the order of its additions are those of a 256-thread block, so
// every width gives the same bits. Each segment's fp64 sum goes to
// partial[x * nH + slot]; k_pr_finish_heavy combines them. No block reads
// what another wrote: a different placement changes the speed only.
struct PrXcdArgs {
  const int32_t *col;             // xcd_scol, or in_col where there is no stream
  const float *contrib_old;
  double *partial;                // [8 * nH], stripe-major
  const mgx_bin_sections *sec;    // [8] device: stripe x's sections over slots
  const uint32_t *lo, *hi;        // [8 * nH] each: segment (x, slot) is col[lo .. hi)
  int64_t nH;
  int64_t V;
  uint32_t hot_k;                 // HOT: floats of dynamic LDS per block
};

// HOT: the block first copies the hottest min(hot_k, stripe length) sources of
// its stripe, contrib_old[off[x] ..), into LDS and gathers those from there.
// The stripe is hot-first inside, so that prefix takes the largest share of
// the gathers a table of this size can; contrib_old is read-only for the
// whole launch. Every gathered value has the same bits either way.
// With one section's loop live at a time every instantiation stays below 64
// VGPRs (8 waves per SIMD) without a bound on the registers.
template <bool HOT, int THREADS>
__global__ void __launch_bounds__(THREADS) k_pr_sweep_xcd(PrXcdArgs X) {
  const int x = blockIdx.x % kXcdStripes;
  const mgx_bin_sections &S = X.sec[x];
  PrArgs A;  // only what pr_row_sum reads
  A.col = X.col;
  A.sp_lo = X.lo + (size_t)x * X.nH;
  A.sp_hi = X.hi + (size_t)x * X.nH;
  double *out = X.partial + (size_t)x * X.nH;
  const int64_t block = blockIdx.x / kXcdStripes;
  const int64_t nblocks = gridDim.x / kXcdStripes;
  auto sweep = [&](auto load) {
    // Every thread takes every step of the 256-lane section (reduce_rows
    // counts them per block, not per team), so its barriers are block-wide.
    auto section = [&](auto lanes, int sec) {
      constexpr int L = decltype(lanes)::value;
      reduce_rows<L, THREADS>(
          S.rows + S.off[sec], S.n[sec], block, nblocks, 0.0, mgx_op_add(),
          [&](int32_t slot, int sub) { return pr_row_sum<L>(A, slot, sub, load); },
          [&](int32_t slot, double acc) { out[slot] = acc; });
    };
    section(std::integral_constant<int, 256>{}, 3);
    section(std::integral_constant<int, 64>{}, 2);
    section(std::integral_constant<int, 16>{}, 1);
    section(std::integral_constant<int, 4>{}, 0);
  };
  if constexpr (HOT) {
    extern __shared__ float hot[];
    const int64_t base = mgx_xcd_stripe_off(X.V, x);
    const int64_t len = mgx_xcd_stripe_off(X.V, x + 1) - base;
    const uint32_t kx = len < (int64_t)X.hot_k ? (uint32_t)len : X.hot_k;
    for (uint32_t i = threadIdx.x; i < kx; i += THREADS) hot[i] = X.contrib_old[base + i];
    __syncthreads();
    sweep(PrLoadHot{X.contrib_old, hot, (uint32_t)base, kx});
  } else {
    sweep(PrLoadGlobal{X.contrib_old});
  }
}

// The instantiation for a block width (MGX_PR_XCD_BLOCK), nullptr for a width
// that is not built. Two blocks of 1024 threads fill a CU's 32 wave slots and
// share its LDS in halves, a table four times that of eight 256-thread blocks;
// 512, 768 and 896 threads measured between the two
// (profiles/lds_wide_blocks.md) and are not built.
using pr_xcd_kernel = void (*)(PrXcdArgs);
constexpr int kXcdDefaultWidth = 1024;

pr_xcd_kernel pr_xcd_kernel_for(bool hot, int threads) {
  switch (threads) {
    case 256: return hot ? k_pr_sweep_xcd<true, 256> : k_pr_sweep_xcd<false, 256>;
    case 1024: return hot ? k_pr_sweep_xcd<true, 1024> : k_pr_sweep_xcd<false, 1024>;
    default: return nullptr;
  }
}

// Heavy rows: sum the 8 stripe partials in stripe order and finish the row.
// A stripe whose segment is empty (equal boundaries) wrote no partial and is
// skipped, so no stale slot is read.
__global__ void __launch_bounds__(kBlock)
k_pr_finish_heavy(PrArgs A, const int32_t *H, const uint32_t *xptr, int64_t nH) {
  float maxd = 0.0f;
  for (int64_t s = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; s < nH;
       s += (int64_t)gridDim.x * blockDim.x) {
    double acc = 0.0;
    uint32_t lo = xptr[s];
    for (int x = 0; x < kXcdStripes; ++x) {
      const uint32_t hi = xptr[(size_t)(x + 1) * nH + s];
      if (hi > lo) acc += A.partial[(size_t)x * nH + s];
      lo = hi;
    }
    pr_finish_row(A, H[s], acc, maxd);
  }
  if (A.delta_max) pr_fold_delta(A, maxd);
}

__global__ void k_pr_init(int64_t n, float r0, const float *inv, float *rank,
                          float *contrib) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    rank[i] = r0;
    contrib[i] = r0 * inv[i];
  }
}

__global__ void k_sum_f32(int64_t n, const float *x, double *out) {
  double acc = 0.0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    acc += (double)x[i];
  block_reduce_atomic(acc, 0.0, mgx_op_add(), [&](double s) { atomicAdd(out, s); });
}

__global__ void k_pr_widen(int64_t n, const float *rank, const double *sum,
                           const int32_t *order, double *out) {
  // order: permuted -> original vertex id (hot-first layout); identity when
  // null. Scatter on device so the D2H stays one contiguous copy.
  const double inv = 1.0 / *sum;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    out[order ? order[i] : i] = (double)rank[i] * inv;
}

// The launch sections of `bins` for this sweep of the run; returns the total
// grid. From the third sweep on, a row of in-degree 0 would be given the
// values it already holds in both ping-pong buffers (rank base_term, contrib
// base_term * inv_outdeg, Linf contribution 0), so bin0 then starts past
// those rows and its grid is sized for the rest.
int64_t pr_fill_sections(const mgx_pagerank_run *run, const mgx_bins &bins,
                         mgx_bin_sections *s) {
  const int64_t nz = bins.n_zero;
  if (!run->skip_zero || run->dist || run->iterations < 2 || nz == 0)
    return mgx_fill_sections(bins, s);
  mgx_bins rest = bins;
  rest.count[0] -= nz;
  rest.grid[0] = mgx_bin_grid(0, rest.count[0]);
  const int64_t goff = mgx_fill_sections(rest, s);
  for (int b = 0; b < 4; ++b) s->off[b] += nz;
  return goff;
}

// One sweep of the XCD-affine layout: the heavy rows' striped launch into the
// partials, the plain sweep over the light rows (the bins_in sections below
// the heavy ones), then the heavy rows' finish.
mgx_status queue_xcd_sweep(mgx_pagerank_run *run, PrArgs A) {
  mgx_context *ctx = run->ctx;
  mgx_graph *g = run->g;
  const int64_t nH = g->xcd_nH;
  if (nH > 0) {
    PrXcdArgs X;
    // The stripe-major column stream where the build made one (lever 6): the
    // same ids at the same offsets mod 4, so the same additions in the same
    // order. Otherwise the segments of in_col between the stripe boundaries.
    if (g->xcd_scol) {
      X.col = g->xcd_scol;
      X.lo = g->xcd_slo;
      X.hi = g->xcd_shi;
    } else {
      X.col = g->in_col;
      X.lo = g->xcd_ptr;
      X.hi = g->xcd_ptr + nH;
    }
    X.contrib_old = A.contrib_old;
    X.partial = run->d_partial;
    X.sec = g->xcd_sec;
    X.nH = nH;
    X.V = g->n_vertices;
    X.hot_k = (uint32_t)run->xcd_lds_floats;
    hipLaunchKernelGGL(pr_xcd_kernel_for(X.hot_k > 0, run->xcd_block),
                       dim3((uint32_t)run->xcd_grid), dim3((uint32_t)run->xcd_block),
                       (size_t)X.hot_k * sizeof(float), ctx->stream, X);
  }
  mgx_bins light = g->bins_in;
  for (int b = g->xcd_heavy_sec; b < 4; ++b) light.count[b] = light.grid[b] = 0;
  const int64_t goff = pr_fill_sections(run, light, &A.bins);
  A.sp_lo = g->in_row_ptr;
  A.sp_hi = g->in_row_ptr + 1;
  A.mode = 0;
  if (goff > 0) {
    hipLaunchKernelGGL(k_pr_sweep, dim3((uint32_t)goff), dim3(kBlock), 0, ctx->stream, A);
  }
  if (nH > 0) {
    hipLaunchKernelGGL(k_pr_finish_heavy, dim3((uint32_t)grid_for(nH)), dim3(kBlock), 0,
                       ctx->stream, A, g->xcd_H, (const uint32_t *)g->xcd_ptr, nH);
  }
  return MGX_OK;
}

mgx_status queue_one_iteration(mgx_pagerank_run *run, bool track_delta) {
  mgx_context *ctx = run->ctx;
  mgx_graph *g = run->g;
  const int64_t V = g->n_vertices;

  PrArgs A;
  A.row_ptr = g->in_row_ptr;
  A.col = g->in_col;
  A.contrib_old = run->contrib[run->cur];
  A.rank_old = run->rank[run->cur];
  A.rank_new = run->rank[1 - run->cur];
  A.contrib_new = run->contrib[1 - run->cur];
  A.inv_outdeg = g->inv_outdeg;
  A.row_base = g->row_begin;
  A.base_term = (float)((1.0 - run->damping) / (double)V);
  A.damping = (float)run->damping;
  A.delta_max = track_delta ? run->d_delta : nullptr;
  A.partial = run->d_partial;

  if (track_delta) MGX_HIP_TRY(hipMemsetAsync(run->d_delta, 0, 4, ctx->stream));

  const int n_stripes = g->n_stripes;
  // in-CSR row count (row_end may be re-padded for the allgather shard).
  const int64_t rows = (g->row_end < V ? g->row_end : V) - g->row_begin;
  if (V > 0) {
    // Event-bracket the whole per-iteration sweep group (1 launch when
    // unstriped, n_stripes launches when striped, heavy + light + finish in
    // the XCD-affine layout): feeds roofline.achieved.
    if (run->ev_used >= (int64_t)run->ev_start.size()) {
      hipEvent_t e0, e1;
      MGX_HIP_TRY(hipEventCreate(&e0));
      MGX_HIP_TRY(hipEventCreate(&e1));
      run->ev_start.push_back(e0);
      run->ev_stop.push_back(e1);
    }
    MGX_HIP_TRY(hipEventRecord(run->ev_start[run->ev_used], ctx->stream));
    if (g->xcd) {
      MGX_TRY(queue_xcd_sweep(run, A));
    } else {
      for (int sIdx = 0; sIdx < n_stripes; ++sIdx) {
        const mgx_bins &bins = n_stripes == 1 ? g->bins_in : g->stripe_bins[sIdx];
        // Only the single launch (mode 0) may leave the zero-degree rows out:
        // the sequential stripes finish every row from its partial.
        const int64_t goff = n_stripes == 1 ? pr_fill_sections(run, bins, &A.bins)
                                            : mgx_fill_sections(bins, &A.bins);
        if (n_stripes == 1) {
          A.sp_lo = g->in_row_ptr;
          A.sp_hi = g->in_row_ptr + 1;
          A.mode = 0;
        } else {
          A.sp_lo = g->stripe_ptr + (size_t)sIdx * rows;
          A.sp_hi = g->stripe_ptr + (size_t)(sIdx + 1) * rows;
          A.mode = sIdx == 0 ? 1 : (sIdx == n_stripes - 1 ? 3 : 2);
        }
        if (goff > 0) {
          hipLaunchKernelGGL(k_pr_sweep, dim3((uint32_t)goff), dim3(kBlock), 0, ctx->stream,
                             A);
        }
      }
    }
    MGX_HIP_TRY(hipEventRecord(run->ev_stop[run->ev_used], ctx->stream));
    ++run->ev_used;
    MGX_HIP_TRY(hipGetLastError());
  }

  // Distributed: every rank owns rows [row_begin,row_end); exchange the new
  // contrib slices so the next gather sees all sources (ncclAllGather over
  // xGMI). The rank vector itself is only needed at finish
  // (normalize) — gathered once there, halving the per-iteration volume.
  if (run->dist) {
    const int64_t shard = run->row_end - run->row_begin;  // equal on all ranks (padded)
    MGX_TRY(mgx_comm_allgather_f32(ctx, A.contrib_new + run->row_begin, A.contrib_new,
                                   (size_t)shard));
  }

  run->cur = 1 - run->cur;
  ++run->iterations;
  // Bounded event ring: fold timings once in a while.
  if (run->ev_used >= 1024) MGX_TRY(run->flush_timing());
  return MGX_OK;
}

}  // namespace

mgx_status mgx_pagerank_run::flush_timing() {
  if (ev_used == 0) return MGX_OK;
  MGX_HIP_TRY(hipStreamSynchronize(ctx->stream));
  for (int64_t i = 0; i < ev_used; ++i) {
    float ms = 0.f;
    MGX_HIP_TRY(hipEventElapsedTime(&ms, ev_start[i], ev_stop[i]));
    sweep_ms_acc += ms;
  }
  launches_acc += ev_used;
  ev_used = 0;
  return MGX_OK;
}

mgx_status mgx_pagerank_queue_iterations(mgx_pagerank_run *run, int64_t n, bool track_delta) {
  for (int64_t i = 0; i < n; ++i) MGX_TRY(queue_one_iteration(run, track_delta));
  return MGX_OK;
}

mgx_status mgx_pagerank_read_delta(mgx_pagerank_run *run, float *out) {
  if (run->dist && mgx_comm_world(run->ctx) > 1) {
    // The sweep's Linf is over OWNED rows only; ranks must agree on the
    // stopping decision or the next iteration's ncclAllGather deadlocks.
    // d_delta holds the f32 bits of a non-negative float (ordered-uint
    // atomicMax), so reinterpreting as float is exact; in-place max.
    MGX_TRY(mgx_comm_allreduce_max_f32(run->ctx, (const float *)run->d_delta,
                                       (float *)run->d_delta));
  }
  uint32_t bits = 0;
  MGX_HIP_TRY(hipMemcpyAsync(&bits, run->d_delta, 4, hipMemcpyDeviceToHost,
                             run->ctx->stream));
  MGX_HIP_TRY(hipStreamSynchronize(run->ctx->stream));
  union {
    uint32_t u;
    float f;
  } cv;
  cv.u = bits;
  *out = cv.f;
  return MGX_OK;
}

mgx_status mgx_pagerank_normalize_download(mgx_pagerank_run *run, double *out_rank) {
  mgx_context *ctx = run->ctx;
  const int64_t V = run->g->n_vertices;
  if (V == 0) return MGX_OK;
  if (run->dist && run->iterations > 0) {
    // Assemble the full rank vector once (deferred from the iterations).
    const int64_t shard = run->row_end - run->row_begin;
    MGX_TRY(mgx_comm_allgather_f32(ctx, run->rank[run->cur] + run->row_begin,
                                   run->rank[run->cur], (size_t)shard));
  }
  // NormalizeRank (reference pagerank.cpp:157-162): divide by the sum.
  MGX_HIP_TRY(hipMemsetAsync(run->d_scratch, 0, sizeof(double), ctx->stream));
  hipLaunchKernelGGL(k_sum_f32, dim3((uint32_t)grid_for(V)), dim3(kBlock), 0, ctx->stream,
                     V, run->rank[run->cur], run->d_scratch);
  hipLaunchKernelGGL(k_pr_widen, dim3((uint32_t)grid_for(V)), dim3(kBlock), 0, ctx->stream,
                     V, run->rank[run->cur], run->d_scratch, run->g->order,
                     run->d_scratch + 1);
  if (out_rank) {
    MGX_HIP_TRY(hipMemcpyAsync(out_rank, run->d_scratch + 1, V * sizeof(double),
                               hipMemcpyDeviceToHost, ctx->stream));
  }
  MGX_HIP_TRY(hipStreamSynchronize(ctx->stream));
  return MGX_OK;
}

namespace {

// Resident blocks per CU of the striped launch of `threads` per block with
// `floats` of dynamic LDS.
mgx_status xcd_blocks_per_cu(int threads, int64_t floats, int *per_cu) {
  MGX_HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(
      per_cu, pr_xcd_kernel_for(floats > 0, threads), threads, (size_t)floats * sizeof(float)));
  return MGX_OK;
}

// Block width of the striped launch, chosen per run: MGX_PR_XCD_BLOCK=<threads>
// forces it; a width without a kernel is an error.
mgx_status pick_xcd_block(int *threads) {
  *threads = kXcdDefaultWidth;
  const char *e = getenv("MGX_PR_XCD_BLOCK");
  if (e && *e) *threads = atoi(e);
  if (!pr_xcd_kernel_for(false, *threads)) {
    mgx_set_error("MGX_PR_XCD_BLOCK=%s: the striped sweep has no kernel of that width",
                  e ? e : "");
    return MGX_ERR_INVALID_ARGUMENT;
  }
  return MGX_OK;
}

// Floats of each stripe's hot prefix that the striped launch keeps in LDS
// (run->xcd_lds_floats), chosen per run once the width is. MGX_PR_XCD_LDS=
// <floats> forces it (0 = the launch without a table), clamped to the longest
// stripe and to what one block may allocate. Unset: the largest multiple of
// 256 floats that leaves the occupancy query's blocks per CU where they are
// with no dynamic LDS, 8 blocks of 256 threads or 2 of 1024; a larger table
// trades resident waves for LDS hits, which measured slower
// (profiles/lds_hot_prefix.md, profiles/lds_wide_blocks.md).
mgx_status pick_xcd_lds(mgx_pagerank_run *run) {
  const int64_t V = run->g->n_vertices;
  const int threads = run->xcd_block;
  int64_t longest = 0;
  for (int x = 0; x < kXcdStripes; ++x) {
    const int64_t len = mgx_xcd_stripe_off(V, x + 1) - mgx_xcd_stripe_off(V, x);
    if (len > longest) longest = len;
  }
  const void *hot_fn = reinterpret_cast<const void *>(pr_xcd_kernel_for(true, threads));
  hipFuncAttributes fa;
  MGX_HIP_TRY(hipFuncGetAttributes(&fa, hot_fn));
  int block_lds = 0;
  MGX_HIP_TRY(hipDeviceGetAttribute(&block_lds, hipDeviceAttributeMaxSharedMemoryPerBlock,
                                    run->ctx->device));
  const int64_t most = ((int64_t)block_lds - (int64_t)fa.sharedSizeBytes) / (int64_t)sizeof(float);
  if (most > 0) {
    // A table of more than 64 KiB is within the device's limit (one block may
    // hold a CU's whole LDS), but the kernel has to be told.
    MGX_HIP_TRY(hipFuncSetAttribute(hot_fn, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)(most * (int64_t)sizeof(float))));
  }
  int64_t k = 0;
  const char *e = getenv("MGX_PR_XCD_LDS");
  if (e && *e) {
    k = atoll(e);
    if (k < 0) k = 0;
  } else {
    constexpr int64_t kStep = 256;
    int want_blocks = 0;
    MGX_TRY(xcd_blocks_per_cu(threads, 0, &want_blocks));
    int64_t lo = 0, hi = most / kStep;  // steps: lo keeps the occupancy, above hi does not fit
    while (lo < hi) {
      const int64_t mid = (lo + hi + 1) / 2;
      int blocks = 0;
      MGX_TRY(xcd_blocks_per_cu(threads, mid * kStep, &blocks));
      if (blocks >= want_blocks) lo = mid;
      else hi = mid - 1;
    }
    k = lo * kStep;
  }
  if (k > longest) k = longest;
  if (k > most) k = most;
  if (k < 0) k = 0;
  run->xcd_lds_floats = k;
  return MGX_OK;
}

mgx_status pagerank_start_common(mgx_context *ctx, mgx_graph *g, double damping,
                                 bool dist, int64_t row_begin, int64_t row_end,
                                 mgx_pagerank_run **out) {
  if (!ctx || !g || !(g->flags & MGX_BUILD_IN_CSR)) {
    mgx_set_error("pagerank needs a graph built with MGX_BUILD_IN_CSR");
    return MGX_ERR_INVALID_ARGUMENT;
  }
  const bool striped = g->xcd && g->xcd_nH > 0;
  int xcd_block = 0;
  if (striped) MGX_TRY(pick_xcd_block(&xcd_block));  // before anything is allocated
  auto *run = new mgx_pagerank_run();
  run->ctx = ctx;
  run->g = g;
  run->damping = damping;
  run->xcd_block = xcd_block;
  run->dist = dist;
  run->row_begin = row_begin;
  run->row_end = row_end;
  if (const char *e = getenv("MGX_PR_SKIP_ZERO")) run->skip_zero = !(*e && atoi(e) == 0);
  const int64_t V = g->n_vertices;
  // Distributed rank/contrib arrays are padded to world*shard.
  const int64_t alloc = dist ? (row_end - row_begin) * (int64_t)mgx_comm_world(ctx) : V;
  const int64_t n = (alloc > V ? alloc : V);
  for (int i = 0; i < 2; ++i) {
    MGX_TRY(ctx->alloc_async((void **)&run->rank[i], n * sizeof(float)));
    MGX_TRY(ctx->alloc_async((void **)&run->contrib[i], n * sizeof(float)));
  }
  MGX_TRY(ctx->alloc_async((void **)&run->d_delta, sizeof(uint32_t)));
  MGX_TRY(ctx->alloc_async((void **)&run->d_scratch, (V + 1) * sizeof(double)));
  if (g->n_stripes > 1) {
    const int64_t rows = (dist ? (row_end < V ? row_end : V) : V) - row_begin;
    MGX_TRY(ctx->alloc_async((void **)&run->d_partial, rows * sizeof(double)));
  }
  if (striped) {
    MGX_TRY(ctx->alloc_async((void **)&run->d_partial,
                             (size_t)kXcdStripes * g->xcd_nH * sizeof(double)));
    MGX_TRY(pick_xcd_lds(run));
    // A grid that is resident at once (occupancy x CUs, a multiple of 8), no
    // larger than the busiest section of the busiest stripe can use: a block
    // takes xcd_block / lanes rows of a section per step.
    int per_cu = 0, cus = 0;
    MGX_TRY(xcd_blocks_per_cu(run->xcd_block, run->xcd_lds_floats, &per_cu));
    MGX_HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device));
    int64_t want = 0;
    for (int x = 0; x < kXcdStripes; ++x) {
      const int lanes[4] = {4, 16, 64, 256};
      for (int b = 0; b < 4; ++b) {
        const int64_t rows_per_block = run->xcd_block / lanes[b];
        const int64_t need = (g->xcd_bins[x].count[b] + rows_per_block - 1) / rows_per_block;
        if (need > want) want = need;
      }
    }
    int64_t per_stripe = (int64_t)per_cu * cus / kXcdStripes;
    if (per_stripe > want) per_stripe = want;
    if (per_stripe < 1) per_stripe = 1;
    run->xcd_grid = (int)(per_stripe * kXcdStripes);
  }
  if (V > 0) {
    const float r0 = (float)(1.0 / (double)V);
    hipLaunchKernelGGL(k_pr_init, dim3((uint32_t)grid_for(V)), dim3(kBlock), 0, ctx->stream,
                       V, r0, g->inv_outdeg, run->rank[0], run->contrib[0]);
    MGX_HIP_TRY(hipGetLastError());
  }
  *out = run;
  return MGX_OK;
}

void pagerank_run_free(mgx_pagerank_run *run) {
  for (int i = 0; i < 2; ++i) {
    if (run->rank[i]) (void)run->ctx->free_async(run->rank[i]);
    if (run->contrib[i]) (void)run->ctx->free_async(run->contrib[i]);
  }
  if (run->d_delta) (void)run->ctx->free_async(run->d_delta);
  if (run->d_scratch) (void)run->ctx->free_async(run->d_scratch);
  if (run->d_partial) (void)run->ctx->free_async(run->d_partial);
  for (auto e : run->ev_start) (void)hipEventDestroy(e);
  for (auto e : run->ev_stop) (void)hipEventDestroy(e);
  delete run;
}

}  // namespace

extern "C" mgx_status mgx_pagerank_start(mgx_context *ctx, mgx_graph *g, double damping,
                                         mgx_pagerank_run **out) {
  return pagerank_start_common(ctx, g, damping, false, 0, g ? g->n_vertices : 0, out);
}

extern "C" mgx_status mgx_pagerank_start_dist(mgx_context *ctx, mgx_graph *g, double damping,
                                              int64_t row_begin, int64_t row_end,
                                              mgx_pagerank_run **out) {
  if (mgx_comm_world(ctx) == 0) {
    mgx_set_error("mgx_comm_init must be called before mgx_pagerank_start_dist");
    return MGX_ERR_INVALID_ARGUMENT;
  }
  return pagerank_start_common(ctx, g, damping, true, row_begin, row_end, out);
}

extern "C" mgx_status mgx_pagerank_iterate(mgx_pagerank_run *run, int64_t n) {
  return mgx_pagerank_queue_iterations(run, n, /*track_delta=*/false);
}

extern "C" mgx_status mgx_pagerank_iterate_eps(mgx_pagerank_run *run, int64_t max_n,
                                               double stop_epsilon, int64_t *done) {
  int64_t i = 0;
  for (; i < max_n; ++i) {
    MGX_TRY(mgx_pagerank_queue_iterations(run, 1, /*track_delta=*/true));
    float delta = 0.f;
    MGX_TRY(mgx_pagerank_read_delta(run, &delta));  // dist: max-allreduced
    if (delta <= (float)stop_epsilon) {
      ++i;
      break;
    }
  }
  if (done) *done = i;
  return MGX_OK;
}

extern "C" int64_t mgx_pagerank_xcd_lds_floats(const mgx_pagerank_run *run) {
  return run->xcd_lds_floats;
}

extern "C" int mgx_pagerank_xcd_block_threads(const mgx_pagerank_run *run) {
  return run->xcd_block;
}

extern "C" mgx_status mgx_pagerank_timing(mgx_pagerank_run *run, double *sweep_ms,
                                          int64_t *launches) {
  MGX_TRY(run->flush_timing());
  if (sweep_ms) *sweep_ms = run->sweep_ms_acc;
  if (launches) *launches = run->launches_acc;
  return MGX_OK;
}

extern "C" mgx_status mgx_pagerank_finish(mgx_pagerank_run *run, double *out_rank) {
  mgx_status s = mgx_pagerank_normalize_download(run, out_rank);
  if (s == MGX_OK) s = run->flush_timing();
  pagerank_run_free(run);
  return s;
}

extern "C" mgx_status mgx_pagerank(mgx_context *ctx, mgx_graph *g, int64_t max_iterations,
                                   double damping, double stop_epsilon, double *out_rank,
                                   mgx_pagerank_stats *stats) {
  mgx_pagerank_run *run = nullptr;
  MGX_TRY(mgx_pagerank_start(ctx, g, damping, &run));
  hipEvent_t it0, it1;
  MGX_HIP_TRY(hipEventCreate(&it0));
  MGX_HIP_TRY(hipEventCreate(&it1));
  MGX_HIP_TRY(hipEventRecord(it0, ctx->stream));

  mgx_status s = MGX_OK;
  if (stop_epsilon > 0.0) {
    // Reference stopping rule (pagerank.cpp:139-151): after each iteration,
    // stop when Linf(new-old) <= eps or the cap is reached.
    for (int64_t i = 0; i < max_iterations && s == MGX_OK; ++i) {
      s = mgx_pagerank_queue_iterations(run, 1, /*track_delta=*/true);
      if (s != MGX_OK) break;
      float delta = 0.f;
      s = mgx_pagerank_read_delta(run, &delta);
      if (delta <= (float)stop_epsilon) break;
    }
  } else {
    s = mgx_pagerank_queue_iterations(run, max_iterations, false);
  }

  MGX_HIP_TRY(hipEventRecord(it1, ctx->stream));

  double download_ms = 0.0;
  if (s == MGX_OK) {
    MGX_HIP_TRY(hipEventSynchronize(it1));
    const auto t0 = std::chrono::steady_clock::now();
    s = mgx_pagerank_normalize_download(run, out_rank);
    const auto t1 = std::chrono::steady_clock::now();
    download_ms = std::chrono::duration<double, std::milli>(t1 - t0).count();
  }

  if (stats && s == MGX_OK) {
    float iter_ms = 0.f;
    MGX_HIP_TRY(hipEventElapsedTime(&iter_ms, it0, it1));
    (void)run->flush_timing();
    stats->iterations = run->iterations;
    stats->iter_ms = iter_ms;
    stats->sweep_ms = run->sweep_ms_acc;
    stats->sweep_launches = run->launches_acc;
    stats->csr_build_ms = g->build_ms;
    stats->download_ms = download_ms;
  }
  MGX_HIP_TRY(hipEventDestroy(it0));
  MGX_HIP_TRY(hipEventDestroy(it1));
  pagerank_run_free(run);
  return s;
}
