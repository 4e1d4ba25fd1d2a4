// Bridges of the undirected multigraph on gfx950 — replaces
// bridges_alg::GetBridges (src/mage/cpp/bridges_module/algorithm/
// bridges.cpp:31-69: recursive low-link DFS, parent skipped by node id,
// candidates filtered by GetEdgesBetweenNodes(from, to).size() == 1). Net
// effect of that rule set: an edge is a bridge iff removing that one edge
// disconnects its component; parallel / antiparallel duplicates and
// self-loops never are.
//
// Tarjan-Vishkin on a BFS forest instead of a DFS (level-synchronous, no
// recursion, no walk from a non-tree edge up to the LCA, which is quadratic on
// deep graphs). All state is int32 / uint32 in the identity vertex layout:
//   parent, level   forest: roots are the WCC min-members (label[v] == v), one
//                   multi-source direction-optimizing BFS from all of them;
//                   parent[v] = minimum-id neighbour one level up,
//                   parent[root] = root            (wcc.hip / bfs.hip)
//   child           non-root vertices stably sorted by parent (siblings in
//                   ascending id), child_ptr[p] = first child of p,
//                   cidx[v] = position of v in child
//   lvl_order       child stably sorted by level, level_ptr[l] its level
//                   offsets: each level list is sorted by parent
//   nd[v]           subtree size, pushed bottom-up with integer atomics, one
//                   per run of siblings in a wave
//   pre[v]          global preorder number in [0, V): roots in ascending id
//                   take the exclusive scan of their tree sizes, then
//                   pre[c] = pre[p] + 1 + (S[cidx[c]] - S[child_ptr[p]]) with S
//                   the exclusive scan of nd over child. subtree(v) is the
//                   interval [pre[v], pre[v] + nd[v]).
//   low[v], high[v] min / max of pre over v's own entries (the hot sweep),
//                   then folded bottom-up over the subtree.
// A non-root v marks {parent[v], v} iff low[v] >= pre[v] and
// high[v] < pre[v] + nd[v]: no non-tree entry leaves the subtree.
//
// S in 32 bits: the sum of nd over all non-roots is about V * depth and
// passes 2^32 long before V does (a 3000-path with 1.5M leaves at its end:
// 4.5e9). S is an unsigned 32-bit scan that wraps. It is only ever used as
// S[cidx[c]] - S[child_ptr[p]], the sum of nd over c's earlier siblings,
// which is < nd[p] <= V < 2^31, and unsigned subtraction modulo 2^32
// recovers any difference below 2^32 exactly.
//
// The parent rule: entry (v, w) with w == parent[v] is the tree edge and is
// skipped, unless row v holds that id two or more times (a duplicate of the
// tree edge is a non-tree edge): then pre[parent] is included. The run of
// parent entries may straddle lanes and waves, so it is counted with the
// row reduction.

#include <climits>
#include <cstring>
#include <vector>

#include <rocprim/rocprim.hpp>

#include "mgx_device.h"

namespace {

struct LoHiArgs {
  const uint32_t *row_ptr;
  const int32_t *col;
  mgx_bin_sections bins;
  const int32_t *parent;
  const uint32_t *pre;
  uint32_t *low, *high;
};

template <int LANES>
__device__ inline void lohi_rows(const LoHiArgs &A, int sec, int64_t block_in_sec) {
  for_bin_row_steps<LANES>(A.bins, sec, block_in_sec, [&](const int32_t *rowp, bool live,
                                                          int sub) {
    uint32_t lo = UINT32_MAX, hi = 0u, npar = 0u;
    int32_t row = -1, par = -1;
    if (live) {
      row = *rowp;
      par = A.parent[row];
      // nontemporal on the col stream only (inside row_gather); pre/low/high
      // live in pool-recycled buffers.
      row_gather<LANES>(A.col, A.row_ptr[row], A.row_ptr[row + 1], sub, [&](int32_t w) {
        if (w == par) {
          ++npar;
        } else {
          const uint32_t p = A.pre[w];
          lo = min(lo, p);
          hi = max(hi, p);
        }
      });
    }
    lo = row_reduce<LANES>(lo, mgx_op_min());
    if constexpr (LANES > 64) __syncthreads();
    hi = row_reduce<LANES>(hi, mgx_op_max());
    if constexpr (LANES > 64) __syncthreads();
    npar = row_reduce<LANES>(npar, mgx_op_add());
    if (sub == 0 && row >= 0) {
      const uint32_t pv = A.pre[row];
      lo = min(lo, pv);
      hi = max(hi, pv);
      if (npar >= 2u) {
        const uint32_t pp = A.pre[par];
        lo = min(lo, pp);
        hi = max(hi, pp);
      }
      A.low[row] = lo;
      A.high[row] = hi;
    }
    if constexpr (LANES > 64) __syncthreads();  // row_reduce's slots are reused
  });
}

__global__ void __launch_bounds__(kBlock) k_br_lohi(LoHiArgs A) {
  for_bin_section(A.bins.goff, [&](auto lanes, int sec, int64_t bis) {
    lohi_rows<decltype(lanes)::value>(A, sec, bis);
  });
}

#define BR_FOR(i, n)                                                         \
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < (n); \
       i += (int64_t)gridDim.x * blockDim.x)

__global__ void k_br_flag_roots(int64_t n, const int32_t *label, uint32_t *flag) {
  BR_FOR(i, n) flag[i] = (label[i] == (int32_t)i) ? 1u : 0u;
}

// Compact the flagged ids in ascending order: out[scan[i]] = i.
__global__ void k_br_scatter_ids(int64_t n, const uint32_t *flag, const uint32_t *scan,
                                 int32_t *out) {
  BR_FOR(i, n) if (flag[i]) out[scan[i]] = (int32_t)i;
}

// level_ptr[l] = first position of level l in the level-sorted keys;
// level_ptr[deepest + 1] = n.
__global__ void k_br_level_ptr(int64_t n, const uint32_t *keys, uint32_t *level_ptr) {
  BR_FOR(i, n) {
    const uint32_t k = keys[i];
    if (i == 0 || keys[i - 1] != k) level_ptr[k] = (uint32_t)i;
    if (i == n - 1) level_ptr[k + 1] = (uint32_t)n;
  }
}

// Sort key of the child lists: the parent, or V for a root (roots sort last).
__global__ void k_br_child_key(int64_t n, const int32_t *parent, uint32_t *key) {
  BR_FOR(i, n) key[i] = parent[i] == (int32_t)i ? (uint32_t)n : (uint32_t)parent[i];
}

__global__ void k_br_child_index(int64_t n, const uint32_t *key_sorted, const int32_t *child,
                                 uint32_t *cidx, uint32_t *child_ptr) {
  BR_FOR(i, n) {
    cidx[child[i]] = (uint32_t)i;
    const uint32_t k = key_sorted[i];
    if (k != (uint32_t)n && (i == 0 || key_sorted[i - 1] != k)) child_ptr[k] = (uint32_t)i;
  }
}

// out[i] = val[ids[i]]
__global__ void k_br_gather(int64_t n, const int32_t *ids, const uint32_t *val, uint32_t *out) {
  BR_FOR(i, n) out[i] = val[ids[i]];
}

// val[ids[i]] = in[i]
__global__ void k_br_scatter(int64_t n, const int32_t *ids, const uint32_t *in, uint32_t *val) {
  BR_FOR(i, n) val[ids[i]] = in[i];
}

// ---- the three per-level passes (list = the vertices of one level >= 1) ----
// A level list is sorted by parent (step 2), so the children of a hub sit in
// adjacent lanes: the two push passes combine each run of equal parents
// inside the wave and issue one atomic per run, not one per child.

// The 64 lanes of a wave hold (p, x) with equal p adjacent. Segmented inclusive
// scan by p (after the step of offset o, x covers the last 2o lanes of the
// lane's run); true in the last lane of each run, which then holds the run's
// value. Must be reached by all 64 lanes.
template <typename Op>
__device__ inline bool run_reduce(int32_t p, uint32_t &x, Op op) {
  const int lane = threadIdx.x & 63;
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t y = __shfl_up(x, o, 64);
    const int32_t q = __shfl_up(p, o, 64);
    if (lane >= o && q == p) x = op(x, y);
  }
  const int32_t next = __shfl_down(p, 1, 64);
  return lane == 63 || next != p;
}

// Grid-stride over whole waves: idle lanes of the last wave carry p = -1.
#define BR_FOR_WAVES(i, n)                                                          \
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x,                 \
               n64_ = ((n) + 63) / 64 * 64;                                         \
       i < n64_; i += (int64_t)gridDim.x * blockDim.x)

__global__ void k_br_push_nd(int64_t n, const int32_t *list, const int32_t *parent,
                             uint32_t *nd) {
  BR_FOR_WAVES(i, n) {
    int32_t p = -1;
    uint32_t x = 0u;
    if (i < n) {
      const int32_t v = list[i];
      p = parent[v];
      x = nd[v];
    }
    if (run_reduce(p, x, mgx_op_add()) && p >= 0) atomicAdd(&nd[p], x);
  }
}

__global__ void k_br_pull_pre(int64_t n, const int32_t *list, const int32_t *parent,
                              const uint32_t *S, const uint32_t *cidx,
                              const uint32_t *child_ptr, uint32_t *pre) {
  BR_FOR(i, n) {
    const int32_t v = list[i];
    const int32_t p = parent[v];
    pre[v] = pre[p] + 1u + (S[cidx[v]] - S[child_ptr[p]]);  // difference mod 2^32 (header)
  }
}

__global__ void k_br_push_lohi(int64_t n, const int32_t *list, const int32_t *parent,
                               uint32_t *low, uint32_t *high) {
  BR_FOR_WAVES(i, n) {
    int32_t p = -1;
    uint32_t lo = UINT32_MAX, hi = 0u;
    if (i < n) {
      const int32_t v = list[i];
      p = parent[v];
      lo = low[v];
      hi = high[v];
    }
    const bool tail = run_reduce(p, lo, mgx_op_min());
    run_reduce(p, hi, mgx_op_max());
    if (tail && p >= 0) {
      atomicMin(&low[p], lo);
      atomicMax(&high[p], hi);
    }
  }
}

// ---- the test ----

__global__ void k_br_flag_bridges(int64_t n, const int32_t *parent, const uint32_t *pre,
                                  const uint32_t *nd, const uint32_t *low, const uint32_t *high,
                                  uint32_t *flag) {
  BR_FOR(i, n) {
    const uint32_t pv = pre[i];
    flag[i] = (parent[i] != (int32_t)i && low[i] >= pv && high[i] < pv + nd[i]) ? 1u : 0u;
  }
}

// key = (min(parent, v) << 32) | max(parent, v)
__global__ void k_br_scatter_pairs(int64_t n, const uint32_t *flag, const uint32_t *scan,
                                   const int32_t *parent, uint64_t *keys) {
  BR_FOR(i, n) if (flag[i]) {
    const uint32_t a = (uint32_t)parent[i], b = (uint32_t)i;
    keys[scan[i]] = ((uint64_t)min(a, b) << 32) | (uint64_t)max(a, b);
  }
}

__global__ void k_br_unpack_pairs(int64_t n, const uint64_t *keys, int64_t *u, int64_t *v) {
  BR_FOR(i, n) {
    u[i] = (int64_t)(keys[i] >> 32);
    v[i] = (int64_t)(keys[i] & 0xFFFFFFFFull);
  }
}

#undef BR_FOR
#undef BR_FOR_WAVES

// Stage boundaries of the last call on this thread.
enum { kStForest, kStSorts, kStSweep, kStLevels, kStages };
thread_local double t_stage_ms[kStages] = {0, 0, 0, 0};

struct Timeline {
  hipStream_t stream;
  std::vector<hipEvent_t> ev;
  std::vector<int> stage;  // stage of the interval ending at ev[i]
  explicit Timeline(hipStream_t s) : stream(s) {}
  ~Timeline() {
    for (hipEvent_t e : ev) (void)hipEventDestroy(e);
  }
  mgx_status mark(int st) {
    hipEvent_t e;
    MGX_HIP_TRY(hipEventCreate(&e));
    ev.push_back(e);
    stage.push_back(st);
    MGX_HIP_TRY(hipEventRecord(e, stream));
    return MGX_OK;
  }
  // After a stream sync: per-stage sums and the whole span.
  mgx_status fold(double *stage_ms, double *total) {
    for (int s = 0; s < kStages; ++s) stage_ms[s] = 0.0;
    *total = 0.0;
    for (size_t i = 1; i < ev.size(); ++i) {
      float ms = 0.f;
      MGX_HIP_TRY(hipEventElapsedTime(&ms, ev[i - 1], ev[i]));
      stage_ms[stage[i]] += ms;
      *total += ms;
    }
    return MGX_OK;
  }
};

int bits_for(int64_t max_value) {
  int b = 1;
  while (b < 32 && (max_value >> b) > 0) ++b;
  return b;
}

struct BridgeState {
  int64_t V = 0, trees = 0, depth = 0, level_launches = 0;
  int32_t *parent = nullptr, *level = nullptr;
  uint32_t *pre = nullptr, *nd = nullptr, *low = nullptr, *high = nullptr;
  uint32_t *flag = nullptr, *scan = nullptr;  // [V] scratch, free after compute
};

inline uint32_t grid1(int64_t n) { return (uint32_t)grid_for(n, 2048); }

// Steps 1-6: everything up to the folded low/high. V > 0, sym-CSR present.
mgx_status bridges_compute(mgx_context *ctx, mgx_graph *g, mgx_scope &B, Timeline &T,
                           BridgeState &S) {
  const int64_t V = g->n_vertices;
  hipStream_t st = ctx->stream;
  S.V = V;

  // ---- 1. forest ----
  MGX_TRY(B.alloc(&S.flag, V));
  MGX_TRY(B.alloc(&S.scan, V));
  int32_t *roots = nullptr;
  MGX_TRY(B.alloc(&roots, V));
  {
    int32_t *label = nullptr;
    MGX_TRY(mgx_wcc_labels_device(B, g, &label));
    hipLaunchKernelGGL(k_br_flag_roots, dim3(grid1(V)), dim3(kBlock), 0, st, V, label, S.flag);
  }
  MGX_TRY(mgx_with_temp(ctx, "bridges root scan", [&](void *tmp, size_t &bytes) {
    return rocprim::exclusive_scan(tmp, bytes, S.flag, S.scan, 0u, V, rocprim::plus<uint32_t>(),
                                   st);
  }));
  hipLaunchKernelGGL(k_br_scatter_ids, dim3(grid1(V)), dim3(kBlock), 0, st, V, S.flag, S.scan,
                     roots);
  {
    uint32_t last_scan = 0, last_flag = 0;
    MGX_HIP_TRY(hipMemcpyAsync(&last_scan, S.scan + V - 1, 4, hipMemcpyDeviceToHost, st));
    MGX_HIP_TRY(hipMemcpyAsync(&last_flag, S.flag + V - 1, 4, hipMemcpyDeviceToHost, st));
    MGX_HIP_TRY(hipStreamSynchronize(st));
    S.trees = (int64_t)last_scan + last_flag;
  }
  if (S.trees < 1 || S.trees > V) {
    mgx_set_error("bridges: %lld roots for %lld vertices", (long long)S.trees, (long long)V);
    return MGX_ERR_HIP;
  }
  MGX_TRY(B.alloc(&S.level, V));
  MGX_TRY(B.alloc(&S.parent, V));
  mgx_bfs_stats bst;
  MGX_TRY(mgx_bfs_device(ctx, g, roots, S.trees, 0, /*directed=*/0, /*max_depth=*/-1,
                         MGX_BFS_AUTO, S.level, S.parent, &bst));
  if (bst.reached != V || bst.depth < 0 || bst.depth >= V) {
    mgx_set_error("bridges: forest reached %lld of %lld vertices, depth %lld",
                  (long long)bst.reached, (long long)V, (long long)bst.depth);
    return MGX_ERR_HIP;
  }
  const int64_t depth = S.depth = bst.depth;
  MGX_TRY(T.mark(kStForest));

  // ---- 2. level lists and child lists ----
  // Child lists first: vertices stably sorted by parent (roots keyed V sort
  // last; equal parents keep the ascending ids of iota).
  uint32_t *iota = nullptr, *ckey = nullptr, *ckey_s = nullptr, *cidx = nullptr;
  uint32_t *child_ptr = nullptr;
  int32_t *child = nullptr;
  MGX_TRY(B.alloc(&iota, V));
  MGX_TRY(B.alloc(&ckey, V));
  MGX_TRY(B.alloc(&ckey_s, V));
  MGX_TRY(B.alloc(&child, V));
  MGX_TRY(B.alloc(&cidx, V));
  MGX_TRY(B.alloc(&child_ptr, V));
  hipLaunchKernelGGL(mgx_k_iota<uint32_t>, dim3(grid1(V)), dim3(kBlock), 0, st, V, iota);
  hipLaunchKernelGGL(k_br_child_key, dim3(grid1(V)), dim3(kBlock), 0, st, V, S.parent, ckey);
  MGX_TRY(mgx_with_temp(ctx, "bridges child sort", [&](void *tmp, size_t &bytes) {
    return rocprim::radix_sort_pairs(tmp, bytes, (const uint32_t *)ckey, ckey_s,
                                     (const uint32_t *)iota, (uint32_t *)child, V, 0,
                                     bits_for(V), st);
  }));
  MGX_HIP_TRY(hipMemsetAsync(child_ptr, 0, V * sizeof(uint32_t), st));
  hipLaunchKernelGGL(k_br_child_index, dim3(grid1(V)), dim3(kBlock), 0, st, V, ckey_s, child,
                     cidx, child_ptr);
  // Level lists: the child array stably sorted by level (only the bits depth
  // needs), so every level list is itself sorted by parent.
  uint32_t *lvl_in = nullptr, *lvl_keys = nullptr, *d_level_ptr = nullptr;
  int32_t *lvl_order = nullptr;
  MGX_TRY(B.alloc(&lvl_in, V));
  MGX_TRY(B.alloc(&lvl_keys, V));
  MGX_TRY(B.alloc(&lvl_order, V));
  MGX_TRY(B.alloc(&d_level_ptr, depth + 2));
  hipLaunchKernelGGL(k_br_gather, dim3(grid1(V)), dim3(kBlock), 0, st, V, child,
                     (const uint32_t *)S.level, lvl_in);
  MGX_TRY(mgx_with_temp(ctx, "bridges level sort", [&](void *tmp, size_t &bytes) {
    return rocprim::radix_sort_pairs(tmp, bytes, (const uint32_t *)lvl_in, lvl_keys,
                                     (const uint32_t *)child, (uint32_t *)lvl_order, V, 0,
                                     bits_for(depth), st);
  }));
  MGX_HIP_TRY(hipMemsetAsync(d_level_ptr, 0xFF, (depth + 2) * sizeof(uint32_t), st));
  hipLaunchKernelGGL(k_br_level_ptr, dim3(grid1(V)), dim3(kBlock), 0, st, V, lvl_keys,
                     d_level_ptr);
  std::vector<uint32_t> lp(depth + 2);
  MGX_HIP_TRY(hipMemcpyAsync(lp.data(), d_level_ptr, (depth + 2) * sizeof(uint32_t),
                             hipMemcpyDeviceToHost, st));
  MGX_HIP_TRY(hipStreamSynchronize(st));
  // The level offsets size every per-level launch: check them before use.
  if (lp[0] != 0u || lp[depth + 1] != (uint32_t)V || lp[1] != (uint32_t)S.trees) {
    mgx_set_error("bridges: inconsistent level lists");
    return MGX_ERR_HIP;
  }
  for (int64_t l = 0; l <= depth; ++l) {
    if (lp[l] >= lp[l + 1]) {
      mgx_set_error("bridges: level %lld is empty or out of order", (long long)l);
      return MGX_ERR_HIP;
    }
  }
  MGX_TRY(T.mark(kStSorts));

  // ---- 3. subtree sizes, deepest level first ----
  MGX_TRY(B.alloc(&S.nd, V));
  MGX_TRY(B.alloc(&S.pre, V));
  MGX_TRY(B.alloc(&S.low, V));
  MGX_TRY(B.alloc(&S.high, V));
  hipLaunchKernelGGL(mgx_k_fill<uint32_t>, dim3(grid1(V)), dim3(kBlock), 0, st, V, 1u, S.nd);
  for (int64_t l = depth; l >= 1; --l) {
    const int64_t n = (int64_t)lp[l + 1] - lp[l];
    hipLaunchKernelGGL(k_br_push_nd, dim3(grid1(n)), dim3(kBlock), 0, st, n, lvl_order + lp[l],
                       S.parent, S.nd);
  }
  MGX_TRY(T.mark(kStLevels));

  // ---- 4. preorder ----
  // Roots (ascending id): exclusive scan of the tree sizes. flag / scan are
  // free again; the sum is V.
  hipLaunchKernelGGL(k_br_gather, dim3(grid1(S.trees)), dim3(kBlock), 0, st, S.trees, roots,
                     S.nd, S.flag);
  MGX_TRY(mgx_with_temp(ctx, "bridges tree scan", [&](void *tmp, size_t &bytes) {
    return rocprim::exclusive_scan(tmp, bytes, S.flag, S.scan, 0u, S.trees,
                                   rocprim::plus<uint32_t>(), st);
  }));
  MGX_HIP_TRY(hipMemsetAsync(S.pre, 0, V * sizeof(uint32_t), st));
  hipLaunchKernelGGL(k_br_scatter, dim3(grid1(S.trees)), dim3(kBlock), 0, st, S.trees, roots,
                     S.scan, S.pre);
  // S = exclusive scan of nd over the child array, modulo 2^32 (header). The
  // roots at its tail are scanned too and never looked at.
  uint32_t *ndc = ckey, *Sx = ckey_s;  // both free after the child index
  hipLaunchKernelGGL(k_br_gather, dim3(grid1(V)), dim3(kBlock), 0, st, V, child, S.nd, ndc);
  MGX_TRY(mgx_with_temp(ctx, "bridges sibling scan", [&](void *tmp, size_t &bytes) {
    return rocprim::exclusive_scan(tmp, bytes, ndc, Sx, 0u, V, rocprim::plus<uint32_t>(), st);
  }));
  MGX_TRY(T.mark(kStSorts));
  for (int64_t l = 1; l <= depth; ++l) {
    const int64_t n = (int64_t)lp[l + 1] - lp[l];
    hipLaunchKernelGGL(k_br_pull_pre, dim3(grid1(n)), dim3(kBlock), 0, st, n, lvl_order + lp[l],
                       S.parent, Sx, cidx, child_ptr, S.pre);
  }
  MGX_TRY(T.mark(kStLevels));

  // ---- 5. local low/high: the one pass over all 2E entries ----
  LoHiArgs A;
  A.row_ptr = g->sym_row_ptr;
  A.col = g->sym_col;
  const int64_t goff = mgx_fill_sections(g->bins_sym, &A.bins);
  A.parent = S.parent;
  A.pre = S.pre;
  A.low = S.low;
  A.high = S.high;
  if (goff > 0) hipLaunchKernelGGL(k_br_lohi, dim3((uint32_t)goff), dim3(kBlock), 0, st, A);
  MGX_TRY(T.mark(kStSweep));

  // ---- 6. fold into parents, deepest level first ----
  for (int64_t l = depth; l >= 1; --l) {
    const int64_t n = (int64_t)lp[l + 1] - lp[l];
    hipLaunchKernelGGL(k_br_push_lohi, dim3(grid1(n)), dim3(kBlock), 0, st, n,
                       lvl_order + lp[l], S.parent, S.low, S.high);
  }
  S.level_launches = 3 * depth;
  MGX_TRY(T.mark(kStLevels));
  return MGX_OK;
}

mgx_status check_sym(mgx_graph *g) {
  if (!(g->flags & MGX_BUILD_SYM_CSR)) {
    mgx_set_error("bridges needs a graph built with MGX_BUILD_SYM_CSR");
    return MGX_ERR_INVALID_ARGUMENT;
  }
  return MGX_OK;
}

}  // namespace

mgx_status mgx_bridges_impl(mgx_context *ctx, mgx_graph *g, int64_t *out_u, int64_t *out_v,
                            int64_t *n_bridges, mgx_bridges_stats *stats) {
  MGX_TRY(check_sym(g));
  const int64_t V = g->n_vertices;
  if (stats) *stats = mgx_bridges_stats{};
  if (n_bridges) *n_bridges = 0;
  if (V == 0) return MGX_OK;

  mgx_scope B(ctx);
  Timeline T(ctx->stream);
  BridgeState S;
  MGX_TRY(T.mark(kStForest));
  MGX_TRY(bridges_compute(ctx, g, B, T, S));
  hipStream_t st = ctx->stream;

  // ---- 7. test, compact, order ----
  hipLaunchKernelGGL(k_br_flag_bridges, dim3(grid1(V)), dim3(kBlock), 0, st, V, S.parent, S.pre,
                     S.nd, S.low, S.high, S.flag);
  MGX_TRY(mgx_with_temp(ctx, "bridges compact scan", [&](void *tmp, size_t &bytes) {
    return rocprim::exclusive_scan(tmp, bytes, S.flag, S.scan, 0u, V, rocprim::plus<uint32_t>(),
                                   st);
  }));
  uint32_t last_scan = 0, last_flag = 0;
  MGX_HIP_TRY(hipMemcpyAsync(&last_scan, S.scan + V - 1, 4, hipMemcpyDeviceToHost, st));
  MGX_HIP_TRY(hipMemcpyAsync(&last_flag, S.flag + V - 1, 4, hipMemcpyDeviceToHost, st));
  MGX_HIP_TRY(hipStreamSynchronize(st));
  const int64_t count = (int64_t)last_scan + last_flag;
  if (count > V - S.trees) {
    mgx_set_error("bridges: %lld bridges in a forest of %lld edges", (long long)count,
                  (long long)(V - S.trees));
    return MGX_ERR_HIP;
  }
  uint64_t *keys = nullptr, *keys_s = nullptr;
  int64_t *d_u = nullptr, *d_v = nullptr;
  if (count > 0) {
    MGX_TRY(B.alloc(&keys, count));
    MGX_TRY(B.alloc(&keys_s, count));
    MGX_TRY(B.alloc(&d_u, count));
    MGX_TRY(B.alloc(&d_v, count));
    hipLaunchKernelGGL(k_br_scatter_pairs, dim3(grid1(V)), dim3(kBlock), 0, st, V, S.flag,
                       S.scan, S.parent, keys);
    MGX_TRY(mgx_with_temp(ctx, "bridges pair sort", [&](void *tmp, size_t &bytes) {
      return rocprim::radix_sort_keys(tmp, bytes, (const uint64_t *)keys, keys_s, count, 0, 64,
                                      st);
    }));
    hipLaunchKernelGGL(k_br_unpack_pairs, dim3(grid1(count)), dim3(kBlock), 0, st, count,
                       keys_s, d_u, d_v);
  }
  MGX_TRY(T.mark(kStSorts));
  if (count > 0) {
    if (out_u)
      MGX_HIP_TRY(hipMemcpyAsync(out_u, d_u, count * sizeof(int64_t), hipMemcpyDeviceToHost,
                                 st));
    if (out_v)
      MGX_HIP_TRY(hipMemcpyAsync(out_v, d_v, count * sizeof(int64_t), hipMemcpyDeviceToHost,
                                 st));
  }
  MGX_HIP_TRY(hipStreamSynchronize(st));
  double total = 0.0;
  MGX_TRY(T.fold(t_stage_ms, &total));
  if (n_bridges) *n_bridges = count;
  if (stats) {
    stats->bridges = count;
    stats->trees = S.trees;
    stats->depth = S.depth;
    stats->nontree_entries = 2 * g->n_edges - (V - S.trees);
    stats->level_launches = S.level_launches;
    stats->forest_ms = t_stage_ms[kStForest];
    stats->ms = total;
  }
  MGX_HIP_TRY(hipGetLastError());
  return MGX_OK;
}

mgx_status mgx_bridges_state_impl(mgx_context *ctx, mgx_graph *g, int64_t *parent,
                                  int64_t *level, int64_t *pre, int64_t *nd, int64_t *low,
                                  int64_t *high) {
  MGX_TRY(check_sym(g));
  const int64_t V = g->n_vertices;
  if (V == 0) return MGX_OK;
  mgx_scope B(ctx);
  Timeline T(ctx->stream);
  BridgeState S;
  MGX_TRY(T.mark(kStForest));
  MGX_TRY(bridges_compute(ctx, g, B, T, S));
  hipStream_t st = ctx->stream;
  int64_t *wide = nullptr;
  MGX_TRY(B.alloc(&wide, V));
  auto emit = [&](auto *src, int64_t *dst) -> mgx_status {
    if (!dst) return MGX_OK;
    using From = std::remove_pointer_t<decltype(src)>;
    hipLaunchKernelGGL((mgx_k_widen<From, int64_t>), dim3(grid1(V)), dim3(kBlock), 0, st, V,
                       (const From *)src, wide);
    MGX_HIP_TRY(hipMemcpyAsync(dst, wide, V * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    return MGX_OK;
  };
  MGX_TRY(emit(S.parent, parent));
  MGX_TRY(emit(S.level, level));
  MGX_TRY(emit(S.pre, pre));
  MGX_TRY(emit(S.nd, nd));
  MGX_TRY(emit(S.low, low));
  MGX_TRY(emit(S.high, high));
  MGX_HIP_TRY(hipStreamSynchronize(st));
  MGX_HIP_TRY(hipGetLastError());
  return MGX_OK;
}

void mgx_bridges_last_stage_ms_impl(double *forest, double *sorts_scans, double *sweep,
                                    double *levels) {
  if (forest) *forest = t_stage_ms[kStForest];
  if (sorts_scans) *sorts_scans = t_stage_ms[kStSorts];
  if (sweep) *sweep = t_stage_ms[kStSweep];
  if (levels) *levels = t_stage_ms[kStLevels];
}
