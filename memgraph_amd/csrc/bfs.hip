// Direction-optimizing single-source BFS on gfx950: hop counts and
// minimum-id parents. Replaces the queue BFS of the reference's
// connectivity_module.cpp:50-71 (undirected level structure) and the level
// sets of neighbors.at_hop / neighbors.by_hop
// (src/mage/cpp/neighbors_module/algorithm/neighbors.cpp:52-160: per-hop
// sets, depth limit; the typed/directed rule of :26-48 is applied by the
// caller when it builds the traversal COO).
//
// State (all int32 / uint32, identity vertex layout):
//   hops[V]     -1 = unreached
//   parent[V]   only when requested; atomicMin target, INT32_MAX = none
//   visited, fcur, fnext   bitmaps of ceil(V/32) words
//   q01, q23    frontier queues for the top-down step, split by the
//               degree class of the queued vertex (the mgx_bins classes:
//               <8, <64, <1024, >=1024 -> 4/16/64/256 lanes per row).
//               A vertex is queued at most once per call, so class 0 grows
//               from the front of q01 and class 1 from its back (2/3 share
//               q23 the same way) and each array needs only V slots.
//   counters    cumulative queue tails per class, degree sum and count of
//               reached vertices, entries scanned by bottom-up levels.
//
// Why bitmaps (CDNA4): the per-edge test "is this neighbour visited / in the
// frontier" is a random gather. One bit per vertex is 2 MB at RMAT-24 and
// 8 MB at RMAT-26, which stays resident in the 4 MB-per-XCD L2 / the
// Infinity Cache; a 4-byte hops[] gather (64 MB / 256 MB) does not.
//
// Top-down: expand the queued frontier, lanes-per-row by class. visited is
// read-only during a level; a neighbour is claimed by atomicOr on fnext, so
// "w is new this level" is the same stable answer for every edge into w and
// atomicMin(parent[w], u) over all of them yields the minimum-id
// predecessor. The claimer writes hops and enqueues w (wave-aggregated: one
// atomicAdd per wave per class). A queue-driven finish kernel then folds
// the new frontier into visited and clears the old frontier's bitmap words,
// so a level costs O(frontier edges), never O(V).
// Bottom-up (symmetric CSR only): every unvisited row scans its sorted
// neighbours against fcur and stops at the first chunk with a hit; the
// lowest hitting lane is the minimum-id predecessor.
// Direction: Beamer's rule with the growing/shrinking guard.
//
// mgx_bfs_device is the traversal itself, seeded from a device list of roots
// (level 0) and leaving hops / parent on the device: bridges.hip runs it from
// every component's minimum member at once. mgx_bfs is the single-source
// wrapper that widens and downloads. With several roots the queue order
// within a level depends on atomics, the results do not: hops is the level
// and parent the atomicMin / lowest-lane minimum, as with one source.

#include <algorithm>
#include <climits>
#include <cstdlib>

#include "mgx_device.h"

namespace {

constexpr int64_t kGridCap = 2048;  // element-wise launches of this file

struct BfsCounters {
  uint32_t tail[4];            // cumulative entries queued per degree class
  uint32_t seed_zero;          // level-0 vertices of a root list that have no entries
  uint32_t pad;
  unsigned long long degsum;   // cumulative degree sum of reached vertices
  unsigned long long reached;  // cumulative reached vertices
  unsigned long long scanned;  // cumulative entries examined bottom-up
};

__device__ inline int degree_class(uint32_t deg) {
  return deg < 8u ? 0 : deg < 64u ? 1 : deg < 1024u ? 2 : 3;
}

// Slot `idx` of class c's queue: even classes grow up from the front of
// their array, odd classes down from the back.
__device__ inline int32_t *qslot(int32_t *q01, int32_t *q23, int64_t V, int c, uint32_t idx) {
  int32_t *q = c < 2 ? q01 : q23;
  return (c & 1) ? q + (V - 1 - (int64_t)idx) : q + idx;
}

// Wave-aggregated enqueue: the lanes with `pred` set (any subset of the
// active lanes) append v to class cls's queue with one atomicAdd per wave
// per class. Must be reached by all currently active lanes together.
__device__ inline void enqueue(bool pred, int cls, int32_t v, int32_t *q01, int32_t *q23,
                               int64_t V, BfsCounters *cnt) {
  const int lane = threadIdx.x & 63;
  for (int c = 0; c < 4; ++c) {
    const bool mine = pred && cls == c;
    const unsigned long long mask = __ballot(mine);
    if (mine) {
      const int leader = __ffsll((long long)mask) - 1;
      const uint32_t rank = (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
      uint32_t base = 0;
      if (lane == leader) base = atomicAdd(&cnt->tail[c], (uint32_t)__popcll(mask));
      base = (uint32_t)__shfl((int)base, leader);
      *qslot(q01, q23, V, c, base + rank) = v;
    }
  }
}

// Sum a per-thread value over the wave (all 64 lanes converged).
__device__ inline unsigned long long wave_sum(unsigned long long x) {
  for (int o = 32; o; o >>= 1) x += __shfl_down(x, o, 64);
  return x;
}

__global__ void k_bfs_init(int64_t n, int32_t *hops, int32_t *parent) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    hops[i] = -1;
    if (parent) parent[i] = INT32_MAX;
  }
}

// Level 0: the n_roots distinct vertices of `roots` (or the one vertex
// `single` when roots is null). One thread per root; the grid covers whole
// waves so the ballot in enqueue() sees converged lanes.
__global__ void k_bfs_seed(const int32_t *roots, int64_t n_roots, int32_t single,
                           const uint32_t *row_ptr, int32_t *hops, int32_t *parent,
                           uint32_t *visited, uint32_t *fcur, int32_t *q01, int32_t *q23,
                           int64_t V, BfsCounters *cnt) {
  const int64_t n64 = (n_roots + 63) / 64 * 64;
  unsigned long long acc_deg = 0, acc_n = 0, acc_zero = 0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n64;
       i += (int64_t)gridDim.x * blockDim.x) {
    const bool live = i < n_roots;
    int32_t r = 0;
    int cls = 0;
    if (live) {
      r = roots ? roots[i] : single;
      const uint32_t deg = row_ptr[r + 1] - row_ptr[r];
      cls = degree_class(deg);
      if (roots && deg == 0u) acc_zero += 1;
      hops[r] = 0;
      if (parent) parent[r] = r;
      atomicOr(&visited[(uint32_t)r >> 5], 1u << (r & 31));
      atomicOr(&fcur[(uint32_t)r >> 5], 1u << (r & 31));
      acc_deg += deg;
      acc_n += 1;
    }
    enqueue(live, cls, r, q01, q23, V, cnt);
  }
  acc_deg = wave_sum(acc_deg);
  acc_n = wave_sum(acc_n);
  acc_zero = wave_sum(acc_zero);
  if ((threadIdx.x & 63) == 0 && acc_n) {
    atomicAdd(&cnt->degsum, acc_deg);
    atomicAdd(&cnt->reached, acc_n);
    if (acc_zero) atomicAdd(&cnt->seed_zero, (uint32_t)acc_zero);
  }
}

// ---- top-down ------------------------------------------------------------

struct BfsTdArgs {
  const uint32_t *row_ptr;
  const int32_t *col;
  int32_t *q01, *q23;
  int64_t V;
  uint32_t start[4], end[4];  // frontier = queue entries [start, end) per class
  int64_t goff[4], grid[4];
  int64_t split3;  // blocks sharing one class-3 row; grid[3] is a multiple of it
  const uint32_t *visited;
  uint32_t *fnext;
  int32_t *hops;
  int32_t *parent;  // nullable
  BfsCounters *cnt;
  int32_t level;
};

template <int LANES>
__device__ inline void td_rows(const BfsTdArgs &A, int c, int64_t block_in_sec,
                               unsigned long long &acc_deg, unsigned long long &acc_n) {
  constexpr int RPB = kBlock / LANES;
  const int64_t nrows = (int64_t)(A.end[c] - A.start[c]);
  const int sub = threadIdx.x % LANES;
  // A workgroup-per-row hub is split over `split` blocks (block k takes
  // every split-th 256-entry chunk): a lone 700k-degree source would
  // otherwise be one block's serial chain of atomics.
  const int64_t split = LANES == 256 ? A.split3 : 1;
  const int64_t row_blocks = A.grid[c] / split;
  const int64_t k = block_in_sec % split;
  for (int64_t base = (block_in_sec / split) * RPB; base < nrows; base += row_blocks * RPB) {
    const int64_t ri = base + threadIdx.x / LANES;
    if (ri >= nrows) continue;
    const int32_t u = *qslot(A.q01, A.q23, A.V, c, A.start[c] + (uint32_t)ri);
    const int64_t s = A.row_ptr[u], e = A.row_ptr[u + 1];
    for (int64_t j = s + k * LANES + sub; j < e; j += split * LANES) {
      const int32_t w = A.col[j];
      const uint32_t word = (uint32_t)w >> 5, bit = 1u << (w & 31);
      bool claimed = false;
      int cls = 0;
      if (!(A.visited[word] & bit)) {
        // A plain read of fnext can only be stale towards "not yet claimed",
        // which falls through to the atomic: it saves most of the atomics
        // on hub words and never changes the result.
        uint32_t old = A.parent ? 0u : A.fnext[word];
        if (!(old & bit)) old = atomicOr(&A.fnext[word], bit);
        if (A.parent) atomicMin(&A.parent[w], u);
        if (!(old & bit)) {
          claimed = true;
          A.hops[w] = A.level + 1;
          const uint32_t deg = A.row_ptr[w + 1] - A.row_ptr[w];
          cls = degree_class(deg);
          acc_deg += deg;
          acc_n += 1;
        }
      }
      enqueue(claimed, cls, w, A.q01, A.q23, A.V, A.cnt);
    }
  }
}

__global__ void __launch_bounds__(kBlock) k_bfs_top_down(BfsTdArgs A) {
  unsigned long long acc_deg = 0, acc_n = 0;
  for_bin_section(A.goff, [&](auto lanes, int c, int64_t bis) {
    td_rows<decltype(lanes)::value>(A, c, bis, acc_deg, acc_n);
  });
  acc_deg = wave_sum(acc_deg);
  acc_n = wave_sum(acc_n);
  if ((threadIdx.x & 63) == 0 && acc_n) {
    atomicAdd(&A.cnt->degsum, acc_deg);
    atomicAdd(&A.cnt->reached, acc_n);
  }
}

// After a top-down level: fold the new frontier (queue entries
// [new_start, new_end) per class) into visited and zero the words of the
// old frontier ([old_start, old_end)) in its bitmap, which becomes the next
// level's fnext.
struct BfsFinishArgs {
  int32_t *q01, *q23;
  int64_t V;
  uint32_t old_start[4], old_end[4], new_end[4];
  uint32_t *visited;
  uint32_t *fold;
};

__global__ void k_bfs_td_finish(BfsFinishArgs A) {
  const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int c = 0; c < 4; ++c) {
    for (int64_t i = A.old_start[c] + tid; i < (int64_t)A.old_end[c]; i += stride) {
      const int32_t v = *qslot(A.q01, A.q23, A.V, c, (uint32_t)i);
      A.fold[(uint32_t)v >> 5] = 0u;
    }
    for (int64_t i = A.old_end[c] + tid; i < (int64_t)A.new_end[c]; i += stride) {
      const int32_t v = *qslot(A.q01, A.q23, A.V, c, (uint32_t)i);
      atomicOr(&A.visited[(uint32_t)v >> 5], 1u << (v & 31));
    }
  }
}

// Bitmap -> queues, only when a bottom-up level is followed by a top-down
// one. One thread per vertex; the grid covers whole waves so the ballot in
// enqueue() sees converged lanes.
__global__ void k_bfs_bitmap_to_queue(int64_t V, const uint32_t *row_ptr, const uint32_t *fcur,
                                      int32_t *q01, int32_t *q23, BfsCounters *cnt) {
  const int64_t n64 = (V + 63) / 64 * 64;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n64;
       i += (int64_t)gridDim.x * blockDim.x) {
    bool in = false;
    int cls = 0;
    if (i < V) {
      in = (fcur[i >> 5] >> (i & 31)) & 1u;
      if (in) cls = degree_class(row_ptr[i + 1] - row_ptr[i]);
    }
    enqueue(in, cls, (int32_t)i, q01, q23, V, cnt);
  }
}

// ---- bottom-up -----------------------------------------------------------

struct BfsBuArgs {
  const uint32_t *row_ptr;
  const int32_t *col;
  mgx_bin_sections bins;
  uint32_t *visited;
  const uint32_t *fcur;
  uint32_t *fnext;
  int32_t *hops;
  int32_t *parent;  // nullable
  BfsCounters *cnt;
  int32_t level;
};

template <int LANES>
__device__ inline void bu_rows(const BfsBuArgs &A, int sec, int64_t block_in_sec,
                               unsigned long long &acc_deg, unsigned long long &acc_n,
                               unsigned long long &acc_scan) {
  const int lane = threadIdx.x & 63;
  __shared__ uint32_t s_hit[4];
  for_bin_rows<LANES>(A.bins, sec, block_in_sec, [&](int32_t row, int sub) {
    if ((A.visited[(uint32_t)row >> 5] >> (row & 31)) & 1u) return;
    const int64_t s = A.row_ptr[row], e = A.row_ptr[row + 1];
    // Everything below is uniform across the LANES lanes that share a row.
    // found = CSR index of the first hit (entries < 2^32 - 1).
    uint32_t found = UINT32_MAX;
    uint32_t examined = 0;
    for (int64_t cb = s; cb < e; cb += LANES) {
      const int64_t j = cb + sub;
      bool hit = false;
      if (j < e) {
        const int32_t w = A.col[j];
        hit = (A.fcur[(uint32_t)w >> 5] >> (w & 31)) & 1u;
      }
      const unsigned long long m = __ballot(hit);
      examined += (uint32_t)(e - cb < LANES ? e - cb : LANES);
      if constexpr (LANES <= 64) {
        const unsigned long long gm =
            LANES == 64 ? m : ((m >> (lane & ~(LANES - 1))) & ((1ull << (LANES & 63)) - 1ull));
        if (gm) {
          found = (uint32_t)(cb + __ffsll((long long)gm) - 1);
          break;
        }
      } else {
        if (lane == 0)
          s_hit[threadIdx.x >> 6] =
              m ? (uint32_t)(cb + (threadIdx.x & ~63u) + __ffsll((long long)m) - 1) : UINT32_MAX;
        __syncthreads();
        const uint32_t f = min(min(s_hit[0], s_hit[1]), min(s_hit[2], s_hit[3]));
        __syncthreads();
        if (f != UINT32_MAX) {
          found = f;
          break;
        }
      }
    }
    if (sub == 0) {
      acc_scan += examined;
      if (found != UINT32_MAX) {
        A.hops[row] = A.level + 1;
        if (A.parent) A.parent[row] = A.col[found];
        atomicOr(&A.visited[(uint32_t)row >> 5], 1u << (row & 31));
        atomicOr(&A.fnext[(uint32_t)row >> 5], 1u << (row & 31));
        acc_deg += e - s;
        acc_n += 1;
      }
    }
  });
}

__global__ void __launch_bounds__(kBlock) k_bfs_bottom_up(BfsBuArgs A) {
  unsigned long long acc_deg = 0, acc_n = 0, acc_scan = 0;
  for_bin_section(A.bins.goff, [&](auto lanes, int sec, int64_t bis) {
    bu_rows<decltype(lanes)::value>(A, sec, bis, acc_deg, acc_n, acc_scan);
  });
  acc_deg = wave_sum(acc_deg);
  acc_n = wave_sum(acc_n);
  acc_scan = wave_sum(acc_scan);
  if ((threadIdx.x & 63) == 0) {
    if (acc_scan) atomicAdd(&A.cnt->scanned, acc_scan);
    if (acc_n) {
      atomicAdd(&A.cnt->degsum, acc_deg);
      atomicAdd(&A.cnt->reached, acc_n);
    }
  }
}

// Widen to the int64 ABI on device before the download.
__global__ void k_bfs_emit(int64_t n, const int32_t *hops, const int32_t *parent,
                           int64_t *out_hops, int64_t *out_parent) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    if (out_hops) out_hops[i] = hops[i];
    if (out_parent) {
      const int32_t p = parent[i];
      out_parent[i] = p == INT32_MAX ? -1 : p;
    }
  }
}

int64_t env_positive(const char *name, int64_t dflt) {
  const char *env = getenv(name);
  if (env && atoll(env) > 0) return atoll(env);
  return dflt;
}

}  // namespace

namespace {

mgx_status bfs_check_args(mgx_graph *g, int directed, int mode) {
  if (mode != MGX_BFS_AUTO && mode != MGX_BFS_TOP_DOWN && mode != MGX_BFS_BOTTOM_UP) {
    mgx_set_error("bfs: unknown mode %d", mode);
    return MGX_ERR_INVALID_ARGUMENT;
  }
  if (directed && mode == MGX_BFS_BOTTOM_UP) {
    mgx_set_error("bfs: bottom-up needs the symmetric CSR (directed=0); the in-CSR is "
                  "not in the identity vertex layout");
    return MGX_ERR_NOT_SUPPORTED;
  }
  if (!(g->flags & (directed ? MGX_BUILD_OUT_CSR : MGX_BUILD_SYM_CSR))) {
    mgx_set_error("bfs(directed=%d) needs a graph built with MGX_BUILD_%s_CSR", directed,
                  directed ? "OUT" : "SYM");
    return MGX_ERR_INVALID_ARGUMENT;
  }
  return MGX_OK;
}

}  // namespace

// The traversal with its seeds and results on the device: level 0 is the
// n_roots distinct vertices of d_roots (or the one vertex `single` when
// d_roots is null); hops [V] and parent [V] (nullable) are the caller's
// buffers and are left holding -1 / INT32_MAX where nothing was reached.
// stats->ms covers init to last level.
mgx_status mgx_bfs_device(mgx_context *ctx, mgx_graph *g, const int32_t *d_roots,
                          int64_t n_roots, int32_t single, int directed, int64_t max_depth,
                          int mode, int32_t *hops, int32_t *parent, mgx_bfs_stats *stats) {
  MGX_TRY(bfs_check_args(g, directed, mode));
  const int64_t V = g->n_vertices;
  const uint32_t *row_ptr = directed ? g->out_row_ptr : g->sym_row_ptr;
  const int32_t *col = directed ? g->out_col : g->sym_col;
  const int64_t total_entries = directed ? g->n_edges : 2 * g->n_edges;
  const int64_t alpha = env_positive("MGX_BFS_ALPHA", 14);
  const int64_t beta = env_positive("MGX_BFS_BETA", 24);
  const int64_t W = (V + 31) / 32;

  int32_t *q01 = nullptr, *q23 = nullptr;
  uint32_t *visited = nullptr, *fcur = nullptr, *fnext = nullptr;
  BfsCounters *d_cnt = nullptr;
  mgx_scope bufs(ctx);
  MGX_TRY(bufs.alloc(&q01, V));
  MGX_TRY(bufs.alloc(&q23, V));
  MGX_TRY(bufs.alloc(&visited, W));
  MGX_TRY(bufs.alloc(&fcur, W));
  MGX_TRY(bufs.alloc(&fnext, W));
  MGX_TRY(bufs.alloc(&d_cnt, 1));

  hipEvent_t ev0, ev1;
  MGX_HIP_TRY(hipEventCreate(&ev0));
  MGX_HIP_TRY(hipEventCreate(&ev1));
  MGX_HIP_TRY(hipEventRecord(ev0, ctx->stream));

  // The caching allocator hands back dirty blocks: clear everything.
  MGX_HIP_TRY(hipMemsetAsync(q01, 0, V * sizeof(int32_t), ctx->stream));
  MGX_HIP_TRY(hipMemsetAsync(q23, 0, V * sizeof(int32_t), ctx->stream));
  MGX_HIP_TRY(hipMemsetAsync(visited, 0, W * sizeof(uint32_t), ctx->stream));
  MGX_HIP_TRY(hipMemsetAsync(fcur, 0, W * sizeof(uint32_t), ctx->stream));
  MGX_HIP_TRY(hipMemsetAsync(fnext, 0, W * sizeof(uint32_t), ctx->stream));
  MGX_HIP_TRY(hipMemsetAsync(d_cnt, 0, sizeof(BfsCounters), ctx->stream));
  hipLaunchKernelGGL(k_bfs_init, dim3((uint32_t)grid_for(V, kGridCap)), dim3(kBlock), 0,
                     ctx->stream, V, hops, parent);
  hipLaunchKernelGGL(k_bfs_seed, dim3((uint32_t)grid_for(n_roots, kGridCap)), dim3(kBlock), 0,
                     ctx->stream, d_roots, n_roots, single, row_ptr, hops, parent, visited, fcur,
                     q01, q23, V, d_cnt);

  // One small D2H readback of the counter block per level.
  BfsCounters h;
  auto read_counters = [&](BfsCounters *dst) -> mgx_status {
    MGX_HIP_TRY(hipMemcpyAsync(dst, d_cnt, sizeof(BfsCounters), hipMemcpyDeviceToHost,
                               ctx->stream));
    MGX_HIP_TRY(hipStreamSynchronize(ctx->stream));
    return MGX_OK;
  };
  MGX_TRY(read_counters(&h));

  // Frontier size, previous level's. Roots of a list that have no entries
  // (isolated vertices: most of the 7.9 M roots of an RMAT-24 forest) are no
  // frontier for the growing guard below: counted, they made level 1 look
  // like a shrinking frontier and kept its 45 ms top-down.
  int64_t n_f = (int64_t)h.reached - (int64_t)h.seed_zero, prev_n_f = 0;
  int64_t m_f = (int64_t)h.degsum;        // frontier degree sum
  int64_t m_u = total_entries - m_f;      // unvisited degree sum
  uint32_t q_start[4] = {0, 0, 0, 0}, q_end[4];
  for (int c = 0; c < 4; ++c) q_end[c] = h.tail[c];
  bool have_queue = true;  // the queues hold exactly the current frontier
  bool bottom_up = mode == MGX_BFS_BOTTOM_UP;
  int64_t level = 0, depth = 0, td_levels = 0, bu_levels = 0, td_scanned = 0;
  uint64_t bu_mask = 0;

  while (n_f > 0 && (max_depth < 0 || level < max_depth)) {
    if (level > V) {
      mgx_set_error("bfs exceeded V levels");
      return MGX_ERR_HIP;
    }
    if (mode == MGX_BFS_AUTO && !directed) {
      // Beamer's rule with the growing/shrinking guard.
      if (!bottom_up && m_f > m_u / alpha && n_f > prev_n_f) bottom_up = true;
      else if (bottom_up && n_f < V / beta && n_f < prev_n_f) bottom_up = false;
    }

    if (!bottom_up) {
      if (!have_queue) {
        for (int c = 0; c < 4; ++c) q_start[c] = h.tail[c];
        hipLaunchKernelGGL(k_bfs_bitmap_to_queue, dim3((uint32_t)grid_for(V, kGridCap)),
                           dim3(kBlock), 0, ctx->stream, V, row_ptr, fcur, q01, q23, d_cnt);
        MGX_TRY(read_counters(&h));
        for (int c = 0; c < 4; ++c) q_end[c] = h.tail[c];
        have_queue = true;
      }
      BfsTdArgs A;
      A.row_ptr = row_ptr;
      A.col = col;
      A.q01 = q01;
      A.q23 = q23;
      A.V = V;
      const int64_t rows_per_block[4] = {64, 16, 4, 1};
      const int64_t cap[4] = {2048, 2048, 2048, 8192};
      int64_t goff = 0;
      for (int c = 0; c < 4; ++c) {
        A.start[c] = q_start[c];
        A.end[c] = q_end[c];
        const int64_t n = (int64_t)q_end[c] - q_start[c];
        const int64_t need = (n + rows_per_block[c] - 1) / rows_per_block[c];
        A.grid[c] = std::min(need, cap[c]);
        if (c == 3) {
          // Few hubs: give each up to 256 blocks, within the same grid cap.
          A.split3 = n > 0 ? std::max<int64_t>(1, std::min<int64_t>(256, cap[3] / n)) : 1;
          A.grid[3] = std::min(n, cap[3] / A.split3) * A.split3;
        }
        A.goff[c] = goff;
        goff += A.grid[c];
      }
      A.visited = visited;
      A.fnext = fnext;
      A.hops = hops;
      A.parent = parent;
      A.cnt = d_cnt;
      A.level = (int32_t)level;
      if (goff > 0)
        hipLaunchKernelGGL(k_bfs_top_down, dim3((uint32_t)goff), dim3(kBlock), 0, ctx->stream,
                           A);
      td_scanned += m_f;
      ++td_levels;
    } else {
      BfsBuArgs A;
      A.row_ptr = row_ptr;
      A.col = col;
      const int64_t goff = mgx_fill_sections(g->bins_sym, &A.bins);
      A.visited = visited;
      A.fcur = fcur;
      A.fnext = fnext;
      A.hops = hops;
      A.parent = parent;
      A.cnt = d_cnt;
      A.level = (int32_t)level;
      if (goff > 0)
        hipLaunchKernelGGL(k_bfs_bottom_up, dim3((uint32_t)goff), dim3(kBlock), 0, ctx->stream,
                           A);
      // No queue describes the old frontier: clear its whole bitmap.
      MGX_HIP_TRY(hipMemsetAsync(fcur, 0, W * sizeof(uint32_t), ctx->stream));
      have_queue = false;
      ++bu_levels;
      if (level < 64) bu_mask |= 1ull << level;
    }

    BfsCounters nh;
    MGX_TRY(read_counters(&nh));
    if (!bottom_up) {
      BfsFinishArgs F;
      F.q01 = q01;
      F.q23 = q23;
      F.V = V;
      int64_t work = 0;
      for (int c = 0; c < 4; ++c) {
        F.old_start[c] = q_start[c];
        F.old_end[c] = q_end[c];
        F.new_end[c] = nh.tail[c];
        work += (int64_t)nh.tail[c] - q_start[c];
        q_start[c] = q_end[c];
        q_end[c] = nh.tail[c];
      }
      F.visited = visited;
      F.fold = fcur;
      hipLaunchKernelGGL(k_bfs_td_finish, dim3((uint32_t)grid_for(work, kGridCap)), dim3(kBlock), 0,
                         ctx->stream, F);
    }
    std::swap(fcur, fnext);

    prev_n_f = n_f;
    n_f = (int64_t)(nh.reached - h.reached);
    m_f = (int64_t)(nh.degsum - h.degsum);
    m_u -= m_f;
    h = nh;
    ++level;
    if (n_f > 0) depth = level;
  }

  MGX_HIP_TRY(hipEventRecord(ev1, ctx->stream));
  MGX_HIP_TRY(hipEventSynchronize(ev1));
  float ms = 0.f;
  MGX_HIP_TRY(hipEventElapsedTime(&ms, ev0, ev1));
  MGX_HIP_TRY(hipEventDestroy(ev0));
  MGX_HIP_TRY(hipEventDestroy(ev1));
  if (stats) {
    stats->depth = depth;
    stats->reached = (int64_t)h.reached;
    stats->entries_scanned = td_scanned + (int64_t)h.scanned;
    stats->top_down_levels = td_levels;
    stats->bottom_up_levels = bu_levels;
    stats->bottom_up_mask = bu_mask;
    stats->ms = ms;
  }
  MGX_HIP_TRY(hipGetLastError());
  return MGX_OK;
}

mgx_status mgx_bfs_impl(mgx_context *ctx, mgx_graph *g, int64_t source, int directed,
                        int64_t max_depth, int mode, int64_t *out_hops, int64_t *out_parent,
                        mgx_bfs_stats *stats) {
  MGX_TRY(bfs_check_args(g, directed, mode));
  const int64_t V = g->n_vertices;
  if (source < 0 || source >= V) {
    mgx_set_error("bfs: source %lld outside [0,%lld)", (long long)source, (long long)V);
    return MGX_ERR_INVALID_ARGUMENT;
  }
  mgx_scope bufs(ctx);
  int32_t *hops = nullptr, *parent = nullptr;
  MGX_TRY(bufs.alloc(&hops, V));
  if (out_parent) MGX_TRY(bufs.alloc(&parent, V));
  MGX_TRY(mgx_bfs_device(ctx, g, nullptr, 1, (int32_t)source, directed, max_depth, mode, hops,
                         parent, stats));

  int64_t *d_out_hops = nullptr, *d_out_parent = nullptr;
  if (out_hops) MGX_TRY(bufs.alloc(&d_out_hops, V));
  if (out_parent) MGX_TRY(bufs.alloc(&d_out_parent, V));
  if (out_hops || out_parent) {
    hipLaunchKernelGGL(k_bfs_emit, dim3((uint32_t)grid_for(V, kGridCap)), dim3(kBlock), 0,
                       ctx->stream, V, hops, parent, d_out_hops, d_out_parent);
    if (out_hops)
      MGX_HIP_TRY(hipMemcpyAsync(out_hops, d_out_hops, V * sizeof(int64_t),
                                 hipMemcpyDeviceToHost, ctx->stream));
    if (out_parent)
      MGX_HIP_TRY(hipMemcpyAsync(out_parent, d_out_parent, V * sizeof(int64_t),
                                 hipMemcpyDeviceToHost, ctx->stream));
  }
  MGX_HIP_TRY(hipStreamSynchronize(ctx->stream));
  MGX_HIP_TRY(hipGetLastError());
  return MGX_OK;
}
