// Node similarity on gfx950: Jaccard and overlap of out-neighbour sets.
// Replaces JaccardFunc / OverlapFunc (node_similarity.hpp:43-68) over the
// sets of GetNeighbors (:107-121), for explicit pairs
// (CalculateSimilarityPairwise, :126-158) and for every pair i < j
// (CalculateSimilarityCartesian, :163-200). The reference rebuilds
// std::set_intersection / std::set_union into fresh std::sets per pair;
// here a pair costs one sorted-set intersection count and one fp64 division.
//
// State:
//   distinct view   uniq_row_ptr[V+1], uniq_col: the out-CSR with repeated
//                   (src, dst) dropped, cached on mgx_graph at the first
//                   call; an alias of the out-CSR when nothing was dropped.
//   pairs           pu, pv (int32), per-pair [lo, hi) = the shorter row's
//                   range for the search pairs and for the merge pairs
//                   (0-length in the list a pair does not belong to), one
//                   mgx_bins over each, common (int64) and sim (fp64).
//   all-pairs       a staging buffer of whole result rows i, at most
//                   MGX_SIM_CHUNK_PAIRS (default 2^27 = 1 GiB) entries,
//                   downloaded chunk by chunk.
//
// A pair is a "row" whose degree is the shorter of its two distinct rows,
// binned into the four lane classes of mgx_bins (4/16/64 lanes or one
// 256-thread workgroup) and swept under for_bin_section.
//   SEARCH  lanes stride over the shorter row (coalesced) and each binary
//           searches the longer row: s * ceil(log2(l+1)) probes.
//   MERGE   one wave per pair (one workgroup when the shorter row has
//           >= 1024 entries) walks both rows in tiles of one element per
//           lane; the A-tile is counted inside the B-tile, then the tile
//           whose last element is smaller advances (both on equality):
//           s + l loads, all coalesced. Rows are strictly increasing and
//           tiles are disjoint, so a common element is counted exactly once:
//           while its A-tile is current every B-tile before its B-tile ends
//           below it and is the one that advances.
//   AUTO    per pair SEARCH when s * ceil(log2(l+1)) < s + l, else MERGE:
//           the operation counts above, not tuned against any graph.
// All-pairs (V <= 65536, so a row's neighbour bitmap is <= 8 KiB): a
// workgroup stages the bitmaps of kTile consecutive rows i in LDS and
// streams every row j above the tile's first row through sub-wave groups by
// j's lane class; a bit test replaces the search and each streamed row is
// used kTile times.

#include <algorithm>
#include <climits>
#include <cstdlib>
#include <cstring>
#include <vector>

#include <rocprim/rocprim.hpp>

#include "mgx_device.h"

namespace {

constexpr int64_t kGridCap = 2048;  // element-wise launches of this file
// All-pairs tile: kTile bitmaps of ceil(V/32) words, interleaved by word.
// At V = 65536 that is 8 * 8 KiB = 64 KiB of the CU's 160 KiB LDS: two
// workgroups (8 waves, 2 per SIMD) stay resident per CU. Smaller V takes
// proportionally less and is bounded by waves, not LDS.
constexpr int kTile = 8;
constexpr int64_t kMaxAllVertices = 65536;  // V(V-1)/2 < 2^31
constexpr int64_t kDefaultChunkPairs = 1ll << 27;  // 1 GiB of fp64

// ---- distinct view ---------------------------------------------------------

__global__ void k_flag_new(int64_t n, const int32_t *col, uint32_t *flag) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    flag[i] = (i == 0 || col[i] != col[i - 1]) ? 1u : 0u;
}

// The first entry of a non-empty row is always kept.
__global__ void k_flag_row_start(int64_t V, const uint32_t *row_ptr, uint32_t *flag) {
  for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < V;
       r += (int64_t)gridDim.x * blockDim.x)
    if (row_ptr[r] < row_ptr[r + 1]) flag[row_ptr[r]] = 1u;
}

__global__ void k_compact(int64_t n, const int32_t *col, const uint32_t *flag,
                          const uint32_t *pos, int32_t *out) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    if (flag[i]) out[pos[i]] = col[i];
}

// pos[row_ptr[r]] kept entries precede row r; rows at the end of the CSR
// (row_ptr[r] == n) start at the total.
__global__ void k_uniq_row_ptr(int64_t V, int64_t n, uint32_t total, const uint32_t *row_ptr,
                               const uint32_t *pos, uint32_t *out) {
  for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r <= V;
       r += (int64_t)gridDim.x * blockDim.x) {
    const uint32_t s = row_ptr[r];
    out[r] = s < n ? pos[s] : total;
  }
}

mgx_status build_distinct_view(mgx_context *ctx, mgx_graph *g) {
  if (g->uniq_row_ptr) return MGX_OK;
  const int64_t V = g->n_vertices, E = g->n_edges;
  if (E == 0) {
    g->uniq_row_ptr = g->out_row_ptr;
    g->uniq_col = g->out_col;
    g->uniq_entries = 0;
    g->uniq_alias = true;
    return MGX_OK;
  }
  mgx_scope bufs(ctx);
  uint32_t *flag = nullptr, *pos = nullptr;
  MGX_TRY(bufs.alloc(&flag, E));
  MGX_TRY(bufs.alloc(&pos, E));
  hipLaunchKernelGGL(k_flag_new, dim3((uint32_t)grid_for(E, kGridCap)), dim3(kBlock), 0,
                     ctx->stream, E, g->out_col, flag);
  hipLaunchKernelGGL(k_flag_row_start, dim3((uint32_t)grid_for(V, kGridCap)), dim3(kBlock), 0,
                     ctx->stream, V, g->out_row_ptr, flag);
  MGX_TRY(mgx_with_temp(ctx, "distinct-view scan", [&](void *tmp, size_t &bytes) {
    return rocprim::exclusive_scan(tmp, bytes, flag, pos, 0u, E, rocprim::plus<uint32_t>(),
                                   ctx->stream);
  }));
  uint32_t last_pos = 0, last_flag = 0;
  MGX_HIP_TRY(hipMemcpyAsync(&last_pos, pos + E - 1, 4, hipMemcpyDeviceToHost, ctx->stream));
  MGX_HIP_TRY(hipMemcpyAsync(&last_flag, flag + E - 1, 4, hipMemcpyDeviceToHost, ctx->stream));
  MGX_HIP_TRY(hipStreamSynchronize(ctx->stream));
  const int64_t total = (int64_t)last_pos + last_flag;
  if (total == E) {
    g->uniq_row_ptr = g->out_row_ptr;
    g->uniq_col = g->out_col;
    g->uniq_alias = true;
  } else {
    uint32_t *rp = nullptr;
    int32_t *uc = nullptr;
    MGX_TRY(bufs.alloc_plain(&rp, V + 1));
    MGX_TRY(bufs.alloc_plain(&uc, total));
    hipLaunchKernelGGL(k_compact, dim3((uint32_t)grid_for(E, kGridCap)), dim3(kBlock), 0,
                       ctx->stream, E, g->out_col, flag, pos, uc);
    hipLaunchKernelGGL(k_uniq_row_ptr, dim3((uint32_t)grid_for(V + 1, kGridCap)), dim3(kBlock),
                       0, ctx->stream, V, E, (uint32_t)total, g->out_row_ptr, pos, rp);
    g->uniq_row_ptr = bufs.give_up(rp);
    g->uniq_col = bufs.give_up(uc);
    g->uniq_alias = false;
  }
  g->uniq_entries = total;
  MGX_HIP_TRY(hipGetLastError());
  return MGX_OK;
}

// ---- shared device pieces ---------------------------------------------------

// ceil(log2(l + 1)) = the bit length of l.
__device__ inline uint32_t bit_length(uint32_t l) { return l ? 32u - (uint32_t)__clz(l) : 0u; }

__device__ inline double quotient(int metric, int64_t common, int64_t da, int64_t db) {
  const int64_t denom = metric == MGX_SIM_JACCARD ? da + db - common : (da < db ? da : db);
  return denom > 0 ? (double)common / (double)denom : 0.0;
}

struct PairArgs {
  const uint32_t *row_ptr;
  const int32_t *col;
  const int32_t *pu, *pv;
  int metric;
  mgx_bin_sections bins;
  int64_t *common;
  double *sim;
};

// The pair's rows as (shorter, longer) CSR ranges; ties keep u first.
struct PairRows {
  uint32_t ss, se, ls, le;
};

__device__ inline PairRows pair_rows(const PairArgs &A, int32_t p) {
  const int32_t u = A.pu[p], v = A.pv[p];
  const uint32_t us = A.row_ptr[u], ue = A.row_ptr[u + 1];
  const uint32_t vs = A.row_ptr[v], ve = A.row_ptr[v + 1];
  PairRows r;
  if (ue - us <= ve - vs) r = {us, ue, vs, ve};
  else r = {vs, ve, us, ue};
  return r;
}

__device__ inline void pair_finish(const PairArgs &A, int32_t p, const PairRows &r,
                                   uint32_t common) {
  A.common[p] = common;
  A.sim[p] = quotient(A.metric, common, r.se - r.ss, r.le - r.ls);
}

// ---- SEARCH ------------------------------------------------------------------

template <int LANES>
__device__ inline void search_rows(const PairArgs &A, int sec, int64_t block_in_sec) {
  reduce_bin_rows<LANES>(
      A.bins, sec, block_in_sec, 0u, mgx_op_add{},
      [&](int32_t p, int sub) {
        const PairRows r = pair_rows(A, p);
        uint32_t hits = 0;
        for (uint32_t j = r.ss + sub; j < r.se; j += LANES) {
          const int32_t x = A.col[j];
          // lower bound of x in the longer row
          uint32_t s = r.ls, e = r.le;
          while (s < e) {
            const uint32_t m = s + ((e - s) >> 1);
            if (A.col[m] < x) s = m + 1;
            else e = m;
          }
          if (s < r.le && A.col[s] == x) ++hits;
        }
        return hits;
      },
      [&](int32_t p, uint32_t hits) { pair_finish(A, p, pair_rows(A, p), hits); });
}

__global__ void __launch_bounds__(kBlock) k_sim_search(PairArgs A) {
  for_bin_section(A.bins.goff, [&](auto lanes, int sec, int64_t bis) {
    search_rows<decltype(lanes)::value>(A, sec, bis);
  });
}

// ---- MERGE -------------------------------------------------------------------

// Position of the first element >= x among the 64 values b held one per lane
// (increasing, padded with INT32_MAX), capped at 63. All 64 lanes call it.
__device__ inline int wave_lower_bound(int32_t b, int32_t x) {
  int pos = 0;
  for (int step = 32; step; step >>= 1) {
    const int32_t bv = __shfl(b, pos + step - 1, 64);
    if (bv < x) pos += step;
  }
  return pos;
}

// One wave per pair: 64-element tiles, the B-tile searched through shuffles.
__device__ inline void merge_wave_rows(const PairArgs &A, int sec, int64_t block_in_sec) {
  for_bin_row_steps<64>(A.bins, sec, block_in_sec, [&](const int32_t *pp, bool live, int sub) {
    if (!live) return;  // whole waves: a wave's 64 lanes share one pair
    const int32_t p = *pp;
    const PairRows r = pair_rows(A, p);
    uint32_t ia = r.ss, ib = r.ls, hits = 0;
    while (ia < r.se && ib < r.le) {
      const uint32_t na = min(64u, r.se - ia), nb = min(64u, r.le - ib);
      const int32_t a = (uint32_t)sub < na ? A.col[ia + sub] : -1;
      const int32_t b = (uint32_t)sub < nb ? A.col[ib + sub] : INT32_MAX;
      const int pos = wave_lower_bound(b, a);
      const int32_t at = __shfl(b, pos, 64);
      if ((uint32_t)sub < na && at == a) ++hits;
      const int32_t a_last = A.col[ia + na - 1], b_last = A.col[ib + nb - 1];
      if (a_last <= b_last) ia += na;
      if (b_last <= a_last) ib += nb;
    }
    hits = row_reduce<64>(hits, mgx_op_add{});
    if (sub == 0) pair_finish(A, p, r, hits);
  });
}

// One workgroup per pair: 256-element tiles, the B-tile staged in LDS.
__device__ inline void merge_block_rows(const PairArgs &A, int sec, int64_t block_in_sec) {
  __shared__ int32_t s_b[kBlock];
  for_bin_row_steps<kBlock>(A.bins, sec, block_in_sec,
                            [&](const int32_t *pp, bool live, int sub) {
    if (!live) return;  // one pair per block: uniform
    const int32_t p = *pp;
    const PairRows r = pair_rows(A, p);
    uint32_t ia = r.ss, ib = r.ls, hits = 0;
    while (ia < r.se && ib < r.le) {
      const uint32_t na = min((uint32_t)kBlock, r.se - ia), nb = min((uint32_t)kBlock, r.le - ib);
      s_b[sub] = (uint32_t)sub < nb ? A.col[ib + sub] : INT32_MAX;
      __syncthreads();
      if ((uint32_t)sub < na) {
        const int32_t a = A.col[ia + sub];
        int pos = 0;
        for (int step = kBlock / 2; step; step >>= 1)
          if (s_b[pos + step - 1] < a) pos += step;
        if (s_b[pos] == a) ++hits;
      }
      const int32_t a_last = A.col[ia + na - 1], b_last = s_b[nb - 1];
      __syncthreads();  // s_b is rewritten by the next tile
      if (a_last <= b_last) ia += na;
      if (b_last <= a_last) ib += nb;
    }
    hits = row_reduce<kBlock>(hits, mgx_op_add{});
    if (sub == 0) pair_finish(A, p, r, hits);
    __syncthreads();  // row_reduce's slots are reused
  });
}

__global__ void __launch_bounds__(kBlock) k_sim_merge(PairArgs A) {
  for_bin_section(A.bins.goff, [&](auto lanes, int sec, int64_t bis) {
    if constexpr (decltype(lanes)::value == kBlock) merge_block_rows(A, sec, bis);
    else merge_wave_rows(A, sec, bis);
  });
}

// ---- pair classification -----------------------------------------------------

// Per pair the shorter row's [lo, hi) goes to the search list or to the
// merge list; the other list gets an empty range, which the binning drops.
__global__ void k_pair_ranges(int64_t n, const uint32_t *row_ptr, const int32_t *pu,
                              const int32_t *pv, int mode, uint32_t *lo_s, uint32_t *hi_s,
                              uint32_t *lo_m, uint32_t *hi_m) {
  for (int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; p < n;
       p += (int64_t)gridDim.x * blockDim.x) {
    const int32_t u = pu[p], v = pv[p];
    const uint32_t du = row_ptr[u + 1] - row_ptr[u], dv = row_ptr[v + 1] - row_ptr[v];
    const uint32_t s = min(du, dv), l = max(du, dv);
    const uint32_t lo = du <= dv ? row_ptr[u] : row_ptr[v];
    bool search = mode == MGX_SIM_SEARCH;
    if (mode == MGX_SIM_AUTO)
      search = (uint64_t)s * bit_length(l) < (uint64_t)s + (uint64_t)l;
    if (lo_s) {
      lo_s[p] = lo;
      hi_s[p] = search ? lo + s : lo;
    }
    if (lo_m) {
      lo_m[p] = lo;
      hi_m[p] = search ? lo : lo + s;
    }
  }
}

// ---- all pairs ----------------------------------------------------------------

struct AllArgs {
  const uint32_t *row_ptr;
  const int32_t *col;
  mgx_bin_sections bins;  // rows of the distinct view with entries
  int64_t V;
  int32_t W;              // bitmap words per row
  int64_t r0, r1;         // this launch writes result rows [r0, r1)
  int64_t base;           // all-pairs index of pair (r0, r0 + 1)
  int metric;
  double *out;            // staging: pair (i, j) at index(i, j) - base
};

// Stream the rows j > i0 of section `sec` against the staged tile, LANES
// lanes per row (the 256-lane class is taken by single waves here).
template <int LANES>
__device__ inline void all_stream(const AllArgs &A, int sec, const uint32_t *bm, int64_t i0,
                                  int nt, const uint32_t (&deg_i)[kTile]) {
  constexpr int RPB = kBlock / LANES;
  const int32_t *rows = A.bins.rows + A.bins.off[sec];
  const int64_t n = A.bins.n[sec];
  const int sub = threadIdx.x % LANES;
  // rows are ascending within a section: first row above i0
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t m = lo + ((hi - lo) >> 1);
    if (rows[m] <= i0) lo = m + 1;
    else hi = m;
  }
  for (int64_t base = lo; base < n; base += RPB) {
    const int64_t ri = base + threadIdx.x / LANES;
    const bool live = ri < n;
    uint32_t cnt[kTile];
#pragma unroll
    for (int t = 0; t < kTile; ++t) cnt[t] = 0;
    int64_t j = 0;
    uint32_t s = 0, e = 0;
    if (live) {
      j = rows[ri];
      s = A.row_ptr[j];
      e = A.row_ptr[j + 1];
    }
    for (uint32_t k = s + sub; k < e; k += LANES) {
      const uint32_t c = (uint32_t)A.col[k];
      const uint32_t *w = bm + (size_t)(c >> 5) * kTile;
      const uint32_t sh = c & 31u;
#pragma unroll
      for (int t = 0; t < kTile; ++t) cnt[t] += (w[t] >> sh) & 1u;
    }
#pragma unroll
    for (int t = 0; t < kTile; ++t) cnt[t] = row_reduce<LANES>(cnt[t], mgx_op_add{});
    if (live && sub == 0) {
      const uint32_t dj = e - s;
#pragma unroll
      for (int t = 0; t < kTile; ++t) {
        const int64_t i = i0 + t;
        if (t < nt && i < j) {
          const int64_t idx = i * (2 * A.V - i - 1) / 2 + (j - i - 1) - A.base;
          A.out[idx] = quotient(A.metric, cnt[t], deg_i[t], dj);
        }
      }
    }
  }
}

__global__ void __launch_bounds__(kBlock) k_sim_all(AllArgs A) {
  extern __shared__ uint32_t bm[];  // [W][kTile]: word w of tile row t at w * kTile + t
  const int64_t i0 = A.r0 + (int64_t)blockIdx.x * kTile;
  const int nt = (int)min((int64_t)kTile, A.r1 - i0);
  for (int k = threadIdx.x; k < A.W * kTile; k += kBlock) bm[k] = 0u;
  __syncthreads();
  uint32_t deg_i[kTile];
#pragma unroll
  for (int t = 0; t < kTile; ++t) {
    deg_i[t] = 0;
    if (t < nt) {
      const uint32_t s = A.row_ptr[i0 + t], e = A.row_ptr[i0 + t + 1];
      deg_i[t] = e - s;
      for (uint32_t k = s + threadIdx.x; k < e; k += kBlock) {
        const uint32_t c = (uint32_t)A.col[k];
        atomicOr(&bm[(size_t)(c >> 5) * kTile + t], 1u << (c & 31u));
      }
    }
  }
  __syncthreads();
  all_stream<4>(A, 0, bm, i0, nt, deg_i);
  all_stream<16>(A, 1, bm, i0, nt, deg_i);
  all_stream<64>(A, 2, bm, i0, nt, deg_i);
  all_stream<64>(A, 3, bm, i0, nt, deg_i);
}

int64_t env_positive(const char *name, int64_t dflt) {
  const char *env = getenv(name);
  if (env && atoll(env) > 0) return atoll(env);
  return dflt;
}

mgx_status check_common(mgx_graph *g, int metric) {
  if (!(g->flags & MGX_BUILD_OUT_CSR)) {
    mgx_set_error("similarity needs a graph built with MGX_BUILD_OUT_CSR");
    return MGX_ERR_INVALID_ARGUMENT;
  }
  if (metric != MGX_SIM_JACCARD && metric != MGX_SIM_OVERLAP) {
    mgx_set_error("similarity: unknown metric %d", metric);
    return MGX_ERR_INVALID_ARGUMENT;
  }
  return MGX_OK;
}

struct Timer {
  hipEvent_t a = nullptr, b = nullptr;
  mgx_status init() {
    MGX_HIP_TRY(hipEventCreate(&a));
    MGX_HIP_TRY(hipEventCreate(&b));
    return MGX_OK;
  }
  ~Timer() {
    if (a) (void)hipEventDestroy(a);
    if (b) (void)hipEventDestroy(b);
  }
  // both events recorded and the stream synchronized
  mgx_status ms(double *out) {
    float f = 0.f;
    MGX_HIP_TRY(hipEventElapsedTime(&f, a, b));
    *out = f;
    return MGX_OK;
  }
};

}  // namespace

mgx_status mgx_similarity_pairs_impl(mgx_context *ctx, mgx_graph *g, int metric, int mode,
                                     const int64_t *u, const int64_t *v, int64_t n_pairs,
                                     double *out_sim, int64_t *out_common,
                                     mgx_similarity_stats *stats) {
  MGX_TRY(check_common(g, metric));
  if (mode != MGX_SIM_AUTO && mode != MGX_SIM_SEARCH && mode != MGX_SIM_MERGE) {
    mgx_set_error("similarity: unknown mode %d", mode);
    return MGX_ERR_INVALID_ARGUMENT;
  }
  if (n_pairs < 0) {
    mgx_set_error("similarity: negative pair count");
    return MGX_ERR_INVALID_ARGUMENT;
  }
  if (n_pairs >= (1ll << 31)) {
    mgx_set_error("similarity: %lld pairs exceed int32 pair indices", (long long)n_pairs);
    return MGX_ERR_TOO_LARGE;
  }
  const int64_t V = g->n_vertices;
  std::vector<int32_t> h_uv((size_t)2 * n_pairs);
  for (int64_t p = 0; p < n_pairs; ++p) {
    if (u[p] < 0 || u[p] >= V || v[p] < 0 || v[p] >= V) {
      mgx_set_error("similarity: pair %lld (%lld, %lld) outside [0,%lld)", (long long)p,
                    (long long)u[p], (long long)v[p], (long long)V);
      return MGX_ERR_INVALID_ARGUMENT;
    }
    h_uv[p] = (int32_t)u[p];
    h_uv[n_pairs + p] = (int32_t)v[p];
  }
  if (stats) *stats = mgx_similarity_stats{};
  if (n_pairs == 0) {
    if (stats) stats->distinct_entries = g->uniq_row_ptr ? g->uniq_entries : 0;
    return MGX_OK;
  }

  Timer prep, run;
  MGX_TRY(prep.init());
  MGX_TRY(run.init());
  MGX_HIP_TRY(hipEventRecord(prep.a, ctx->stream));
  MGX_TRY(build_distinct_view(ctx, g));

  const int64_t n = n_pairs;
  const bool want_s = mode != MGX_SIM_MERGE, want_m = mode != MGX_SIM_SEARCH;
  int32_t *d_uv = nullptr;
  uint32_t *lo_s = nullptr, *hi_s = nullptr, *lo_m = nullptr, *hi_m = nullptr;
  int64_t *d_common = nullptr;
  double *d_sim = nullptr;
  mgx_scope bufs(ctx);
  MGX_TRY(bufs.alloc(&d_uv, 2 * n));
  if (want_s) {
    MGX_TRY(bufs.alloc(&lo_s, n));
    MGX_TRY(bufs.alloc(&hi_s, n));
  }
  if (want_m) {
    MGX_TRY(bufs.alloc(&lo_m, n));
    MGX_TRY(bufs.alloc(&hi_m, n));
  }
  MGX_TRY(bufs.alloc(&d_common, n));
  MGX_TRY(bufs.alloc(&d_sim, n));
  MGX_HIP_TRY(hipMemcpyAsync(d_uv, h_uv.data(), 2 * n * sizeof(int32_t), hipMemcpyHostToDevice,
                             ctx->stream));
  // Pairs with an empty shorter row are dropped by the binning: their
  // common count and quotient are the zeros written here.
  MGX_HIP_TRY(hipMemsetAsync(d_common, 0, n * sizeof(int64_t), ctx->stream));
  MGX_HIP_TRY(hipMemsetAsync(d_sim, 0, n * sizeof(double), ctx->stream));
  hipLaunchKernelGGL(k_pair_ranges, dim3((uint32_t)grid_for(n, kGridCap)), dim3(kBlock), 0,
                     ctx->stream, n, g->uniq_row_ptr, d_uv, d_uv + n, mode, lo_s, hi_s, lo_m,
                     hi_m);
  mgx_bins bins_s, bins_m;
  if (want_s)
    MGX_TRY(mgx_build_bins_range(bufs, lo_s, hi_s, n, /*include_zero=*/false, &bins_s));
  if (want_m)
    MGX_TRY(mgx_build_bins_range(bufs, lo_m, hi_m, n, /*include_zero=*/false, &bins_m));
  MGX_HIP_TRY(hipEventRecord(prep.b, ctx->stream));

  PairArgs A;
  A.row_ptr = g->uniq_row_ptr;
  A.col = g->uniq_col;
  A.pu = d_uv;
  A.pv = d_uv + n;
  A.metric = metric;
  A.common = d_common;
  A.sim = d_sim;
  MGX_HIP_TRY(hipEventRecord(run.a, ctx->stream));
  if (want_s) {
    const int64_t grid = mgx_fill_sections(bins_s, &A.bins);
    if (grid > 0)
      hipLaunchKernelGGL(k_sim_search, dim3((uint32_t)grid), dim3(kBlock), 0, ctx->stream, A);
  }
  if (want_m) {
    const int64_t grid = mgx_fill_sections(bins_m, &A.bins);
    if (grid > 0)
      hipLaunchKernelGGL(k_sim_merge, dim3((uint32_t)grid), dim3(kBlock), 0, ctx->stream, A);
  }
  MGX_HIP_TRY(hipEventRecord(run.b, ctx->stream));

  MGX_HIP_TRY(hipMemcpyAsync(out_sim, d_sim, n * sizeof(double), hipMemcpyDeviceToHost,
                             ctx->stream));
  if (out_common)
    MGX_HIP_TRY(hipMemcpyAsync(out_common, d_common, n * sizeof(int64_t),
                               hipMemcpyDeviceToHost, ctx->stream));
  MGX_HIP_TRY(hipStreamSynchronize(ctx->stream));
  if (stats) {
    stats->pairs = n;
    for (int b = 0; b < 4; ++b) {
      stats->search_pairs += bins_s.count[b];
      stats->merge_pairs += bins_m.count[b];
    }
    stats->distinct_entries = g->uniq_entries;
    MGX_TRY(prep.ms(&stats->prep_ms));
    MGX_TRY(run.ms(&stats->ms));
  }
  MGX_HIP_TRY(hipGetLastError());
  return MGX_OK;
}

mgx_status mgx_similarity_all_impl(mgx_context *ctx, mgx_graph *g, int metric, double *out_sim,
                                   mgx_similarity_stats *stats) {
  MGX_TRY(check_common(g, metric));
  const int64_t V = g->n_vertices;
  if (V > kMaxAllVertices) {
    mgx_set_error("similarity_all: V=%lld gives >= 2^31 pairs", (long long)V);
    return MGX_ERR_TOO_LARGE;
  }
  if (stats) *stats = mgx_similarity_stats{};
  const int64_t total = V * (V - 1) / 2;
  if (total == 0) return MGX_OK;

  Timer prep, run;
  MGX_TRY(prep.init());
  MGX_TRY(run.init());
  MGX_HIP_TRY(hipEventRecord(prep.a, ctx->stream));
  MGX_TRY(build_distinct_view(ctx, g));
  if (!g->uniq_bins_built) {
    MGX_TRY(mgx_build_bins_range(ctx, g->uniq_row_ptr, g->uniq_row_ptr + 1, V,
                                 /*include_zero=*/false, &g->uniq_bins));
    g->uniq_bins_built = true;
  }
  // Whole result rows per chunk; a chunk always holds at least one row.
  const int64_t cap = std::max(env_positive("MGX_SIM_CHUNK_PAIRS", kDefaultChunkPairs), V - 1);
  const int64_t staging_pairs = std::min(cap, total);
  double *d_out = nullptr;
  mgx_scope bufs(ctx);
  MGX_TRY(bufs.alloc(&d_out, staging_pairs));
  MGX_HIP_TRY(hipEventRecord(prep.b, ctx->stream));

  AllArgs A;
  A.row_ptr = g->uniq_row_ptr;
  A.col = g->uniq_col;
  mgx_fill_sections(g->uniq_bins, &A.bins);
  A.V = V;
  A.W = (int32_t)((V + 31) / 32);
  A.metric = metric;
  A.out = d_out;
  const size_t lds = (size_t)A.W * kTile * sizeof(uint32_t);  // <= 64 KiB
  MGX_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k_sim_all),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));

  auto row_base = [&](int64_t i) { return i * (2 * V - i - 1) / 2; };
  double ms_acc = 0.0;
  int64_t chunks = 0;
  for (int64_t r0 = 0; r0 < V - 1;) {
    int64_t r1 = r0 + 1;  // rows [r0, r1): as many whole rows as fit
    while (r1 < V - 1 && row_base(r1 + 1) - row_base(r0) <= cap) ++r1;
    const int64_t n = row_base(r1) - row_base(r0);
    A.r0 = r0;
    A.r1 = r1;
    A.base = row_base(r0);
    MGX_HIP_TRY(hipEventRecord(run.a, ctx->stream));
    // Rows without entries are not streamed: their pairs are these zeros.
    MGX_HIP_TRY(hipMemsetAsync(d_out, 0, n * sizeof(double), ctx->stream));
    const int64_t tiles = (r1 - r0 + kTile - 1) / kTile;
    hipLaunchKernelGGL(k_sim_all, dim3((uint32_t)tiles), dim3(kBlock), lds, ctx->stream, A);
    MGX_HIP_TRY(hipEventRecord(run.b, ctx->stream));
    MGX_HIP_TRY(hipMemcpyAsync(out_sim + A.base, d_out, n * sizeof(double),
                               hipMemcpyDeviceToHost, ctx->stream));
    MGX_HIP_TRY(hipStreamSynchronize(ctx->stream));
    double ms = 0.0;
    MGX_TRY(run.ms(&ms));
    ms_acc += ms;
    ++chunks;
    r0 = r1;
  }
  if (stats) {
    stats->pairs = total;
    stats->distinct_entries = g->uniq_entries;
    stats->chunks = chunks;
    stats->ms = ms_acc;
    MGX_TRY(prep.ms(&stats->prep_ms));
  }
  MGX_HIP_TRY(hipGetLastError());
  return MGX_OK;
}
