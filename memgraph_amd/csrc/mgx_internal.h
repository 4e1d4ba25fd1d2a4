// Internal structures of libmgx_analytics (gfx950-only HIP).
#ifndef MGX_INTERNAL_H
#define MGX_INTERNAL_H

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <map>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/mgx_analytics.h"

// Set per-thread error detail and return a status.
void mgx_set_error(const char *fmt, ...);

#define MGX_HIP_TRY(expr)                                                     \
  do {                                                                        \
    hipError_t _e = (expr);                                                   \
    if (_e != hipSuccess) {                                                   \
      mgx_set_error("%s:%d: %s failed: %s", __FILE__, __LINE__, #expr,        \
                    hipGetErrorString(_e));                                   \
      (void)hipGetLastError(); /* consume the sticky per-thread error so a  \
                                  later rocprim dispatch doesn't inherit it */ \
      return MGX_ERR_HIP;                                                     \
    }                                                                         \
  } while (0)

#define MGX_TRY(expr)                                                         \
  do {                                                                        \
    mgx_status _s = (expr);                                                   \
    if (_s != MGX_OK) return _s;                                              \
  } while (0)

struct mgx_comm_state;  // comm.cpp (RCCL)

// The box's ROCm 7.0.x runtime mis-reserves plain hipMalloc requests that
// are >4 GiB and NOT a multiple of 2^32 bytes: the returned range overlaps
// live allocations and writing past the low 32 bits of the size faults
// ("write to a read-only page"). Every multi-GB allocation that ever
// worked here was an exact 2^32 multiple (power-of-two element counts);
// the first non-aligned huge malloc (Louvain coarsen's total-sized w at
// RMAT-25) hit the bug. Round such sizes up to the next 2^32 multiple.
inline size_t mgx_safe_size(size_t bytes) {
  if (bytes >= (4ull << 30) && (bytes & 0xFFFFFFFFull) != 0)
    bytes = (bytes + 0xFFFFFFFFull) & ~0xFFFFFFFFull;
  return bytes;
}

template <typename T>
inline hipError_t mgx_hip_malloc(T **p, size_t bytes) {
  return hipMalloc((void **)p, mgx_safe_size(bytes));
}

struct mgx_context {
  int device = -1;
  hipStream_t stream = nullptr;
  // Caching allocator for large transient buffers (sort keys, COO staging):
  // a size-bucketed free list over plain hipMalloc, so repeated multi-GB
  // allocation page-table setup (measured up to ~1 s per RMAT-26 build) is
  // paid once per process. Reuse is safe without syncs because every
  // consumer enqueues on ctx->stream: the previous owner's work precedes
  // the next owner's in stream order.
  //
  // Deliberately NOT hipMallocAsync: on the MI355X box's ROCm 7.0.x runtime
  // a plain hipMalloc issued while the stream-ordered pool holds
  // pending-free-then-reallocated blocks reclaims (and zeroes) the live
  // blocks' pages — measured in the r02 Louvain storm (counts[] nonzero,
  // then hipMalloc(row_ptr), then counts[] all-zero at disjoint VA; see
  // profiles/r02_summary.md). One allocator family avoids the bug class.
  std::mutex cache_mu;
  std::unordered_map<void *, size_t> cache_live;  // ptr -> rounded bytes
  std::multimap<size_t, void *> cache_free;       // rounded bytes -> ptr
  size_t cache_free_bytes = 0;
  mgx_status alloc_async(void **p, size_t bytes);
  mgx_status free_async(void *p);
  void cache_trim();  // hipFree every cached free block
  // Release the cache if a coming plain hipMalloc of `want` bytes would
  // leave the device under the safety margin (see alloc_async).
  void ensure_margin(size_t want);
  // Grow-only device workspace for rocPRIM temp storage etc.
  void *workspace = nullptr;
  size_t workspace_bytes = 0;
  // Louvain coarsen col/w ping-pong arenas. The ROCm 7.0.x runtime
  // misplaces >4 GiB hipMallocs once the VA space is fragmented
  // (profiles/r02_summary.md), and the coarsen's total-sized col/w are
  // the only such allocations issued mid-run — so they come from these
  // grow-only arenas, sized and allocated at mgx_louvain entry before
  // any per-level churn. [2] because level k's graph must stay live
  // while level k+1 is being written.
  void *louv_col[2] = {nullptr, nullptr};
  void *louv_w[2] = {nullptr, nullptr};
  size_t louv_col_bytes[2] = {0, 0};
  size_t louv_w_bytes[2] = {0, 0};
  int louv_flip = 0;
  mgx_comm_state *comm = nullptr;

  mgx_status reserve(size_t bytes, void **out);
};

// Owner of the transient device buffers of a function or block: what it still
// holds when it goes out of scope is released, on every return path (a release
// that fails there is ignored). A count of 0 allocates one element.
struct mgx_scope {
  mgx_context *ctx;
  std::vector<std::pair<void *, bool>> owned;  // block, whether from the cache
  explicit mgx_scope(mgx_context *c) : ctx(c) {}
  mgx_scope(const mgx_scope &) = delete;
  mgx_scope &operator=(const mgx_scope &) = delete;
  ~mgx_scope();
  template <typename T>
  mgx_status alloc(T **p, int64_t count) {  // ctx->alloc_async / free_async
    return take((void **)p, (size_t)(count > 0 ? count : 1) * sizeof(T), true);
  }
  template <typename T>
  mgx_status alloc_plain(T **p, int64_t count) {  // mgx_hip_malloc / hipFree
    return take((void **)p, (size_t)(count > 0 ? count : 1) * sizeof(T), false);
  }
  void release(void *p) { drop(p, true); }  // free p now
  // Stop owning p without freeing it; returns p, for the line that stores it
  // into whatever owns it from then on.
  template <typename T>
  T *give_up(T *p) {
    drop(p, false);
    return p;
  }
  mgx_status take(void **p, size_t bytes, bool cached);
  void drop(void *p, bool free_it);
};

// Test support, not part of the public ABI. Returns how many blocks all the
// scopes of the process own right now, then arms the failure countdown: the
// fail_at-th scope allocation from now on returns MGX_ERR_OUT_OF_MEMORY on
// the host, before any HIP call; -1 disarms it.
extern "C" int64_t mgx_test_scope_hook(int64_t fail_at);
// The same for the persistent arrays of the online modules (mgx_dev_array,
// mgx_online.h). Returns how many blocks they hold right now, then overrides
// the first capacity of every growth site: > 0 replaces it, so that a few
// vertices already make every array grow with live contents; -1 restores the
// sites' own values.
extern "C" int64_t mgx_test_state_hook(int64_t first_cap);
int64_t mgx_state_first_cap(int64_t site_first_cap);  // the override, if one is set
void mgx_state_blocks_add(int64_t delta);

// Degree bins for the fused sweep kernels. Rows are classified by degree;
// within a bin rows are in ascending id order (stable 2-bit radix sort) so
// adjacent lanes read adjacent CSR ranges.
//   bin0: deg < 8     -> 4 lanes/row
//   bin1: 8..63       -> 16 lanes/row
//   bin2: 64..1023    -> 64 lanes (one wave)/row
//   bin3: >= 1024     -> one 256-thread workgroup/row
struct mgx_bins {
  int32_t *rows = nullptr;  // [n_rows] device: bin0 rows, then bin1, ...
  int64_t count[4] = {0, 0, 0, 0};
  // The first n_zero rows of bin0 (counted in count[0]) are the rows of degree
  // 0, when the list includes them: a sweep that has nothing to do for such
  // rows starts bin0 past them.
  int64_t n_zero = 0;
  // Launch geometry (computed host-side at build).
  int64_t grid[4] = {0, 0, 0, 0};
  int64_t total_grid() const { return grid[0] + grid[1] + grid[2] + grid[3]; }
};

// Blocks for `count` rows of bin b: rows-per-block {64,16,4,1}; grid-stride
// caps keep the dispatch bounded (guide G11) while >> 256 CUs stay fed.
inline int64_t mgx_bin_grid(int b, int64_t count) {
  const int64_t rows_per_block[4] = {64, 16, 4, 1};
  const int64_t cap[4] = {2048, 2048, 2048, 8192};
  const int64_t need = (count + rows_per_block[b] - 1) / rows_per_block[b];
  return count ? (need < cap[b] ? need : cap[b]) : 0;
}

struct mgx_graph {
  int64_t n_vertices = 0;
  int64_t n_edges = 0;
  uint32_t flags = 0;

  // in-CSR: row = destination, cols = sources (PageRank/Katz pull).
  // For sharded graphs, rows cover [row_begin, row_end) and in_row_ptr has
  // (row_end - row_begin + 1) entries; in_col holds only owned edges.
  uint32_t *in_row_ptr = nullptr;
  int32_t *in_col = nullptr;
  int64_t in_edges = 0;  // == n_edges unless sharded
  int64_t row_begin = 0, row_end = 0;  // == [0, n_vertices) unless sharded

  // out-degree data (always global, all vertices). When `order` is set,
  // the in-CSR lives in a HOT-FIRST PERMUTED vertex space: vertices are
  // renumbered by descending out-degree so the most-gathered contrib
  // entries pack into the lowest addresses (L2/L3-resident under power-law
  // skew). order[new] = original id; out_degree/inv_outdeg are in the
  // permuted space. Outputs are scattered back to original ids at download.
  // Sharded graphs keep the identity layout (contiguous dst ranges).
  uint32_t *out_degree = nullptr;
  float *inv_outdeg = nullptr;
  int32_t *order = nullptr;  // [V] new -> original, or nullptr (identity)

  // out-CSR (row = source, cols = destinations; identity layout) for
  // directed Brandes BFS.
  uint32_t *out_row_ptr = nullptr;
  int32_t *out_col = nullptr;

  // in-CSR edge weights, built only with MGX_BUILD_NO_PERM|WEIGHTED
  // (directed LabelRankT).
  float *in_w = nullptr;

  // symmetric CSR (WCC/Louvain): each input edge twice.
  uint32_t *sym_row_ptr = nullptr;
  int32_t *sym_col = nullptr;
  float *sym_w = nullptr;  // only with MGX_BUILD_WEIGHTED

  mgx_bins bins_in;   // over in-CSR rows
  mgx_bins bins_sym;  // over sym-CSR rows
  mgx_bins bins_out;  // over out-CSR rows

  // Source-striped in-CSR view (PageRank at large V): cols are sorted
  // within each row, so stripe s of row v is the contiguous sub-range
  // [stripe_ptr[s*rows + v], stripe_ptr[(s+1)*rows + v]) whose sources lie
  // in [s*stripe_width, (s+1)*stripe_width) — the gathered contrib stripe
  // then fits in the Infinity Cache. n_stripes == 1 => unstriped.
  int n_stripes = 1;
  int64_t stripe_width = 0;
  uint32_t *stripe_ptr = nullptr;          // [(n_stripes+1) * rows]
  mgx_bins stripe_bins[16];                // per stripe (max 16)

  // XCD-affine striping (PageRank, permuted single-GPU layout; DESIGN.md
  // lever 4). `order` is the hot-first sort dealt to 8 stripes in 16-vertex
  // granules (mgx_xcd_deal.h), so stripe x is the id range [off[x], off[x+1])
  // and is hot-first inside. Heavy rows (whole in-degree >= xcd_heavy_min:
  // the bins_in sections from xcd_heavy_sec on) are swept in one launch whose
  // block b gathers only stripe b & 7, so each XCD's L2 caches its own eighth
  // of contrib; light rows keep the unstriped sweep. Slot s is heavy row
  // xcd_H[s]; stripe x of it is the col range
  // [xcd_ptr[x*nH + s], xcd_ptr[(x+1)*nH + s]). xcd_bins[x] lists the slots
  // with a non-empty stripe-x segment, binned by segment length.
  bool xcd = false;
  int xcd_heavy_min = 0;
  int xcd_heavy_sec = 4;
  int64_t xcd_nH = 0;
  const int32_t *xcd_H = nullptr;  // [nH], a view into bins_in.rows (not owned)
  uint32_t *xcd_ptr = nullptr;     // [9 * nH]
  mgx_bins xcd_bins[8];
  struct mgx_bin_sections *xcd_sec = nullptr;  // [8] device: xcd_bins as launch sections
  // Stripe-major column stream (lever 6, mgx_xcd_stream.h): the columns of the
  // non-empty segments copied into the order the striped launch reads them,
  // so that each stripe reads one contiguous window and shares no cache line
  // with another. Segment (x, s) is xcd_scol[xcd_slo[x*nH + s] ..
  // xcd_shi[x*nH + s]), the same ids as its in_col range and at the same
  // offset mod 4 where the section's vector body depends on it.
  // xcd_stream_ints is the stream's length, -1 when none was built
  // (MGX_PR_XCD_STREAM=0, or a length past uint32): the launch then reads
  // in_col through xcd_ptr.
  int32_t *xcd_scol = nullptr;
  uint32_t *xcd_slo = nullptr;  // [8 * nH]
  uint32_t *xcd_shi = nullptr;  // [8 * nH]
  int64_t xcd_stream_ints = -1;

  // Deduplicated view of the out-CSR (similarity.hip), built at the first
  // similarity call. When the out-CSR has no repeated (src, dst) both
  // pointers alias out_row_ptr / out_col (uniq_alias) and own nothing.
  // uniq_bins: rows of the view with entries, for the all-pairs sweep.
  uint32_t *uniq_row_ptr = nullptr;
  int32_t *uniq_col = nullptr;
  int64_t uniq_entries = 0;
  bool uniq_alias = false;
  mgx_bins uniq_bins;
  bool uniq_bins_built = false;

  double build_ms = 0.0;
};

// graph_build.hip entry points (device COO is int32).
mgx_status mgx_build_from_device_coo(mgx_context *ctx, const int32_t *d_src,
                                     const int32_t *d_dst, const float *d_w,
                                     int64_t n_vertices, int64_t n_edges, uint32_t flags,
                                     mgx_graph *g);
mgx_status mgx_gen_rmat_device(mgx_context *ctx, int scale, int64_t n_edges, uint64_t seed,
                               double a, double b, double c, int32_t *d_src, int32_t *d_dst);
mgx_status mgx_gen_uniform_device(mgx_context *ctx, int64_t n_vertices, int64_t n_edges,
                                  uint64_t seed, int32_t *d_src, int32_t *d_dst);
mgx_status mgx_gen_weights_device(mgx_context *ctx, int64_t n_edges, uint64_t seed, float *d_w);
// Build the degree-bin work lists for a CSR with `rows` rows.
mgx_status mgx_build_bins(mgx_context *ctx, const uint32_t *row_ptr, int64_t rows,
                          mgx_bins *bins);
// Degree-bin work lists from explicit per-row [lo, hi) ranges; rows with
// zero degree are dropped unless include_zero, and then lead bin0 (n_zero).
mgx_status mgx_build_bins_range(mgx_context *ctx, const uint32_t *lo, const uint32_t *hi,
                                int64_t rows, bool include_zero, mgx_bins *bins);
// The same for a work list that is itself transient: bins->rows belongs to the
// caller's scope `own`.
mgx_status mgx_build_bins_range(mgx_scope &own, const uint32_t *lo, const uint32_t *hi,
                                int64_t rows, bool include_zero, mgx_bins *bins);
// Source-stripe the (sorted) in-CSR of g; n_stripes chosen from V (env
// MGX_PR_STRIPES overrides; 1 = disabled). When g->xcd is set (decided
// before the renumbering, see mgx_xcd_wanted) it builds the heavy-row XCD
// stripe view instead and leaves n_stripes at 1.
mgx_status mgx_build_stripes(mgx_context *ctx, mgx_graph *g);
// Whether a permuted single-GPU build of V vertices takes the XCD-affine
// layout: MGX_PR_XCD=1/0 forces it on/off for any V, MGX_PR_STRIPES set
// disables it, and unset it is on for V >= 1.5 * 2^25 (measured threshold).
bool mgx_xcd_wanted(int64_t n_vertices);

// Sharded in-CSR build: keeps only edges with dst in [row_begin,row_end);
// out_degree stays global.
mgx_status mgx_build_sharded_in_csr(mgx_context *ctx, const int32_t *d_src,
                                    const int32_t *d_dst, int64_t n_vertices,
                                    int64_t n_edges, int64_t row_begin, int64_t row_end,
                                    mgx_graph *g);

// pagerank.hip
struct mgx_pagerank_run {
  mgx_context *ctx = nullptr;
  mgx_graph *g = nullptr;
  double damping = 0.85;
  float *rank[2] = {nullptr, nullptr};     // ping-pong f32 [V]
  float *contrib[2] = {nullptr, nullptr};  // ping-pong f32 [V]
  int cur = 0;
  uint32_t *d_delta = nullptr;  // Linf as ordered-uint f32
  double *d_scratch = nullptr;  // sum + f64 output [V+1]
  // fp64 row partials: [rows] for the sequential striped sweep, [8 * nH]
  // (stripe-major) for the XCD-striped one.
  double *d_partial = nullptr;
  int xcd_grid = 0;  // XCD-striped launch: resident grid, a multiple of 8
  // XCD-striped launch: threads per block, chosen when the run starts
  // (MGX_PR_XCD_BLOCK); 0 when the run has no striped launch.
  int xcd_block = 0;
  // XCD-striped launch: floats of each stripe's hot prefix held in LDS per
  // block (0 = none), chosen when the run starts (MGX_PR_XCD_LDS).
  int64_t xcd_lds_floats = 0;
  // Rows of in-degree 0 leave the sweep from the third iteration on
  // (MGX_PR_SKIP_ZERO=0 keeps them in).
  bool skip_zero = true;
  int64_t iterations = 0;
  // HIP-event timing of the sweep kernel (the dominant kernel).
  std::vector<hipEvent_t> ev_start, ev_stop;
  int64_t ev_used = 0;
  double sweep_ms_acc = 0.0;
  int64_t launches_acc = 0;
  // distributed
  bool dist = false;
  int64_t row_begin = 0, row_end = 0;

  mgx_status flush_timing();  // sync + fold events into sweep_ms_acc
};

mgx_status mgx_pagerank_queue_iterations(mgx_pagerank_run *run, int64_t n, bool track_delta);
mgx_status mgx_pagerank_read_delta(mgx_pagerank_run *run, float *out);  // syncs
mgx_status mgx_pagerank_normalize_download(mgx_pagerank_run *run, double *out_rank);

// wcc.hip
mgx_status mgx_wcc_impl(mgx_context *ctx, mgx_graph *g, int64_t *out_component,
                        int64_t *n_components);
// Device-output form (bridges.hip): min-member labels, label[v] = smallest id
// of v's component, in a context allocation of V int32 that the caller's scope
// `own` owns. Needs V > 0 and the sym-CSR; has synchronized when it returns.
mgx_status mgx_wcc_labels_device(mgx_scope &own, mgx_graph *g, int32_t **out_label);
// katz.hip
mgx_status mgx_katz_impl(mgx_context *ctx, mgx_graph *g, double alpha, double epsilon,
                         double *out_centrality, int64_t *iterations);
// louvain.hip
mgx_status mgx_louvain_impl(mgx_context *ctx, mgx_graph *g, double threshold,
                            int64_t *out_community, int64_t *n_communities);
// betweenness.hip
mgx_status mgx_betweenness_impl(mgx_context *ctx, mgx_graph *g, int directed, int normalize,
                                double *out_bc);

// bfs.hip
mgx_status mgx_bfs_impl(mgx_context *ctx, mgx_graph *g, int64_t source, int directed,
                        int64_t max_depth, int mode, int64_t *out_hops, int64_t *out_parent,
                        mgx_bfs_stats *stats);
// Device-output form (bridges.hip): level 0 is the n_roots distinct vertices
// of the device list d_roots (or the one vertex `single` when d_roots is
// null); hops [V] and parent [V] (nullable) are caller-owned int32 device
// buffers, left at -1 / INT32_MAX where nothing was reached, parent[root] =
// root. Same argument checks, direction rule and stats as mgx_bfs.
mgx_status mgx_bfs_device(mgx_context *ctx, mgx_graph *g, const int32_t *d_roots,
                          int64_t n_roots, int32_t single, int directed, int64_t max_depth,
                          int mode, int32_t *hops, int32_t *parent, mgx_bfs_stats *stats);

// bridges.hip
mgx_status mgx_bridges_impl(mgx_context *ctx, mgx_graph *g, int64_t *out_u, int64_t *out_v,
                            int64_t *n_bridges, mgx_bridges_stats *stats);
mgx_status mgx_bridges_state_impl(mgx_context *ctx, mgx_graph *g, int64_t *parent,
                                  int64_t *level, int64_t *pre, int64_t *nd, int64_t *low,
                                  int64_t *high);
void mgx_bridges_last_stage_ms_impl(double *forest, double *sorts_scans, double *sweep,
                                    double *levels);

// similarity.hip
mgx_status mgx_similarity_pairs_impl(mgx_context *ctx, mgx_graph *g, int metric, int mode,
                                     const int64_t *u, const int64_t *v, int64_t n_pairs,
                                     double *out_sim, int64_t *out_common,
                                     mgx_similarity_stats *stats);
mgx_status mgx_similarity_all_impl(mgx_context *ctx, mgx_graph *g, int metric, double *out_sim,
                                   mgx_similarity_stats *stats);

// comm.cpp (RCCL)
mgx_status mgx_comm_allgather_f32(mgx_context *ctx, const float *send, float *recv,
                                  size_t per_rank_count);
mgx_status mgx_comm_allreduce_max_f32(mgx_context *ctx, const float *send, float *recv);
int mgx_comm_world(mgx_context *ctx);  // 0 if no comm

#endif  // MGX_INTERNAL_H
