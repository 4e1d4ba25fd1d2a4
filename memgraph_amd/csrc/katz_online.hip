// Online (dynamic) Katz centrality on gfx950 — replaces the reference's
// online katz_alg (/root/reference/query_modules/katz_centrality_module/
// algorithm/katz.cpp):
//   SetKatz (:356-378) / KatzCentralityLoop (:211-240): omega_i = A^T
//     omega_{i-1}, c_i = c_{i-1} + a^i omega_i, lr/ur bounds (ur with
//     gamma), loop until the active set is epsilon-separated (Converged
//     :139-186 post the k-override at :146: adjacent-pair separation of
//     active centralities sorted descending).
//   UpdateKatz (:380-468): omega deltas propagated level-by-level along the
//     CURRENT graph's out-edges from the updated-node closure (UpdateLevel
//     :253-313), skipping created-edge instances; new-edge adds, deleted-
//     edge subtracts against the OLD omegas; centrality refresh for the
//     updated set (i==1 special case :308-311); lr/ur refresh WITHOUT gamma
//     (:434-440); re-activation by ur >= min_lr - eps; deleted-vertex
//     erasure; continuation with gamma = degmax/(1 - a*degmax) (:396 — the
//     reference uses a, not a^2, here; replicated).
//
// MI355X-native state: per-iteration dense fp64 omega/centrality arrays in
// HBM keyed by node SLOT (host map memgraph-id -> slot survives graph
// changes), the reference's O(iters*V) history design kept deliberately —
// the update path needs old omegas per level. The iteration gather runs as
// a two-bin (thread-per-small-row / block-per-hub-row) pull over the
// in-CSR; convergence sorts centralities on device (rocPRIM radix, stable:
// ties resolve by ascending sort order == the oracle's documented
// divergence from std::partial_sort's unspecified tie order).
//
// Created-edge identity: the module-side contract passes created edges as
// (from,to) pairs; parallel edges contribute identically to every omega
// sum, so skipping "the first k instances of (v,w) in v's sorted out-run"
// is value-equivalent to the reference's skip-by-edge-id (katz_centrality_
// online_module.cpp:110-114) for any id assignment. Documented; pinned by
// the exact-match tests against the sequential oracle (itself pinned 1e-12
// against the compiled reference core, tests/test_konline_cpu.py).
//
// Deterministic parity: fp64 sums here are computed in CSR order per row by
// a single lane (small rows) or a fixed-shape wave reduction (hub rows);
// both reorder additions vs the oracle's adjacency order — parity bar is
// 1e-9 relative (tests), not bit equality.

#include <cstring>
#include <map>
#include <set>
#include <unordered_map>
#include <vector>

#include <rocprim/rocprim.hpp>

#include "mgx_online.h"

namespace {

constexpr uint32_t kBigRow = 256;  // >=: block-per-row gather

constexpr int64_t kFirstSlots = 256;  // first capacity of the slot-space arrays

struct KOnState {
  mgx_slot_table slots;  // alive: slot present in the centrality maps

  // per-iteration history (device, slot space, capacity >= slots_cap())
  std::vector<mgx_dev_array<double>> omega, cent;
  mgx_dev_array<double> lr, ur;
  mgx_dev_array<uint8_t> d_active;
  // mirrors the reference's std::set; sized to the slot table where it is used
  std::vector<uint8_t> active_h;
  // What every slot-space array holds at least: kon_grow_slots grows d_active last.
  int64_t slots_cap() const { return d_active.cap; }
  int64_t iteration = 0;
  double alpha = 0.2, eps = 1e-2;
  bool initialized = false;
};

KOnState &g_k = *new KOnState;  // never deleted: see mgx_online.h

// ---- kernels -------------------------------------------------------------

// Fused gather + centrality/bounds update for one iteration over SMALL rows
// (KatzCentralityLoop body :218-235). Arrays indexed by SLOT; the graph is
// in dense space.
struct IterArgs {
  const uint32_t *in_row_ptr;  // dense
  const int32_t *in_col;       // dense sources
  const int32_t *dense2slot;
  const int32_t *rows;  // dense row list for this kernel
  int64_t n_rows;
  const double *omega_prev;  // slot space
  double *omega_out;
  const double *cent_prev;
  double *cent_out;
  double *lr;
  double *ur;
  double a_pow_i;    // alpha^i
  double a_pow_ig;   // alpha^(i+1) * gamma
};

__device__ inline void iter_finish(const IterArgs &A, int32_t slot, double acc) {
  A.omega_out[slot] = acc;
  const double c = A.cent_prev[slot] + A.a_pow_i * acc;
  A.cent_out[slot] = c;
  A.lr[slot] = c;
  A.ur[slot] = c + A.a_pow_ig * acc;
}

__global__ void k_iter_small(IterArgs A) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < A.n_rows;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int32_t v = A.rows[i];
    double acc = 0.0;
    for (uint32_t j = A.in_row_ptr[v]; j < A.in_row_ptr[v + 1]; ++j)
      acc += A.omega_prev[A.dense2slot[A.in_col[j]]];
    iter_finish(A, A.dense2slot[v], acc);
  }
}

__global__ void __launch_bounds__(kBlock) k_iter_big(IterArgs A) {
  __shared__ double red[kBlock / 64];
  for (int64_t bi = blockIdx.x; bi < A.n_rows; bi += gridDim.x) {
    const int32_t v = A.rows[bi];
    double acc = 0.0;
    for (uint32_t j = A.in_row_ptr[v] + threadIdx.x; j < A.in_row_ptr[v + 1];
         j += kBlock)
      acc += A.omega_prev[A.dense2slot[A.in_col[j]]];
    for (int o = 32; o; o >>= 1) acc += __shfl_down(acc, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) iter_finish(A, A.dense2slot[v], red[0] + red[1] + red[2] + red[3]);
    __syncthreads();
  }
}

// ordered-u64 transform of f64 (monotone): negatives handled.
__device__ inline uint64_t f64_key_desc(double x) {
  uint64_t b = __double_as_longlong(x);
  b ^= (b >> 63) ? ~0ull : 0x8000000000000000ull;
  return ~b;  // descending via ascending radix sort
}

__global__ void k_conv_keys(int64_t n_active, const int32_t *active_slots,
                            const double *cent, uint64_t *keys) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n_active;
       i += (int64_t)gridDim.x * blockDim.x)
    keys[i] = f64_key_desc(cent[active_slots[i]]);
}

// Converged (:177-184): not converged iff any adjacent sorted pair has
// ur[i] - eps >= lr[i-1].
__global__ void k_conv_check(int64_t n_active, const int32_t *sorted_slots,
                             const double *lr, const double *ur, double eps,
                             uint32_t *not_conv) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x + 1; i < n_active;
       i += (int64_t)gridDim.x * blockDim.x) {
    if (ur[sorted_slots[i]] - eps >= lr[sorted_slots[i - 1]]) atomicOr(not_conv, 1u);
  }
}

// ---- update-level kernels ------------------------------------------------

// Frontier-closure round (UpdateLevel :271-291): each listed dense node v
// contributes delta = omega_new[i-1][v] - omega_old[i-1][v] to every CURRENT
// out-edge (v,w) except the first newcnt(v,w) instances of each sorted
// w-run, marks w updated, and collects newly updated nodes.
struct LevelArgs {
  const int32_t *front;  // dense ids, this round
  int64_t n_front;
  const uint32_t *out_row_ptr;
  const int32_t *out_col;  // sorted within row
  const int32_t *dense2slot;
  const double *omega_new_prev;  // slot space (level i-1)
  const double *omega_old_prev;
  double *omega_new_cur;  // level i (slot space), atomicAdd
  uint32_t *updated;      // dense space flags (u32: atomicExch needs 32-bit)
  int32_t *next;          // collect newly updated dense ids
  unsigned long long *n_next;
  // new-edge multiplicity per (src,dst) pair, sorted by (src<<32|dst)
  const uint64_t *new_pairs;
  const uint32_t *new_cnt;
  int64_t n_new_pairs;
};

__device__ inline uint32_t newcnt_of(const LevelArgs &A, int32_t v, int32_t w) {
  int64_t lo = 0, hi = A.n_new_pairs;
  const uint64_t key = ((uint64_t)(uint32_t)v << 32) | (uint32_t)w;
  while (lo < hi) {
    int64_t mid = (lo + hi) / 2;
    if (A.new_pairs[mid] < key) lo = mid + 1;
    else hi = mid;
  }
  if (lo < A.n_new_pairs && A.new_pairs[lo] == key) return A.new_cnt[lo];
  return 0;
}

__global__ void k_level_round(LevelArgs A) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < A.n_front;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int32_t v = A.front[i];
    const int32_t vs = A.dense2slot[v];
    const double delta = A.omega_new_prev[vs] - A.omega_old_prev[vs];
    const uint32_t s = A.out_row_ptr[v], e = A.out_row_ptr[v + 1];
    int32_t run_w = -1;
    uint32_t skipped = 0, toskip = 0;
    for (uint32_t j = s; j < e; ++j) {
      const int32_t w = A.out_col[j];
      if (w != run_w) {
        run_w = w;
        skipped = 0;
        toskip = A.n_new_pairs ? newcnt_of(A, v, w) : 0;
      }
      // mark updated + enqueue (reference :281-284) — for EVERY out-edge,
      // including created ones
      if (!atomicExch(&A.updated[w], 1u)) {
        unsigned long long at = atomicAdd(A.n_next, 1ull);
        A.next[at] = w;
      }
      if (skipped < toskip) {  // skip created instance (:287)
        ++skipped;
        continue;
      }
      atomicAdd(&A.omega_new_cur[A.dense2slot[w]], delta);
    }
  }
}

// omega_new[i][v] += omega_new[i-1][w] per created edge (w,v) (:294-296);
// omega_new[i][v] -= omega_old[i-1][w] per deleted edge (:299-301).
// Edges arrive as slot pairs; deleted-edge w may be a dead slot (value
// still present in history).
__global__ void k_edge_terms(int64_t n_new, const int32_t *new_ws, const int32_t *new_vs,
                             int64_t n_del, const int32_t *del_ws, const int32_t *del_vs,
                             const double *omega_new_prev, const double *omega_old_prev,
                             double *omega_new_cur) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n_new + n_del;
       i += (int64_t)gridDim.x * blockDim.x) {
    if (i < n_new) {
      atomicAdd(&omega_new_cur[new_vs[i]], omega_new_prev[new_ws[i]]);
    } else {
      const int64_t d = i - n_new;
      atomicAdd(&omega_new_cur[del_vs[d]], -omega_old_prev[del_ws[d]]);
    }
  }
}

// centrality refresh for the updated set (:304-312)
__global__ void k_cent_level(int64_t n_upd, const int32_t *upd_slots, int64_t level,
                             double a_pow_i, const double *omega_new_cur,
                             const double *omega_old_cur, const double *cent_prev,
                             double *cent_cur) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n_upd;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int32_t w = upd_slots[i];
    if (level != 1) {
      cent_cur[w] = cent_prev[w] + a_pow_i * omega_new_cur[w];
    } else {
      cent_cur[w] += a_pow_i * (omega_new_cur[w] - omega_old_cur[w]);
    }
  }
}

// lr/ur refresh for updated nodes after all levels (:434-440; NO gamma)
__global__ void k_bounds_refresh(int64_t n_upd, const int32_t *upd_slots,
                                 const double *cent_top, const double *omega_top,
                                 double a_pow_i1, double *lr, double *ur) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n_upd;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int32_t w = upd_slots[i];
    lr[w] = cent_top[w];
    ur[w] = cent_top[w] + a_pow_i1 * omega_top[w];
  }
}

__global__ void k_copy_f64(int64_t n, const double *in, double *out) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    out[i] = in[i];
}

__global__ void k_gather_out(int64_t V, const int32_t *dense2slot, const double *cent,
                             double *out) {
  for (int64_t v = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; v < V;
       v += (int64_t)gridDim.x * blockDim.x)
    out[v] = cent[dense2slot[v]];
}

// ---- host helpers --------------------------------------------------------

mgx_status kon_grow_slots(mgx_context *ctx, int64_t need) {
  auto grow = [&](mgx_dev_array<double> &a, double init) {
    return a.ensure(ctx, need, kFirstSlots, a.cap, mgx_fill_value(ctx, init));
  };
  for (size_t i = 0; i < g_k.omega.size(); ++i)
    MGX_TRY(grow(g_k.omega[i], i == 0 ? 1.0 : 0.0));
  for (auto &c : g_k.cent) MGX_TRY(grow(c, 0.0));
  MGX_TRY(grow(g_k.lr, 0.0));
  MGX_TRY(grow(g_k.ur, 0.0));
  return g_k.d_active.ensure(ctx, need, kFirstSlots, g_k.d_active.cap, mgx_fill_zero(ctx));
}

mgx_status kon_add_iteration(mgx_context *ctx, double omega_init) {
  mgx_dev_array<double> w, c;
  MGX_TRY(w.ensure(ctx, g_k.slots_cap(), kFirstSlots, 0, mgx_fill_value(ctx, omega_init)));
  MGX_TRY(c.ensure(ctx, g_k.slots_cap(), kFirstSlots, 0, mgx_fill_value(ctx, 0.0)));
  g_k.omega.push_back(std::move(w));
  g_k.cent.push_back(std::move(c));
  return MGX_OK;
}

struct KMaps {
  mgx_scope own;                  // of the device lists
  int32_t *dense2slot = nullptr;  // device
  std::vector<int32_t> d2s_h;
  int64_t V = 0;
  // dense row lists by in-degree bin
  int32_t *small_rows = nullptr, *big_rows = nullptr;
  int64_t n_small = 0, n_big = 0;
  explicit KMaps(mgx_context *ctx) : own(ctx) {}
};

// Slots (created where unseen) and in-degree bins for the graph's vertices.
mgx_status kon_build_maps(mgx_graph *g, const int64_t *dense_to_mg, KMaps *m) {
  mgx_context *ctx = m->own.ctx;
  const int64_t V = g ? g->n_vertices : 0;
  m->V = V;
  g_k.slots.map_dense(dense_to_mg, V, /*create=*/true, &m->d2s_h, nullptr);
  g_k.active_h.resize(g_k.slots.size(), 0);
  MGX_TRY(mgx_upload_i32(m->own, m->d2s_h, &m->dense2slot));
  // in-degree bins from the in-CSR (host-side row_ptr copy)
  if (V > 0 && g && g->in_row_ptr) {
    std::vector<uint32_t> rp(V + 1);
    MGX_HIP_TRY(hipMemcpyAsync(rp.data(), g->in_row_ptr, (V + 1) * 4,
                               hipMemcpyDeviceToHost, ctx->stream));
    MGX_HIP_TRY(hipStreamSynchronize(ctx->stream));
    std::vector<int32_t> sm, bg;
    for (int64_t v = 0; v < V; ++v) {
      const uint32_t d = rp[v + 1] - rp[v];
      if (d >= kBigRow) bg.push_back((int32_t)v);
      else sm.push_back((int32_t)v);
    }
    m->n_small = (int64_t)sm.size();
    m->n_big = (int64_t)bg.size();
    MGX_TRY(mgx_upload_i32(m->own, sm, &m->small_rows));
    MGX_TRY(mgx_upload_i32(m->own, bg, &m->big_rows));
    MGX_HIP_TRY(hipStreamSynchronize(ctx->stream));
  }
  return MGX_OK;
}

// KatzCentralityLoop (:211-240) continuation over the current graph.
mgx_status kon_loop(mgx_context *ctx, mgx_graph *g, const KMaps &m, double gamma) {
  const int64_t V = m.V;
  // active slot list (the reference's std::set iterates ascending mg id;
  // ordering is irrelevant pre-sort — the sort key decides)
  std::vector<int32_t> act;
  for (size_t s = 0; s < g_k.active_h.size(); ++s)
    if (g_k.active_h[s]) act.push_back((int32_t)s);
  const int64_t n_active = (int64_t)act.size();
  int32_t *d_act = nullptr, *d_act_sorted = nullptr;
  uint64_t *d_keys = nullptr, *d_keys_sorted = nullptr;
  uint32_t *d_flag = nullptr;
  mgx_scope bufs(ctx);
  MGX_TRY(bufs.alloc_plain(&d_act, n_active));
  MGX_TRY(bufs.alloc_plain(&d_act_sorted, n_active));
  MGX_TRY(bufs.alloc_plain(&d_keys, n_active));
  MGX_TRY(bufs.alloc_plain(&d_keys_sorted, n_active));
  MGX_TRY(bufs.alloc_plain(&d_flag, 1));
  if (n_active > 0)
    MGX_HIP_TRY(hipMemcpyAsync(d_act, act.data(), n_active * 4, hipMemcpyHostToDevice,
                               ctx->stream));

  mgx_status st = MGX_OK;
  while (true) {
    MGX_TRY(kon_add_iteration(ctx, 0.0));
    ++g_k.iteration;
    const int64_t i = g_k.iteration;
    IterArgs A;
    A.in_row_ptr = g->in_row_ptr;
    A.in_col = g->in_col;
    A.dense2slot = m.dense2slot;
    A.omega_prev = g_k.omega[i - 1];
    A.omega_out = g_k.omega[i];
    A.cent_prev = g_k.cent[i - 1];
    A.cent_out = g_k.cent[i];
    A.lr = g_k.lr;
    A.ur = g_k.ur;
    A.a_pow_i = pow(g_k.alpha, (double)i);
    A.a_pow_ig = pow(g_k.alpha, (double)(i + 1)) * gamma;
    if (m.n_small > 0) {
      A.rows = m.small_rows;
      A.n_rows = m.n_small;
      hipLaunchKernelGGL(k_iter_small, dim3((uint32_t)grid_for(m.n_small)), dim3(kBlock),
                         0, ctx->stream, A);
    }
    if (m.n_big > 0) {
      A.rows = m.big_rows;
      A.n_rows = m.n_big;
      hipLaunchKernelGGL(k_iter_big, dim3((uint32_t)(m.n_big < 4096 ? m.n_big : 4096)),
                         dim3(kBlock), 0, ctx->stream, A);
    }
    // convergence: sort active by centrality desc (stable => ties keep the
    // ascending-slot input order) + adjacent-pair check
    if (n_active <= 1) break;
    hipLaunchKernelGGL(k_conv_keys, dim3((uint32_t)grid_for(n_active)), dim3(kBlock), 0,
                       ctx->stream, n_active, d_act, g_k.cent[i], d_keys);
    st = mgx_with_temp(ctx, "katz_online convergence sort", [&](void *tmp, size_t &bytes) {
      return rocprim::radix_sort_pairs(tmp, bytes, d_keys, d_keys_sorted, d_act, d_act_sorted,
                                       n_active, 0, 64, ctx->stream);
    });
    if (st != MGX_OK) break;
    MGX_HIP_TRY(hipMemsetAsync(d_flag, 0, 4, ctx->stream));
    hipLaunchKernelGGL(k_conv_check, dim3((uint32_t)grid_for(n_active)), dim3(kBlock), 0,
                       ctx->stream, n_active, d_act_sorted, g_k.lr, g_k.ur, g_k.eps,
                       d_flag);
    uint32_t not_conv = 0;
    MGX_HIP_TRY(hipMemcpyAsync(&not_conv, d_flag, 4, hipMemcpyDeviceToHost, ctx->stream));
    MGX_HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (!not_conv) break;
    if (g_k.iteration > 10000) {
      mgx_set_error("katz_online did not converge in 10000 iterations");
      st = MGX_ERR_HIP;
      break;
    }
  }
  (void)V;
  return st;
}

mgx_status kon_output(mgx_context *ctx, const KMaps &m, double *out) {
  if (!out || m.V == 0) return MGX_OK;
  double *d_out = nullptr;
  mgx_scope bufs(ctx);
  MGX_TRY(bufs.alloc(&d_out, m.V));
  hipLaunchKernelGGL(k_gather_out, dim3((uint32_t)grid_for(m.V)), dim3(kBlock), 0,
                     ctx->stream, m.V, m.dense2slot, g_k.cent[g_k.iteration], d_out);
  MGX_HIP_TRY(hipMemcpyAsync(out, d_out, m.V * 8, hipMemcpyDeviceToHost, ctx->stream));
  MGX_HIP_TRY(hipStreamSynchronize(ctx->stream));
  return MGX_OK;
}

int64_t kon_max_degree_dense(mgx_context *ctx, mgx_graph *g) {
  // out-degree max over current graph (MaxDegree :119-128 uses Neighbours =
  // out-neighbours of the directed view)
  const int64_t V = g->n_vertices;
  std::vector<uint32_t> rp(V + 1);
  (void)hipMemcpyAsync(rp.data(), g->out_row_ptr, (V + 1) * 4, hipMemcpyDeviceToHost,
                       ctx->stream);
  (void)hipStreamSynchronize(ctx->stream);
  int64_t m = 0;
  for (int64_t v = 0; v < V; ++v) {
    const int64_t d = (int64_t)(rp[v + 1] - rp[v]);
    if (d > m) m = d;
  }
  return m;
}

}  // namespace

extern "C" int mgx_konline_initialized(void) {
  return (g_k.initialized && !g_k.cent.empty() && g_k.iteration > 0) ? 1 : 0;
}

extern "C" mgx_status mgx_konline_reset(mgx_context *ctx) {
  (void)ctx;
  g_k = KOnState{};
  return MGX_OK;
}

extern "C" int64_t mgx_konline_iterations(void) { return g_k.iteration; }

extern "C" mgx_status mgx_konline_set(mgx_context *ctx, mgx_graph *g,
                                      const int64_t *dense_to_mg, double alpha,
                                      double epsilon, double *out) {
  if (g && !((g->flags & MGX_BUILD_IN_CSR) && (g->flags & MGX_BUILD_OUT_CSR) &&
             (g->flags & MGX_BUILD_NO_PERM))) {
    mgx_set_error("konline_set needs IN_CSR|OUT_CSR|NO_PERM (identity layout)");
    return MGX_ERR_INVALID_ARGUMENT;
  }
  MGX_HIP_TRY(hipSetDevice(ctx->device));
  g_k = KOnState{};
  g_k.alpha = alpha;
  g_k.eps = epsilon;
  g_k.initialized = true;
  const int64_t V = g ? g->n_vertices : 0;
  KMaps m(ctx);
  MGX_TRY(kon_build_maps(g, dense_to_mg, &m));
  for (int64_t v = 0; v < V; ++v) g_k.slots.alive[m.d2s_h[v]] = 1;
  MGX_TRY(kon_grow_slots(ctx, V > 0 ? V : 1));
  // Init (:30-47): centralities[0]=0, omegas[0]=1, lr=ur=0
  MGX_TRY(kon_add_iteration(ctx, 1.0));  // omega[0]=1, cent[0]=0
  if (V == 0 || g->n_edges == 0) {  // :363-365
    if (out)
      for (int64_t v = 0; v < V; ++v) out[v] = 0.0;
    return MGX_OK;
  }
  const double dm = (double)kon_max_degree_dense(ctx, g);
  const double gamma = dm / (1.0 - (alpha * alpha * dm));  // :368
  for (int64_t v = 0; v < V; ++v) g_k.active_h[m.d2s_h[v]] = 1;
  MGX_TRY(kon_loop(ctx, g, m, gamma));
  return kon_output(ctx, m, out);
}

extern "C" mgx_status mgx_konline_get(mgx_context *ctx, const int64_t *dense_to_mg,
                                      int64_t V, double *out, int *consistent) {
  MGX_HIP_TRY(hipSetDevice(ctx->device));
  // IsInconsistent (:322-338): both directions (graph ⊆ state, state ⊆ graph)
  bool ok = true;
  int64_t n_alive = 0;
  for (auto a : g_k.slots.alive)
    if (a) ++n_alive;
  KMaps m(ctx);
  m.V = V;
  g_k.slots.map_dense(dense_to_mg, V, /*create=*/false, &m.d2s_h, &ok);
  if (n_alive != V) ok = false;
  if (consistent) *consistent = ok ? 1 : 0;
  if (!ok || !out || V == 0) return MGX_OK;
  MGX_TRY(mgx_upload_i32(m.own, m.d2s_h, &m.dense2slot));
  return kon_output(ctx, m, out);
}

extern "C" mgx_status mgx_konline_update(mgx_context *ctx, mgx_graph *g,
                                         const int64_t *dense_to_mg,
                                         const int64_t *created_v, int64_t n_cv,
                                         const int64_t *created_e, int64_t n_ce,
                                         const int64_t *deleted_v, int64_t n_dv,
                                         const int64_t *deleted_e, int64_t n_de,
                                         double *out) {
  if (g && !((g->flags & MGX_BUILD_IN_CSR) && (g->flags & MGX_BUILD_OUT_CSR) &&
             (g->flags & MGX_BUILD_NO_PERM))) {
    mgx_set_error("konline_update needs IN_CSR|OUT_CSR|NO_PERM (identity layout)");
    return MGX_ERR_INVALID_ARGUMENT;
  }
  MGX_HIP_TRY(hipSetDevice(ctx->device));
  const int64_t V = g ? g->n_vertices : 0;
  if (V == 0 || !g || g->n_edges == 0) {  // :390-393 re-init on empty graph
    const double a = g_k.alpha, e = g_k.eps;
    MGX_TRY(mgx_konline_set(ctx, g, dense_to_mg, a, e, out));
    return MGX_OK;
  }

  // new vertices get slots + history entries (:399-404)
  for (int64_t i = 0; i < n_cv; ++i) {
    const int32_t s = g_k.slots.slot_of(created_v[i], 0);
    g_k.slots.alive[s] = 1;
  }
  MGX_TRY(kon_grow_slots(ctx, g_k.slots.size()));
  // omega[0][new]=1 / cent[i][new]=0: kon_grow_slots fills growth with
  // exactly those defaults, so nothing to write unless the slot existed
  // before (revival) — handle revival explicitly:
  // (cheap: n_cv writes)
  for (int64_t i = 0; i < n_cv; ++i) {
    const int32_t s = g_k.slots.find(created_v[i]);
    const double one = 1.0, zero = 0.0;
    MGX_HIP_TRY(hipMemcpyAsync(g_k.omega[0] + s, &one, 8, hipMemcpyHostToDevice,
                               ctx->stream));
    for (auto &c : g_k.cent)
      MGX_HIP_TRY(hipMemcpyAsync(c + s, &zero, 8, hipMemcpyHostToDevice, ctx->stream));
    MGX_HIP_TRY(hipStreamSynchronize(ctx->stream));
  }

  KMaps m(ctx);
  MGX_TRY(kon_build_maps(g, dense_to_mg, &m));
  for (int64_t v = 0; v < V; ++v) g_k.slots.alive[m.d2s_h[v]] = 1;
  // a vertex of the graph that created_v did not announce got its slot just now
  MGX_TRY(kon_grow_slots(ctx, g_k.slots.size()));

  const double dm = (double)kon_max_degree_dense(ctx, g);
  const double gamma = dm / (1.0 - (g_k.alpha * dm));  // :396 — a, not a^2

  // updated set (:407-415), as host mg ids -> dense ids (edges reference
  // nodes of the current graph except deleted-edge endpoints that are gone)
  std::unordered_map<int64_t, int32_t> mg2dense;
  mg2dense.reserve((size_t)V * 2);
  for (int64_t v = 0; v < V; ++v) mg2dense.emplace(dense_to_mg[v], (int32_t)v);
  std::set<int64_t> updated_mg;
  for (int64_t i = 0; i < n_ce; ++i) {
    updated_mg.insert(created_e[2 * i]);
    updated_mg.insert(created_e[2 * i + 1]);
  }
  for (int64_t i = 0; i < n_de; ++i) {
    updated_mg.insert(deleted_e[2 * i]);
    updated_mg.insert(deleted_e[2 * i + 1]);
  }

  // created-edge multiplicity per dense (src,dst) pair, sorted
  std::vector<uint64_t> pair_keys;
  std::vector<uint32_t> pair_cnt;
  {
    std::map<uint64_t, uint32_t> mult;
    for (int64_t i = 0; i < n_ce; ++i) {
      auto fs = mg2dense.find(created_e[2 * i]);
      auto ts = mg2dense.find(created_e[2 * i + 1]);
      if (fs == mg2dense.end() || ts == mg2dense.end()) continue;
      mult[((uint64_t)(uint32_t)fs->second << 32) | (uint32_t)ts->second]++;
    }
    for (auto &[k, c] : mult) {
      pair_keys.push_back(k);
      pair_cnt.push_back(c);
    }
  }
  // The device temporaries of the update: gone before the loop allocates.
  {
    mgx_scope bufs(ctx);
    uint64_t *d_pairs = nullptr;
    uint32_t *d_cnt = nullptr;
    MGX_TRY(bufs.alloc_plain(&d_pairs, (int64_t)pair_keys.size()));
    MGX_TRY(bufs.alloc_plain(&d_cnt, (int64_t)pair_cnt.size()));
    if (!pair_keys.empty()) {
      MGX_HIP_TRY(hipMemcpyAsync(d_pairs, pair_keys.data(), pair_keys.size() * 8,
                                 hipMemcpyHostToDevice, ctx->stream));
      MGX_HIP_TRY(hipMemcpyAsync(d_cnt, pair_cnt.data(), pair_cnt.size() * 4,
                                 hipMemcpyHostToDevice, ctx->stream));
    }

    // edge term slot arrays
    std::vector<int32_t> new_ws, new_vs, del_ws, del_vs;
    for (int64_t i = 0; i < n_ce; ++i) {
      const int32_t w = g_k.slots.find(created_e[2 * i]);
      const int32_t v = g_k.slots.find(created_e[2 * i + 1]);
      if (w < 0 || v < 0) continue;
      new_ws.push_back(w);
      new_vs.push_back(v);
    }
    for (int64_t i = 0; i < n_de; ++i) {
      const int32_t w = g_k.slots.find(deleted_e[2 * i]);
      const int32_t v = g_k.slots.find(deleted_e[2 * i + 1]);
      if (w < 0 || v < 0) continue;
      del_ws.push_back(w);
      del_vs.push_back(v);
    }
    int32_t *d_new_ws = nullptr, *d_new_vs = nullptr, *d_del_ws = nullptr,
            *d_del_vs = nullptr;
    MGX_TRY(mgx_upload_i32(bufs, new_ws, &d_new_ws));
    MGX_TRY(mgx_upload_i32(bufs, new_vs, &d_new_vs));
    MGX_TRY(mgx_upload_i32(bufs, del_ws, &d_del_ws));
    MGX_TRY(mgx_upload_i32(bufs, del_vs, &d_del_vs));

    // context_new omegas: new_omega[0] = 1 for all current nodes; levels
    // 1..iteration computed below. Keep as separate device arrays.
    std::vector<double *> new_omega(g_k.iteration + 1, nullptr);
    for (int64_t i = 0; i <= g_k.iteration; ++i)
      MGX_TRY(bufs.alloc_plain(&new_omega[i], g_k.slots_cap()));
    hipLaunchKernelGGL(mgx_k_fill<double>, dim3((uint32_t)grid_for(g_k.slots_cap())),
                       dim3(kBlock), 0, ctx->stream, g_k.slots_cap(), 1.0, new_omega[0]);

    // updated/frontier state in dense space
    uint32_t *d_updated = nullptr;
    int32_t *d_front = nullptr, *d_next = nullptr;
    unsigned long long *d_nn = nullptr;
    MGX_TRY(bufs.alloc_plain(&d_updated, V));
    MGX_TRY(bufs.alloc_plain(&d_front, V));
    MGX_TRY(bufs.alloc_plain(&d_next, V));
    MGX_TRY(bufs.alloc_plain(&d_nn, 1));
    std::vector<uint32_t> upd_h(V, 0);
    std::vector<int32_t> front_h;
    for (auto mg : updated_mg) {
      auto it = mg2dense.find(mg);
      if (it == mg2dense.end()) continue;  // deleted endpoint: not a graph node
      if (!upd_h[it->second]) {
        upd_h[it->second] = 1;
        front_h.push_back(it->second);
      }
    }

    for (int64_t lvl = 1; lvl <= g_k.iteration; ++lvl) {
      // new_omega[lvl] = old omega[lvl] (:266-268; only current slots matter)
      MGX_HIP_TRY(hipMemcpyAsync(new_omega[lvl], g_k.omega[lvl], g_k.slots_cap() * 8,
                                 hipMemcpyDeviceToDevice, ctx->stream));
      MGX_HIP_TRY(hipMemcpyAsync(d_updated, upd_h.data(), V * 4,
                                 hipMemcpyHostToDevice, ctx->stream));
      // frontier rounds: every updated node processes its out-edges exactly
      // once per level; nodes marked mid-level join later rounds
      std::vector<int32_t> front = front_h;
      MGX_HIP_TRY(hipStreamSynchronize(ctx->stream));
      while (!front.empty()) {
        MGX_HIP_TRY(hipMemcpyAsync(d_front, front.data(), front.size() * 4,
                                   hipMemcpyHostToDevice, ctx->stream));
        MGX_HIP_TRY(hipMemsetAsync(d_nn, 0, 8, ctx->stream));
        LevelArgs L;
        L.front = d_front;
        L.n_front = (int64_t)front.size();
        L.out_row_ptr = g->out_row_ptr;
        L.out_col = g->out_col;
        L.dense2slot = m.dense2slot;
        L.omega_new_prev = new_omega[lvl - 1];
        L.omega_old_prev = g_k.omega[lvl - 1];
        L.omega_new_cur = new_omega[lvl];
        L.updated = d_updated;
        L.next = d_next;
        L.n_next = d_nn;
        L.new_pairs = d_pairs;
        L.new_cnt = d_cnt;
        L.n_new_pairs = (int64_t)pair_keys.size();
        hipLaunchKernelGGL(k_level_round, dim3((uint32_t)grid_for(L.n_front)), dim3(kBlock),
                           0, ctx->stream, L);
        unsigned long long nn = 0;
        MGX_HIP_TRY(hipMemcpyAsync(&nn, d_nn, 8, hipMemcpyDeviceToHost, ctx->stream));
        MGX_HIP_TRY(hipStreamSynchronize(ctx->stream));
        front.assign(nn, 0);
        if (nn > 0) {
          MGX_HIP_TRY(hipMemcpyAsync(front.data(), d_next, nn * 4, hipMemcpyDeviceToHost,
                                     ctx->stream));
          MGX_HIP_TRY(hipStreamSynchronize(ctx->stream));
        }
      }
      // next level's initial front/updated = the closure so far
      {
        std::vector<uint32_t> cur(V);
        MGX_HIP_TRY(hipMemcpyAsync(cur.data(), d_updated, V * 4,
                                   hipMemcpyDeviceToHost, ctx->stream));
        MGX_HIP_TRY(hipStreamSynchronize(ctx->stream));
        upd_h = cur;
        front_h.clear();
        for (int64_t v = 0; v < V; ++v)
          if (upd_h[v]) front_h.push_back((int32_t)v);
      }
      // edge terms (:294-301)
      if (!new_ws.empty() || !del_ws.empty()) {
        hipLaunchKernelGGL(k_edge_terms,
                           dim3((uint32_t)grid_for((int64_t)(new_ws.size() + del_ws.size()))),
                           dim3(kBlock), 0, ctx->stream, (int64_t)new_ws.size(), d_new_ws,
                           d_new_vs, (int64_t)del_ws.size(), d_del_ws, d_del_vs,
                           new_omega[lvl - 1], g_k.omega[lvl - 1], new_omega[lvl]);
      }
      // centralities for the updated set (:304-312)
      std::vector<int32_t> upd_slots;
      for (auto v : front_h) upd_slots.push_back(m.d2s_h[v]);
      mgx_scope slot_bufs(ctx);
      int32_t *d_upd_slots = nullptr;
      MGX_TRY(mgx_upload_i32(slot_bufs, upd_slots, &d_upd_slots));
      hipLaunchKernelGGL(k_cent_level, dim3((uint32_t)grid_for((int64_t)upd_slots.size())),
                         dim3(kBlock), 0, ctx->stream, (int64_t)upd_slots.size(),
                         d_upd_slots, lvl, pow(g_k.alpha, (double)lvl), new_omega[lvl],
                         g_k.omega[lvl], g_k.cent[lvl - 1], g_k.cent[lvl]);
      MGX_HIP_TRY(hipStreamSynchronize(ctx->stream));
    }

    // merge new omegas into state (:427-431)
    for (int64_t lvl = 1; lvl <= g_k.iteration; ++lvl) {
      MGX_HIP_TRY(hipMemcpyAsync(g_k.omega[lvl], new_omega[lvl], g_k.slots_cap() * 8,
                                 hipMemcpyDeviceToDevice, ctx->stream));
    }
    MGX_HIP_TRY(hipStreamSynchronize(ctx->stream));

    // lr/ur refresh for updated nodes (:434-440; no gamma)
    {
      std::vector<int32_t> upd_slots;
      for (auto v : front_h) upd_slots.push_back(m.d2s_h[v]);
      mgx_scope slot_bufs(ctx);
      int32_t *d_upd_slots = nullptr;
      MGX_TRY(mgx_upload_i32(slot_bufs, upd_slots, &d_upd_slots));
      hipLaunchKernelGGL(k_bounds_refresh,
                         dim3((uint32_t)grid_for((int64_t)upd_slots.size())), dim3(kBlock),
                         0, ctx->stream, (int64_t)upd_slots.size(), d_upd_slots,
                         g_k.cent[g_k.iteration], g_k.omega[g_k.iteration],
                         pow(g_k.alpha, (double)(g_k.iteration + 1)), g_k.lr, g_k.ur);
      MGX_HIP_TRY(hipStreamSynchronize(ctx->stream));
    }

    // re-activation (:442-455): min lr over active, then ur >= min_lr - eps
    {
      std::vector<double> lr_h(g_k.slots_cap()), ur_h(g_k.slots_cap());
      MGX_HIP_TRY(hipMemcpyAsync(lr_h.data(), g_k.lr, g_k.slots_cap() * 8,
                                 hipMemcpyDeviceToHost, ctx->stream));
      MGX_HIP_TRY(hipMemcpyAsync(ur_h.data(), g_k.ur, g_k.slots_cap() * 8,
                                 hipMemcpyDeviceToHost, ctx->stream));
      MGX_HIP_TRY(hipStreamSynchronize(ctx->stream));
      double min_lr = 1e300;
      for (size_t s = 0; s < g_k.active_h.size(); ++s)
        if (g_k.active_h[s] && lr_h[s] < min_lr) min_lr = lr_h[s];
      for (int64_t v = 0; v < V; ++v) {
        const int32_t s = m.d2s_h[v];
        if (ur_h[s] >= (min_lr - g_k.eps)) g_k.active_h[s] = 1;
      }
    }
    // deleted vertices (:458-464)
    for (int64_t i = 0; i < n_dv; ++i) {
      const int32_t s = g_k.slots.find(deleted_v[i]);
      if (s < 0) continue;
      g_k.slots.alive[s] = 0;
      g_k.active_h[s] = 0;
    }
  }

  MGX_TRY(kon_loop(ctx, g, m, gamma));
  return kon_output(ctx, m, out);
}
