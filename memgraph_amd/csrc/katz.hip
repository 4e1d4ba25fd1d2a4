// Katz centrality on gfx950 — replaces katz_alg::SetKatz / KatzCentralityLoop
// (reference katz.cpp:393-414, :226-255) with dense fp64 state:
//   omega_i(v) = sum_{u->v} omega_{i-1}(u)      (in-CSR gather sweep)
//   c_i = c_{i-1} + alpha^i * omega_i ; lr = c_i ; ur = c_i + alpha^{i+1}*omega_i*gamma
// Convergence replicates Converged (katz.cpp:165-215) AFTER the k-override
// at :172: stable sort all centralities descending (ties -> smaller node id,
// as the oracle documents) and require ur(v_i) - eps < lr(v_{i-1}) for every
// adjacent sorted pair. gamma = degmax/(1 - alpha^2*degmax) in IEEE
// semantics (katz.cpp:403-404) — including the divergent-series regime.

#include <cstring>

#include <rocprim/rocprim.hpp>

#include "mgx_device.h"

namespace {

struct KatzArgs {
  const uint32_t *row_ptr;
  const int32_t *col;
  mgx_bin_sections bins;
  const double *omega_old;
  double *omega_new;
  double *centrality;
  double *lr;
  double *ur;
  double a_i;    // alpha^iteration
  double a_i1g;  // alpha^(iteration+1) * gamma
};

template <int LANES>
__device__ inline void katz_rows(const KatzArgs &A, int sec, int64_t block_in_sec) {
  reduce_bin_rows<LANES>(
      A.bins, sec, block_in_sec, 0.0, mgx_op_add(),
      [&](int32_t row, int sub) {
        double acc = 0.0;
        row_gather<LANES>(A.col, A.row_ptr[row], A.row_ptr[row + 1], sub,
                          [&](int32_t c) { acc += A.omega_old[c]; });
        return acc;
      },
      [&](int32_t row, double acc) {
        A.omega_new[row] = acc;
        const double c = A.centrality[row] + A.a_i * acc;
        A.centrality[row] = c;
        A.lr[row] = c;                       // katz.cpp:247
        A.ur[row] = c + A.a_i1g * acc;       // katz.cpp:248-250
      });
}

__global__ void __launch_bounds__(kBlock) k_katz_sweep(KatzArgs A) {
  for_bin_section(A.bins.goff, [&](auto lanes, int sec, int64_t bis) {
    katz_rows<decltype(lanes)::value>(A, sec, bis);
  });
}

__global__ void k_scatter_f64(int64_t n, const double *in, const int32_t *order,
                              double *out) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    out[order ? order[i] : i] = in[i];
}

// Stage the convergence-sort input in ORIGINAL vertex order so the stable
// descending radix sort breaks centrality ties by original id — the
// oracle's (documented) tie rule — while values stay permuted indices for
// the lr/ur lookups.
__global__ void k_sort_stage(int64_t n, const double *cent, const int32_t *order,
                             double *keys, uint32_t *vals) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t old = order ? order[i] : i;
    keys[old] = cent[i];
    vals[old] = (uint32_t)i;
  }
}

__global__ void k_max_u32(int64_t n, const uint32_t *x, uint32_t *out) {
  uint32_t m = 0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    m = max(m, x[i]);
  block_reduce_atomic(m, 0u, mgx_op_max(), [&](uint32_t s) { atomicMax(out, s); });
}

// Adjacent-pair convergence test over the descending-sorted order
// (katz.cpp:206-213): violation if ur(order[i]) - eps >= lr(order[i-1]).
__global__ void k_katz_check(int64_t n, const uint32_t *order, const double *lr,
                             const double *ur, double eps, uint32_t *violated) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x + 1; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    if (ur[order[i]] - eps >= lr[order[i - 1]]) atomicOr(violated, 1u);
  }
}

}  // namespace

mgx_status mgx_katz_impl(mgx_context *ctx, mgx_graph *g, double alpha, double epsilon,
                         double *out_centrality, int64_t *iterations) {
  if (!(g->flags & MGX_BUILD_IN_CSR)) {
    mgx_set_error("katz needs a graph built with MGX_BUILD_IN_CSR");
    return MGX_ERR_INVALID_ARGUMENT;
  }
  const int64_t V = g->n_vertices;
  if (iterations) *iterations = 0;
  if (V == 0) return MGX_OK;
  if (out_centrality) {
    for (int64_t v = 0; v < V; ++v) out_centrality[v] = 0.0;
  }
  // SetKatz early-outs on an edgeless graph (katz.cpp:398-400).
  if (g->n_edges == 0) return MGX_OK;

  // MaxDegree over OUT-degrees (katz.cpp:137-148 / mg_graph.hpp:96-109).
  mgx_scope bufs(ctx);
  uint32_t *d_max = nullptr;
  MGX_TRY(bufs.alloc(&d_max, 1));
  MGX_HIP_TRY(hipMemsetAsync(d_max, 0, 4, ctx->stream));
  hipLaunchKernelGGL(k_max_u32, dim3((uint32_t)grid_for(V)), dim3(kBlock), 0, ctx->stream,
                     V, g->out_degree, d_max);
  uint32_t deg_max = 0;
  MGX_HIP_TRY(hipMemcpyAsync(&deg_max, d_max, 4, hipMemcpyDeviceToHost, ctx->stream));
  MGX_HIP_TRY(hipStreamSynchronize(ctx->stream));
  bufs.release(d_max);
  const double gamma = (double)deg_max / (1.0 - alpha * alpha * (double)deg_max);

  double *omega[2] = {nullptr, nullptr}, *cent = nullptr, *lr = nullptr, *ur = nullptr;
  MGX_TRY(bufs.alloc(&omega[0], V));
  MGX_TRY(bufs.alloc(&omega[1], V));
  MGX_TRY(bufs.alloc(&cent, V));
  MGX_TRY(bufs.alloc(&lr, V));
  MGX_TRY(bufs.alloc(&ur, V));
  hipLaunchKernelGGL(mgx_k_fill<double>, dim3((uint32_t)grid_for(V)), dim3(kBlock), 0, ctx->stream,
                     V, 1.0, omega[0]);  // omega_0 = 1 (katz.cpp:41-44)
  MGX_HIP_TRY(hipMemsetAsync(cent, 0, V * sizeof(double), ctx->stream));
  MGX_HIP_TRY(hipMemsetAsync(lr, 0, V * sizeof(double), ctx->stream));
  MGX_HIP_TRY(hipMemsetAsync(ur, 0, V * sizeof(double), ctx->stream));

  // Sort buffers for the convergence test.
  double *keys_in = nullptr, *keys_out = nullptr;
  uint32_t *vals_in = nullptr, *vals_out = nullptr, *d_flag = nullptr;
  MGX_TRY(bufs.alloc(&keys_in, V));
  MGX_TRY(bufs.alloc(&keys_out, V));
  MGX_TRY(bufs.alloc(&vals_in, V));
  MGX_TRY(bufs.alloc(&vals_out, V));
  MGX_TRY(bufs.alloc(&d_flag, 1));

  KatzArgs A;
  A.row_ptr = g->in_row_ptr;
  A.col = g->in_col;
  const int64_t goff = mgx_fill_sections(g->bins_in, &A.bins);
  A.centrality = cent;
  A.lr = lr;
  A.ur = ur;

  int cur = 0;
  int64_t iter = 0;
  mgx_status status = MGX_OK;
  while (true) {
    ++iter;
    A.omega_old = omega[cur];
    A.omega_new = omega[1 - cur];
    A.a_i = pow(alpha, (double)iter);
    A.a_i1g = pow(alpha, (double)(iter + 1)) * gamma;
    hipLaunchKernelGGL(k_katz_sweep, dim3((uint32_t)goff), dim3(kBlock), 0, ctx->stream, A);
    cur = 1 - cur;

    // Stable descending sort of (centrality, original id): the stage kernel
    // places entries in original-id order, so stability gives the oracle's
    // tie rule; values are permuted indices for the lr/ur lookups.
    hipLaunchKernelGGL(k_sort_stage, dim3((uint32_t)grid_for(V)), dim3(kBlock), 0,
                       ctx->stream, V, cent, g->order, keys_in, vals_in);
    status = mgx_with_temp(ctx, "katz convergence sort", [&](void *tmp, size_t &bytes) {
      return rocprim::radix_sort_pairs_desc(tmp, bytes, keys_in, keys_out, vals_in, vals_out,
                                            V, 0, 64, ctx->stream);
    });
    if (status != MGX_OK) break;

    MGX_HIP_TRY(hipMemsetAsync(d_flag, 0, 4, ctx->stream));
    hipLaunchKernelGGL(k_katz_check, dim3((uint32_t)grid_for(V)), dim3(kBlock), 0,
                       ctx->stream, V, vals_out, lr, ur, epsilon, d_flag);
    uint32_t violated = 0;
    MGX_HIP_TRY(hipMemcpyAsync(&violated, d_flag, 4, hipMemcpyDeviceToHost, ctx->stream));
    MGX_HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (!violated) break;
    if (iter > 1000000) {  // safety net, not in reference
      mgx_set_error("katz did not converge in 1e6 iterations");
      status = MGX_ERR_INVALID_ARGUMENT;
      break;
    }
  }

  if (status == MGX_OK && out_centrality) {
    // in-CSR lives in the hot-first permuted space: scatter back to
    // original ids on device, then one contiguous D2H.
    double *scat = keys_in;  // reuse
    hipLaunchKernelGGL(k_scatter_f64, dim3((uint32_t)grid_for(V)), dim3(kBlock), 0,
                       ctx->stream, V, cent, g->order, scat);
    MGX_HIP_TRY(hipMemcpyAsync(out_centrality, scat, V * sizeof(double),
                               hipMemcpyDeviceToHost, ctx->stream));
    MGX_HIP_TRY(hipStreamSynchronize(ctx->stream));
  }
  if (iterations) *iterations = iter;
  MGX_HIP_TRY(hipGetLastError());
  return status;
}
