// Weakly connected components on gfx950 — replaces Weak
// (reference connectivity_module.cpp:41-87).
//
// Min-label propagation over the symmetric CSR with pointer-jumping
// compression; at the fixpoint label[v] = min vertex id of v's component.
// Component ids are then renumbered by ascending representative id, which
// is EXACTLY the reference's BFS discovery order (the reference roots its
// BFS at the first unvisited vertex in scan order, i.e. each component is
// discovered at its min member — DESIGN.md), so emitted ids are bit-exact.

#include <cstring>

#include <rocprim/rocprim.hpp>

#include "mgx_device.h"

namespace {

struct WccArgs {
  const uint32_t *row_ptr;
  const int32_t *col;
  mgx_bin_sections bins;
  int32_t *label;       // in-place (async min-propagation is monotone-safe)
  uint32_t *changed;
};

template <int LANES>
__device__ inline bool wcc_rows(const WccArgs &A, int sec, int64_t block_in_sec) {
  bool changed = false;
  reduce_bin_rows<LANES>(
      A.bins, sec, block_in_sec, INT32_MAX, mgx_op_min(),
      [&](int32_t row, int sub) {
        int32_t m = INT32_MAX;
        row_gather<LANES>(A.col, A.row_ptr[row], A.row_ptr[row + 1], sub,
                          [&](int32_t c) { m = min(m, A.label[c]); });
        return m;
      },
      [&](int32_t row, int32_t m) {
        if (m < A.label[row]) {
          A.label[row] = m;
          changed = true;
        }
      });
  return changed;
}

__global__ void __launch_bounds__(kBlock) k_wcc_sweep(WccArgs A) {
  bool ch = false;
  for_bin_section(A.bins.goff, [&](auto lanes, int sec, int64_t bis) {
    ch = wcc_rows<decltype(lanes)::value>(A, sec, bis);
  });
  if (ch) atomicOr(A.changed, 1u);
}

// Pointer jumping: label[v] <- label[label[v]] until per-pass fixpoint
// (monotone decreasing; races only skip a shortcut, never break it).
__global__ void k_wcc_jump(int64_t n, int32_t *label, uint32_t *changed) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int32_t l = label[i];
    const int32_t ll = label[l];
    if (ll < l) {
      label[i] = ll;
      atomicOr(changed, 1u);
    }
  }
}

// Renumber by ascending representative id: flag roots, exclusive-scan,
// comp[v] = scan[label[v]].
__global__ void k_wcc_flag_roots(int64_t n, const int32_t *label, uint32_t *flag) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    flag[i] = (label[i] == (int32_t)i) ? 1u : 0u;
}

__global__ void k_wcc_emit(int64_t n, const int32_t *label, const uint32_t *scan,
                           int64_t *out) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    out[i] = (int64_t)scan[label[i]];
}

}  // namespace

// Min-member labels left on the device: *out_label is a context allocation
// of V int32 owned by the caller's scope `own` (V > 0, sym-CSR present; all
// work is queued on ctx->stream and the fixpoint loop has synchronized when
// this returns).
mgx_status mgx_wcc_labels_device(mgx_scope &own, mgx_graph *g, int32_t **out_label) {
  mgx_context *ctx = own.ctx;
  const int64_t V = g->n_vertices;
  mgx_scope bufs(ctx);
  int32_t *label = nullptr;
  uint32_t *d_changed = nullptr;
  MGX_TRY(own.alloc(&label, V));
  MGX_TRY(bufs.alloc(&d_changed, 1));
  hipLaunchKernelGGL(mgx_k_iota<int32_t>, dim3((uint32_t)grid_for(V)), dim3(kBlock), 0,
                     ctx->stream, V, label);

  WccArgs A;
  A.row_ptr = g->sym_row_ptr;
  A.col = g->sym_col;
  const int64_t goff = mgx_fill_sections(g->bins_sym, &A.bins);
  A.label = label;
  A.changed = d_changed;

  uint32_t h_changed = 1;
  while (h_changed) {
    MGX_HIP_TRY(hipMemsetAsync(d_changed, 0, 4, ctx->stream));
    if (goff > 0)
      hipLaunchKernelGGL(k_wcc_sweep, dim3((uint32_t)goff), dim3(kBlock), 0, ctx->stream, A);
    hipLaunchKernelGGL(k_wcc_jump, dim3((uint32_t)grid_for(V)), dim3(kBlock), 0, ctx->stream,
                       V, label, d_changed);
    MGX_HIP_TRY(hipMemcpyAsync(&h_changed, d_changed, 4, hipMemcpyDeviceToHost,
                               ctx->stream));
    MGX_HIP_TRY(hipStreamSynchronize(ctx->stream));
  }
  *out_label = label;
  return MGX_OK;
}

mgx_status mgx_wcc_impl(mgx_context *ctx, mgx_graph *g, int64_t *out_component,
                        int64_t *n_components) {
  if (!(g->flags & MGX_BUILD_SYM_CSR)) {
    mgx_set_error("wcc needs a graph built with MGX_BUILD_SYM_CSR");
    return MGX_ERR_INVALID_ARGUMENT;
  }
  const int64_t V = g->n_vertices;
  if (V == 0) {
    if (n_components) *n_components = 0;
    return MGX_OK;
  }

  mgx_scope bufs(ctx);
  int32_t *label = nullptr;
  MGX_TRY(mgx_wcc_labels_device(bufs, g, &label));

  // Renumber + count.
  uint32_t *flag = nullptr, *scan = nullptr;
  MGX_TRY(bufs.alloc(&flag, V));
  MGX_TRY(bufs.alloc(&scan, V + 1));
  hipLaunchKernelGGL(k_wcc_flag_roots, dim3((uint32_t)grid_for(V)), dim3(kBlock), 0,
                     ctx->stream, V, label, flag);
  MGX_TRY(mgx_with_temp(ctx, "wcc root scan", [&](void *tmp, size_t &bytes) {
    return rocprim::exclusive_scan(tmp, bytes, flag, scan, 0u, V, rocprim::plus<uint32_t>(),
                                   ctx->stream);
  }));

  int64_t *d_out = nullptr;
  MGX_TRY(bufs.alloc(&d_out, V));
  hipLaunchKernelGGL(k_wcc_emit, dim3((uint32_t)grid_for(V)), dim3(kBlock), 0, ctx->stream,
                     V, label, scan, d_out);
  if (out_component) {
    MGX_HIP_TRY(hipMemcpyAsync(out_component, d_out, V * sizeof(int64_t),
                               hipMemcpyDeviceToHost, ctx->stream));
  }
  if (n_components) {
    uint32_t last_scan = 0, last_flag = 0;
    MGX_HIP_TRY(hipMemcpyAsync(&last_scan, scan + V - 1, 4, hipMemcpyDeviceToHost,
                               ctx->stream));
    MGX_HIP_TRY(hipMemcpyAsync(&last_flag, flag + V - 1, 4, hipMemcpyDeviceToHost,
                               ctx->stream));
    MGX_HIP_TRY(hipStreamSynchronize(ctx->stream));
    *n_components = (int64_t)last_scan + last_flag;
  }
  MGX_HIP_TRY(hipStreamSynchronize(ctx->stream));
  MGX_HIP_TRY(hipGetLastError());
  return MGX_OK;
}
