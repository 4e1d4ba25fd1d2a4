// Device side of the online modules' persistent state (pronline.hip,
// katz_online.hip, labelrankt.hip): the grow-only arrays a state struct owns.
// The host side, slot table and capacity rule, is mgx_slot_table.h.
//
// A module's state lives behind a reference to a `new`ed struct that is never
// deleted, and reset is the move-assignment of a fresh struct: the arrays free
// their blocks then, and no HIP call runs from a static destructor, when the
// runtime may be gone.
// Include from .hip files only.
#ifndef MGX_ONLINE_H
#define MGX_ONLINE_H

#include <vector>

#include "mgx_device.h"
#include "mgx_slot_table.h"

// What ensure() writes into a new block before the old contents are copied in.
inline auto mgx_fill_none() {
  return [](auto *, int64_t) { return MGX_OK; };
}
inline auto mgx_fill_zero(mgx_context *ctx) {
  return [ctx](auto *p, int64_t n) -> mgx_status {
    MGX_HIP_TRY(hipMemsetAsync(p, 0, (size_t)n * sizeof(*p), ctx->stream));
    return MGX_OK;
  };
}
template <typename T>
inline auto mgx_fill_value(mgx_context *ctx, T v) {
  return [ctx, v](T *p, int64_t n) {
    hipLaunchKernelGGL(mgx_k_fill<T>, dim3((uint32_t)grid_for(n)), dim3(kBlock), 0, ctx->stream,
                       n, v, p);
    return MGX_OK;
  };
}

// A persistent, grow-only device array of a state struct: plain hipMalloc
// (mgx_hip_malloc), never the context cache. Move-only; reads as its pointer.
template <typename T>
struct mgx_dev_array {
  T *ptr = nullptr;
  int64_t cap = 0;  // elements

  mgx_dev_array() = default;
  mgx_dev_array(mgx_dev_array &&o) noexcept : ptr(o.ptr), cap(o.cap) {
    o.ptr = nullptr;
    o.cap = 0;
  }
  mgx_dev_array &operator=(mgx_dev_array &&o) noexcept {
    if (this != &o) {
      reset();
      ptr = o.ptr;
      cap = o.cap;
      o.ptr = nullptr;
      o.cap = 0;
    }
    return *this;
  }
  ~mgx_dev_array() { reset(); }
  operator T *() const { return ptr; }

  void reset() {
    if (ptr) {
      (void)hipFree(ptr);
      mgx_state_blocks_add(-1);
    }
    ptr = nullptr;
    cap = 0;
  }

  // Take over block p of c elements from the scope that allocated it
  // (alloc_plain); the block held so far is freed.
  void adopt(mgx_scope &own, T *p, int64_t c) {
    reset();
    ptr = own.give_up(p);
    cap = c;
    mgx_state_blocks_add(1);
  }

  // Room for `need` elements: mgx_grown_cap from first_cap. A new block is
  // initialised by fill(block, capacity), receives the first `keep` elements
  // of the old one and replaces it once that copy has completed. On any
  // failure ptr and cap are as they were.
  template <typename Fill>
  mgx_status ensure(mgx_context *ctx, int64_t need, int64_t first_cap, int64_t keep,
                    Fill fill) {
    const int64_t grown_cap = mgx_grown_cap(cap, mgx_state_first_cap(first_cap), need);
    if (grown_cap == cap) return MGX_OK;
    mgx_scope grown(ctx);
    T *np = nullptr;
    MGX_TRY(grown.alloc_plain(&np, grown_cap));
    MGX_TRY(fill(np, grown_cap));
    if (ptr) {
      if (keep > 0)
        MGX_HIP_TRY(hipMemcpyAsync(np, ptr, (size_t)keep * sizeof(T), hipMemcpyDeviceToDevice,
                                   ctx->stream));
      MGX_HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    adopt(grown, np, grown_cap);
    return MGX_OK;
  }
};

// A host list as a device array owned by `own` (plain allocation; an empty list
// still gets one element's room). The copy is queued on the scope's stream.
inline mgx_status mgx_upload_i32(mgx_scope &own, const std::vector<int32_t> &v, int32_t **d) {
  MGX_TRY(own.alloc_plain(d, (int64_t)v.size()));
  if (!v.empty())
    MGX_HIP_TRY(hipMemcpyAsync(*d, v.data(), v.size() * 4, hipMemcpyHostToDevice,
                               own.ctx->stream));
  return MGX_OK;
}

#endif  // MGX_ONLINE_H
