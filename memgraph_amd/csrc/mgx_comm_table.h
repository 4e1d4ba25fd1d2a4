// Community-keyed open-addressing table shared by the Louvain and Leiden
// sweeps: i32 keys (-1 = empty), f64 values, power-of-two capacity, linear
// probing, no deletion. The table is a per-wave LDS region for rows under 256
// neighbours and a region of a global pool for hub rows; the helpers take
// ordinary pointers and must inline so that the address space is inferred at
// the call site (LDS callers keep ds_ atomics). Include from .hip files only.
#ifndef MGX_COMM_TABLE_H
#define MGX_COMM_TABLE_H

#include <hip/hip_runtime.h>

#include <cstdint>

// Home slot of community cid; mask = capacity - 1.
__device__ __forceinline__ uint32_t comm_slot(int32_t cid, uint32_t mask) {
  return ((uint32_t)cid * 2654435761u) & mask;
}

// vals[cid] += w, claiming a slot for cid on first sight. The capacity is at
// least twice the number of distinct keys a row can insert, so the probe ends.
__device__ __forceinline__ void comm_add(int32_t *keys, double *vals, uint32_t mask,
                                         int32_t cid, double w) {
  uint32_t h = comm_slot(cid, mask);
  while (true) {
    const int32_t prev = atomicCAS(&keys[h], -1, cid);
    if (prev == -1 || prev == cid) break;
    h = (h + 1) & mask;
  }
  atomicAdd(&vals[h], w);
}

// The value stored for cid (0.0 and *found = false when it has none), after
// all comm_add calls are visible. kStopAtEmpty ends the probe at the first
// empty slot; without it every one of the cap slots is examined, so an entry
// is found even where the probe chain to it is broken.
template <bool kStopAtEmpty>
__device__ __forceinline__ double comm_find(const int32_t *keys, const double *vals,
                                            uint32_t mask, uint32_t cap, int32_t cid,
                                            bool *found) {
  uint32_t h = comm_slot(cid, mask);
  double v = 0.0;
  *found = false;
  for (uint32_t probe = 0; probe < cap; ++probe) {
    const int32_t k = keys[h];
    if (k == cid) {
      v = vals[h];
      *found = true;
      break;
    }
    if (kStopAtEmpty && k == -1) break;
    h = (h + 1) & mask;
  }
  return v;
}

// Wave-level LDS completion + compiler ordering: a per-wave table region is
// touched only by its wave's 64 lanes, so draining lgkmcnt after the write
// phase makes every lane's LDS writes visible to every lane's subsequent
// reads (no cross-wave traffic => no s_barrier needed).
__device__ __forceinline__ void wave_lds_fence() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}

#endif  // MGX_COMM_TABLE_H
