// Dealt hot-first renumbering for the XCD-striped PageRank sweep.
//
// Hot-first positions (descending out-degree) are dealt to 8 stripes in
// granules of 16 vertices — one 64-byte line of the f32 contrib vector:
// position p lies in granule q = p / 16, which goes to stripe q % 8 as that
// stripe's granule number q / 8. Each stripe is a contiguous id range
// [off[x], off[x+1]) that is hot-first inside, and the eight stripes carry
// near-equal shares of the gathers. Only the last granule overall can be
// partial, and it is the last one of its stripe, so the map is a bijection
// onto [0, V) for every V.
//
// Plain C++ (host and device): checked on the CPU by tests/test_xcd_deal_cpu.py.
#ifndef MGX_XCD_DEAL_H
#define MGX_XCD_DEAL_H

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MGX_HD __host__ __device__
#else
#define MGX_HD
#endif

constexpr int kXcdStripes = 8;
constexpr int kXcdGranule = 16;

// First id of stripe x (x in 0..8; x = 8 gives V): the exact prefix sum of
// the stripe sizes.
MGX_HD inline int64_t mgx_xcd_stripe_off(int64_t V, int x) {
  const int64_t G = (V + kXcdGranule - 1) / kXcdGranule;  // granules, the last may be partial
  if (G == 0) return 0;
  const int64_t rem = G % kXcdStripes;
  // granules q < G with q % 8 < x
  const int64_t before = (G / kXcdStripes) * x + (rem < x ? rem : x);
  int64_t off = before * kXcdGranule;
  if ((G - 1) % kXcdStripes < x) off -= G * kXcdGranule - V;  // the partial granule's gap
  return off;
}

// Hot-first position p in [0, V) -> dealt vertex id.
MGX_HD inline int64_t mgx_xcd_deal(int64_t p, int64_t V) {
  const int64_t q = p / kXcdGranule;
  const int x = (int)(q % kXcdStripes);
  return mgx_xcd_stripe_off(V, x) + (q / kXcdStripes) * kXcdGranule + p % kXcdGranule;
}

#endif  // MGX_XCD_DEAL_H
