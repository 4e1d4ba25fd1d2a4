// Where a stripe segment lies in the stripe-major column stream of the
// XCD-striped PageRank sweep (mgx_graph::xcd_scol, DESIGN.md lever 6).
//
// The stream holds the heavy rows' columns in the order the striped launch
// reads them: stripe by stripe, within a stripe the 256-, 64-, 16- and 4-lane
// sections in turn, within a section the order of the stripe's row list. Each
// segment gets an allotment of ints, and a segment's allotment starts where
// the exclusive sum of the allotments before it (from the stripe's base, a
// multiple of kXcdStreamAlign) puts it.
//
// The 64- and 256-lane sections read a segment [lo, hi) of in_col as a scalar
// head up to 16-byte alignment, int4 vectors and a scalar tail, so which lane
// adds which element depends on lo mod 4. Such a segment therefore starts in
// the stream at an offset = lo (mod 4): its allotment is a multiple of 4 that
// starts at a multiple of 4 (those two sections come first in a stripe) and
// the segment sits (lo & 3) ints into it. The 4- and 16-lane sections have no
// alignment logic and are packed back to back.
//
// Plain C++ (host and device): checked on the CPU by
// tests/test_xcd_stream_cpu.py.
#ifndef MGX_XCD_STREAM_H
#define MGX_XCD_STREAM_H

#include "mgx_xcd_deal.h"

// A stripe's window starts at a multiple of this many ints (128 bytes), so no
// cache line of the stream holds columns of two stripes.
constexpr uint32_t kXcdStreamAlign = 32;

// Whether bin section `sec` (0..3: 4, 16, 64, 256 lanes) reads its segments
// with the aligned vector body.
MGX_HD inline bool mgx_xcd_seg_aligned(int sec) { return sec >= 2; }

// Ints allotted to the segment [lo, lo + len) of in_col.
MGX_HD inline uint32_t mgx_xcd_seg_allot(uint32_t lo, uint32_t len, bool aligned) {
  return aligned ? ((lo & 3u) + len + 3u) & ~3u : len;
}

// First int of the segment, given the start `pos` of its allotment.
MGX_HD inline uint32_t mgx_xcd_seg_start(uint32_t pos, uint32_t lo, bool aligned) {
  return aligned ? pos + (lo & 3u) : pos;
}

// First int of the next stripe's window after a stripe that ends at `end`.
MGX_HD inline uint64_t mgx_xcd_stream_round(uint64_t end) {
  return (end + kXcdStreamAlign - 1) / kXcdStreamAlign * kXcdStreamAlign;
}

#endif  // MGX_XCD_STREAM_H
