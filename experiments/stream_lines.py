"""Cache lines the XCD-striped PageRank launch touches when it reads its
column ids, counted on the CPU (profiles/stream_cols.md, DESIGN.md lever 6).

usage: python experiments/stream_lines.py [scale ...]     (default 20 22)

The script follows the product's layout: RMAT (seed 1, edge factor 16),
hot-first order by descending out-degree (stable), dealt to 8 stripes in
granules of 16 ids (mgx_xcd_deal.h), rows in id order, columns sorted, one
segment per (row, stripe). For the rows of in-degree >= 64 (the heavy rows)
and of in-degree 8..63 it prints the non-empty segments, their mean and median
length, and the 64- and 128-byte lines they touch in the row-major in_col,
every segment counted on its own because another XCD reads its neighbours,
against the same ints read as one contiguous stream ("ideal"). For the heavy
rows it also prints the length of the stripe-major stream with its alignment
padding (mgx_xcd_stream.h), whose windows are read front to back.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from memgraph_amd.rmat import gen_rmat  # noqa: E402

STRIPES, GRANULE, ALIGN = 8, 16, 32


def stripe_off(nv, x):
    g = (nv + GRANULE - 1) // GRANULE
    rem = g % STRIPES
    off = ((g // STRIPES) * x + min(rem, x)) * GRANULE
    if g and (g - 1) % STRIPES < x:
        off -= g * GRANULE - nv
    return off


def segments(scale):
    """Start and length in in_col of every (row, stripe) segment, [V, 8], and
    the rows' in-degrees."""
    nv = 1 << scale
    src, dst = gen_rmat(scale, 16 << scale, seed=1)
    hot = np.argsort(-np.bincount(src, minlength=nv), kind="stable")
    p = np.arange(nv)
    q = p // GRANULE
    off = np.array([stripe_off(nv, x) for x in range(STRIPES + 1)])
    new_id = np.empty(nv, dtype=np.int64)
    new_id[hot] = off[q % STRIPES] + (q // STRIPES) * GRANULE + p % GRANULE
    nsrc, ndst = new_id[src], new_id[dst]
    indeg = np.bincount(ndst, minlength=nv)
    row_ptr = np.concatenate([[0], np.cumsum(indeg)])
    stripe_of = np.searchsorted(off, nsrc, side="right") - 1
    length = np.bincount(ndst * STRIPES + stripe_of, minlength=nv * STRIPES).reshape(nv, STRIPES)
    # Columns are sorted within a row, so the stripes of a row follow each other.
    start = row_ptr[:-1, None] + np.cumsum(length, axis=1) - length
    return start, length, indeg


def lines(start, length, line_bytes):
    per = line_bytes // 4
    return int(((start + length - 1) // per - start // per + 1).sum())


def stream_ints(start, length):
    """Length of the stripe-major stream of these rows: per stripe the
    segments of >= 64 ints in allotments of ((lo & 3) + len + 3) & ~3, the
    shorter ones packed, the stripe's window rounded up to ALIGN ints."""
    total = 0
    for x in range(STRIPES):
        lo, ln = start[:, x], length[:, x]
        wide = ln >= 64
        ints = int(((((lo[wide] & 3) + ln[wide] + 3) >> 2) << 2).sum()) + int(ln[~wide].sum())
        total += (ints + ALIGN - 1) // ALIGN * ALIGN
    return total


def main():
    scales = [int(a) for a in sys.argv[1:]] or [20, 22]
    print("scale rows share_of_E segments mean median x64 x128 stream_ints/ints")
    for scale in scales:
        start, length, indeg = segments(scale)
        edges = int(indeg.sum())
        for name, rows in (("in-degree>=64", indeg >= 64), ("in-degree8..63", (indeg >= 8) & (indeg < 64))):
            s, ln = start[rows].ravel(), length[rows].ravel()
            keep = ln > 0
            s, ln = s[keep], ln[keep]
            ints = int(ln.sum())
            ratios = [lines(s, ln, b) / -(-ints * 4 // b) for b in (64, 128)]
            stream = stream_ints(start[rows], length[rows]) / ints
            print(f"{scale} {name} {ints / edges:.2f} {len(ln):.2e} {ln.mean():.1f} "
                  f"{int(np.median(ln))} x{ratios[0]:.2f} x{ratios[1]:.2f} {stream:.4f}")


if __name__ == "__main__":
    main()
