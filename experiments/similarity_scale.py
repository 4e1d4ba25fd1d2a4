"""Node similarity at scale: RMAT-20 (E = 16 V, seed 1, out-CSR). In one
process, on one graph, Jaccard:

  (a) 2^22 seeded random pairs,
  (b) every pair i < j among the 2048 highest out-degree vertices,
      each in AUTO, forced SEARCH and forced MERGE (HIP-event stats.ms);
  (c) mgx_similarity_all at RMAT-14: kernel ms, prep ms, the rest of the host
      clock (download into pageable memory) and the chunk count.

Before any timing the three modes are checked bit-equal on (a) and (b), and
(c) against the pairs path on its first 2^20 pairs. One warm-up call per
variant (the parity calls), then REPEATS timed calls with the variants
alternated; median and min/max are reported.

Algorithmic bytes of the timed kernels (what the formulation has to move,
caches aside). A pair whose shorter row is empty is dropped by the binning
and costs the kernels nothing (its zeros are written during prep). Every
other pair: 44 B fixed (its 4-B work-list entry, two 4-B ids, four 4-B
row_ptr entries, the 8-B count and the 8-B quotient) plus, with s <= l the
distinct degrees,
  SEARCH  4 s (the shorter row) + 4 s ceil(log2(l+1)) (one 4-B probe per step)
  MERGE   4 (s + l)
  AUTO    whichever the rule s ceil(log2(l+1)) < s + l picks.
All-pairs: each tile of 8 rows streams every row above its first row once
(4 B per entry, and the tile's own rows once more for the bitmaps), and every
pair is cleared and written once on the device (16 B).

Usage: python experiments/similarity_scale.py [scale] [out.json] [all_scale]
"""
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from memgraph_amd.native import (BUILD_OUT_CSR, SIM_AUTO, SIM_JACCARD, SIM_MERGE,  # noqa: E402
                                 SIM_SEARCH, Native, SimilarityStats)

SCALE = int(sys.argv[1]) if len(sys.argv) > 1 else 20
OUT = sys.argv[2] if len(sys.argv) > 2 else None
ALL_SCALE = int(sys.argv[3]) if len(sys.argv) > 3 else 14
REPEATS = 7
PEAK_BYTES_PER_S = 8.0e12  # HBM3E spec, the peak every roofline in DESIGN.md uses
MODES = {"auto": SIM_AUTO, "search": SIM_SEARCH, "merge": SIM_MERGE}
_I64 = ctypes.POINTER(ctypes.c_int64)
_F64 = ctypes.POINTER(ctypes.c_double)

nat = Native()
assert nat.device_count() > 0, "similarity_scale needs a HIP device"
ctx = nat.init(0)


def host_edges(scale):
    """The same deterministic edge stream the device graph is built from."""
    nv, ne = 1 << scale, 16 << scale
    src = np.zeros(ne, dtype=np.int64)
    dst = np.zeros(ne, dtype=np.int64)
    nat._check(nat.lib.mgx_gen_edges_to_host(
        ctx, ctypes.c_int(1), ctypes.c_int(scale), ctypes.c_int64(nv), ctypes.c_int64(ne),
        ctypes.c_uint64(1), ctypes.c_double(0.57), ctypes.c_double(0.19),
        ctypes.c_double(0.19), src.ctypes.data_as(_I64), dst.ctypes.data_as(_I64)),
        "mgx_gen_edges_to_host")
    return nv, ne, src, dst


def distinct_degrees(nv, src, dst):
    keys = np.unique(src * nv + dst)
    return np.bincount(keys // nv, minlength=nv), len(keys)


def summary(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1], "n": len(xs)}


def bit_length(x):
    out = np.zeros(len(x), dtype=np.int64)
    nz = x > 0
    out[nz] = np.floor(np.log2(x[nz])).astype(np.int64) + 1
    return out


def algorithmic_bytes(ddeg, u, v):
    s = np.minimum(ddeg[u], ddeg[v]).astype(np.int64)
    l = np.maximum(ddeg[u], ddeg[v]).astype(np.int64)
    search = 4 * s + 4 * s * bit_length(l)
    merge = 4 * (s + l)
    merge[s == 0] = 0   # dropped by the binning
    search[s == 0] = 0
    pick_search = s * bit_length(l) < s + l
    fixed = 44 * int((s > 0).sum())
    return {"search": int(fixed + search.sum()), "merge": int(fixed + merge.sum()),
            "auto": int(fixed + np.where(pick_search, search, merge).sum())}


def call_pairs(g, u, v, mode, sim, common):
    st = SimilarityStats()
    nat._check(nat.lib.mgx_similarity_pairs(
        ctx, g, ctypes.c_int(SIM_JACCARD), ctypes.c_int(mode), u.ctypes.data_as(_I64),
        v.ctypes.data_as(_I64), ctypes.c_int64(len(u)), sim.ctypes.data_as(_F64),
        common.ctypes.data_as(_I64), ctypes.byref(st)), "mgx_similarity_pairs")
    return st


V, E, src, dst = host_edges(SCALE)
ddeg, n_distinct = distinct_degrees(V, src, dst)
outdeg = np.bincount(src, minlength=V)
del src, dst
g = nat.graph_rmat(ctx, SCALE, E, seed=1, flags=BUILD_OUT_CSR)
print(f"RMAT-{SCALE}: V={V} E={E} distinct={n_distinct} "
      f"(built in {nat.graph_build_ms(g):.0f} ms)", flush=True)

rng = np.random.default_rng(1)
hubs = np.sort(np.argsort(-outdeg, kind="stable")[:2048])
hi, hj = np.triu_indices(len(hubs), 1)
workloads = {
    "a_random_pairs": (rng.integers(0, V, 1 << 22), rng.integers(0, V, 1 << 22)),
    "b_hub_pairs": (hubs[hi], hubs[hj]),
}

result = {
    "graph": {"kind": "rmat", "scale": SCALE, "V": V, "E": E, "seed": 1,
              "flags": "BUILD_OUT_CSR", "distinct_entries": n_distinct},
    "metric": "jaccard", "repeats": REPEATS,
}
parity_ok = True
for name, (u, v) in workloads.items():
    u = np.ascontiguousarray(u, dtype=np.int64)
    v = np.ascontiguousarray(v, dtype=np.int64)
    n = len(u)
    bufs = {m: (np.zeros(n), np.zeros(n, dtype=np.int64)) for m in MODES}
    first = {m: call_pairs(g, u, v, MODES[m], *bufs[m]) for m in MODES}  # parity + warm-up
    equal = all(np.array_equal(bufs["auto"][0], bufs[m][0]) and
                np.array_equal(bufs["auto"][1], bufs[m][1]) for m in ("search", "merge"))
    parity_ok &= equal and first["auto"].distinct_entries == n_distinct
    ms = {m: [] for m in MODES}
    prep = {m: [] for m in MODES}
    for _ in range(REPEATS):  # alternate: drift on a shared host hits all alike
        for m in MODES:
            st = call_pairs(g, u, v, MODES[m], *bufs[m])
            ms[m].append(st.ms)
            prep[m].append(st.prep_ms)
    ab = algorithmic_bytes(ddeg, u, v)
    s = np.minimum(ddeg[u], ddeg[v])
    l = np.maximum(ddeg[u], ddeg[v])
    entry = {"pairs": n, "modes_bit_equal": bool(equal),
             "nonzero_common": int((bufs["auto"][1] > 0).sum()),
             "shorter_degree_mean": float(s.mean()), "longer_degree_mean": float(l.mean()),
             "longer_degree_max": int(l.max()),
             "auto_search_pairs": int(first["auto"].search_pairs),
             "auto_merge_pairs": int(first["auto"].merge_pairs)}
    for m in MODES:
        med = summary(ms[m])["median"]
        entry[m] = {"ms_event": summary(ms[m]), "prep_ms_event": summary(prep[m]),
                    "pairs_per_s": n / (med * 1e-3), "algorithmic_bytes": ab[m],
                    "roofline_frac_of_8TBps": ab[m] / (med * 1e-3) / PEAK_BYTES_PER_S}
    result[name] = entry
    print(name, json.dumps(entry, indent=1), flush=True)
    del bufs
nat.graph_destroy(ctx, g)

# (c) all pairs
AV, AE, asrc, adst = host_edges(ALL_SCALE)
addeg, a_distinct = distinct_degrees(AV, asrc, adst)
del asrc, adst
ga = nat.graph_rmat(ctx, ALL_SCALE, AE, seed=1, flags=BUILD_OUT_CSR)
total = AV * (AV - 1) // 2
out = np.zeros(total)


def call_all():
    st = SimilarityStats()
    t0 = time.perf_counter()
    nat._check(nat.lib.mgx_similarity_all(ctx, ga, ctypes.c_int(SIM_JACCARD),
                                          out.ctypes.data_as(_F64), ctypes.byref(st)),
               "mgx_similarity_all")
    return (time.perf_counter() - t0) * 1e3, st


call_all()  # warm-up; then parity on the first 2^20 pairs (rows 0..)
k = min(total, 1 << 20)
rows = 0
while rows * (2 * AV - rows - 1) // 2 < k:
    rows += 1
pi = np.repeat(np.arange(rows), AV - 1 - np.arange(rows))[:k].astype(np.int64)
pj = np.concatenate([np.arange(i + 1, AV) for i in range(rows)])[:k].astype(np.int64)
psim, pcommon = np.zeros(k), np.zeros(k, dtype=np.int64)
call_pairs(ga, pi, pj, SIM_AUTO, psim, pcommon)
all_equal = bool(np.array_equal(out[:k], psim))
parity_ok &= all_equal
runs = [call_all() for _ in range(REPEATS)]
st = runs[0][1]
kernel = summary([s.ms for _, s in runs])
# entries streamed: tile t reads its own rows and every row above its first
csum = np.concatenate([[0], np.cumsum(addeg)])
firsts = np.arange(0, AV - 1, 8)
streamed = int(((csum[AV] - csum[np.minimum(firsts + 1, AV)]) +
                (csum[np.minimum(firsts + 8, AV)] - csum[firsts])).sum())
alg = 4 * streamed + 16 * total
result["c_all_pairs"] = {
    "graph": {"kind": "rmat", "scale": ALL_SCALE, "V": AV, "E": AE, "seed": 1,
              "distinct_entries": a_distinct},
    "pairs": total, "chunks": int(st.chunks), "equals_pairs_path_on_first_2^20": all_equal,
    "kernel_ms_event": kernel,
    "prep_ms_event": summary([s.prep_ms for _, s in runs]),
    "host_ms": summary([h for h, _ in runs]),
    "download_ms_host_minus_events": summary([h - s.ms - s.prep_ms for h, s in runs]),
    "pairs_per_s_kernel": total / (kernel["median"] * 1e-3),
    "entries_streamed": streamed, "algorithmic_bytes": int(alg),
    "roofline_frac_of_8TBps": alg / (kernel["median"] * 1e-3) / PEAK_BYTES_PER_S,
}
print("c_all_pairs", json.dumps(result["c_all_pairs"], indent=1), flush=True)
result["parity_ok"] = bool(parity_ok)
if OUT:
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(result, f, indent=1)
nat.graph_destroy(ctx, ga)
nat.destroy(ctx)
assert parity_ok
print("OK", flush=True)
