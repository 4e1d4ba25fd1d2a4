"""BFS at scale: RMAT-24 (E = 16 V, seed 1, symmetric CSR — BASELINE.json
config 3), source = the max-degree vertex. In one process, on one graph:

  * mgx_wcc ms (host clock around the call, no download),
  * mgx_bfs ms in AUTO and forced TOP_DOWN (HIP-event stats.ms, and the host
    clock around the same no-download call for a like-for-like WCC figure),
  * per-mode stats, TEPS = input edges inside the source's component / ms,
  * parity: AUTO hops == TOP_DOWN hops bit-exact, reached == the size of the
    source's component from mgx_wcc.

One warm-up call per variant, then REPEATS timed calls; median and min/max
are reported. Usage: python experiments/bfs_scale.py [scale] [out.json]
"""
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from memgraph_amd.native import (BFS_AUTO, BFS_TOP_DOWN, BUILD_SYM_CSR, BfsStats,  # noqa: E402
                                 Native)

SCALE = int(sys.argv[1]) if len(sys.argv) > 1 else 24
OUT = sys.argv[2] if len(sys.argv) > 2 else None
REPEATS = 7
PEAK_BYTES_PER_S = 8.0e12  # HBM3E spec, the peak every roofline in DESIGN.md uses
V = 1 << SCALE
E = 16 * V
_I64 = ctypes.POINTER(ctypes.c_int64)

nat = Native()
assert nat.device_count() > 0, "bfs_scale needs a HIP device"
ctx = nat.init(0)

# The same deterministic edge stream the device graph is built from.
src = np.zeros(E, dtype=np.int64)
dst = np.zeros(E, dtype=np.int64)
nat._check(nat.lib.mgx_gen_edges_to_host(
    ctx, ctypes.c_int(1), ctypes.c_int(SCALE), ctypes.c_int64(V), ctypes.c_int64(E),
    ctypes.c_uint64(1), ctypes.c_double(0.57), ctypes.c_double(0.19), ctypes.c_double(0.19),
    src.ctypes.data_as(_I64), dst.ctypes.data_as(_I64)), "mgx_gen_edges_to_host")
deg = np.bincount(src, minlength=V) + np.bincount(dst, minlength=V)
source = int(deg.argmax())
print(f"RMAT-{SCALE}: V={V} E={E} source={source} degree={int(deg[source])}", flush=True)

g = nat.graph_rmat(ctx, SCALE, E, seed=1, flags=BUILD_SYM_CSR)
print(f"graph built ({nat.graph_build_ms(g):.0f} ms)", flush=True)


def summary(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1], "n": len(xs)}


def time_wcc():
    n = ctypes.c_int64()
    t0 = time.perf_counter()
    nat._check(nat.lib.mgx_wcc(ctx, g, None, ctypes.byref(n)), "mgx_wcc")
    return (time.perf_counter() - t0) * 1e3


def time_bfs(mode):
    st = BfsStats()
    t0 = time.perf_counter()
    nat._check(nat.lib.mgx_bfs(ctx, g, ctypes.c_int64(source), ctypes.c_int(0),
                               ctypes.c_int64(-1), ctypes.c_int(mode), None, None,
                               ctypes.byref(st)), "mgx_bfs")
    return (time.perf_counter() - t0) * 1e3, st


# Parity first (these calls are also the warm-up of every variant).
comp, n_comp = nat.wcc(ctx, g, V)
hops_auto, _, st_auto = nat.bfs(ctx, g, V, source, mode=BFS_AUTO)
hops_td, _, st_td = nat.bfs(ctx, g, V, source, mode=BFS_TOP_DOWN)
comp_size = int((comp == comp[source]).sum())
edges_in_comp = int((comp[src] == comp[source]).sum())
parity = {
    "auto_equals_top_down_hops": bool(np.array_equal(hops_auto, hops_td)),
    "reached_auto": int(st_auto.reached),
    "reached_top_down": int(st_td.reached),
    "wcc_component_size": comp_size,
    "reached_equals_component": bool(st_auto.reached == comp_size == st_td.reached
                                     == int((hops_auto >= 0).sum())),
}
print("parity", parity, flush=True)
del comp, hops_td, src, dst

# Alternate the variants so drift on a shared host hits all of them alike.
wcc_ms, bfs = [], {BFS_AUTO: [], BFS_TOP_DOWN: []}
for _ in range(REPEATS):
    wcc_ms.append(time_wcc())
    for mode in (BFS_AUTO, BFS_TOP_DOWN):
        bfs[mode].append(time_bfs(mode))


def bfs_report(mode):
    host = [h for h, _ in bfs[mode]]
    ev = [st.ms for _, st in bfs[mode]]
    st = bfs[mode][0][1]
    ms = summary(ev)["median"]
    # Algorithmic bytes: each examined CSR entry is one 4-B col read; each
    # reached vertex costs its two row_ptr reads and one hops write; plus the
    # per-call clears (hops, two queues, three bitmaps). The per-entry bitmap
    # gathers are the cache-resident part and are not counted as HBM bytes.
    words = (V + 31) // 32
    alg_bytes = 4 * st.entries_scanned + 12 * st.reached + 12 * V + 12 * words
    return {
        "ms_event": summary(ev),
        "ms_host_no_download": summary(host),
        "depth": int(st.depth),
        "reached": int(st.reached),
        "entries_scanned": int(st.entries_scanned),
        "top_down_levels": int(st.top_down_levels),
        "bottom_up_levels": int(st.bottom_up_levels),
        "bottom_up_mask": int(st.bottom_up_mask),
        "teps": edges_in_comp / (ms * 1e-3),
        "algorithmic_bytes": int(alg_bytes),
        "roofline_frac_of_8TBps": alg_bytes / (ms * 1e-3) / PEAK_BYTES_PER_S,
    }


result = {
    "graph": {"kind": "rmat", "scale": SCALE, "V": V, "E": E, "seed": 1,
              "flags": "BUILD_SYM_CSR", "source": source, "source_degree": int(deg[source]),
              "edges_in_source_component": edges_in_comp, "wcc_components": int(n_comp)},
    "repeats": REPEATS,
    "wcc_ms_host_no_download": summary(wcc_ms),
    "bfs_auto": bfs_report(BFS_AUTO),
    "bfs_top_down": bfs_report(BFS_TOP_DOWN),
    "parity": parity,
    "alpha": int(os.environ.get("MGX_BFS_ALPHA", "14")),
    "beta": int(os.environ.get("MGX_BFS_BETA", "24")),
}
print(json.dumps(result, indent=1), flush=True)
if OUT:
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(result, f, indent=1)

nat.graph_destroy(ctx, g)
nat.destroy(ctx)
assert parity["auto_equals_top_down_hops"] and parity["reached_equals_component"]
print("OK", flush=True)
