"""Bridges at scale: RMAT-24 (E = 16 V, seed 1, symmetric CSR), one process,
one graph:

  * mgx_bridges ms (HIP-event stats.ms: the whole call minus the download) and
    its split into forest (WCC + BFS), sorts and scans, the low/high sweep and
    the 3 * depth per-level launches (mgx_bridges_last_stage_ms);
  * mgx_wcc and mgx_bfs (AUTO, from the max-degree vertex) on the same graph,
    alternated with it, as the yardstick: host clock around no-download calls,
    and the same host clock around mgx_bridges for a like-for-like figure;
  * the 4096-path, to put a number on the per-level launch cost;
  * checks: at RMAT-18 pairs and all six state arrays equal
    tests/bridges_ref.py::forest_state; at the full scale two necessary
    conditions: every reported pair differs by one BFS level, and every
    degree-1 vertex's edge is reported.

One warm-up call per variant, then REPEATS timed calls; median and min/max are
reported. There is no pass/fail threshold on time.
Usage: python experiments/bridges_scale.py [scale] [out.json]
"""
import ctypes
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
import bridges_ref  # noqa: E402
from memgraph_amd.native import (BFS_AUTO, BUILD_SYM_CSR, BfsStats, BridgesStats,  # noqa: E402
                                 Native)
from memgraph_amd.rmat import gen_rmat  # noqa: E402

SCALE = int(sys.argv[1]) if len(sys.argv) > 1 else 24
OUT = sys.argv[2] if len(sys.argv) > 2 else None
CHECK_SCALE = min(18, SCALE)
REPEATS = 7
_I64 = ctypes.POINTER(ctypes.c_int64)

nat = Native()
assert nat.device_count() > 0, "bridges_scale needs a HIP device"
ctx = nat.init(0)


def summary(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1], "n": len(xs)}


def time_bridges(g, u, v):
    st = BridgesStats()
    n = ctypes.c_int64()
    t0 = time.perf_counter()
    nat._check(nat.lib.mgx_bridges(ctx, g, u.ctypes.data_as(_I64), v.ctypes.data_as(_I64),
                                   ctypes.byref(n), ctypes.byref(st)), "mgx_bridges")
    host = (time.perf_counter() - t0) * 1e3
    return host, st, nat.bridges_last_stage_ms()


def bridges_report(runs):
    st = runs[0][1]
    rep = {
        "ms_event": summary([s.ms for _, s, _ in runs]),
        "ms_host_with_download": summary([h for h, _, _ in runs]),
        "bridges": int(st.bridges), "trees": int(st.trees), "depth": int(st.depth),
        "nontree_entries": int(st.nontree_entries), "level_launches": int(st.level_launches),
    }
    for stage in ("forest", "sorts_scans", "sweep", "levels"):
        rep["ms_" + stage] = summary([sp[stage] for _, _, sp in runs])
    return rep


# ---- equality with forest_state at the check scale ----
cv = 1 << CHECK_SCALE
csrc, cdst = gen_rmat(CHECK_SCALE, 16 * cv, seed=1)
g = nat.graph_from_coo(ctx, csrc, cdst, cv, flags=BUILD_SYM_CSR)
pairs, st = nat.bridges(ctx, g, cv)
state = nat.bridges_state(ctx, g, cv)
nat.graph_destroy(ctx, g)
fs = bridges_ref.forest_state(cv, csrc, cdst)
check = {"scale": CHECK_SCALE, "bridges": int(st.bridges), "trees": int(st.trees),
         "depth": int(st.depth),
         "pairs_equal": [tuple(r) for r in pairs.tolist()] == fs.bridges,
         "state_equal": all(np.array_equal(state[k], getattr(fs, k))
                            for k in bridges_ref.STATE_ARRAYS)}
print("check", check, flush=True)
assert check["pairs_equal"] and check["state_equal"]
del csrc, cdst, state, fs

# ---- the per-level launch cost: a 4096-path ----
pn = 4096
g = nat.graph_from_coo(ctx, np.arange(pn - 1), np.arange(1, pn), pn, flags=BUILD_SYM_CSR)
pu, pv = np.zeros(pn, dtype=np.int64), np.zeros(pn, dtype=np.int64)
time_bridges(g, pu, pv)
path_runs = [time_bridges(g, pu, pv) for _ in range(REPEATS)]
nat.graph_destroy(ctx, g)
path = bridges_report(path_runs)
assert path["bridges"] == pn - 1 and path["depth"] == pn - 1
path["us_per_level_launch"] = 1e3 * path["ms_levels"]["median"] / path["level_launches"]
print("path4096", json.dumps(path), flush=True)

# ---- the scale graph ----
V = 1 << SCALE
E = 16 * V
src = np.zeros(E, dtype=np.int64)
dst = np.zeros(E, dtype=np.int64)
nat._check(nat.lib.mgx_gen_edges_to_host(
    ctx, ctypes.c_int(1), ctypes.c_int(SCALE), ctypes.c_int64(V), ctypes.c_int64(E),
    ctypes.c_uint64(1), ctypes.c_double(0.57), ctypes.c_double(0.19), ctypes.c_double(0.19),
    src.ctypes.data_as(_I64), dst.ctypes.data_as(_I64)), "mgx_gen_edges_to_host")
deg = np.bincount(src, minlength=V) + np.bincount(dst, minlength=V)
source = int(deg.argmax())
g = nat.graph_rmat(ctx, SCALE, E, seed=1, flags=BUILD_SYM_CSR)
print(f"RMAT-{SCALE}: V={V} E={E} built in {nat.graph_build_ms(g):.0f} ms", flush=True)

u, v = np.zeros(V, dtype=np.int64), np.zeros(V, dtype=np.int64)
_, st, _ = time_bridges(g, u, v)  # warm-up, and the result that is checked
nb = int(st.bridges)
level = np.zeros(V, dtype=np.int64)
nat._check(nat.lib.mgx_bridges_state(ctx, g, None, level.ctypes.data_as(_I64), None, None,
                                     None, None), "mgx_bridges_state")
# a degree-1 vertex has one entry, to another vertex: that edge is a bridge
one = deg == 1
leaf_keys = np.concatenate([
    (np.minimum(src, dst)[m] << 32) | np.maximum(src, dst)[m] for m in (one[src], one[dst])])
got_keys = (u[:nb] << 32) | v[:nb]
necessary = {
    "pairs_sorted_u_lt_v": bool((u[:nb] < v[:nb]).all() and (np.diff(got_keys) > 0).all()),
    "every_pair_one_level_apart": bool((np.abs(level[u[:nb]] - level[v[:nb]]) == 1).all()),
    "degree1_vertices": int(one.sum()),
    "every_degree1_edge_reported": bool(np.isin(leaf_keys, got_keys).all()),
}
print("necessary", necessary, flush=True)
del src, dst, level, leaf_keys, got_keys


def time_wcc():
    n = ctypes.c_int64()
    t0 = time.perf_counter()
    nat._check(nat.lib.mgx_wcc(ctx, g, None, ctypes.byref(n)), "mgx_wcc")
    return (time.perf_counter() - t0) * 1e3


def time_bfs():
    bst = BfsStats()
    t0 = time.perf_counter()
    nat._check(nat.lib.mgx_bfs(ctx, g, ctypes.c_int64(source), ctypes.c_int(0),
                               ctypes.c_int64(-1), ctypes.c_int(BFS_AUTO), None, None,
                               ctypes.byref(bst)), "mgx_bfs")
    return (time.perf_counter() - t0) * 1e3


time_wcc()
time_bfs()
# Alternate the variants so drift on a shared host hits all of them alike.
wcc_ms, bfs_ms, runs = [], [], []
for _ in range(REPEATS):
    wcc_ms.append(time_wcc())
    bfs_ms.append(time_bfs())
    runs.append(time_bridges(g, u, v))

rep = bridges_report(runs)
yard = summary(wcc_ms)["median"] + summary(bfs_ms)["median"]
stages = {s: rep["ms_" + s]["median"] for s in ("forest", "sorts_scans", "sweep", "levels")}
result = {
    "graph": {"kind": "rmat", "scale": SCALE, "V": V, "E": E, "seed": 1,
              "flags": "BUILD_SYM_CSR", "bfs_source": source},
    "repeats": REPEATS,
    "bridges": rep,
    "wcc_ms_host_no_download": summary(wcc_ms),
    "bfs_auto_ms_host_no_download": summary(bfs_ms),
    "bridges_over_wcc_plus_bfs": rep["ms_event"]["median"] / yard,
    "largest_stage": max(stages, key=stages.get),
    "necessary_conditions": necessary,
    "forest_state_check": check,
    "path4096": path,
}
print(json.dumps(result, indent=1), flush=True)
if OUT:
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(result, f, indent=1)

nat.graph_destroy(ctx, g)
nat.destroy(ctx)
assert necessary["pairs_sorted_u_lt_v"] and necessary["every_pair_one_level_apart"]
assert necessary["every_degree1_edge_reported"]
print("OK", flush=True)
