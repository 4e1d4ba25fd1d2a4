"""ctypes bindings for libmgx_analytics.so (the gfx950 compute library).

Product-path plumbing for bench.py and the GPU tests. Fails loudly when the
library is missing or no HIP device is present — there is no CPU fallback.
"""
import ctypes
import os

import numpy as np

_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_DIR, "lib", "libmgx_analytics.so")

BUILD_IN_CSR = 1
BUILD_SYM_CSR = 2
BUILD_WEIGHTED = 4
BUILD_OUT_CSR = 8
BUILD_NO_PERM = 16

UNIQUE_ID_BYTES = 128

_I64 = ctypes.POINTER(ctypes.c_int64)
_F64 = ctypes.POINTER(ctypes.c_double)


class PagerankStats(ctypes.Structure):
    _fields_ = [
        ("iterations", ctypes.c_int64),
        ("iter_ms", ctypes.c_double),
        ("sweep_ms", ctypes.c_double),
        ("sweep_launches", ctypes.c_int64),
        ("csr_build_ms", ctypes.c_double),
        ("download_ms", ctypes.c_double),
    ]


BFS_AUTO = 0
BFS_TOP_DOWN = 1
BFS_BOTTOM_UP = 2


class BfsStats(ctypes.Structure):
    _fields_ = [
        ("depth", ctypes.c_int64),
        ("reached", ctypes.c_int64),
        ("entries_scanned", ctypes.c_int64),
        ("top_down_levels", ctypes.c_int64),
        ("bottom_up_levels", ctypes.c_int64),
        ("bottom_up_mask", ctypes.c_uint64),
        ("ms", ctypes.c_double),
    ]


class BridgesStats(ctypes.Structure):
    _fields_ = [
        ("bridges", ctypes.c_int64),
        ("trees", ctypes.c_int64),
        ("depth", ctypes.c_int64),
        ("nontree_entries", ctypes.c_int64),
        ("level_launches", ctypes.c_int64),
        ("forest_ms", ctypes.c_double),
        ("ms", ctypes.c_double),
    ]


SIM_JACCARD = 0
SIM_OVERLAP = 1
SIM_AUTO = 0
SIM_SEARCH = 1
SIM_MERGE = 2


class SimilarityStats(ctypes.Structure):
    _fields_ = [
        ("pairs", ctypes.c_int64),
        ("search_pairs", ctypes.c_int64),
        ("merge_pairs", ctypes.c_int64),
        ("distinct_entries", ctypes.c_int64),
        ("chunks", ctypes.c_int64),
        ("prep_ms", ctypes.c_double),
        ("ms", ctypes.c_double),
    ]


ERR_OUT_OF_MEMORY = 5


class MgxError(RuntimeError):
    def __init__(self, message, status=None):
        super().__init__(message)
        self.status = status


class Native:
    def __init__(self, path=LIB_PATH):
        if not os.path.exists(path):
            raise MgxError(f"{path} not built — run `make` / __graft_entry__.build()")
        self.lib = ctypes.CDLL(path)
        self.lib.mgx_status_string.restype = ctypes.c_char_p
        self.lib.mgx_last_error.restype = ctypes.c_char_p
        self.lib.mgx_graph_build_ms.restype = ctypes.c_double
        self.lib.mgx_graph_num_vertices.restype = ctypes.c_int64
        self.lib.mgx_graph_num_edges.restype = ctypes.c_int64
        self.lib.mgx_graph_local_edges.restype = ctypes.c_int64
        self.lib.mgx_graph_xcd_heavy_rows.restype = ctypes.c_int64
        self.lib.mgx_graph_xcd_stream_ints.restype = ctypes.c_int64
        self.lib.mgx_graph_in_zero_rows.restype = ctypes.c_int64
        self.lib.mgx_pagerank_xcd_lds_floats.restype = ctypes.c_int64

    def _check(self, status, what):
        if status != 0:
            msg = self.lib.mgx_status_string(status).decode()
            detail = self.lib.mgx_last_error().decode()
            raise MgxError(f"{what}: {msg} ({detail})", status)

    def device_count(self):
        return self.lib.mgx_device_count()

    def init(self, device=0):
        ctx = ctypes.c_void_p()
        self._check(self.lib.mgx_init(device, ctypes.byref(ctx)), "mgx_init")
        return ctx

    def destroy(self, ctx):
        self.lib.mgx_destroy(ctx)

    def sync(self, ctx):
        self._check(self.lib.mgx_sync(ctx), "mgx_sync")

    def test_scope_hook(self, fail_at=-1):
        """Test support: device blocks the library's scopes own right now, in
        the whole process. Then arms the fail_at-th scope allocation from now
        on to fail as out of memory on the host; -1 disarms."""
        self.lib.mgx_test_scope_hook.restype = ctypes.c_int64
        return self.lib.mgx_test_scope_hook(ctypes.c_int64(fail_at))

    def test_state_hook(self, first_cap=-1):
        """Test support: device blocks the online modules' persistent arrays
        hold right now, in the whole process. Then makes every such array
        start at first_cap elements instead of its own first capacity, so that
        tiny graphs already grow them; -1 restores the arrays' own values."""
        self.lib.mgx_test_state_hook.restype = ctypes.c_int64
        return self.lib.mgx_test_state_hook(ctypes.c_int64(first_cap))

    # --- graphs ---
    def graph_from_coo(self, ctx, src, dst, n_vertices, weights=None, flags=BUILD_IN_CSR):
        src = np.ascontiguousarray(src, dtype=np.int64)
        dst = np.ascontiguousarray(dst, dtype=np.int64)
        pw = None
        if weights is not None:
            weights = np.ascontiguousarray(weights, dtype=np.float64)
            pw = weights.ctypes.data_as(_F64)
        g = ctypes.c_void_p()
        self._check(
            self.lib.mgx_graph_from_coo(ctx, src.ctypes.data_as(_I64),
                                        dst.ctypes.data_as(_I64), pw,
                                        ctypes.c_int64(n_vertices),
                                        ctypes.c_int64(len(src)), ctypes.c_uint32(flags),
                                        ctypes.byref(g)), "mgx_graph_from_coo")
        return g

    def graph_rmat(self, ctx, scale, n_edges, seed=1, a=0.57, b=0.19, c=0.19,
                   flags=BUILD_IN_CSR, weight_seed=7):
        g = ctypes.c_void_p()
        self._check(
            self.lib.mgx_graph_rmat(ctx, ctypes.c_int(scale), ctypes.c_int64(n_edges),
                                    ctypes.c_uint64(seed), ctypes.c_double(a),
                                    ctypes.c_double(b), ctypes.c_double(c),
                                    ctypes.c_uint32(flags), ctypes.c_uint64(weight_seed),
                                    ctypes.byref(g)), "mgx_graph_rmat")
        return g

    def graph_uniform(self, ctx, n_vertices, n_edges, seed=42, flags=BUILD_IN_CSR,
                      weight_seed=7):
        g = ctypes.c_void_p()
        self._check(
            self.lib.mgx_graph_uniform(ctx, ctypes.c_int64(n_vertices),
                                       ctypes.c_int64(n_edges), ctypes.c_uint64(seed),
                                       ctypes.c_uint32(flags), ctypes.c_uint64(weight_seed),
                                       ctypes.byref(g)), "mgx_graph_uniform")
        return g

    def graph_rmat_sharded(self, ctx, scale, n_edges, row_begin, row_end, seed=1, a=0.57,
                           b=0.19, c=0.19):
        g = ctypes.c_void_p()
        self._check(
            self.lib.mgx_graph_rmat_sharded(ctx, ctypes.c_int(scale),
                                            ctypes.c_int64(n_edges), ctypes.c_uint64(seed),
                                            ctypes.c_double(a), ctypes.c_double(b),
                                            ctypes.c_double(c), ctypes.c_int64(row_begin),
                                            ctypes.c_int64(row_end), ctypes.byref(g)),
            "mgx_graph_rmat_sharded")
        return g

    def graph_destroy(self, ctx, g):
        self.lib.mgx_graph_destroy(ctx, g)

    def graph_build_ms(self, g):
        return self.lib.mgx_graph_build_ms(g)

    def graph_xcd_heavy_rows(self, g):
        """Rows PageRank sweeps XCD-striped, or -1 when that layout is off."""
        return self.lib.mgx_graph_xcd_heavy_rows(g)

    def graph_xcd_stream_ints(self, g):
        """Ints of the striped sweep's stripe-major column stream, or -1 when
        the graph has none."""
        return self.lib.mgx_graph_xcd_stream_ints(g)

    def graph_in_zero_rows(self, g):
        """Rows with no in-edges, left out of the steady-state PageRank sweep."""
        return self.lib.mgx_graph_in_zero_rows(g)

    # --- algorithms ---
    def pagerank(self, ctx, g, n_vertices, max_iterations=100, damping=0.85, eps=1e-5):
        out = np.zeros(n_vertices, dtype=np.float64)
        stats = PagerankStats()
        self._check(
            self.lib.mgx_pagerank(ctx, g, ctypes.c_int64(max_iterations),
                                  ctypes.c_double(damping), ctypes.c_double(eps),
                                  out.ctypes.data_as(_F64), ctypes.byref(stats)),
            "mgx_pagerank")
        return out, stats

    def pagerank_start(self, ctx, g, damping=0.85):
        run = ctypes.c_void_p()
        self._check(self.lib.mgx_pagerank_start(ctx, g, ctypes.c_double(damping),
                                                ctypes.byref(run)), "mgx_pagerank_start")
        return run

    def pagerank_start_dist(self, ctx, g, row_begin, row_end, damping=0.85):
        run = ctypes.c_void_p()
        self._check(
            self.lib.mgx_pagerank_start_dist(ctx, g, ctypes.c_double(damping),
                                             ctypes.c_int64(row_begin),
                                             ctypes.c_int64(row_end), ctypes.byref(run)),
            "mgx_pagerank_start_dist")
        return run

    def pagerank_iterate(self, run, n):
        self._check(self.lib.mgx_pagerank_iterate(run, ctypes.c_int64(n)),
                    "mgx_pagerank_iterate")

    def pagerank_xcd_lds_floats(self, run):
        """Floats per block of the striped launch's LDS hot prefix (0 = none)."""
        return self.lib.mgx_pagerank_xcd_lds_floats(run)

    def pagerank_xcd_block_threads(self, run):
        """Threads per block of the striped launch (0 = no striped launch)."""
        return self.lib.mgx_pagerank_xcd_block_threads(run)

    def pagerank_timing(self, run):
        ms = ctypes.c_double()
        n = ctypes.c_int64()
        self._check(self.lib.mgx_pagerank_timing(run, ctypes.byref(ms), ctypes.byref(n)),
                    "mgx_pagerank_timing")
        return ms.value, n.value

    def pagerank_finish(self, run, n_vertices=0, want_rank=True):
        out = np.zeros(n_vertices, dtype=np.float64) if want_rank else None
        p = out.ctypes.data_as(_F64) if want_rank and n_vertices else None
        self._check(self.lib.mgx_pagerank_finish(run, p), "mgx_pagerank_finish")
        return out

    def wcc(self, ctx, g, n_vertices):
        out = np.zeros(n_vertices, dtype=np.int64)
        n = ctypes.c_int64()
        self._check(self.lib.mgx_wcc(ctx, g, out.ctypes.data_as(_I64), ctypes.byref(n)),
                    "mgx_wcc")
        return out, n.value

    def bfs_status(self, ctx, g, n_vertices, source, directed=False, max_depth=-1,
                   mode=BFS_AUTO, want_parent=False):
        """Raw call: (status, hops, parent_or_None, stats) without raising."""
        hops = np.full(n_vertices, -1, dtype=np.int64)
        parent = np.full(n_vertices, -1, dtype=np.int64) if want_parent else None
        stats = BfsStats()
        status = self.lib.mgx_bfs(ctx, g, ctypes.c_int64(source),
                                  ctypes.c_int(1 if directed else 0),
                                  ctypes.c_int64(max_depth), ctypes.c_int(mode),
                                  hops.ctypes.data_as(_I64),
                                  parent.ctypes.data_as(_I64) if want_parent else None,
                                  ctypes.byref(stats))
        return status, hops, parent, stats

    def bfs(self, ctx, g, n_vertices, source, directed=False, max_depth=-1, mode=BFS_AUTO,
            want_parent=False):
        status, hops, parent, stats = self.bfs_status(ctx, g, n_vertices, source, directed,
                                                      max_depth, mode, want_parent)
        self._check(status, "mgx_bfs")
        return hops, parent, stats

    def bridges_status(self, ctx, g, n_vertices):
        """Raw call: (status, pairs[k,2], stats) without raising."""
        u = np.full(max(n_vertices, 1), -1, dtype=np.int64)
        v = np.full(max(n_vertices, 1), -1, dtype=np.int64)
        n = ctypes.c_int64(0)
        stats = BridgesStats()
        status = self.lib.mgx_bridges(ctx, g, u.ctypes.data_as(_I64), v.ctypes.data_as(_I64),
                                      ctypes.byref(n), ctypes.byref(stats))
        pairs = np.stack([u[:n.value], v[:n.value]], axis=1)
        return status, pairs, stats

    def bridges(self, ctx, g, n_vertices):
        """Bridges as (u < v) rows sorted by (u, v), and the call's stats."""
        status, pairs, stats = self.bridges_status(ctx, g, n_vertices)
        self._check(status, "mgx_bridges")
        return pairs, stats

    def bridges_state(self, ctx, g, n_vertices):
        """Test support: dict of the int64 [V] arrays parent, level, pre, nd, low, high."""
        names = ("parent", "level", "pre", "nd", "low", "high")
        out = {k: np.full(n_vertices, -1, dtype=np.int64) for k in names}
        self._check(
            self.lib.mgx_bridges_state(ctx, g, *[out[k].ctypes.data_as(_I64) for k in names]),
            "mgx_bridges_state")
        return out

    def bridges_last_stage_ms(self):
        """Split of this thread's last bridges call: forest, sorts_scans, sweep, levels."""
        vals = [ctypes.c_double() for _ in range(4)]
        self.lib.mgx_bridges_last_stage_ms.restype = None
        self.lib.mgx_bridges_last_stage_ms(*[ctypes.byref(x) for x in vals])
        return dict(zip(("forest", "sorts_scans", "sweep", "levels"), (x.value for x in vals)))

    def similarity_pairs_status(self, ctx, g, u, v, metric, mode=SIM_AUTO):
        """Raw call: (status, sim, common, stats) without raising."""
        u = np.ascontiguousarray(u, dtype=np.int64)
        v = np.ascontiguousarray(v, dtype=np.int64)
        assert u.shape == v.shape and u.ndim == 1
        n = len(u)
        sim = np.full(n, np.nan, dtype=np.float64)
        common = np.full(n, -1, dtype=np.int64)
        stats = SimilarityStats()
        status = self.lib.mgx_similarity_pairs(ctx, g, ctypes.c_int(metric),
                                               ctypes.c_int(mode), u.ctypes.data_as(_I64),
                                               v.ctypes.data_as(_I64), ctypes.c_int64(n),
                                               sim.ctypes.data_as(_F64),
                                               common.ctypes.data_as(_I64),
                                               ctypes.byref(stats))
        return status, sim, common, stats

    def similarity_pairs(self, ctx, g, u, v, metric, mode=SIM_AUTO):
        status, sim, common, stats = self.similarity_pairs_status(ctx, g, u, v, metric, mode)
        self._check(status, "mgx_similarity_pairs")
        return sim, common, stats

    def similarity_all_status(self, ctx, g, n_vertices, metric):
        """Raw call: (status, sim_or_None, stats); nothing is sized when the
        pair count is out of range (the library refuses before writing)."""
        stats = SimilarityStats()
        sim = None
        if 0 <= n_vertices <= 65536:
            sim = np.full(n_vertices * (n_vertices - 1) // 2, np.nan, dtype=np.float64)
        status = self.lib.mgx_similarity_all(ctx, g, ctypes.c_int(metric),
                                             sim.ctypes.data_as(_F64) if sim is not None
                                             else None, ctypes.byref(stats))
        return status, sim, stats

    def similarity_all(self, ctx, g, n_vertices, metric):
        status, sim, stats = self.similarity_all_status(ctx, g, n_vertices, metric)
        self._check(status, "mgx_similarity_all")
        return sim, stats

    def katz(self, ctx, g, n_vertices, alpha=0.2, epsilon=1e-2):
        out = np.zeros(n_vertices, dtype=np.float64)
        iters = ctypes.c_int64()
        self._check(
            self.lib.mgx_katz(ctx, g, ctypes.c_double(alpha), ctypes.c_double(epsilon),
                              out.ctypes.data_as(_F64), ctypes.byref(iters)), "mgx_katz")
        return out, iters.value

    def louvain(self, ctx, g, n_vertices, threshold=1e-6):
        out = np.zeros(n_vertices, dtype=np.int64)
        n = ctypes.c_int64()
        self._check(
            self.lib.mgx_louvain(ctx, g, ctypes.c_double(threshold),
                                 out.ctypes.data_as(_I64), ctypes.byref(n)), "mgx_louvain")
        return out, n.value

    def betweenness(self, ctx, g, n_vertices, directed=True, normalize=True):
        out = np.zeros(n_vertices, dtype=np.float64)
        self._check(
            self.lib.mgx_betweenness(ctx, g, ctypes.c_int(1 if directed else 0),
                                     ctypes.c_int(1 if normalize else 0),
                                     out.ctypes.data_as(_F64)), "mgx_betweenness")
        return out

    # --- online pagerank (walk state is process-global, like the
    #     reference's context — algorithm_online/pagerank.cpp:49) ---
    def pronline_set(self, ctx, g, dense_to_mg, R=10, eps=0.2, seed=1):
        dense_to_mg = np.ascontiguousarray(dense_to_mg, dtype=np.int64)
        V = len(dense_to_mg)
        rank = np.zeros(V)
        self._check(
            self.lib.mgx_pronline_set(ctx, g, dense_to_mg.ctypes.data_as(_I64),
                                      ctypes.c_int64(R), ctypes.c_double(eps),
                                      ctypes.c_uint64(seed),
                                      rank.ctypes.data_as(_F64)),
            "mgx_pronline_set")
        return rank

    def pronline_get(self, ctx, dense_to_mg):
        dense_to_mg = np.ascontiguousarray(dense_to_mg, dtype=np.int64)
        V = len(dense_to_mg)
        rank = np.zeros(V)
        consistent = ctypes.c_int(0)
        self._check(
            self.lib.mgx_pronline_get(ctx, dense_to_mg.ctypes.data_as(_I64),
                                      ctypes.c_int64(V), rank.ctypes.data_as(_F64),
                                      ctypes.byref(consistent)),
            "mgx_pronline_get")
        return rank, consistent.value

    def pronline_update(self, ctx, g, dense_to_mg, cv=(), ce=(), dv=(), de=()):
        dense_to_mg = np.ascontiguousarray(dense_to_mg, dtype=np.int64)
        V = len(dense_to_mg)
        cv = np.ascontiguousarray(cv, dtype=np.int64)
        dv = np.ascontiguousarray(dv, dtype=np.int64)
        ce = np.ascontiguousarray(np.asarray(ce, dtype=np.int64).reshape(-1))
        de = np.ascontiguousarray(np.asarray(de, dtype=np.int64).reshape(-1))
        rank = np.zeros(V)
        self._check(
            self.lib.mgx_pronline_update(
                ctx, g, dense_to_mg.ctypes.data_as(_I64), cv.ctypes.data_as(_I64),
                ctypes.c_int64(len(cv)), ce.ctypes.data_as(_I64),
                ctypes.c_int64(len(ce) // 2), dv.ctypes.data_as(_I64),
                ctypes.c_int64(len(dv)), de.ctypes.data_as(_I64),
                ctypes.c_int64(len(de) // 2), rank.ctypes.data_as(_F64)),
            "mgx_pronline_update")
        return rank

    def pronline_reset(self, ctx):
        self._check(self.lib.mgx_pronline_reset(ctx), "mgx_pronline_reset")

    def pronline_stats(self, ctx):
        w = ctypes.c_int64(0)
        lw = ctypes.c_int64(0)
        le = ctypes.c_int64(0)
        self._check(self.lib.mgx_pronline_stats(ctx, ctypes.byref(w), ctypes.byref(lw),
                                                ctypes.byref(le)),
                    "mgx_pronline_stats")
        return w.value, lw.value, le.value

    # --- online katz (state is process-global, like the reference's
    #     context — query_modules katz.cpp:105) ---
    def konline_set(self, ctx, g, dense_to_mg, alpha=0.2, eps=1e-2):
        dense_to_mg = np.ascontiguousarray(dense_to_mg, dtype=np.int64)
        V = len(dense_to_mg)
        out = np.zeros(V)
        self._check(
            self.lib.mgx_konline_set(ctx, g, dense_to_mg.ctypes.data_as(_I64),
                                     ctypes.c_double(alpha), ctypes.c_double(eps),
                                     out.ctypes.data_as(_F64)),
            "mgx_konline_set")
        return out

    def konline_get(self, ctx, dense_to_mg):
        dense_to_mg = np.ascontiguousarray(dense_to_mg, dtype=np.int64)
        V = len(dense_to_mg)
        out = np.zeros(V)
        consistent = ctypes.c_int(0)
        self._check(
            self.lib.mgx_konline_get(ctx, dense_to_mg.ctypes.data_as(_I64),
                                     ctypes.c_int64(V), out.ctypes.data_as(_F64),
                                     ctypes.byref(consistent)),
            "mgx_konline_get")
        return out, consistent.value

    def konline_update(self, ctx, g, dense_to_mg, cv=(), ce=(), dv=(), de=()):
        dense_to_mg = np.ascontiguousarray(dense_to_mg, dtype=np.int64)
        cv = np.ascontiguousarray(cv, dtype=np.int64)
        dv = np.ascontiguousarray(dv, dtype=np.int64)
        ce = np.ascontiguousarray(np.asarray(ce, dtype=np.int64).reshape(-1))
        de = np.ascontiguousarray(np.asarray(de, dtype=np.int64).reshape(-1))
        out = np.zeros(len(dense_to_mg))
        self._check(
            self.lib.mgx_konline_update(
                ctx, g, dense_to_mg.ctypes.data_as(_I64), cv.ctypes.data_as(_I64),
                ctypes.c_int64(len(cv)), ce.ctypes.data_as(_I64),
                ctypes.c_int64(len(ce) // 2), dv.ctypes.data_as(_I64),
                ctypes.c_int64(len(dv)), de.ctypes.data_as(_I64),
                ctypes.c_int64(len(de) // 2), out.ctypes.data_as(_F64)),
            "mgx_konline_update")
        return out

    def konline_reset(self, ctx):
        self._check(self.lib.mgx_konline_reset(ctx), "mgx_konline_reset")

    def konline_iterations(self):
        self.lib.mgx_konline_iterations.restype = ctypes.c_int64
        return self.lib.mgx_konline_iterations()

    # --- LabelRankT online community detection (process-global state) ---
    def lrt_set(self, ctx, g, dense_to_mg, directed=False, weighted=False,
                similarity_threshold=0.7, exponent=4.0, min_value=0.1,
                w_selfloop=1.0, max_iterations=100, max_updates=5):
        dense_to_mg = np.ascontiguousarray(dense_to_mg, dtype=np.int64)
        out = np.full(len(dense_to_mg), -1, dtype=np.int64)
        self._check(
            self.lib.mgx_lrt_set(ctx, g, dense_to_mg.ctypes.data_as(_I64),
                                 ctypes.c_int(1 if directed else 0),
                                 ctypes.c_int(1 if weighted else 0),
                                 ctypes.c_double(similarity_threshold),
                                 ctypes.c_double(exponent),
                                 ctypes.c_double(min_value),
                                 ctypes.c_double(w_selfloop),
                                 ctypes.c_int64(max_iterations),
                                 ctypes.c_int64(max_updates),
                                 out.ctypes.data_as(_I64)),
            "mgx_lrt_set")
        return out

    def lrt_get(self, ctx, g, dense_to_mg):
        dense_to_mg = np.ascontiguousarray(dense_to_mg, dtype=np.int64)
        out = np.full(len(dense_to_mg), -1, dtype=np.int64)
        ran = ctypes.c_int(0)
        self._check(
            self.lib.mgx_lrt_get(ctx, g, dense_to_mg.ctypes.data_as(_I64),
                                 out.ctypes.data_as(_I64), ctypes.byref(ran)),
            "mgx_lrt_get")
        return out, ran.value

    def lrt_update(self, ctx, g, dense_to_mg, mv=(), me=(), dv=(), de=()):
        dense_to_mg = np.ascontiguousarray(dense_to_mg, dtype=np.int64)
        mv = np.ascontiguousarray(mv, dtype=np.int64)
        dv = np.ascontiguousarray(dv, dtype=np.int64)
        me = np.ascontiguousarray(np.asarray(me, dtype=np.int64).reshape(-1))
        de = np.ascontiguousarray(np.asarray(de, dtype=np.int64).reshape(-1))
        out = np.full(len(dense_to_mg), -1, dtype=np.int64)
        self._check(
            self.lib.mgx_lrt_update(
                ctx, g, dense_to_mg.ctypes.data_as(_I64), mv.ctypes.data_as(_I64),
                ctypes.c_int64(len(mv)), me.ctypes.data_as(_I64),
                ctypes.c_int64(len(me) // 2), dv.ctypes.data_as(_I64),
                ctypes.c_int64(len(dv)), de.ctypes.data_as(_I64),
                ctypes.c_int64(len(de) // 2), out.ctypes.data_as(_I64)),
            "mgx_lrt_update")
        return out

    def lrt_reset(self, ctx):
        self._check(self.lib.mgx_lrt_reset(ctx), "mgx_lrt_reset")

    # --- leiden ---
    def leiden(self, ctx, g, n_vertices, gamma=1.0, theta=0.01, resolution=0.01,
               max_iterations=(1 << 62), seed=1, cap=64):
        hier = np.full(n_vertices * cap, -1, dtype=np.int64)
        levels = np.zeros(n_vertices, dtype=np.int64)
        self._check(
            self.lib.mgx_leiden(ctx, g, ctypes.c_double(gamma), ctypes.c_double(theta),
                                ctypes.c_double(resolution),
                                ctypes.c_int64(max_iterations), ctypes.c_uint64(seed),
                                ctypes.c_int64(cap), hier.ctypes.data_as(_I64),
                                levels.ctypes.data_as(_I64)),
            "mgx_leiden")
        return hier.reshape(n_vertices, cap), levels

    # --- comm ---
    def comm_unique_id(self):
        buf = (ctypes.c_char * UNIQUE_ID_BYTES)()
        self._check(self.lib.mgx_comm_unique_id(buf), "mgx_comm_unique_id")
        return bytes(buf)

    def comm_init(self, ctx, rank, world, id_bytes):
        buf = (ctypes.c_char * UNIQUE_ID_BYTES).from_buffer_copy(id_bytes)
        self._check(self.lib.mgx_comm_init(ctx, rank, world, buf), "mgx_comm_init")
