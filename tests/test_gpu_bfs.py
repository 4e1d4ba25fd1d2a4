"""GPU parity: mgx_bfs hop counts and minimum-id parents, bit-exact against
tests/bfs_ref.py (itself pinned to the reference's neighbors level sets by
tests/test_bfs_cpu.py), in every traversal mode."""
import json
import os

import numpy as np
import pytest

from bfs_ref import adjacency, bfs_ref, neighbors_coo, neighbors_expected_rows
from memgraph_amd.native import (BFS_AUTO, BFS_BOTTOM_UP, BFS_TOP_DOWN, BUILD_IN_CSR,
                                 BUILD_OUT_CSR, BUILD_SYM_CSR, Native)
from memgraph_amd.rmat import gen_rmat

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")

UNDIRECTED_MODES = (BFS_AUTO, BFS_TOP_DOWN, BFS_BOTTOM_UP)
DIRECTED_MODES = (BFS_AUTO, BFS_TOP_DOWN)

ERR_INVALID_ARGUMENT = 3
ERR_NOT_SUPPORTED = 7


@pytest.fixture(scope="module")
def nat():
    n = Native()
    if n.device_count() == 0:
        pytest.fail("gpu test run but no HIP device visible")
    return n


@pytest.fixture(scope="module")
def ctx(nat):
    c = nat.init(0)
    yield c
    nat.destroy(c)


class Graph:
    """One device graph with both traversal CSRs."""

    def __init__(self, nat, ctx, nv, src, dst, flags=BUILD_SYM_CSR | BUILD_OUT_CSR):
        self.nat, self.ctx, self.nv = nat, ctx, nv
        self.src = np.asarray(src, dtype=np.int64)
        self.dst = np.asarray(dst, dtype=np.int64)
        self.g = nat.graph_from_coo(ctx, self.src, self.dst, nv, flags=flags)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.nat.graph_destroy(self.ctx, self.g)

    def bfs(self, source, directed, mode, max_depth=-1):
        return self.nat.bfs(self.ctx, self.g, self.nv, source, directed=directed,
                            max_depth=max_depth, mode=mode, want_parent=True)

    def check(self, source, directed=False, max_depth=-1, modes=None):
        """Every mode equals bfs_ref bit-exactly; returns (ref, {mode: stats})."""
        ref = bfs_ref(self.nv, self.src, self.dst, source, directed=directed,
                      max_depth=max_depth)
        if modes is None:
            modes = DIRECTED_MODES if directed else UNDIRECTED_MODES
        all_stats = {}
        for mode in modes:
            hops, parent, st = self.bfs(source, directed, mode, max_depth)
            tag = (source, directed, max_depth, mode)
            assert np.array_equal(hops, ref.hops), tag
            assert np.array_equal(parent, ref.parent), tag
            assert st.reached == ref.reached, tag
            assert st.depth == ref.depth, tag
            assert st.top_down_levels + st.bottom_up_levels >= ref.depth, tag
            if mode == BFS_TOP_DOWN:
                assert st.bottom_up_levels == 0 and st.bottom_up_mask == 0, tag
                assert st.entries_scanned == ref.entries_scanned, tag
            if mode == BFS_BOTTOM_UP:
                assert st.top_down_levels == 0, tag
            # hops-only call (no parent buffer) takes the other kernel path
            hops2, none, _ = self.nat.bfs(self.ctx, self.g, self.nv, source,
                                          directed=directed, max_depth=max_depth, mode=mode)
            assert none is None
            assert np.array_equal(hops2, ref.hops), tag
            all_stats[mode] = st
        return ref, all_stats


def test_neighbors_goldens(nat, ctx):
    with open(os.path.join(GOLDEN, "neighbors_e2e.json")) as f:
        cases = json.load(f)
    assert len(cases) == 7
    for case in cases:
        nv, src, dst, source = neighbors_coo(case)
        with Graph(nat, ctx, nv, src, dst) as G:
            for mode in DIRECTED_MODES:
                hops, _, _ = G.bfs(source, True, mode, max_depth=case["distance"])
                got = neighbors_expected_rows(case, hops)
                exp = [set(r) for r in case["expected"]]
                if case["procedure"] == "by_hop":
                    assert got == exp, case["name"]
                else:
                    assert sorted(map(sorted, got)) == sorted(map(sorted, exp)), case["name"]
            G.check(source, directed=True, max_depth=case["distance"])


@pytest.mark.parametrize("nv", [1, 2, 31, 32, 33, 63, 64, 65, 257])
def test_bitmap_tail_words(nat, ctx, nv):
    rng = np.random.default_rng(11)
    ne = 2 * nv
    src, dst = rng.integers(0, nv, ne), rng.integers(0, nv, ne)
    with Graph(nat, ctx, nv, src, dst) as G:
        for source in sorted({0, nv // 2, nv - 1}):
            G.check(source)
            G.check(source, directed=True)
    with Graph(nat, ctx, nv, [], []) as G:  # no edges: the source is isolated
        for source in sorted({0, nv - 1}):
            ref, _ = G.check(source)
            G.check(source, directed=True)
            exp = np.full(nv, -1)
            exp[source] = 0
            assert np.array_equal(ref.hops, exp)


def test_self_loops_and_duplicate_edges(nat, ctx):
    src = [0, 0, 1, 2, 2, 3, 5, 5]
    dst = [0, 1, 2, 2, 3, 4, 5, 6]  # self-loops at 0, 2 and 5
    with Graph(nat, ctx, 7, src, dst) as G:
        for s in (0, 4, 5):
            G.check(s)
            G.check(s, directed=True)
    rng = np.random.default_rng(3)
    s1, d1 = rng.integers(0, 90, 150), rng.integers(0, 90, 150)
    with Graph(nat, ctx, 90, np.tile(s1, 3), np.tile(d1, 3)) as G:  # each edge 3 times
        ref, _ = G.check(int(s1[0]))
        G.check(int(s1[0]), directed=True)
    single = bfs_ref(90, s1, d1, int(s1[0]))
    assert np.array_equal(ref.hops, single.hops) and np.array_equal(ref.parent, single.parent)


def test_two_components(nat, ctx):
    # component A: 0..49 ring; component B: 50..79 ring
    a = np.arange(50)
    b = 50 + np.arange(30)
    src = np.concatenate([a, b])
    dst = np.concatenate([(a + 1) % 50, 50 + (b - 50 + 1) % 30])
    with Graph(nat, ctx, 80, src, dst) as G:
        ref, _ = G.check(3)
        assert (ref.hops[50:] == -1).all() and (ref.parent[50:] == -1).all()
        assert (ref.hops[:50] >= 0).all()
        for mode in UNDIRECTED_MODES:
            hops, parent, st = G.bfs(3, False, mode)
            assert (hops[50:] == -1).all() and (parent[50:] == -1).all()
            assert st.reached == 50


def test_directed_chain(nat, ctx):
    src, dst = np.arange(9), np.arange(1, 10)  # 0->1->...->9
    with Graph(nat, ctx, 10, src, dst) as G:
        ref, _ = G.check(5, directed=True)
        assert ref.hops.tolist() == [-1] * 5 + [0, 1, 2, 3, 4]
        ref, _ = G.check(5, directed=False)
        assert ref.hops.tolist() == [5, 4, 3, 2, 1, 0, 1, 2, 3, 4]


def test_path_graph_depth_limits(nat, ctx):
    n = 300
    src, dst = np.arange(n - 1), np.arange(1, n)
    with Graph(nat, ctx, n, src, dst) as G:
        for limit in (0, 1, 7, -1):
            want_depth = n - 1 if limit < 0 else min(limit, n - 1)
            for directed in (False, True):
                ref, stats = G.check(0, directed=directed, max_depth=limit)
                assert ref.depth == want_depth
                assert (ref.hops[want_depth + 1:] == -1).all()
                assert ref.hops[:want_depth + 1].tolist() == list(range(want_depth + 1))
                for st in stats.values():
                    assert st.depth == want_depth


def test_star_with_second_hub(nat, ctx):
    # hub 0 with 1500 leaves 1..1500 (the 256-lane bin); leaf 7 carries a
    # second hub 1501 with 199 leaves of its own (degree 200, the 64-lane bin).
    leaves = np.arange(1, 1501)
    src = np.concatenate([np.zeros(1500, dtype=np.int64), [7], np.full(199, 1501)])
    dst = np.concatenate([leaves, [1501], 1502 + np.arange(199)])
    nv = 1502 + 199
    with Graph(nat, ctx, nv, src, dst) as G:
        rp, _ = adjacency(nv, src, dst, False)
        deg = np.diff(rp)
        assert deg[0] >= 1024 and 64 <= deg[1501] < 1024
        for source in (0, 3, 1501, nv - 1):
            G.check(source)
            G.check(source, directed=True)


def test_random_bit_exact(nat, ctx):
    rng = np.random.default_rng(11)
    for _ in range(6):
        nv = int(rng.integers(2, 2000))
        ne = int(rng.integers(0, 6000))
        src = rng.integers(0, nv, ne)
        dst = rng.integers(0, nv, ne)
        source = int(rng.integers(0, nv))
        with Graph(nat, ctx, nv, src, dst) as G:
            G.check(source)
            G.check(source, directed=True)


def test_rmat12_switches_direction_and_back(nat, ctx):
    """RMAT-12 (E = 16 V, seed 3) from its max-degree vertex 0 (degree 4941):
    frontier sizes 1, 1341, 1950, 31; 3323 of 4096 reached; depth 3. With
    alpha = 14, beta = 24 levels 1 and 2 run bottom-up, 0 and 3 top-down.

    TOP_DOWN entries_scanned is compared with bfs_ref's exact count, 131070:
    the degree sum of every expanded frontier, the last one (31 vertices,
    35 entries) included, since it has to be expanded to learn that it is
    the last. The degree sum over hops < depth alone is 131035."""
    nv = 1 << 12
    src, dst = gen_rmat(12, 16 << 12, seed=3)
    rp, _ = adjacency(nv, src, dst, False)
    deg = np.diff(rp)
    source = int(deg.argmax())
    assert source == 0 and deg[0] == 4941
    with Graph(nat, ctx, nv, src, dst, flags=BUILD_SYM_CSR) as G:
        ref, stats = G.check(source)
    assert ref.frontier_sizes == [1, 1341, 1950, 31]
    assert (ref.reached, ref.depth) == (3323, 3)
    for mode, st in stats.items():
        print("rmat12 mode", mode, "scanned", st.entries_scanned, "td", st.top_down_levels,
              "bu", st.bottom_up_levels, "mask", bin(st.bottom_up_mask), "ref scanned",
              ref.entries_scanned)
        assert st.reached == 3323 and st.depth == 3
    assert stats[BFS_TOP_DOWN].entries_scanned == ref.entries_scanned
    auto = stats[BFS_AUTO]
    assert auto.bottom_up_levels >= 1
    assert auto.top_down_levels >= 2
    assert auto.bottom_up_mask & 1 == 0
    n_levels = auto.top_down_levels + auto.bottom_up_levels
    first_bu = min(l for l in range(n_levels) if auto.bottom_up_mask >> l & 1)
    assert any(not (auto.bottom_up_mask >> l & 1) for l in range(first_bu + 1, n_levels)), \
        "no top-down level after a bottom-up one"


def test_rmat16_modes_agree(nat, ctx):
    nv = 1 << 16
    src, dst = gen_rmat(16, 16 * (1 << 16), seed=3)  # the graph of test_wcc_rmat
    rp, _ = adjacency(nv, src, dst, False)
    source = int(np.diff(rp).argmax())
    with Graph(nat, ctx, nv, src, dst, flags=BUILD_SYM_CSR) as G:
        ref, stats = G.check(source)
        assert (ref.reached, ref.depth) == (46669, 4)
        outs = [G.bfs(source, False, m) for m in UNDIRECTED_MODES]
    for hops, parent, _ in outs[1:]:
        assert np.array_equal(hops, outs[0][0]) and np.array_equal(parent, outs[0][1])
    assert stats[BFS_AUTO].bottom_up_levels >= 1


def test_reuse_one_graph_two_sources(nat, ctx):
    rng = np.random.default_rng(23)
    nv = 700
    src, dst = rng.integers(0, nv, 1500), rng.integers(0, nv, 1500)
    with Graph(nat, ctx, nv, src, dst) as G:
        G.check(int(src[0]))
        G.check(int(dst[-1]))  # stale bitmaps/queues/counters would show here
        G.check(int(src[0]), directed=True)
        G.check(int(src[0]))


def test_errors(nat, ctx):
    with Graph(nat, ctx, 4, [0, 1], [1, 2]) as G:
        for bad in (-1, 4):
            status, _, _, _ = nat.bfs_status(ctx, G.g, 4, bad)
            assert status == ERR_INVALID_ARGUMENT
        status, _, _, _ = nat.bfs_status(ctx, G.g, 4, 0, directed=True, mode=BFS_BOTTOM_UP)
        assert status == ERR_NOT_SUPPORTED
        for bad_mode in (3, -1):
            status, _, _, _ = nat.bfs_status(ctx, G.g, 4, 0, mode=bad_mode)
            assert status == ERR_INVALID_ARGUMENT
        assert b"mode" in nat.lib.mgx_last_error()
        hops, _, _ = nat.bfs(ctx, G.g, 4, 0)  # the context is still usable
        assert hops.tolist() == [0, 1, 2, -1]
    with Graph(nat, ctx, 4, [0, 1], [1, 2], flags=BUILD_IN_CSR) as G:
        for directed in (False, True):
            status, _, _, _ = nat.bfs_status(ctx, G.g, 4, 0, directed=directed)
            assert status == ERR_INVALID_ARGUMENT
    with Graph(nat, ctx, 4, [0, 1], [1, 2], flags=BUILD_SYM_CSR) as G:
        status, _, _, _ = nat.bfs_status(ctx, G.g, 4, 0, directed=True)
        assert status == ERR_INVALID_ARGUMENT
        assert b"OUT" in nat.lib.mgx_last_error()
