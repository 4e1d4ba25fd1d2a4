"""Error paths release their device buffers (mgx_scope, mgx_internal.h).

Success paths never leaked, so the ordinary suite cannot see the difference.
mgx_test_scope_hook makes the k-th scope allocation of a call fail on the
host as out of memory; for k = 1, 2, ... until the call gets through, every
failing call must report out-of-memory, leave no scope-owned block behind, and
leave the context and graph able to reproduce the un-armed result exactly.

Only the six stateless entry points are armed: wcc, bfs, katz, betweenness,
bridges and leiden. None of them writes to the graph (read from their code:
no assignment to a graph field, no lazily built view), so a failure between
two allocations cannot leave graph state half built. The online modules and
the first similarity call on a graph update persistent state in steps and are
not armed here.

Leiden runs with max_iterations=2. Left unlimited it takes 121 levels on this
graph, because the star gives up one leaf per level, and about 25 allocations
a level would carry it far past the cap on k below. Two iterations still fill
the hub pool, refine, upload a new level at its own size and sweep that second
level.

Scope allocations per call on this graph, i.e. the first k that succeeds
minus one, as measured: wcc 5, bfs 10, katz 11, betweenness 5, bridges 31,
leiden 56 (the largest; the loop's cap is 500).
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from memgraph_amd.native import (BUILD_IN_CSR, BUILD_OUT_CSR, BUILD_SYM_CSR,  # noqa: E402
                                 BUILD_WEIGHTED, ERR_OUT_OF_MEMORY, MgxError, Native)

pytestmark = pytest.mark.gpu

K_CAP = 500


def tiny_graph():
    """Two 6-cliques joined by one edge, a star with 300 leaves (its centre is
    past Leiden's 256-neighbour hub threshold), four isolated vertices."""
    src, dst, w = [], [], []
    for base in (0, 6):
        for i in range(6):
            for j in range(i + 1, 6):
                src.append(base + i)
                dst.append(base + j)
                w.append(2.0)
    src.append(5), dst.append(6), w.append(1.0)
    centre = 12
    for leaf in range(13, 313):
        src.append(centre), dst.append(leaf), w.append(1.0)
    return 317, src, dst, w


@pytest.fixture(scope="module")
def nat():
    n = Native()
    if n.device_count() == 0:
        pytest.skip("no HIP device")
    return n


@pytest.fixture(scope="module")
def world(nat):
    ctx = nat.init(0)
    V, src, dst, w = tiny_graph()
    g = nat.graph_from_coo(ctx, src, dst, V, weights=w,
                           flags=BUILD_IN_CSR | BUILD_SYM_CSR | BUILD_OUT_CSR | BUILD_WEIGHTED)
    yield ctx, g, V
    nat.test_scope_hook(-1)
    nat.graph_destroy(ctx, g)
    nat.destroy(ctx)


def calls(nat, ctx, g, V):
    """name -> callable returning the arrays that make up the result."""
    def wcc():
        comp, n = nat.wcc(ctx, g, V)
        return comp, np.array([n])

    def bfs():
        hops, parent, stats = nat.bfs(ctx, g, V, 0, want_parent=True)
        return hops, parent, np.array([stats.depth, stats.reached])

    def katz():
        cent, iterations = nat.katz(ctx, g, V)
        return cent, np.array([iterations])

    def betweenness():
        return (nat.betweenness(ctx, g, V, directed=False),)

    def bridges():
        pairs, stats = nat.bridges(ctx, g, V)
        return pairs, np.array([stats.bridges, stats.trees, stats.depth])

    def leiden():
        return nat.leiden(ctx, g, V, seed=3, cap=16, max_iterations=2)

    return {f.__name__: f for f in (wcc, bfs, katz, betweenness, bridges, leiden)}


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


@pytest.mark.parametrize("name", ["wcc", "bfs", "katz", "betweenness", "bridges", "leiden"])
def test_failed_allocation_leaves_nothing_behind(nat, world, name):
    ctx, g, V = world
    call = calls(nat, ctx, g, V)[name]
    assert nat.test_scope_hook(-1) == 0
    kept = call()
    assert nat.test_scope_hook(-1) == 0, "scope blocks outstanding after a clean run"
    if name == "leiden":
        assert kept[1].max() >= 2, "the graph is meant to give Leiden a second level"

    k = 1
    while True:
        assert k < K_CAP, f"{name}: still failing at allocation {k}"
        nat.test_scope_hook(k)
        try:
            got, status = call(), 0
        except MgxError as e:
            got, status = None, e.status
        outstanding = nat.test_scope_hook(-1)  # also disarms
        if status == 0:
            break
        assert status == ERR_OUT_OF_MEMORY, (name, k, status)
        assert outstanding == 0, f"{name}: {outstanding} blocks left after failing allocation {k}"
        assert same(call(), kept), f"{name}: result changed after failing allocation {k}"
        assert nat.test_scope_hook(-1) == 0
        k += 1
    print(f"{name}: {k - 1} scope allocations per call")
    assert k > 1, f"{name}: the hook never fired"
    assert outstanding == 0
    assert same(got, kept)
