"""GPU parity on one small graph whose rows land in all four degree bins of
both the in-CSR and the symmetric CSR, so that a wrong section offset, lanes
per row or row reduction in the shared sweep scaffold (mgx_device.h) shows in
every algorithm that uses it: WCC, Katz, PageRank and bottom-up / top-down BFS.

The graph (V = 1307, every out-degree <= 2, so Katz stays convergent):
  sources 4..1103 -> 0   in-degree 1100: bin 3, one workgroup per row
  sources 4..103  -> 1   in-degree 100:  bin 2, one wave per row
  sources 104..123 -> 2  in-degree 20:   bin 1, 16 lanes per row
  sources 200..202 -> 3  in-degree 3:    bin 0, 4 lanes per row
  chain 1104 -> 1105 -> ... -> 1299, edges 0 -> 1200, 1 -> 1201, 2 -> 1202
  1300..1303 isolated
  1304, 1305, 1306: in-degrees 65, 66, 67 (bin 2) on neighbouring ids, so the
  wide rows start on several residues mod 4 (head / int4 body / tail of the
  column gather).
"""
import numpy as np
import pytest

from bfs_ref import bfs_ref
from memgraph_amd.native import (BFS_BOTTOM_UP, BFS_TOP_DOWN, BUILD_IN_CSR, BUILD_SYM_CSR,
                                 Native)

pytestmark = pytest.mark.gpu

NV = 1307
PR_TOL = 1e-6     # tests/test_gpu_pagerank.py
KATZ_TOL = 1e-9   # tests/test_gpu_wcc_katz.py


def build_edges():
    src, dst = [], []

    def fan_in(sources, target):
        src.extend(sources)
        dst.extend([target] * len(sources))

    fan_in(range(4, 1104), 0)
    fan_in(range(4, 104), 1)
    fan_in(range(104, 124), 2)
    fan_in(range(200, 203), 3)
    src.extend(range(1104, 1299))
    dst.extend(range(1105, 1300))
    src.extend([0, 1, 2])
    dst.extend([1200, 1201, 1202])
    fan_in(range(300, 365), 1304)
    fan_in(range(400, 466), 1305)
    fan_in(range(500, 567), 1306)
    return np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)


SRC, DST = build_edges()


def bin_counts(deg):
    return [int(((deg >= lo) & (deg < hi)).sum())
            for lo, hi in ((0, 8), (8, 64), (64, 1024), (1024, 1 << 62))]


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


@pytest.fixture(scope="module")
def graph(nat, ctx):
    g = nat.graph_from_coo(ctx, SRC, DST, NV, flags=BUILD_IN_CSR | BUILD_SYM_CSR)
    yield g
    nat.graph_destroy(ctx, g)


def test_fixture_covers_every_bin():
    outdeg = np.bincount(SRC, minlength=NV)
    indeg = np.bincount(DST, minlength=NV)
    assert outdeg.max() == 2
    assert all(n > 0 for n in bin_counts(indeg)), bin_counts(indeg)
    assert all(n > 0 for n in bin_counts(indeg + outdeg)), bin_counts(indeg + outdeg)
    assert indeg[[0, 1, 2, 3]].tolist() == [1100, 100, 20, 3]
    assert indeg[1304:1307].tolist() == [65, 66, 67]
    # wide-row starts of the symmetric CSR (identity layout) mod 4
    starts = np.concatenate([[0], np.cumsum(indeg + outdeg)])[:-1]
    assert len({int(starts[v]) % 4 for v in (1, 1304, 1305, 1306)}) >= 3


def test_wcc(nat, ctx, graph, oracle):
    comp, n = nat.wcc(ctx, graph, NV)
    exp, n_exp = oracle.wcc(NV, SRC, DST)
    assert n == n_exp
    assert np.array_equal(comp, exp)


@pytest.mark.parametrize("alpha,epsilon", [(0.2, 1e-2), (0.1, 1e-3)])
def test_katz(nat, ctx, graph, oracle, alpha, epsilon):
    cent, iters = nat.katz(ctx, graph, NV, alpha=alpha, epsilon=epsilon)
    exp, iters_exp = oracle.katz(NV, SRC, DST, alpha=alpha, epsilon=epsilon)
    assert iters == iters_exp
    assert np.abs(cent - exp).max() < KATZ_TOL


def test_pagerank(nat, ctx, graph, oracle):
    rank, stats = nat.pagerank(ctx, graph, NV)
    exp, iters = oracle.pagerank(NV, SRC, DST)
    assert stats.iterations == iters
    assert np.abs(rank - exp).max() <= PR_TOL


def test_pagerank_striped(nat, ctx, oracle, monkeypatch):
    # Three source stripes: every stripe's own bin list goes through the same
    # section fill, and the sweep runs in its first / middle / last modes.
    monkeypatch.setenv("MGX_PR_STRIPES", "3")
    g = nat.graph_from_coo(ctx, SRC, DST, NV, flags=BUILD_IN_CSR)
    try:
        rank, stats = nat.pagerank(ctx, g, NV)
    finally:
        nat.graph_destroy(ctx, g)
    exp, iters = oracle.pagerank(NV, SRC, DST)
    assert stats.iterations == iters
    assert np.abs(rank - exp).max() <= PR_TOL


@pytest.fixture(scope="module")
def bfs_expected():
    return bfs_ref(NV, SRC, DST, 0, directed=False)


@pytest.mark.parametrize("mode", [BFS_BOTTOM_UP, BFS_TOP_DOWN])
def test_bfs_from_hub(nat, ctx, graph, bfs_expected, mode):
    ref = bfs_expected
    hops, parent, st = nat.bfs(ctx, graph, NV, 0, directed=False, mode=mode, want_parent=True)
    assert np.array_equal(hops, ref.hops)
    assert np.array_equal(parent, ref.parent)
    assert st.reached == ref.reached and st.depth == ref.depth
