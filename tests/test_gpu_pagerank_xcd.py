"""GPU parity of the XCD-striped PageRank sweep (MGX_PR_XCD=1: dealt hot-first
renumbering, one striped launch over the heavy rows, light rows unstriped, a
finish kernel over the heavy rows).

Every case is compared two ways:
  (a) against the fp64 oracle at the project's bar, 1e-6 absolute after equal
      iterations (tests/test_gpu_pagerank.py);
  (b) against the same graph built with MGX_PR_XCD=0 in the same process, per
      vertex: |a - b| <= 2^-21 * max(|a|, |b|). The two paths compute the same
      fp64 row sums in a different association and round them to f32, so they
      can differ only where an fp64 value sits on an f32 rounding boundary, and
      such a flip propagates damped by d: 8 f32 ulps is a loose bound on that.
      A dropped or doubled edge in a row of in-degree d moves that row by about
      1/d >= 1e-4 for every row here, which the oracle bar alone would not
      catch at ranks of ~1e-4 and below.
The largest ratio |a - b| / max(|a|, |b|) of each case is printed.
"""
import numpy as np
import pytest

from memgraph_amd.native import BUILD_IN_CSR, BUILD_SYM_CSR, Native

pytestmark = pytest.mark.gpu

PR_TOL = 1e-6      # tests/test_gpu_pagerank.py
KATZ_TOL = 1e-9    # tests/test_gpu_wcc_katz.py
REL_TOL = 2.0 ** -21
HEAVY_MIN = 64     # default heavy_min: bins 2 and 3 of the in-CSR


def bins_graph():
    """The tests/test_gpu_bins.py graph, V = 1307 (not a multiple of 16): heavy
    rows of in-degree 1100, 100, 65, 66 and 67, whose stripe segments land in
    bins 1 and 2 and several of which are empty."""
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
    return 1307, np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)


def wide_row_graph():
    """V = 10000: vertex 0 fed by sources 100..9599 (in-degree 9500) plus a
    ring. The 9500 sources have out-degree 2 and are hot-first, dealt about
    1187 to each stripe: every stripe's segment is >= 1024, bin 3."""
    nv = 10000
    ring = np.arange(nv, dtype=np.int64)
    fan = np.arange(100, 9600, dtype=np.int64)
    src = np.concatenate([fan, ring])
    dst = np.concatenate([np.zeros(len(fan), dtype=np.int64), (ring + 1) % nv])
    return nv, src, dst


def ring_fan_graph(nv):
    """70 parallel edges into vertex 0 from (up to) 3 distinct sources, plus a
    ring: a heavy row on a graph with few granules, most stripes empty for
    every row. At V = 1 it is 70 self-loops."""
    sources = np.array([nv // 4, nv // 2, (3 * nv) // 4], dtype=np.int64) % nv
    fan = np.resize(sources, 70)
    if nv == 1:
        return nv, fan, np.zeros(70, dtype=np.int64)
    ring = np.arange(nv, dtype=np.int64)
    src = np.concatenate([fan, ring])
    dst = np.concatenate([np.zeros(70, dtype=np.int64), (ring + 1) % nv])
    return nv, src, dst


def heavy_rows(nv, dst, heavy_min=HEAVY_MIN):
    return int((np.bincount(dst, minlength=nv) >= heavy_min).sum())


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
def rmat16(oracle):
    scale = 16
    src, dst = oracle.gen_rmat(scale, 16 << scale, seed=1)
    return 1 << scale, src, dst


class Built:
    """A graph built with MGX_PR_XCD set to `xcd` ("1" or "0")."""

    def __init__(self, nat, ctx, monkeypatch, graph, xcd, flags=BUILD_IN_CSR,
                 heavy_min=None):
        self.nat, self.ctx = nat, ctx
        self.nv, self.src, self.dst = graph
        monkeypatch.delenv("MGX_PR_STRIPES", raising=False)
        if heavy_min is None:
            monkeypatch.delenv("MGX_PR_XCD_HEAVY_MIN", raising=False)
        else:
            monkeypatch.setenv("MGX_PR_XCD_HEAVY_MIN", str(heavy_min))
        monkeypatch.setenv("MGX_PR_XCD", xcd)
        self.g = nat.graph_from_coo(ctx, self.src, self.dst, self.nv, flags=flags)
        want = heavy_rows(self.nv, self.dst, heavy_min or HEAVY_MIN) if xcd == "1" else -1
        got = nat.graph_xcd_heavy_rows(self.g)
        if got != want:
            self.close()
            pytest.fail(f"MGX_PR_XCD={xcd}: {got} striped heavy rows, expected {want}")

    def close(self):
        self.nat.graph_destroy(self.ctx, self.g)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def check_both_ways(nat, ctx, oracle, monkeypatch, graph, heavy_min=None, **kw):
    nv, src, dst = graph
    with Built(nat, ctx, monkeypatch, graph, "1", heavy_min=heavy_min) as b:
        rank, stats = nat.pagerank(ctx, b.g, nv, **kw)
    with Built(nat, ctx, monkeypatch, graph, "0") as b:
        base, base_stats = nat.pagerank(ctx, b.g, nv, **kw)
    exp, iters = oracle.pagerank(nv, src, dst, **kw)
    err = np.abs(rank - exp).max()
    ratio = (np.abs(rank - base) / np.maximum(np.abs(rank), np.abs(base))).max()
    print(f"V={nv} iterations={stats.iterations} oracle_linf={err:.3e} "
          f"xcd_vs_plain_max_ratio={ratio:.3e} (bound {REL_TOL:.3e})")
    assert stats.iterations == iters
    assert base_stats.iterations == iters
    assert err <= PR_TOL                       # (a)
    assert ratio <= REL_TOL                    # (b)
    return rank


def test_bins_graph(nat, ctx, oracle, monkeypatch):
    graph = bins_graph()
    assert heavy_rows(graph[0], graph[2]) == 5
    check_both_ways(nat, ctx, oracle, monkeypatch, graph)


def test_bins_graph_heavy_min_8(nat, ctx, oracle, monkeypatch):
    # MGX_PR_XCD_HEAVY_MIN=8: the 16-lane section is striped too (the row of
    # in-degree 20), and only the 4-lane section stays in the light sweep.
    graph = bins_graph()
    assert heavy_rows(graph[0], graph[2], 8) == 6
    check_both_ways(nat, ctx, oracle, monkeypatch, graph, heavy_min=8)


def test_wide_row_every_segment_in_bin3(nat, ctx, oracle, monkeypatch):
    check_both_ways(nat, ctx, oracle, monkeypatch, wide_row_graph())


@pytest.mark.parametrize("nv", [40, 1, 15, 16, 17, 127, 128, 129])
def test_multi_edge_fan_on_tiny_v(nat, ctx, oracle, monkeypatch, nv):
    # Fewer granules than stripes, V around the granule and 8-granule edges:
    # a non-bijective dealt order fails the scatter back to original ids.
    graph = ring_fan_graph(nv)
    assert heavy_rows(graph[0], graph[2]) == 1
    check_both_ways(nat, ctx, oracle, monkeypatch, graph)


def test_rmat16_20_iterations(nat, ctx, oracle, monkeypatch, rmat16):
    rank = check_both_ways(nat, ctx, oracle, monkeypatch, rmat16, max_iterations=20, eps=0.0)
    assert abs(rank.sum() - 1.0) < 1e-9


@pytest.mark.parametrize("eps", [1e-3, 1e-7])
def test_stop_epsilon(nat, ctx, oracle, monkeypatch, eps):
    # The Linf fold is split over the light-row and the finish kernels.
    check_both_ways(nat, ctx, oracle, monkeypatch, bins_graph(), max_iterations=500, eps=eps)


def test_chunked_run_equals_oneshot(nat, ctx, monkeypatch, rmat16):
    # Partials and ping-pong buffers are reused across iterations and chunks.
    nv = rmat16[0]
    with Built(nat, ctx, monkeypatch, rmat16, "1") as b:
        run = nat.pagerank_start(ctx, b.g)
        nat.pagerank_iterate(run, 7)
        nat.pagerank_iterate(run, 13)
        nat.sync(ctx)
        _, launches = nat.pagerank_timing(run)
        chunked = nat.pagerank_finish(run, nv)
        one, _ = nat.pagerank(ctx, b.g, nv, max_iterations=20, eps=0.0)
    assert launches == 20  # one event bracket per whole sweep
    assert np.array_equal(chunked, one)


def test_katz_on_the_dealt_numbering(nat, ctx, oracle, monkeypatch):
    # The in-CSR numbering changes for every consumer of the graph.
    graph = bins_graph()
    nv, src, dst = graph
    with Built(nat, ctx, monkeypatch, graph, "1", flags=BUILD_IN_CSR | BUILD_SYM_CSR) as b:
        cent, iters = nat.katz(ctx, b.g, nv, alpha=0.1, epsilon=1e-3)
    exp, iters_exp = oracle.katz(nv, src, dst, alpha=0.1, epsilon=1e-3)
    assert iters == iters_exp
    assert np.abs(cent - exp).max() < KATZ_TOL
