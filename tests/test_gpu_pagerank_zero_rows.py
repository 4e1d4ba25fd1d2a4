"""Rows of in-degree 0 leave the PageRank sweep from a run's third iteration on
(MGX_PR_SKIP_ZERO, on unless set to 0): their rank is (1-d)/N and their contrib
(1-d)/N * inv_outdeg in both ping-pong buffers after the first two sweeps.

Every case runs with MGX_PR_SKIP_ZERO unset against =0 on the same graph
(np.array_equal: the rows that stay are computed exactly as before) and against
the fp64 oracle (1e-6, equal iterations), with MGX_PR_XCD both 0 and 1.
"""
import numpy as np
import pytest

from memgraph_amd.native import BUILD_IN_CSR, Native

pytestmark = pytest.mark.gpu

PR_TOL = 1e-6
KATZ_TOL = 1e-9    # tests/test_gpu_wcc_katz.py


def zero_rows_graph():
    """V = 300. 150 vertices have no in-edges: ids 0..99 and every third id of
    100..249, so that by id they are interleaved with rows of in-degree 1..7.
    Their out-degrees are 0, 1 and 40 in turn (40 for twenty of them, whose
    edges give ids 250..289 in-degree 20). Ids 290 and 291 have in-degree 70
    (striped heavy rows under MGX_PR_XCD=1); every other id has in-degree
    1..7."""
    nv = 300
    zero = list(range(100)) + list(range(100, 250, 3))
    zset = set(zero)
    sinks = list(range(250, 290))
    heavy = [290, 291]
    light = [v for v in range(100, nv) if v not in zset and v not in sinks and v not in heavy]
    fed = light + sinks + heavy            # every vertex with in-edges
    want = {v: 1 + i % 7 for i, v in enumerate(light)}
    src, dst = [], []
    n40 = nxt = 0
    for k, z in enumerate(zero):
        if k % 3 == 1:                      # out-degree 1, into a light row
            t = light[nxt]
            nxt += 1
            src.append(z)
            dst.append(t)
            want[t] -= 1
        elif k % 3 == 2 and n40 < 20:       # out-degree 40, into the sinks
            n40 += 1
            src.extend([z] * len(sinks))
            dst.extend(sinks)
    for t in light:
        for j in range(want[t]):
            src.append(fed[(t * 5 + j * 11) % len(fed)])
            dst.append(t)
    for h in heavy:
        for j in range(70):
            src.append(fed[(h + j * 3) % len(fed)])
            dst.append(h)
    src = np.asarray(src, dtype=np.int64)
    dst = np.asarray(dst, dtype=np.int64)
    indeg = np.bincount(dst, minlength=nv)
    outdeg = np.bincount(src, minlength=nv)
    assert (indeg[zero] == 0).all() and int((indeg == 0).sum()) == 150
    assert sorted(set(outdeg[zero])) == [0, 1, 40]
    assert set(indeg[light]) == set(range(1, 8))
    assert (indeg[sinks] == 20).all() and (indeg[heavy] == 70).all()
    return nv, src, dst


def ring_graph(nv=100):
    """A ring plus chords 0 -> 50 and 1 -> 75 (a bare ring is stationary from
    the start and the oracle stops after one iteration): no row is empty."""
    ring = np.arange(nv, dtype=np.int64)
    src = np.concatenate([ring, [0, 1]])
    dst = np.concatenate([(ring + 1) % nv, [50, 75]])
    return nv, src, dst


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
def base_graph():
    return zero_rows_graph()


class Built:
    """`graph` built with MGX_PR_XCD = xcd; skip(on) sets the switch for the
    runs started after it."""

    def __init__(self, nat, ctx, monkeypatch, graph, xcd, flags=BUILD_IN_CSR):
        self.nat, self.ctx, self.mp = nat, ctx, monkeypatch
        self.nv, self.src, self.dst = graph
        for name in ("MGX_PR_STRIPES", "MGX_PR_XCD_HEAVY_MIN", "MGX_PR_XCD_LDS",
                     "MGX_PR_SKIP_ZERO"):
            monkeypatch.delenv(name, raising=False)
        monkeypatch.setenv("MGX_PR_XCD", xcd)
        self.g = nat.graph_from_coo(ctx, self.src, self.dst, self.nv, flags=flags)
        zeros = int((np.bincount(self.dst, minlength=self.nv) == 0).sum()) if self.nv else 0
        got = nat.graph_in_zero_rows(self.g)
        if got != zeros:
            self.close()
            pytest.fail(f"n_zero = {got}, the graph has {zeros} rows without in-edges")

    def skip(self, on):
        if on:
            self.mp.delenv("MGX_PR_SKIP_ZERO", raising=False)
        else:
            self.mp.setenv("MGX_PR_SKIP_ZERO", "0")

    def close(self):
        self.nat.graph_destroy(self.ctx, self.g)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def check_skip(nat, ctx, oracle, monkeypatch, graph, xcd, **kw):
    nv, src, dst = graph
    exp, iters = oracle.pagerank(nv, src, dst, **kw)
    with Built(nat, ctx, monkeypatch, graph, xcd) as b:
        b.skip(False)
        full, full_stats = nat.pagerank(ctx, b.g, nv, **kw)
        b.skip(True)
        rank, stats = nat.pagerank(ctx, b.g, nv, **kw)
    err = np.abs(rank - exp).max()
    print(f"V={nv} xcd={xcd} iterations={stats.iterations} (oracle {iters}) "
          f"oracle_linf={err:.3e} max|skip - full|={np.abs(rank - full).max():.3e}")
    assert stats.iterations == iters
    assert full_stats.iterations == iters
    assert np.array_equal(rank, full)
    assert err <= PR_TOL
    return rank


@pytest.mark.parametrize("xcd", ["0", "1"])
@pytest.mark.parametrize("iterations", [1, 2, 3, 20])
def test_fixed_iterations(nat, ctx, oracle, monkeypatch, base_graph, xcd, iterations):
    # 1 and 2: the two full sweeps; 3: the first that skips; 20: steady state.
    check_skip(nat, ctx, oracle, monkeypatch, base_graph, xcd,
               max_iterations=iterations, eps=0.0)


@pytest.mark.parametrize("xcd", ["0", "1"])
@pytest.mark.parametrize("eps", [1e-3, 1e-7])
def test_stop_epsilon(nat, ctx, oracle, monkeypatch, base_graph, xcd, eps):
    # The skipped rows' Linf term is |base - r0| in sweep 1 and 0 afterwards.
    check_skip(nat, ctx, oracle, monkeypatch, base_graph, xcd, max_iterations=500, eps=eps)


@pytest.mark.parametrize("xcd", ["0", "1"])
def test_chunked_runs(nat, ctx, oracle, monkeypatch, base_graph, xcd):
    nv, src, dst = base_graph
    with Built(nat, ctx, monkeypatch, base_graph, xcd) as b:
        run = nat.pagerank_start(ctx, b.g)
        for n in (1, 1, 5):
            nat.pagerank_iterate(run, n)
        chunked = nat.pagerank_finish(run, nv)
        one, _ = nat.pagerank(ctx, b.g, nv, max_iterations=7, eps=0.0)
        assert np.array_equal(chunked, one)

        # The rule keys on the run's iteration count, not on the graph: a run
        # started after another has skipped sweeps all rows twice again.
        run = nat.pagerank_start(ctx, b.g)
        nat.pagerank_iterate(run, 3)
        nat.pagerank_finish(run, nv)
        second, stats = nat.pagerank(ctx, b.g, nv, max_iterations=20, eps=0.0)
        b.skip(False)
        full, _ = nat.pagerank(ctx, b.g, nv, max_iterations=20, eps=0.0)
    exp, _ = oracle.pagerank(nv, src, dst, max_iterations=20, eps=0.0)
    assert stats.iterations == 20
    assert np.array_equal(second, full)
    assert np.abs(second - exp).max() <= PR_TOL
    exp7, _ = oracle.pagerank(nv, src, dst, max_iterations=7, eps=0.0)
    assert np.abs(chunked - exp7).max() <= PR_TOL


@pytest.mark.parametrize("xcd", ["0", "1"])
def test_graph_with_no_edges(nat, ctx, monkeypatch, xcd):
    # From the third sweep on nothing is launched; each sweep still records its
    # event bracket and counts as an iteration.
    empty = np.zeros(0, dtype=np.int64)
    with Built(nat, ctx, monkeypatch, (5, empty, empty), xcd) as b:
        assert nat.graph_in_zero_rows(b.g) == 5
        run = nat.pagerank_start(ctx, b.g)
        nat.pagerank_iterate(run, 5)
        nat.sync(ctx)
        _, launches = nat.pagerank_timing(run)
        rank = nat.pagerank_finish(run, 5)
    assert launches == 5
    # rank * (1 / sum) in fp64: the uniform vector to a few ulps.
    assert (rank == rank[0]).all() and abs(rank[0] - 0.2) <= 1e-15


@pytest.mark.parametrize("xcd", ["0", "1"])
def test_ring_has_no_zero_rows(nat, ctx, oracle, monkeypatch, xcd):
    graph = ring_graph()
    with Built(nat, ctx, monkeypatch, graph, xcd) as b:
        assert nat.graph_in_zero_rows(b.g) == 0
    check_skip(nat, ctx, oracle, monkeypatch, graph, xcd, max_iterations=20, eps=0.0)


@pytest.mark.parametrize("xcd", ["0", "1"])
def test_katz_with_the_zero_rows_in_front(nat, ctx, oracle, monkeypatch, base_graph, xcd):
    # Katz sweeps bin0 whole; only the order of the rows inside it changed.
    nv, src, dst = base_graph
    with Built(nat, ctx, monkeypatch, base_graph, xcd) as b:
        cent, iters = nat.katz(ctx, b.g, nv, alpha=0.1, epsilon=1e-3)
    exp, iters_exp = oracle.katz(nv, src, dst, alpha=0.1, epsilon=1e-3)
    assert iters == iters_exp
    fin = np.isfinite(exp)
    assert np.array_equal(np.isfinite(cent), fin)
    assert np.abs(cent[fin] - exp[fin]).max() < KATZ_TOL
