"""The hot prefix of each XCD stripe in LDS (MGX_PR_XCD_LDS, DESIGN.md "Memory
layout levers" item 5) changes where the striped launch reads contrib from,
not what it adds up.

Every case builds its graph once with MGX_PR_XCD=1 and runs PageRank once per
MGX_PR_XCD_LDS value on that same graph (the value is read when a run starts):
  (a) every result is np.array_equal to the MGX_PR_XCD_LDS=0 run, which is the
      launch without a table - exact equality, because the gathered values have
      the same bits and the fp64 additions keep their order;
  (b) every result is within 1e-6 of the fp64 oracle after equal iterations
      (the bar of tests/test_gpu_pagerank.py).
K is in floats per block; None leaves the variable unset (the automatic size).
"""
import numpy as np
import pytest

from memgraph_amd.native import BUILD_IN_CSR, Native

pytestmark = pytest.mark.gpu

PR_TOL = 1e-6
HEAVY_MIN = 64
ALL = 1 << 20   # clamps to each stripe's length: every striped gather hits LDS


def bins_graph():
    """V = 1307 (stripes of ~160 ids, one partial granule): heavy rows of
    in-degree 1100, 100, 65, 66 and 67 whose stripe segments land in the 16-
    and 64-lane sections, several of them empty, over rows of in-degree 20, 3
    and 1."""
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
    """V = 10000: vertex 0 fed by 9500 sources of out-degree 2, dealt ~1187 to
    each stripe, so all 8 segments of the row land in the 256-lane section (the
    hand-unrolled body with its head and tail loops); plus a ring."""
    nv = 10000
    ring = np.arange(nv, dtype=np.int64)
    fan = np.arange(100, 9600, dtype=np.int64)
    src = np.concatenate([fan, ring])
    dst = np.concatenate([np.zeros(len(fan), dtype=np.int64), (ring + 1) % nv])
    return nv, src, dst


def ring_fan_graph(nv):
    """70 parallel edges into vertex 0 from up to 3 sources, plus a ring: one
    heavy row on a graph with fewer granules than stripes, so stripes are empty
    or much shorter than K. At V = 1 it is 70 self-loops."""
    sources = np.array([nv // 4, nv // 2, (3 * nv) // 4], dtype=np.int64) % nv
    fan = np.resize(sources, 70)
    if nv == 1:
        return nv, fan, np.zeros(70, dtype=np.int64)
    ring = np.arange(nv, dtype=np.int64)
    src = np.concatenate([fan, ring])
    dst = np.concatenate([np.zeros(70, dtype=np.int64), (ring + 1) % nv])
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
def rmat16(oracle):
    scale = 16
    src, dst = oracle.gen_rmat(scale, 16 << scale, seed=1)
    return 1 << scale, src, dst


class Striped:
    """`graph` built with MGX_PR_XCD=1; the striped launch must have rows."""

    def __init__(self, nat, ctx, monkeypatch, graph, heavy_min=None):
        self.nat, self.ctx, self.mp = nat, ctx, monkeypatch
        self.nv, self.src, self.dst = graph
        monkeypatch.delenv("MGX_PR_STRIPES", raising=False)
        monkeypatch.delenv("MGX_PR_SKIP_ZERO", raising=False)
        if heavy_min is None:
            monkeypatch.delenv("MGX_PR_XCD_HEAVY_MIN", raising=False)
        else:
            monkeypatch.setenv("MGX_PR_XCD_HEAVY_MIN", str(heavy_min))
        monkeypatch.setenv("MGX_PR_XCD", "1")
        self.g = nat.graph_from_coo(ctx, self.src, self.dst, self.nv, flags=BUILD_IN_CSR)
        want = int((np.bincount(self.dst, minlength=self.nv) >= (heavy_min or HEAVY_MIN)).sum())
        got = nat.graph_xcd_heavy_rows(self.g)
        if got != want or want == 0:
            self.close()
            pytest.fail(f"{got} striped heavy rows, expected {want} > 0")

    def set_k(self, k):
        if k is None:
            self.mp.delenv("MGX_PR_XCD_LDS", raising=False)
        else:
            self.mp.setenv("MGX_PR_XCD_LDS", str(k))

    def close(self):
        self.nat.graph_destroy(self.ctx, self.g)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def check_ks(nat, ctx, oracle, monkeypatch, graph, ks, heavy_min=None, **kw):
    """One build, one run per K (and one with K = 0); returns the K = 0 rank."""
    nv, src, dst = graph
    exp, iters = oracle.pagerank(nv, src, dst, **kw)
    with Striped(nat, ctx, monkeypatch, graph, heavy_min=heavy_min) as b:
        b.set_k(0)
        base, base_stats = nat.pagerank(ctx, b.g, nv, **kw)
        assert base_stats.iterations == iters
        base_err = np.abs(base - exp).max()
        print(f"V={nv} K=0 iterations={iters} oracle_linf={base_err:.3e}")
        assert base_err <= PR_TOL
        for k in ks:
            b.set_k(k)
            rank, stats = nat.pagerank(ctx, b.g, nv, **kw)
            err = np.abs(rank - exp).max()
            diff = np.abs(rank - base).max()
            print(f"V={nv} K={k} iterations={stats.iterations} oracle_linf={err:.3e} "
                  f"max|rank - rank(K=0)|={diff:.3e}")
            assert stats.iterations == iters
            assert np.array_equal(rank, base), f"K={k}"      # (a)
            assert err <= PR_TOL, f"K={k}"                   # (b)
    return base


def test_bins_graph(nat, ctx, oracle, monkeypatch):
    # Stripes of ~160 ids: 16 is exactly one granule, 17 crosses one, 48 is a
    # part of every stripe, ALL clamps to each stripe's own length.
    check_ks(nat, ctx, oracle, monkeypatch, bins_graph(), [0, 1, 16, 17, 48, None, ALL])


def test_table_size_follows_the_switch(nat, ctx, monkeypatch):
    # Read when a run starts, so one graph serves runs with different K. The
    # longest stripe of V = 1307 (82 granules dealt to 8 stripes) is 176 ids.
    with Striped(nat, ctx, monkeypatch, bins_graph()) as b:
        for k, want in [(0, 0), (1, 1), (17, 17), (ALL, 176), (None, 176)]:
            b.set_k(k)
            run = nat.pagerank_start(ctx, b.g)
            got = nat.pagerank_xcd_lds_floats(run)
            nat.pagerank_finish(run, want_rank=False)
            assert got == want, f"K={k}"


def test_wide_row_every_segment_in_the_256_lane_section(nat, ctx, oracle, monkeypatch):
    check_ks(nat, ctx, oracle, monkeypatch, wide_row_graph(), [0, 256, None, ALL])


@pytest.mark.parametrize("nv", [1, 15, 17, 129])
def test_ring_fan_short_and_empty_stripes(nat, ctx, oracle, monkeypatch, nv):
    check_ks(nat, ctx, oracle, monkeypatch, ring_fan_graph(nv), [None, ALL])


def test_bins_graph_heavy_min_8(nat, ctx, oracle, monkeypatch):
    # The 16-lane section is striped too; its segments fall to the 4-lane one.
    check_ks(nat, ctx, oracle, monkeypatch, bins_graph(), [0, None], heavy_min=8)


def test_rmat16_20_iterations(nat, ctx, oracle, monkeypatch, rmat16):
    rank = check_ks(nat, ctx, oracle, monkeypatch, rmat16, [0, None], max_iterations=20, eps=0.0)
    assert abs(rank.sum() - 1.0) < 1e-9


def test_chunked_run_equals_oneshot(nat, ctx, monkeypatch, rmat16):
    # The table is refilled from the current ping-pong buffer on every sweep.
    nv = rmat16[0]
    with Striped(nat, ctx, monkeypatch, rmat16) as b:
        b.set_k(None)
        run = nat.pagerank_start(ctx, b.g)
        nat.pagerank_iterate(run, 7)
        nat.pagerank_iterate(run, 13)
        nat.sync(ctx)
        _, launches = nat.pagerank_timing(run)
        chunked = nat.pagerank_finish(run, nv)
        one, _ = nat.pagerank(ctx, b.g, nv, max_iterations=20, eps=0.0)
        b.set_k(0)
        plain, _ = nat.pagerank(ctx, b.g, nv, max_iterations=20, eps=0.0)
    assert launches == 20
    assert np.array_equal(chunked, one)
    assert np.array_equal(chunked, plain)
