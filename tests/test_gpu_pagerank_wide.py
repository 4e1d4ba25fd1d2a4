"""Blocks wider than 256 threads in the XCD-striped launch (MGX_PR_XCD_BLOCK,
DESIGN.md "Memory layout levers" item 5) share one larger LDS table. A wide
block is THREADS / 256 teams of four waves in the 256-lane section and takes
THREADS / LANES segments per step in the others; every segment keeps its lanes
and the order of its additions, so the width changes the speed only.

Every case builds its graph once with MGX_PR_XCD=1 and runs PageRank once per
(width, K) on that same graph (both switches are read when a run starts):
  (a) every result is np.array_equal to the run with MGX_PR_XCD_BLOCK=256 and
      MGX_PR_XCD_LDS=0, the narrow launch without a table;
  (b) every result is within 1e-6 of the fp64 oracle after equal iterations
      (the bar of tests/test_gpu_pagerank.py).
K is in floats per block; None leaves MGX_PR_XCD_LDS unset (the automatic size).
"""
import numpy as np
import pytest

from memgraph_amd.native import BUILD_IN_CSR, Native

pytestmark = pytest.mark.gpu

PR_TOL = 1e-6
HEAVY_MIN = 64
ALL = 1 << 20        # clamps to each stripe's length: every striped gather hits LDS
WIDTHS = [256, 1024]  # every width the library is built for
WIDE = [w for w in WIDTHS if w > 256]
DEFAULT_WIDTH = 1024  # what the library runs with MGX_PR_XCD_BLOCK unset


def bins_graph():
    """V = 1307 (stripes of ~160 ids, one partial granule): heavy rows of
    in-degree 1100, 100, 65, 66 and 67 whose stripe segments land in the 4-,
    16- and 64-lane sections, several of them empty, over rows of in-degree
    20, 3 and 1 (the graph of tests/test_gpu_pagerank_lds.py)."""
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


def hub_graph(nv, hubs):
    """Vertices 0 .. hubs-1 are each fed by the same 9500 sources, dealt ~1187
    to each stripe, so all 8 segments of every hub row land in the 256-lane
    section; plus a ring."""
    ring = np.arange(nv, dtype=np.int64)
    fan = np.arange(100, 9600, dtype=np.int64)
    src = np.concatenate([np.tile(fan, hubs), ring])
    dst = np.concatenate([np.repeat(np.arange(hubs, dtype=np.int64), len(fan)), (ring + 1) % nv])
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

    def __init__(self, nat, ctx, monkeypatch, graph):
        self.nat, self.ctx, self.mp = nat, ctx, monkeypatch
        self.nv, self.src, self.dst = graph
        for name in ("MGX_PR_STRIPES", "MGX_PR_SKIP_ZERO", "MGX_PR_XCD_HEAVY_MIN",
                     "MGX_PR_XCD_BLOCK", "MGX_PR_XCD_LDS"):
            monkeypatch.delenv(name, raising=False)
        monkeypatch.setenv("MGX_PR_XCD", "1")
        self.g = nat.graph_from_coo(ctx, self.src, self.dst, self.nv, flags=BUILD_IN_CSR)
        want = int((np.bincount(self.dst, minlength=self.nv) >= HEAVY_MIN).sum())
        got = nat.graph_xcd_heavy_rows(self.g)
        if got != want or want == 0:
            self.close()
            pytest.fail(f"{got} striped heavy rows, expected {want} > 0")

    def set(self, width, k):
        for name, v in (("MGX_PR_XCD_BLOCK", width), ("MGX_PR_XCD_LDS", k)):
            if v is None:
                self.mp.delenv(name, raising=False)
            else:
                self.mp.setenv(name, str(v))

    def geometry(self):
        """(threads per block, table floats) a run started now would use."""
        run = self.nat.pagerank_start(self.ctx, self.g)
        got = (self.nat.pagerank_xcd_block_threads(run), self.nat.pagerank_xcd_lds_floats(run))
        self.nat.pagerank_finish(run, want_rank=False)
        return got

    def close(self):
        self.nat.graph_destroy(self.ctx, self.g)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def check_widths(nat, ctx, oracle, monkeypatch, graph, ks, widths=WIDTHS, **kw):
    """One build, one run with 256 threads and no table, one per (width, K)."""
    nv, src, dst = graph
    exp, iters = oracle.pagerank(nv, src, dst, **kw)
    with Striped(nat, ctx, monkeypatch, graph) as b:
        b.set(256, 0)
        base, base_stats = nat.pagerank(ctx, b.g, nv, **kw)
        assert base_stats.iterations == iters
        base_err = np.abs(base - exp).max()
        print(f"V={nv} 256 threads K=0 iterations={iters} oracle_linf={base_err:.3e}")
        assert base_err <= PR_TOL
        for width in widths:
            for k in ks:
                if (width, k) == (256, 0):
                    continue
                b.set(width, k)
                rank, stats = nat.pagerank(ctx, b.g, nv, **kw)
                err = np.abs(rank - exp).max()
                diff = np.abs(rank - base).max()
                print(f"V={nv} {width} threads K={k} iterations={stats.iterations} "
                      f"oracle_linf={err:.3e} max|rank - base|={diff:.3e}")
                assert stats.iterations == iters
                assert np.array_equal(rank, base), f"{width} threads, K={k}"   # (a)
                assert err <= PR_TOL, f"{width} threads, K={k}"               # (b)


def test_mixed_sections(nat, ctx, oracle, monkeypatch):
    # Segments in the 4-, 16- and 64-lane sections, several stripes' lists
    # shorter than one block step; 17 crosses a granule of the ~160-id stripes.
    check_widths(nat, ctx, oracle, monkeypatch, bins_graph(), [0, 17, None, ALL])


def test_one_row_idle_teams_at_the_barriers(nat, ctx, oracle, monkeypatch):
    # One 256-lane segment per stripe: one live team per block step, the other
    # teams only attend the barriers.
    check_widths(nat, ctx, oracle, monkeypatch, hub_graph(10000, 1), [0, 256, None, ALL])


def test_five_rows_uneven_team_count(nat, ctx, oracle, monkeypatch):
    # 5 segments per stripe are no multiple of the 4 teams: the last block has
    # one team live and three past the end.
    check_widths(nat, ctx, oracle, monkeypatch, hub_graph(12000, 5), [0, None])


def test_many_rows_several_steps_per_block(nat, ctx, oracle, monkeypatch):
    # 602 segments per stripe are more than the resident grid's teams take in
    # one step (CUs x blocks per CU x teams / 8), so blocks loop in the
    # 256-lane section, and in its last step only some blocks and teams are
    # live while every thread still takes every barrier of its block.
    check_widths(nat, ctx, oracle, monkeypatch, hub_graph(12000, 602), [None], widths=WIDE,
                 max_iterations=3, eps=0.0)


@pytest.mark.parametrize("nv", [1, 15, 129])
def test_fewer_granules_than_stripes(nat, ctx, oracle, monkeypatch, nv):
    check_widths(nat, ctx, oracle, monkeypatch, ring_fan_graph(nv), [None, ALL])


def test_table_above_64_kib(nat, ctx, oracle, monkeypatch):
    # RMAT-18: stripes of 32,768 ids, so a table of 17,000 floats (68,000 B) is
    # larger than 64 KiB and shorter than the stripe.
    scale = 18
    nv = 1 << scale
    src, dst = oracle.gen_rmat(scale, 16 << scale, seed=1)
    graph = (nv, src, dst)
    with Striped(nat, ctx, monkeypatch, graph) as b:
        for width in WIDE:
            b.set(width, 17000)
            assert b.geometry() == (width, 17000)
            b.set(width, None)
            threads, auto = b.geometry()
            print(f"{width} threads: automatic table of {auto} floats")
            assert threads == width and auto % 256 == 0 and 0 < auto <= 32768
        # A 256-thread block keeps the clamp it had: the device's per-block
        # shared-memory limit less the kernel's static LDS (the four reduction
        # slots, 32 B). MI355X reports the whole 160 KiB of a CU as that limit,
        # so 17,000 floats pass unclamped at 256 threads too.
        b.set(256, 17000)
        assert b.geometry() == (256, 17000)
    check_widths(nat, ctx, oracle, monkeypatch, graph, [17000, None], max_iterations=5, eps=0.0)


@pytest.mark.parametrize("width", WIDE)
def test_chunked_run_equals_oneshot(nat, ctx, monkeypatch, rmat16, width):
    # The table is refilled from the current ping-pong buffer on every sweep.
    nv = rmat16[0]
    with Striped(nat, ctx, monkeypatch, rmat16) as b:
        b.set(width, None)
        run = nat.pagerank_start(ctx, b.g)
        nat.pagerank_iterate(run, 7)
        nat.pagerank_iterate(run, 13)
        nat.sync(ctx)
        _, launches = nat.pagerank_timing(run)
        chunked = nat.pagerank_finish(run, nv)
        one, _ = nat.pagerank(ctx, b.g, nv, max_iterations=20, eps=0.0)
        b.set(256, 0)
        plain, _ = nat.pagerank(ctx, b.g, nv, max_iterations=20, eps=0.0)
    assert launches == 20
    assert np.array_equal(chunked, one)
    assert np.array_equal(chunked, plain)


def test_width_follows_the_switch(nat, ctx, monkeypatch):
    with Striped(nat, ctx, monkeypatch, bins_graph()) as b:
        for width in WIDTHS:
            b.set(width, None)
            assert b.geometry()[0] == width
        b.set(None, None)
        assert b.geometry()[0] == DEFAULT_WIDTH
        # A width the library has no kernel for is an error, not a fallback.
        b.set(512, None)
        with pytest.raises(Exception, match="MGX_PR_XCD_BLOCK"):
            nat.pagerank_start(ctx, b.g)
