"""The stripe-major column stream of the XCD-striped PageRank sweep
(MGX_PR_XCD_STREAM, DESIGN.md "Memory layout levers" item 6) changes where the
striped launch reads its column ids from, not what it adds up.

Every case builds its graph twice with MGX_PR_XCD=1: with MGX_PR_XCD_STREAM=0
(the launch reads in_col between the stripe boundaries) and with the variable
unset (the launch reads the stream), asserts through mgx_graph_xcd_stream_ints
which of the two each build is, and runs PageRank on both:
  (a) the two results are np.array_equal - exact, because a segment sits in
      the stream at the same offset mod 4 as in in_col, so every lane adds the
      same values in the same order;
  (b) each is within 1e-6 of the fp64 oracle after equal iterations (the bar
      of tests/test_gpu_pagerank.py).
"""
import numpy as np
import pytest

from memgraph_amd.native import BUILD_IN_CSR, Native

from test_gpu_pagerank_lds import bins_graph, ring_fan_graph

pytestmark = pytest.mark.gpu

PR_TOL = 1e-6
STRIPES, GRANULE = 8, 16


def hub_graph():
    """V = 10000: vertices 0..3 are each fed by the same 9500 sources, plus a
    ring. The sources deal ~1187 to each stripe, so all 8 segments of each hub
    row land in the 256-lane section; the hub rows are 9501 long and adjacent
    in the renumbered CSR, so their segments start at every residue mod 4."""
    nv = 10000
    ring = np.arange(nv, dtype=np.int64)
    fan = np.arange(100, 9600, dtype=np.int64)
    src = np.concatenate([fan, fan, fan, fan, ring])
    dst = np.concatenate([np.full(len(fan), h, dtype=np.int64) for h in range(4)]
                         + [(ring + 1) % nv])
    return nv, src, dst


def stripe_off(nv, x):
    """mgx_xcd_stripe_off: first id of stripe x."""
    g = (nv + GRANULE - 1) // GRANULE
    if g == 0:
        return 0
    rem = g % STRIPES
    off = ((g // STRIPES) * x + min(rem, x)) * GRANULE
    if (g - 1) % STRIPES < x:
        off -= g * GRANULE - nv
    return off


def host_segments(graph, rows):
    """[(start, length)] of the 8 stripe segments of each of `rows` (original
    ids) in the renumbered in-CSR as the build lays it out: hot-first by
    descending out-degree (stable, ties by id), dealt to 8 stripes in granules
    of 16, rows in id order, columns sorted."""
    nv, src, dst = graph
    hot = np.argsort(-np.bincount(src, minlength=nv), kind="stable")
    p = np.arange(nv)
    q = p // GRANULE
    off = np.array([stripe_off(nv, x) for x in range(STRIPES + 1)])
    new_id = np.empty(nv, dtype=np.int64)
    new_id[hot] = off[q % STRIPES] + (q // STRIPES) * GRANULE + p % GRANULE
    assert np.array_equal(np.sort(new_id), p)
    nsrc, ndst = new_id[src], new_id[dst]
    row_ptr = np.concatenate([[0], np.cumsum(np.bincount(ndst, minlength=nv))])
    out = []
    for r in rows:
        cols = np.sort(nsrc[ndst == new_id[r]])
        cut = np.searchsorted(cols, off)
        out.extend((int(row_ptr[new_id[r]] + cut[x]), int(cut[x + 1] - cut[x]))
                   for x in range(STRIPES))
    return out


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


class Pair:
    """`graph` built twice with MGX_PR_XCD=1: `.plain` with MGX_PR_XCD_STREAM=0
    and `.stream` with it unset. Both must have striped rows; only the second
    may have a stream."""

    def __init__(self, nat, ctx, monkeypatch, graph, heavy_min=None):
        self.nat, self.ctx, self.mp = nat, ctx, monkeypatch
        self.nv, src, dst = graph
        self.graphs = []
        monkeypatch.delenv("MGX_PR_STRIPES", raising=False)
        monkeypatch.delenv("MGX_PR_SKIP_ZERO", raising=False)
        if heavy_min is None:
            monkeypatch.delenv("MGX_PR_XCD_HEAVY_MIN", raising=False)
        else:
            monkeypatch.setenv("MGX_PR_XCD_HEAVY_MIN", str(heavy_min))
        monkeypatch.setenv("MGX_PR_XCD", "1")
        want = int((np.bincount(dst, minlength=self.nv) >= (heavy_min or 64)).sum())
        try:
            monkeypatch.setenv("MGX_PR_XCD_STREAM", "0")
            self.plain = self.build(src, dst)
            monkeypatch.delenv("MGX_PR_XCD_STREAM")
            self.stream = self.build(src, dst)
            for g in self.graphs:
                got = nat.graph_xcd_heavy_rows(g)
                assert got == want and want > 0, f"{got} striped heavy rows, expected {want} > 0"
            assert nat.graph_xcd_stream_ints(self.plain) == -1
            self.stream_ints = nat.graph_xcd_stream_ints(self.stream)
            assert self.stream_ints > 0
        except BaseException:
            self.close()
            raise

    def build(self, src, dst):
        g = self.nat.graph_from_coo(self.ctx, src, dst, self.nv, flags=BUILD_IN_CSR)
        self.graphs.append(g)
        return g

    def set_k(self, k):
        if k is None:
            self.mp.delenv("MGX_PR_XCD_LDS", raising=False)
        else:
            self.mp.setenv("MGX_PR_XCD_LDS", str(k))

    def set_width(self, width):
        self.mp.setenv("MGX_PR_XCD_BLOCK", str(width))

    def close(self):
        for g in self.graphs:
            self.nat.graph_destroy(self.ctx, g)
        self.graphs = []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def check_pair(nat, ctx, oracle, monkeypatch, graph, ks=(None,), widths=(1024,),
               heavy_min=None, **kw):
    """Both builds once; one run on each per (width, K). Returns the last
    stream rank."""
    nv, src, dst = graph
    exp, iters = oracle.pagerank(nv, src, dst, **kw)
    rank = None
    with Pair(nat, ctx, monkeypatch, graph, heavy_min=heavy_min) as b:
        for width in widths:
            b.set_width(width)
            for k in ks:
                b.set_k(k)
                base, base_stats = nat.pagerank(ctx, b.plain, nv, **kw)
                rank, stats = nat.pagerank(ctx, b.stream, nv, **kw)
                base_err = np.abs(base - exp).max()
                err = np.abs(rank - exp).max()
                diff = np.abs(rank - base).max()
                print(f"V={nv} width={width} K={k} stream_ints={b.stream_ints} "
                      f"iterations={stats.iterations}/{iters} oracle_linf plain={base_err:.3e} "
                      f"stream={err:.3e} max|stream - plain|={diff:.3e}")
                assert base_stats.iterations == iters and stats.iterations == iters
                assert np.array_equal(rank, base), f"width={width} K={k}"   # (a)
                assert base_err <= PR_TOL and err <= PR_TOL, f"width={width} K={k}"  # (b)
    return rank


def test_bins_graph(nat, ctx, oracle, monkeypatch):
    # 4-, 16- and 64-lane segments, several empty.
    check_pair(nat, ctx, oracle, monkeypatch, bins_graph(), ks=[0, 17, None],
               widths=[256, 1024])


def test_bins_graph_heavy_min_8(nat, ctx, oracle, monkeypatch):
    check_pair(nat, ctx, oracle, monkeypatch, bins_graph(), ks=[0, 17, None],
               widths=[256, 1024], heavy_min=8)


def test_hub_graph_segment_starts_cover_every_residue():
    # Host side only: what the next test relies on.
    segs = host_segments(hub_graph(), rows=range(4))
    assert len(segs) == 32
    assert all(length >= 1024 for _, length in segs), segs
    assert {start % 4 for start, _ in segs} == {0, 1, 2, 3}, segs


def test_hub_graph_256_lane_segments_at_every_residue(nat, ctx, oracle, monkeypatch):
    check_pair(nat, ctx, oracle, monkeypatch, hub_graph(), ks=[0, None], widths=[256, 1024])


@pytest.mark.parametrize("nv", [1, 15, 17, 129])
def test_ring_fan_short_and_empty_stripes(nat, ctx, oracle, monkeypatch, nv):
    check_pair(nat, ctx, oracle, monkeypatch, ring_fan_graph(nv))


def test_rmat16_20_iterations(nat, ctx, oracle, monkeypatch, rmat16):
    rank = check_pair(nat, ctx, oracle, monkeypatch, rmat16, max_iterations=20, eps=0.0)
    assert abs(rank.sum() - 1.0) < 1e-9


def test_rmat16_chunked_run_equals_oneshot(nat, ctx, monkeypatch, rmat16):
    nv = rmat16[0]
    with Pair(nat, ctx, monkeypatch, rmat16) as b:
        b.set_k(None)
        run = nat.pagerank_start(ctx, b.stream)
        nat.pagerank_iterate(run, 7)
        nat.pagerank_iterate(run, 13)
        nat.sync(ctx)
        _, launches = nat.pagerank_timing(run)
        chunked = nat.pagerank_finish(run, nv)
        one, _ = nat.pagerank(ctx, b.stream, nv, max_iterations=20, eps=0.0)
        plain, _ = nat.pagerank(ctx, b.plain, nv, max_iterations=20, eps=0.0)
    assert launches == 20
    assert np.array_equal(chunked, one)
    assert np.array_equal(chunked, plain)


def test_rmat16_delta_path_stops_with_the_oracle(nat, ctx, oracle, monkeypatch, rmat16):
    check_pair(nat, ctx, oracle, monkeypatch, rmat16, max_iterations=50, eps=1e-7)
