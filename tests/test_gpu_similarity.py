"""GPU parity: mgx_similarity_pairs / mgx_similarity_all, bit-exact against
tests/similarity_ref.py (itself pinned to the reference's e2e expectations by
tests/test_similarity_cpu.py), in every mode and for both metrics."""
import os
import subprocess
import sys

import numpy as np
import pytest

import similarity_ref as ref
from bfs_ref import bfs_ref
from memgraph_amd.native import (BUILD_IN_CSR, BUILD_OUT_CSR, BUILD_SYM_CSR, SIM_AUTO,
                                 SIM_JACCARD, SIM_MERGE, SIM_OVERLAP, SIM_SEARCH, Native)
from memgraph_amd.rmat import gen_rmat, gen_uniform
from test_similarity_cpu import assert_rows, case_rows, load_cases

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
METRICS = (SIM_JACCARD, SIM_OVERLAP)
MODES = (SIM_AUTO, SIM_SEARCH, SIM_MERGE)
assert (SIM_JACCARD, SIM_OVERLAP) == (ref.JACCARD, ref.OVERLAP)

OK = 0
ERR_INVALID_ARGUMENT = 3
ERR_TOO_LARGE = 4

# One row per side of every lane-class boundary (8 / 64 / 1024) and of the
# 64- and 256-element merge tiles.
CLASS_DEGREES = [0, 1, 3, 4, 5, 7, 8, 9, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024,
                 1025, 2049]


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
    def __init__(self, nat, ctx, nv, src, dst, flags=BUILD_OUT_CSR):
        self.nat, self.ctx, self.nv = nat, ctx, nv
        self.src = np.asarray(src, dtype=np.int64)
        self.dst = np.asarray(dst, dtype=np.int64)
        self.g = nat.graph_from_coo(ctx, self.src, self.dst, nv, flags=flags)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.nat.graph_destroy(self.ctx, self.g)

    def pairs(self, u, v, metric, mode=SIM_AUTO):
        return self.nat.similarity_pairs(self.ctx, self.g, u, v, metric, mode)

    def all(self, metric):
        return self.nat.similarity_all(self.ctx, self.g, self.nv, metric)

    def check_pairs(self, u, v, sets=None, expected=None):
        """Every mode and metric equals the restatement bit for bit; returns
        {(metric, mode): stats}."""
        if sets is None:
            sets = ref.neighbor_sets(self.nv, self.src, self.dst)
        out = {}
        for metric in METRICS:
            exp = expected[metric] if expected else ref.pairs_from_sets(sets, u, v, metric)
            for mode in MODES:
                sim, common, st = self.pairs(u, v, metric, mode)
                tag = (metric, mode)
                assert np.array_equal(common, exp[1]), tag
                assert np.array_equal(sim, exp[0]), tag  # bit-equal: no NaNs, no -0.0
                assert st.pairs == len(u), tag
                if mode == SIM_SEARCH:
                    assert st.merge_pairs == 0, tag
                if mode == SIM_MERGE:
                    assert st.search_pairs == 0, tag
                out[tag] = st
        return out


def rows_to_coo(rows):
    src = np.concatenate([np.full(len(c), r, dtype=np.int64) for r, c in enumerate(rows)])
    dst = np.concatenate([np.asarray(c, dtype=np.int64) for c in rows])
    return src, dst


@pytest.fixture(scope="module")
def class_graph():
    """V = 4096; row r < 21 is a seeded random subset of [0, V) with
    CLASS_DEGREES[r] elements; all 441 ordered pairs with their expected
    values, computed once."""
    nv = 4096
    rng = np.random.default_rng(2024)
    rows = [np.sort(rng.choice(nv, d, replace=False)) for d in CLASS_DEGREES]
    src, dst = rows_to_coo(rows)
    perm = rng.permutation(len(src))  # the build sorts: give it unsorted input
    src, dst = src[perm], dst[perm]
    n = len(CLASS_DEGREES)
    u = np.repeat(np.arange(n), n)
    v = np.tile(np.arange(n), n)
    sets = ref.neighbor_sets(nv, src, dst)
    expected = {m: ref.pairs_from_sets(sets, u, v, m) for m in METRICS}
    return dict(nv=nv, src=src, dst=dst, u=u, v=v, expected=expected)


# ---- 1. fixtures ---------------------------------------------------------------

def test_reference_fixtures(nat, ctx):
    cases = [c for c in load_cases() if c["expected"] is not None]
    assert len(cases) == 10
    for case in cases:
        def gpu_pairs(nv, src, dst, u, v, metric, mode=SIM_AUTO):
            with Graph(nat, ctx, nv, src, dst) as G:
                return G.pairs(u, v, metric, mode)[0]

        def gpu_all(nv, src, dst, metric):
            with Graph(nat, ctx, nv, src, dst) as G:
                return G.all(metric)[0]

        for mode in MODES:
            rows = case_rows(case, lambda *a: gpu_pairs(*a, mode=mode), gpu_all)
            assert_rows(case, rows)
        # and exactly the restatement, both entry points on every fixture graph
        exact = case_rows(case, lambda *a: ref.pairs(*a)[0], ref.all_pairs)
        assert case_rows(case, gpu_pairs, gpu_all) == exact, case["name"]
        dense = {n: i for i, n in enumerate(case["nodes"])}
        nv = len(dense)
        src = [dense[a] for a, _ in case["edges"]]
        dst = [dense[b] for _, b in case["edges"]]
        with Graph(nat, ctx, nv, src, dst) as G:
            G.check_pairs(np.repeat(np.arange(nv), nv), np.tile(np.arange(nv), nv))
            for metric in METRICS:
                assert np.array_equal(G.all(metric)[0], ref.all_pairs(nv, src, dst, metric))


# ---- 2. lane-class boundaries ----------------------------------------------------

def test_lane_class_boundaries(nat, ctx, class_graph):
    c = class_graph
    with Graph(nat, ctx, c["nv"], c["src"], c["dst"]) as G:
        stats = G.check_pairs(c["u"], c["v"], expected=c["expected"])
    n = len(CLASS_DEGREES)
    zero_len = 2 * n - 1  # every pair with row 0 (no entries) on either side
    for metric in METRICS:
        st = stats[(metric, SIM_AUTO)]
        assert st.search_pairs + st.merge_pairs == n * n - zero_len
        assert st.search_pairs > 0 and st.merge_pairs > 0
        assert stats[(metric, SIM_SEARCH)].search_pairs == n * n - zero_len
        assert stats[(metric, SIM_MERGE)].merge_pairs == n * n - zero_len
        assert st.distinct_entries == len(c["src"])
    # self pairs: 1.0, or 0.0 for the empty row
    diag = c["expected"][SIM_JACCARD][0][np.arange(n) * n + np.arange(n)]
    assert diag.tolist() == [0.0] + [1.0] * (n - 1)


# ---- 3. tile edges ---------------------------------------------------------------

def test_tile_edges(nat, ctx):
    nv = 4096
    rng = np.random.default_rng(7)
    evens = np.arange(0, nv, 2)
    odds = np.arange(1, nv, 2)
    threes = np.arange(0, nv, 3)
    rows = [evens, threes, odds]                                   # 0, 1, 2
    for n in (64, 65, 128, 1024):                                  # 3..10: identical twins
        r = np.sort(rng.choice(nv, n, replace=False))
        rows += [r, r.copy()]
    rows += [np.arange(0, 100), np.arange(2000, 2200)]             # 11, 12: disjoint ranges
    big = np.sort(rng.choice(nv, 200, replace=False))
    shared = big[[63, 64, 127, 128]]
    rows += [big, shared]                                          # 13, 14: A subset of B
    # 15: the same four shared elements among 125 that B lacks: here A is
    # the row that spans several tiles
    others = np.setdiff1d(np.arange(nv), big)
    rows += [np.sort(np.concatenate([shared, rng.choice(others, 125, replace=False)]))]
    src, dst = rows_to_coo(rows)
    pairs = [(0, 1), (0, 2), (3, 4), (5, 6), (7, 8), (9, 10), (11, 12), (12, 11), (14, 13),
             (13, 14), (15, 13), (13, 15), (0, 9), (9, 1)]
    pairs += [(b, a) for a, b in pairs]
    u = np.array([p[0] for p in pairs])
    v = np.array([p[1] for p in pairs])
    with Graph(nat, ctx, nv, src, dst) as G:
        G.check_pairs(u, v)
        for mode in MODES:
            sim, common, _ = G.pairs(u, v, SIM_JACCARD, mode)
            got = dict(zip(pairs, zip(common.tolist(), sim.tolist())))
            assert got[(0, 1)][0] == 683                       # multiples of 6 below 4096
            assert got[(0, 2)] == (0, 0.0)                     # evens against odds
            for a, n in ((3, 64), (5, 65), (7, 128), (9, 1024)):
                assert got[(a, a + 1)] == (n, 1.0)
            assert got[(11, 12)] == (0, 0.0) and got[(12, 11)] == (0, 0.0)
            assert got[(14, 13)][0] == 4 and got[(13, 14)][0] == 4
            assert got[(15, 13)][0] == 4 and got[(13, 15)][0] == 4
            ov, _, _ = G.pairs([14], [13], SIM_OVERLAP, mode)
            assert ov.tolist() == [1.0]


# ---- 4. duplicates ---------------------------------------------------------------

def test_duplicates_and_self_loops(nat, ctx, class_graph):
    c = class_graph
    n = len(CLASS_DEGREES)
    loops = np.arange(1, n)
    base_src = np.concatenate([c["src"], loops])
    base_dst = np.concatenate([c["dst"], loops])
    keys = np.unique(base_src * c["nv"] + base_dst)  # sorted: CSR order
    d_src, d_dst = keys // c["nv"], keys % c["nv"]
    rng = np.random.default_rng(99)
    rep = rng.integers(1, 4, len(keys))
    first = np.r_[True, d_src[1:] != d_src[:-1]]
    last = np.r_[d_src[1:] != d_src[:-1], True]
    rep[first] = 2  # a duplicate at every row start
    rep[last] = 3   # and at every row end (a one-entry row is both: 3 copies)
    assert (rep[~first & ~last] > 1).any() and (rep == 1).any()
    m_src, m_dst = np.repeat(d_src, rep), np.repeat(d_dst, rep)
    perm = rng.permutation(len(m_src))
    m_src, m_dst = m_src[perm], m_dst[perm]
    sets = ref.neighbor_sets(c["nv"], d_src, d_dst)
    assert all(r in sets[r] for r in loops)  # self-loop membership
    with Graph(nat, ctx, c["nv"], d_src, d_dst) as D, \
            Graph(nat, ctx, c["nv"], m_src, m_dst) as M:
        sd = D.check_pairs(c["u"], c["v"], sets=sets)
        sm = M.check_pairs(c["u"], c["v"], sets=sets)
        for key in sd:
            assert sd[key].distinct_entries == len(keys)  # duplicate-free: == E
            assert sm[key].distinct_entries == len(keys)
            assert sm[key].search_pairs == sd[key].search_pairs
            assert sm[key].merge_pairs == sd[key].merge_pairs
        assert len(m_src) > len(keys)
        iu, iv = np.triu_indices(c["nv"], 1)
        sel = iu < 24
        for metric in METRICS:
            a, b = D.all(metric), M.all(metric)
            assert np.array_equal(a[0], b[0])
            assert b[1].distinct_entries == len(keys)
            # the rows with entries against everything, by the pairs path
            exp, _, _ = D.pairs(iu[sel], iv[sel], metric, SIM_SEARCH)
            assert np.array_equal(a[0][:sel.sum()], exp)
            assert not a[0][sel.sum():].any()


# ---- 5. RMAT scale 12 ------------------------------------------------------------

def test_rmat12(nat, ctx):
    scale = 12
    nv = 1 << scale
    src, dst = gen_rmat(scale, 16 * nv, seed=1)
    outdeg = np.bincount(src, minlength=nv)
    rng = np.random.default_rng(12)
    hubs = np.argsort(-outdeg, kind="stable")[:32]
    leaves = np.flatnonzero(outdeg == 1)[:32]
    assert len(leaves) == 32
    u = np.concatenate([rng.integers(0, nv, 20000), np.repeat(hubs, 32), np.repeat(hubs, 32)])
    v = np.concatenate([rng.integers(0, nv, 20000), np.tile(hubs, 32), np.tile(leaves, 32)])
    sets = ref.neighbor_sets(nv, src, dst)
    with Graph(nat, ctx, nv, src, dst) as G:
        stats = G.check_pairs(u, v, sets=sets)
        st = stats[(SIM_JACCARD, SIM_AUTO)]
        assert st.search_pairs > 0 and st.merge_pairs > 0
        assert st.distinct_entries == sum(len(s) for s in sets) < len(src)


# ---- 6. all pairs ----------------------------------------------------------------

@pytest.mark.parametrize("nv", [1, 2, 33, 257, 1000])
def test_all_pairs_uniform(nat, ctx, nv):
    src, dst = gen_uniform(nv, 8 * nv, seed=nv)
    with Graph(nat, ctx, nv, src, dst) as G:
        for metric in METRICS:
            sim, st = G.all(metric)
            assert sim.shape == (nv * (nv - 1) // 2,)
            assert np.array_equal(sim, ref.all_pairs(nv, src, dst, metric)), metric
            assert st.pairs == len(sim)
            assert st.chunks == (1 if nv > 1 else 0)


def test_all_pairs_rmat10_equals_pairs(nat, ctx):
    nv = 1 << 10
    src, dst = gen_rmat(10, 16 * nv, seed=1)
    iu, iv = np.triu_indices(nv, 1)  # row-major i < j
    with Graph(nat, ctx, nv, src, dst) as G:
        for metric in METRICS:
            exp, _, _ = G.pairs(iu, iv, metric)
            sim, _ = G.all(metric)
            assert np.array_equal(sim, exp), metric


def test_all_pairs_every_lane_class(nat, ctx):
    # streamed rows on both sides of 8 / 64 / 1024 entries, tile rows likewise
    nv = 1500
    rng = np.random.default_rng(41)
    degs = {0: 1400, 3: 1024, 7: 1023, 8: 65, 9: 64, 15: 63, 16: 9, 17: 8, 700: 7, 701: 1,
            1490: 1025, 1499: 300}
    rows = [np.sort(rng.choice(nv, degs.get(r, int(rng.integers(0, 4))), replace=False))
            for r in range(nv)]
    src, dst = rows_to_coo(rows)
    iu, iv = np.triu_indices(nv, 1)
    with Graph(nat, ctx, nv, src, dst) as G:
        for metric in METRICS:
            exp, _, _ = G.pairs(iu, iv, metric, SIM_SEARCH)
            sim, _ = G.all(metric)
            assert np.array_equal(sim, exp), metric
        sets = ref.neighbor_sets(nv, src, dst)
        hub = sorted(degs)
        u, v = np.repeat(hub, len(hub)), np.tile(hub, len(hub))
        G.check_pairs(u, v, sets=sets)


CHUNK_CHILD = """
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from memgraph_amd.native import BUILD_OUT_CSR, Native
from memgraph_amd.rmat import gen_uniform
nat = Native()
ctx = nat.init(0)
src, dst = gen_uniform(257, 8 * 257, seed=257)
g = nat.graph_from_coo(ctx, src, dst, 257, flags=BUILD_OUT_CSR)
chunks = []
for metric in (0, 1):
    sim, st = nat.similarity_all(ctx, g, 257, metric)
    np.save(sys.argv[2] + "_%d.npy" % metric, sim)
    chunks.append(st.chunks)
nat.graph_destroy(ctx, g)
nat.destroy(ctx)
print("chunks", *chunks)
"""


def test_all_pairs_chunked(nat, ctx, tmp_path):
    nv = 257
    env = dict(os.environ, MGX_SIM_CHUNK_PAIRS="1000")
    r = subprocess.run([sys.executable, "-c", CHUNK_CHILD, REPO, str(tmp_path / "sim")],
                       env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    chunks = [int(x) for x in r.stdout.split()[1:]]
    # 1000-pair chunks of whole rows over 32896 pairs
    assert all(c >= 33 for c in chunks), chunks
    src, dst = gen_uniform(nv, 8 * nv, seed=nv)
    with Graph(nat, ctx, nv, src, dst) as G:
        for metric in METRICS:
            sim, st = G.all(metric)
            assert st.chunks == 1
            assert np.array_equal(np.load(str(tmp_path / "sim") + "_%d.npy" % metric), sim)


# ---- 7. errors -------------------------------------------------------------------

def test_errors(nat, ctx):
    src, dst = [0, 1, 2], [1, 2, 0]
    with Graph(nat, ctx, 3, src, dst, flags=BUILD_IN_CSR | BUILD_SYM_CSR) as G:
        assert nat.similarity_pairs_status(ctx, G.g, [0], [1], SIM_JACCARD)[0] == \
            ERR_INVALID_ARGUMENT
        assert nat.similarity_all_status(ctx, G.g, 3, SIM_JACCARD)[0] == ERR_INVALID_ARGUMENT
        with pytest.raises(Exception, match="OUT_CSR"):
            nat.similarity_pairs(ctx, G.g, [0], [1], SIM_JACCARD)
    with Graph(nat, ctx, 3, src, dst) as G:
        for u, v in (([-1], [0]), ([0], [-1]), ([3], [0]), ([0], [3]), ([0, 1, 3], [0, 1, 2])):
            assert nat.similarity_pairs_status(ctx, G.g, u, v, SIM_JACCARD)[0] == \
                ERR_INVALID_ARGUMENT
        assert nat.similarity_pairs_status(ctx, G.g, [0], [1], 7)[0] == ERR_INVALID_ARGUMENT
        assert nat.similarity_pairs_status(ctx, G.g, [0], [1], SIM_JACCARD, 7)[0] == \
            ERR_INVALID_ARGUMENT
        assert nat.similarity_all_status(ctx, G.g, 3, 7)[0] == ERR_INVALID_ARGUMENT
        status, sim, common, st = nat.similarity_pairs_status(ctx, G.g, [], [], SIM_OVERLAP)
        assert status == OK and len(sim) == 0 and len(common) == 0 and st.pairs == 0
        # a refused call writes nothing
        status, sim, common, _ = nat.similarity_pairs_status(ctx, G.g, [0, 3], [1, 1],
                                                             SIM_JACCARD)
        assert status == ERR_INVALID_ARGUMENT
        assert np.isnan(sim).all() and (common == -1).all()
        # and the graph still answers
        sim, common, _ = G.pairs([0, 0], [1, 0], SIM_JACCARD)
        assert sim.tolist() == [0.0, 1.0] and common.tolist() == [0, 1]
    nv = 65537
    rng = np.random.default_rng(1)
    with Graph(nat, ctx, nv, rng.integers(0, nv, 16), rng.integers(0, nv, 16)) as G:
        status, sim, _ = nat.similarity_all_status(ctx, G.g, nv, SIM_JACCARD)
        assert status == ERR_TOO_LARGE and sim is None
        with pytest.raises(Exception, match="too large"):
            nat.similarity_all(ctx, G.g, nv, SIM_JACCARD)
        sim, _, _ = G.pairs([0, nv - 1], [nv - 1, nv - 1], SIM_JACCARD)  # pairs still fine
        assert sim.shape == (2,)


# ---- 8. reuse --------------------------------------------------------------------

def test_reuse_and_bfs_afterwards(nat, ctx):
    nv = 2000
    src, dst = gen_uniform(nv, 6 * nv, seed=8)
    src = np.concatenate([src, src[:500]])  # duplicates: the view is a copy, not an alias
    dst = np.concatenate([dst, dst[:500]])
    rng = np.random.default_rng(8)
    u, v = rng.integers(0, nv, 3000), rng.integers(0, nv, 3000)
    with Graph(nat, ctx, nv, src, dst, flags=BUILD_OUT_CSR | BUILD_SYM_CSR) as G:
        a = G.pairs(u, v, SIM_JACCARD)
        b = G.pairs(u, v, SIM_JACCARD)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        assert a[2].distinct_entries == b[2].distinct_entries < len(src)
        all1, _ = G.all(SIM_OVERLAP)
        all2, _ = G.all(SIM_OVERLAP)
        assert np.array_equal(all1, all2)
        exp = ref.pairs(nv, src, dst, u, v, SIM_JACCARD)
        assert np.array_equal(a[0], exp[0]) and np.array_equal(a[1], exp[1])
        for source in (0, nv - 1):
            r = bfs_ref(nv, src, dst, source, directed=True)
            hops, parent, _ = nat.bfs(ctx, G.g, nv, source, directed=True, want_parent=True)
            assert np.array_equal(hops, r.hops) and np.array_equal(parent, r.parent)
