"""GPU parity: mgx_bridges pairs, bit-exact against tests/bridges_ref.py
(bridges_dfs, brute force, or a closed form where stated), and the six
forest / interval state arrays of mgx_bridges_state bit-for-bit against
forest_state."""
import numpy as np
import pytest

import bridges_ref as ref
from memgraph_amd.native import BUILD_IN_CSR, BUILD_OUT_CSR, BUILD_SYM_CSR, Native
from memgraph_amd.rmat import gen_rmat, gen_uniform
from test_bridges_cpu import case_coo, case_expected_pairs, load_cases

pytestmark = pytest.mark.gpu

ERR_INVALID_ARGUMENT = 3


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


def as_pairs(p):
    return [tuple(r) for r in np.asarray(p).tolist()]


def run(nat, ctx, nv, src, dst, expected=None, state=True, tag=None):
    """Pairs == expected (default: bridges_dfs); all six state arrays ==
    forest_state; stats consistent. Returns (pairs, stats, forest_state)."""
    src = np.asarray(src, dtype=np.int64).reshape(-1)
    dst = np.asarray(dst, dtype=np.int64).reshape(-1)
    g = nat.graph_from_coo(ctx, src, dst, nv, flags=BUILD_SYM_CSR)
    try:
        pairs, st = nat.bridges(ctx, g, nv)
        got_state = nat.bridges_state(ctx, g, nv) if state else None
    finally:
        nat.graph_destroy(ctx, g)
    if expected is None:
        expected = ref.bridges_dfs(nv, src, dst)
    assert as_pairs(pairs) == expected, tag
    assert st.bridges == len(expected), tag
    fs = None
    if state:
        fs = ref.forest_state(nv, src, dst)
        assert fs.bridges == expected, tag
        for name in ref.STATE_ARRAYS:
            assert np.array_equal(got_state[name], getattr(fs, name)), (tag, name)
        assert (st.trees, st.depth) == (fs.trees, fs.depth), tag
        assert st.level_launches == 3 * fs.depth, tag
        assert st.nontree_entries == 2 * len(src) - (nv - fs.trees), tag
    assert st.ms > 0 and 0 < st.forest_ms <= st.ms, tag
    return pairs, st, fs


def test_goldens(nat, ctx):
    cases = load_cases()
    assert len(cases) == 10
    for case in cases:
        nv, src, dst, _ = case_coo(case)
        exp = case_expected_pairs(case)
        assert ref.bridges_dfs(nv, src, dst) == exp
        run(nat, ctx, nv, src, dst, expected=exp, tag=case["name"])


def test_random_multigraphs_against_bruteforce(nat, ctx):
    graphs = ref.random_multigraphs()
    assert len(graphs) == 300
    for i, (nv, src, dst) in enumerate(graphs):
        run(nat, ctx, nv, src, dst, expected=ref.bridges_bruteforce(nv, src, dst), tag=i)


def test_multiplicity(nat, ctx):
    def pairs(nv, edges):
        p, _, _ = run(nat, ctx, nv, [a for a, _ in edges], [b for _, b in edges], tag=edges)
        return as_pairs(p)

    assert pairs(2, [(0, 1)]) == [(0, 1)]
    assert pairs(2, [(1, 0)]) == [(0, 1)]
    assert pairs(2, [(0, 1), (0, 1)]) == []  # doubled, same direction
    assert pairs(2, [(0, 1), (1, 0)]) == []  # antiparallel
    assert pairs(2, [(0, 1), (0, 1), (0, 1)]) == []  # tripled
    assert pairs(2, [(0, 1), (1, 0), (0, 1)]) == []
    assert pairs(2, [(0, 1), (0, 0)]) == [(0, 1)]  # self-loop on either endpoint
    assert pairs(2, [(0, 1), (1, 1)]) == [(0, 1)]
    assert pairs(2, [(0, 1), (0, 0), (1, 1), (1, 1)]) == [(0, 1)]
    assert pairs(3, [(0, 1), (1, 2), (1, 1), (2, 2), (2, 1)]) == [(0, 1)]
    # NeighborCycle: {3,4},{3,4} is not a bridge, {4,5} is
    assert pairs(6, [(0, 1), (1, 2), (2, 3), (3, 0), (3, 4), (3, 4), (4, 5)]) == [(4, 5)]


RING = 12


def hub_graph(degree, ties, n_before):
    """A ring of RING vertices and a hub of sym degree exactly `degree`: `ties`
    edges to the ring vertex `a` and degree - ties leaves. The hub has the
    largest id, so a is its parent and every leaf's parent is the hub; n_before
    leaves have ids below a, which puts a's run at position n_before of the
    hub's sorted row. Returns (nv, src, dst, expected pairs)."""
    n_leaves = degree - ties
    assert 0 <= n_before <= n_leaves
    base = list(range(RING - 1))  # ring vertices 0..RING-2, and a
    a = RING - 1 + n_before
    leaves = [RING - 1 + i for i in range(n_before)] + \
             [RING + i for i in range(n_before, n_leaves)]
    hub = RING + n_leaves
    ring = base + [a]
    edges = [(ring[i], ring[(i + 1) % RING]) for i in range(RING)]
    edges += [(hub, a) if t % 2 else (a, hub) for t in range(ties)]
    edges += [(hub, x) if i % 3 else (x, hub) for i, x in enumerate(leaves)]
    expected = sorted([(x, hub) for x in leaves] + ([(a, hub)] if ties == 1 else []))
    return hub + 1, [e[0] for e in edges], [e[1] for e in edges], expected


@pytest.mark.parametrize("degree", [7, 8, 63, 64, 1023, 1024, 1100])
def test_degree_class_boundaries(nat, ctx, degree):
    for ties in (1, 2):
        n_leaves = degree - ties
        places = {0, n_leaves // 2, n_leaves}  # the run at the start, middle, end
        if degree == 1100:
            places |= {63, 255}  # the two-entry run across a 64- and a 256-entry boundary
        for n_before in sorted(places):
            nv, src, dst, exp = hub_graph(degree, ties, n_before)
            rp, _, cols = ref.sym_csr(nv, src, dst)
            hub, a = nv - 1, RING - 1 + n_before
            row = cols[rp[hub]:rp[hub + 1]]
            assert len(row) == degree
            assert row[n_before:n_before + ties].tolist() == [a] * ties
            assert ref.bridges_dfs(nv, src, dst) == exp
            _, _, fs = run(nat, ctx, nv, src, dst, expected=exp, tag=(degree, ties, n_before))
            assert fs.parent[hub] == a


def test_components(nat, ctx):
    _, st, _ = run(nat, ctx, 100, [], [], expected=[])
    assert (st.trees, st.depth, st.bridges, st.level_launches) == (100, 0, 0, 0)
    case = [c for c in load_cases() if c["name"].endswith("HandmadeDisconnectedGraph")][0]
    nv, src, dst, _ = case_coo(case)
    _, st, _ = run(nat, ctx, nv, src, dst, expected=case_expected_pairs(case))
    assert nv == 26 and st.trees == 3
    # the minimum-id vertex is isolated; so are 4 and the last one
    _, st, fs = run(nat, ctx, 8, [1, 2, 3, 5], [2, 3, 1, 6])
    assert st.trees == 5 and fs.bridges == [(5, 6)]  # {0}, {1,2,3}, {4}, {5,6}, {7}
    _, st, _ = run(nat, ctx, 1, [], [], expected=[])
    assert st.trees == 1
    _, st, _ = run(nat, ctx, 1, [0, 0], [0, 0], expected=[])
    assert st.trees == 1


def test_depth(nat, ctx):
    n = 4096
    a = np.arange(n - 1)
    _, st, _ = run(nat, ctx, n, a, a + 1, expected=[(i, i + 1) for i in range(n - 1)])
    assert (st.bridges, st.depth, st.trees) == (n - 1, n - 1, 1)
    assert st.level_launches == 3 * (n - 1)
    ring = np.arange(n)
    _, st, _ = run(nat, ctx, n, ring, (ring + 1) % n, expected=[])
    assert st.depth == n // 2
    # chords (64k, 64k + 64): every path edge below 4032 lies on a cycle
    c = np.arange(0, n - 64, 64)
    exp = [(i, i + 1) for i in range(c[-1] + 64, n - 1)]
    assert len(exp) == 63
    run(nat, ctx, n, np.concatenate([a, c]), np.concatenate([a + 1, c + 64]), expected=exp)


def test_uniform_14(nat, ctx):
    nv = 1 << 14
    src, dst = gen_uniform(nv, nv * 12 // 10, seed=5)
    pairs, st, fs = run(nat, ctx, nv, src, dst)
    assert st.bridges > 1000 and st.trees > 100 and st.depth > 5


def test_rmat_14(nat, ctx):
    nv = 1 << 14
    src, dst = gen_rmat(14, 8 * nv, seed=3)
    pairs, st, fs = run(nat, ctx, nv, src, dst)
    assert st.bridges > 100 and st.trees > 100
    assert np.diff(ref.sym_csr(nv, src, dst)[0]).max() >= 1024  # the 256-lane bin is in play


def test_comet_scan_overflow(nat, ctx):
    """Path 0-1-...-2999, 1,500,000 leaves on vertex 2999, chord (10, 20). The
    sum of nd over the non-roots, which the sibling scan runs over, is about
    4.5e9 > 2^32. Bridges in closed form: every edge except the ten path edges
    10-11 ... 19-20 and the chord."""
    n_path, n_leaves = 3000, 1_500_000
    nv = n_path + n_leaves
    a = np.arange(n_path - 1)
    leaves = n_path + np.arange(n_leaves)
    src = np.concatenate([a, np.full(n_leaves, n_path - 1), [10]])
    dst = np.concatenate([a + 1, leaves, [20]])
    g = nat.graph_from_coo(ctx, src, dst, nv, flags=BUILD_SYM_CSR)
    try:
        pairs, st = nat.bridges(ctx, g, nv)
        state = nat.bridges_state(ctx, g, nv)
    finally:
        nat.graph_destroy(ctx, g)
    assert int(state["nd"].sum()) - nv > 1 << 32  # the scan did pass 2^32
    assert len(pairs) == st.bridges == 2989 + n_leaves
    # the chord makes 20 a child of 10 at level 11: the far end is 9 levels nearer
    assert (st.trees, st.depth) == (1, n_path - 9)
    got = set(as_pairs(pairs[:n_path]))
    for i in range(10, 20):
        assert (i, i + 1) not in got
    assert (10, 20) not in got
    assert as_pairs(pairs[:11]) == [(i, i + 1) for i in range(10)] + [(20, 21)]
    assert tuple(pairs[-1]) == (n_path - 1, nv - 1)
    tail = pairs[2989:]
    assert (tail[:, 0] == n_path - 1).all()
    assert np.array_equal(tail[:, 1], leaves)  # every leaf, in order
    # the preorder is a permutation of [0, V); the leaves are numbered last, in id order
    assert np.array_equal(np.sort(state["pre"]), np.arange(nv))
    assert np.array_equal(state["pre"][n_path:], leaves)
    assert state["nd"][0] == nv and state["nd"][n_path - 1] == n_leaves + 1


def test_deterministic_and_leaves_bfs_wcc_alone(nat, ctx):
    nv = 3000
    rng = np.random.default_rng(7)
    src, dst = rng.integers(0, nv, 3300), rng.integers(0, nv, 3300)
    g = nat.graph_from_coo(ctx, src, dst, nv, flags=BUILD_SYM_CSR | BUILD_OUT_CSR)
    try:
        comp0, n0 = nat.wcc(ctx, g, nv)
        hops0, par0, bst0 = nat.bfs(ctx, g, nv, int(src[0]), want_parent=True)
        p1, st1 = nat.bridges(ctx, g, nv)
        s1 = nat.bridges_state(ctx, g, nv)
        p2, st2 = nat.bridges(ctx, g, nv)
        s2 = nat.bridges_state(ctx, g, nv)
        comp1, n1 = nat.wcc(ctx, g, nv)
        hops1, par1, bst1 = nat.bfs(ctx, g, nv, int(src[0]), want_parent=True)
    finally:
        nat.graph_destroy(ctx, g)
    assert np.array_equal(p1, p2) and len(p1) > 50
    assert (st1.bridges, st1.trees, st1.depth) == (st2.bridges, st2.trees, st2.depth)
    for name in ref.STATE_ARRAYS:
        assert np.array_equal(s1[name], s2[name]), name
    assert as_pairs(p1) == ref.bridges_dfs(nv, src, dst)
    assert n0 == n1 == st1.trees and np.array_equal(comp0, comp1)
    assert np.array_equal(hops0, hops1) and np.array_equal(par0, par1)
    assert (bst0.depth, bst0.reached) == (bst1.depth, bst1.reached)


def test_needs_sym_csr(nat, ctx):
    for flags in (BUILD_IN_CSR, BUILD_OUT_CSR):
        g = nat.graph_from_coo(ctx, [0, 1], [1, 2], 4, flags=flags)
        try:
            status, pairs, _ = nat.bridges_status(ctx, g, 4)
            assert status == ERR_INVALID_ARGUMENT and len(pairs) == 0
            assert nat.lib.mgx_last_error() == \
                b"bridges needs a graph built with MGX_BUILD_SYM_CSR"
            with pytest.raises(RuntimeError, match="MGX_BUILD_SYM_CSR"):
                nat.bridges_state(ctx, g, 4)
        finally:
            nat.graph_destroy(ctx, g)
    g = nat.graph_from_coo(ctx, [0, 1], [1, 2], 4, flags=BUILD_SYM_CSR)
    try:  # the context is still usable
        pairs, _ = nat.bridges(ctx, g, 4)
        assert as_pairs(pairs) == [(0, 1), (1, 2)]
    finally:
        nat.graph_destroy(ctx, g)
