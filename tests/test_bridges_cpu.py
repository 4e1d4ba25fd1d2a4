"""No GPU: the two restatements of tests/bridges_ref.py against the reference's
own fixtures (tests/golden/bridges_e2e.json), against each other and against
brute force. The GPU tests then compare the library with these."""
import json
import os

import numpy as np

import bridges_ref as ref
from memgraph_amd.rmat import gen_uniform

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_cases():
    with open(os.path.join(GOLDEN, "bridges_e2e.json")) as f:
        return json.load(f)


def case_coo(case):
    """(nv, src, dst, dense) with dense ids in node creation order."""
    dense = {n: i for i, n in enumerate(case["nodes"])}
    src = [dense[a] for a, _ in case["edges"]]
    dst = [dense[b] for _, b in case["edges"]]
    return len(dense), src, dst, dense


def case_expected_pairs(case):
    _, _, _, dense = case_coo(case)
    return sorted((min(dense[a], dense[b]), max(dense[a], dense[b]))
                  for a, b in case["expected"])


def check_state(st, nv, src, dst):
    """Invariants of forest_state that do not depend on its own arithmetic."""
    ids = np.arange(nv)
    roots = ids[st.parent == ids]
    assert len(roots) == st.trees
    assert (st.level[roots] == 0).all()
    nonroot = ids[st.parent != ids]
    assert (st.level[nonroot] == st.level[st.parent[nonroot]] + 1).all()
    assert np.array_equal(np.sort(st.pre), ids)
    # a subtree is a preorder interval nested in its parent's
    p = st.parent[nonroot]
    assert (st.pre[nonroot] > st.pre[p]).all()
    assert (st.pre[nonroot] + st.nd[nonroot] <= st.pre[p] + st.nd[p]).all()
    assert st.nd[roots].sum() == nv
    assert (st.low <= st.pre).all() and (st.high >= st.pre).all()


def test_goldens_both_restatements():
    cases = load_cases()
    assert len(cases) == 10
    assert sum(c["kind"] == "e2e" for c in cases) == 3
    for case in cases:
        nv, src, dst, _ = case_coo(case)
        exp = case_expected_pairs(case)
        assert ref.bridges_dfs(nv, src, dst) == exp, case["name"]
        st = ref.forest_state(nv, src, dst)
        assert st.bridges == exp, case["name"]
        check_state(st, nv, src, dst)
        assert ref.bridges_bruteforce(nv, src, dst) == exp, case["name"]


def test_disconnected_golden_forest():
    case = [c for c in load_cases() if c["name"].endswith("HandmadeDisconnectedGraph")][0]
    nv, src, dst, _ = case_coo(case)
    st = ref.forest_state(nv, src, dst)
    assert nv == 26 and st.trees == 3
    assert np.flatnonzero(st.parent == np.arange(nv)).tolist() == [0, 8, 10]
    assert st.pre[[0, 8, 10]].tolist() == [0, 8, 10]  # tree sizes 8, 2, 16


def test_random_multigraphs_three_ways():
    graphs = ref.random_multigraphs()
    assert len(graphs) == 300
    n_bridges = n_loops = n_multi = 0
    for nv, src, dst in graphs:
        assert 2 <= nv <= 40 and len(src) <= 2 * nv
        brute = ref.bridges_bruteforce(nv, src, dst)
        assert ref.bridges_dfs(nv, src, dst) == brute, (nv, src, dst)
        st = ref.forest_state(nv, src, dst)
        assert st.bridges == brute, (nv, src, dst)
        check_state(st, nv, src, dst)
        n_bridges += len(brute)
        n_loops += sum(a == b for a, b in zip(src, dst))
        n_multi += sum(c > 1 for c in ref.pair_multiplicity(nv, src, dst).values())
    assert n_bridges > 300 and n_loops > 100 and n_multi > 100


def test_multiplicity_rules():
    def both(nv, edges):
        src, dst = [a for a, _ in edges], [b for _, b in edges]
        d = ref.bridges_dfs(nv, src, dst)
        assert ref.forest_state(nv, src, dst).bridges == d
        assert ref.bridges_bruteforce(nv, src, dst) == d
        return d

    assert both(2, [(0, 1)]) == [(0, 1)]
    assert both(2, [(1, 0)]) == [(0, 1)]
    assert both(2, [(0, 1), (0, 1)]) == []
    assert both(2, [(0, 1), (1, 0)]) == []
    assert both(2, [(0, 1), (0, 1), (1, 0)]) == []
    assert both(2, [(0, 1), (0, 0), (1, 1)]) == [(0, 1)]
    assert both(6, [(0, 1), (1, 2), (2, 3), (3, 0), (3, 4), (3, 4), (4, 5)]) == [(4, 5)]


def test_uniform_4096_dfs_equals_forest():
    nv = 1 << 12
    src, dst = gen_uniform(nv, nv * 12 // 10, seed=5)
    d = ref.bridges_dfs(nv, src, dst)
    st = ref.forest_state(nv, src, dst)
    assert st.bridges == d
    check_state(st, nv, src, dst)
    assert len(d) > 100 and st.trees > 1 and st.depth > 3


def test_deep_path_no_recursion_limit():
    n = 5000
    src, dst = np.arange(n - 1), np.arange(1, n)
    d = ref.bridges_dfs(n, src, dst)
    assert d == [(i, i + 1) for i in range(n - 1)]
    st = ref.forest_state(n, src, dst)
    assert st.bridges == d and st.depth == n - 1
