"""tests/similarity_ref.py (the expected value of every GPU similarity test)
against the reference's own e2e expectations and the edge cases of
node_similarity.hpp. No GPU."""
import json
import os

import numpy as np

import similarity_ref as ref

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "node_similarity_e2e.json")
METRIC = {"jaccard": ref.JACCARD, "overlap": ref.OVERLAP}


def load_cases():
    with open(GOLDEN) as f:
        return json.load(f)


def case_coo(case):
    """(nv, src, dst, dense) with dense ids = creation (scan) order."""
    dense = {n: i for i, n in enumerate(case["nodes"])}
    src = [dense[a] for a, _ in case["edges"]]
    dst = [dense[b] for _, b in case["edges"]]
    return len(case["nodes"]), src, dst, dense


def case_rows(case, pairs_fn, all_fn):
    """[(node1, node2, similarity)] of a value case in the reference's order."""
    nv, src, dst, dense = case_coo(case)
    metric = METRIC[case["procedure"].split("_")[0]]
    nodes = case["nodes"]
    if case["src"] is None:
        sim = all_fn(nv, src, dst, metric)
        return [(nodes[i], nodes[j], sim[ref.pair_index(nv, i, j)])
                for i in range(nv) for j in range(i + 1, nv)]
    sim = pairs_fn(nv, src, dst, [dense[x] for x in case["src"]],
                   [dense[x] for x in case["dst"]], metric)
    return list(zip(case["src"], case["dst"], sim))


def assert_rows(case, rows):
    exp = case["expected"]
    assert len(rows) == len(exp), case["name"]
    for (a, b, s), (ea, eb, es) in zip(rows, exp):
        assert (a, b) == (ea, eb), case["name"]
        assert abs(s - es) <= 1e-4, (case["name"], a, b, s, es)  # YAML rounds to 4 places


def test_fixture_inventory():
    cases = load_cases()
    assert len(cases) == 12
    values = [c for c in cases if c["expected"] is not None]
    errors = [c for c in cases if c["expected"] is None]
    assert len(values) == 10 and len(errors) == 2
    for c in errors:
        assert len(c["src"]) != len(c["dst"])
        assert c["exception_yaml"]
    for c in cases:
        if len(c["nodes"]) == 8:
            assert c["nodes"][-2:] == [6, 7]  # the isolated nodes
            assert all(6 not in e and 7 not in e for e in c["edges"])


def test_restatement_reproduces_value_fixtures():
    for case in load_cases():
        if case["expected"] is None:
            continue
        rows = case_rows(case, lambda *a: ref.pairs(*a)[0], ref.all_pairs)
        assert_rows(case, rows)


def test_length_mismatch_message():
    for case in load_cases():
        if case["expected"] is not None:
            continue
        nv, src, dst, dense = case_coo(case)
        try:
            ref.pairs(nv, src, dst, [dense[x] for x in case["src"]],
                      [dense[x] for x in case["dst"]], ref.JACCARD)
        except ValueError as e:
            assert str(e) == "The node lists must be the same length."
        else:
            raise AssertionError(case["name"])


def test_self_pair():
    # 0 -> {1, 2}; 3 has no out-edges
    for metric in (ref.JACCARD, ref.OVERLAP):
        sim, common = ref.pairs(4, [0, 0], [1, 2], [0, 3], [0, 3], metric)
        assert sim.tolist() == [1.0, 0.0]
        assert common.tolist() == [2, 0]


def test_empty_sets():
    for metric in (ref.JACCARD, ref.OVERLAP):
        # both empty; one empty (either side)
        sim, common = ref.pairs(4, [0, 0], [1, 2], [1, 1, 0], [2, 0, 3], metric)
        assert sim.tolist() == [0.0, 0.0, 0.0]
        assert common.tolist() == [0, 0, 0]


def test_self_loop_is_a_member():
    # 0 -> {0, 1}, 2 -> {0}: the self-loop puts 0 in its own set
    sim, common = ref.pairs(3, [0, 0, 2], [0, 1, 0], [0], [2], ref.JACCARD)
    assert common.tolist() == [1] and sim.tolist() == [0.5]
    sim, _ = ref.pairs(3, [0, 0, 2], [0, 1, 0], [0], [2], ref.OVERLAP)
    assert sim.tolist() == [1.0]


def test_multi_edges_count_once():
    src, dst = [0, 0, 1, 1], [2, 3, 3, 4]
    u, v = [0, 0, 1], [1, 0, 1]
    rng = np.random.default_rng(3)
    rep = rng.integers(1, 4, len(src))
    src2, dst2 = np.repeat(src, rep), np.repeat(dst, rep)
    for metric in (ref.JACCARD, ref.OVERLAP):
        a = ref.pairs(5, src, dst, u, v, metric)
        b = ref.pairs(5, src2, dst2, u, v, metric)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        assert np.array_equal(ref.all_pairs(5, src, dst, metric),
                              ref.all_pairs(5, src2, dst2, metric))
    assert ref.pairs(5, src, dst, u, v, ref.JACCARD)[0].tolist() == [1 / 3, 1.0, 1.0]


def test_all_pairs_layout():
    nv = 6
    rng = np.random.default_rng(5)
    src, dst = rng.integers(0, nv, 14), rng.integers(0, nv, 14)
    for metric in (ref.JACCARD, ref.OVERLAP):
        sim = ref.all_pairs(nv, src, dst, metric)
        assert len(sim) == nv * (nv - 1) // 2
        ii = [i for i in range(nv) for j in range(i + 1, nv)]
        jj = [j for i in range(nv) for j in range(i + 1, nv)]
        assert [ref.pair_index(nv, i, j) for i, j in zip(ii, jj)] == list(range(len(sim)))
        assert np.array_equal(sim, ref.pairs(nv, src, dst, ii, jj, metric)[0])
