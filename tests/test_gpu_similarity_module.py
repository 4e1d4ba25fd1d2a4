"""The drop-in node_similarity.so against the mgp host mock: registered
signatures, the reference's twelve jaccard / overlap e2e cases, row order,
the length-mismatch message, and that cosine is not offered."""
import os
import sys

import pytest

import similarity_ref as ref
from test_similarity_cpu import METRIC, assert_rows, case_coo, load_cases

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "mock"))
from harness import ModuleHost  # noqa: E402

pytestmark = pytest.mark.gpu


def mg_id(fixture_id):
    """Non-contiguous memgraph ids, nothing like the dense scan ids."""
    return 10 * fixture_id + 3


def load_case(h, case):
    nv, src, dst, _ = case_coo(case)
    h.load_graph([mg_id(n) for n in case["nodes"]], src, dst)
    if case["src"] is not None:
        h.override_arg_node_list(0, [mg_id(n) for n in case["src"]])
        h.override_arg_node_list(1, [mg_id(n) for n in case["dst"]])


def call_rows(h, proc):
    return [(h.row_int(i, "node1"), h.row_int(i, "node2"), h.row_double(i, "similarity"))
            for i in h.call(proc)]


def test_registered_signatures():
    h = ModuleHost("node_similarity")
    procs = h.procedures()
    assert list(procs) == ["jaccard", "jaccard_pairwise", "overlap", "overlap_pairwise"]
    results = [("node1", "node"), ("node2", "node"), ("similarity", "float")]
    for name in ("jaccard", "overlap"):
        assert procs[name] == {"args": [], "results": results}
    for name in ("jaccard_pairwise", "overlap_pairwise"):
        assert procs[name] == {"args": [("src_nodes", "list"), ("dst_nodes", "list")],
                               "results": results}


def test_reference_e2e_cases():
    h = ModuleHost("node_similarity")
    cases = load_cases()
    assert len(cases) == 12
    n_values = n_errors = 0
    for case in cases:
        load_case(h, case)
        if case["expected"] is None:
            with pytest.raises(RuntimeError) as e:
                h.call(case["procedure"])
            # node_similarity.hpp:129-131; the e2e YAML keeps an older wording
            assert str(e.value) == "procedure error: The node lists must be the same length."
            assert case["exception_yaml"] != "The node lists must be the same length."
            n_errors += 1
            continue
        rows = call_rows(h, case["procedure"])
        back = {mg_id(n): n for n in case["nodes"]}
        rows = [(back[a], back[b], s) for a, b, s in rows]
        assert_rows(case, rows)
        # exactly the restatement
        nv, src, dst, dense = case_coo(case)
        metric = METRIC[case["procedure"].split("_")[0]]
        if case["src"] is None:
            exp = ref.all_pairs(nv, src, dst, metric).tolist()
        else:
            exp = ref.pairs(nv, src, dst, [dense[x] for x in case["src"]],
                            [dense[x] for x in case["dst"]], metric)[0].tolist()
        assert [s for _, _, s in rows] == exp, case["name"]
        n_values += 1
    assert (n_values, n_errors) == (10, 2)


def test_all_pairs_row_order_and_count():
    h = ModuleHost("node_similarity")
    # scan order is creation order, not id order: 50, 7, 31, 2, 90, 11
    ids = [50, 7, 31, 2, 90, 11]
    src = [0, 0, 1, 1, 2, 3, 3, 3, 5, 5, 0]
    dst = [1, 2, 2, 3, 0, 0, 1, 3, 2, 2, 1]  # a self-loop (3, 3), multi-edges (5, 2), (0, 1)
    nv = len(ids)
    for proc, metric in (("jaccard", ref.JACCARD), ("overlap", ref.OVERLAP)):
        h.load_graph(ids, src, dst)
        rows = call_rows(h, proc)
        assert len(rows) == nv * (nv - 1) // 2
        assert [(a, b) for a, b, _ in rows] == [(ids[i], ids[j]) for i in range(nv)
                                                for j in range(i + 1, nv)]
        assert [s for _, _, s in rows] == ref.all_pairs(nv, src, dst, metric).tolist()
        assert any(s > 0 for _, _, s in rows) and any(s == 0 for _, _, s in rows)


def test_pairwise_list_order_and_repeats():
    h = ModuleHost("node_similarity")
    ids = [50, 7, 31, 2]
    src, dst = [0, 0, 1, 1, 2], [1, 2, 2, 3, 2]
    u, v = [3, 0, 0, 1, 2, 0], [0, 1, 0, 0, 2, 1]  # self pairs, a repeat, an empty row
    for proc, metric in (("jaccard_pairwise", ref.JACCARD), ("overlap_pairwise", ref.OVERLAP)):
        h.load_graph(ids, src, dst)
        h.override_arg_node_list(0, [ids[x] for x in u])
        h.override_arg_node_list(1, [ids[x] for x in v])
        rows = call_rows(h, proc)
        assert [(a, b) for a, b, _ in rows] == [(ids[a], ids[b]) for a, b in zip(u, v)]
        assert [s for _, _, s in rows] == ref.pairs(4, src, dst, u, v, metric)[0].tolist()
        h.load_graph(ids, src, dst)
        h.override_arg_node_list(0, [])
        h.override_arg_node_list(1, [])
        assert h.call(proc) == []


def test_fewer_than_two_nodes_gives_no_rows():
    h = ModuleHost("node_similarity")
    for ids, src, dst in (([], [], []), ([4], [], []), ([4], [0], [0])):
        for proc in ("jaccard", "overlap"):
            h.load_graph(ids, src, dst)
            assert h.call(proc) == []


def test_too_many_nodes_for_all_pairs_is_an_error_message():
    h = ModuleHost("node_similarity")
    nv = 65537  # V(V-1)/2 = 2^31 + 32768 rows
    ids = list(range(100, 100 + nv))
    for proc in ("jaccard", "overlap"):
        h.load_graph(ids, [0, 1], [1, 2])
        with pytest.raises(RuntimeError, match="too large"):
            h.call(proc)
    # the pairwise procedures have no such limit
    h.load_graph(ids, [0, 1], [1, 1])
    h.override_arg_node_list(0, [ids[0], ids[nv - 1]])
    h.override_arg_node_list(1, [ids[1], ids[0]])
    assert call_rows(h, "jaccard_pairwise") == [(ids[0], ids[1], 1.0),
                                                (ids[nv - 1], ids[0], 0.0)]


def test_length_mismatch_message():
    h = ModuleHost("node_similarity")
    for proc in ("jaccard_pairwise", "overlap_pairwise"):
        h.load_graph([1, 2, 3], [0, 1], [1, 2])
        h.override_arg_node_list(0, [1, 2])
        h.override_arg_node_list(1, [1, 2, 3])
        with pytest.raises(RuntimeError, match="The node lists must be the same length\\.$"):
            h.call(proc)


def test_cosine_is_not_registered():
    h = ModuleHost("node_similarity")
    h.load_graph([1, 2], [0], [1])
    for proc in ("cosine", "cosine_pairwise"):
        assert proc not in h.procedures()
        with pytest.raises(AssertionError, match="not found"):
            h.call(proc)
