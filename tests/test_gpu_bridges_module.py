"""The drop-in bridges.so against the mgp host mock: the registered signature,
the reference's three e2e cases, row orientation and scan-order rows, and the
graphs that give no rows."""
import os
import sys

import pytest

import bridges_ref as ref
from test_bridges_cpu import case_coo, load_cases

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "mock"))
from harness import ModuleHost  # noqa: E402

pytestmark = pytest.mark.gpu


def mg_id(fixture_id):
    """Non-contiguous memgraph ids, nothing like the dense scan ids."""
    return 7 * fixture_id + 1000


def call_rows(h):
    return [(h.row_int(i, "node_from"), h.row_int(i, "node_to")) for i in h.call("get")]


def scan_order_rows(ids, src, dst):
    """The bridge edges as (from, to) memgraph ids in edge scan order: vertices
    in creation order, each one's out-edges in creation order."""
    bridges = set(ref.bridges_dfs(len(ids), src, dst))
    edges = sorted(range(len(src)), key=lambda e: (src[e], e))
    return [(ids[src[e]], ids[dst[e]]) for e in edges
            if (min(src[e], dst[e]), max(src[e], dst[e])) in bridges]


def test_registered_signature():
    h = ModuleHost("bridges")
    assert h.procedures() == {"get": {"args": [],
                                      "results": [("node_from", "node"), ("node_to", "node")]}}


def test_reference_e2e_cases():
    h = ModuleHost("bridges")
    cases = [c for c in load_cases() if c["kind"] == "e2e"]
    assert len(cases) == 3
    for case in cases:
        nv, src, dst, _ = case_coo(case)
        ids = [mg_id(n) for n in case["nodes"]]
        h.load_graph(ids, src, dst)
        rows = call_rows(h)
        assert rows == scan_order_rows(ids, src, dst), case["name"]
        # the YAML's rows, which the reference's query puts in ORDER BY from_id, to_id
        back = {mg_id(n): n for n in case["nodes"]}
        assert sorted((back[a], back[b]) for a, b in rows) == \
            [tuple(r) for r in case["expected"]], case["name"]


def test_unit_cases_row_sets():
    h = ModuleHost("bridges")
    for case in [c for c in load_cases() if c["kind"] == "unit"]:
        nv, src, dst, _ = case_coo(case)
        ids = [mg_id(n) for n in case["nodes"]]
        h.load_graph(ids, src, dst)
        assert call_rows(h) == scan_order_rows(ids, src, dst), case["name"]


def test_orientation_and_scan_order():
    h = ModuleHost("bridges")
    # scan order is creation order, not id order
    ids = [50, 7, 31, 2, 90, 11, 64, 23]
    # bridges stored "backwards" (from a later vertex to an earlier one): 4->0, 5->4, 6->3;
    # a triangle 1-2-3 hanging off 0 by the forward bridge 0->1; an antiparallel 5<->7 pair
    src = [4, 5, 6, 0, 1, 2, 3, 5, 7]
    dst = [0, 4, 3, 1, 2, 3, 1, 7, 5]
    h.load_graph(ids, src, dst)
    rows = call_rows(h)
    assert rows == [(50, 7), (90, 50), (11, 90), (64, 2)]
    assert rows == scan_order_rows(ids, src, dst)
    # one more scan order of the same graph: the rows follow it
    perm = [3, 6, 0, 5, 1, 4, 2, 7]  # new dense id of old dense id
    ids2 = [0] * 8
    for old, new in enumerate(perm):
        ids2[new] = ids[old]
    src2, dst2 = [perm[x] for x in src], [perm[x] for x in dst]
    h.load_graph(ids2, src2, dst2)
    rows2 = call_rows(h)
    assert sorted(rows2) == sorted(rows)
    assert rows2 == scan_order_rows(ids2, src2, dst2) and rows2 != rows


def test_no_rows():
    h = ModuleHost("bridges")
    for ids, src, dst in (([], [], []), ([4], [], []), ([4], [0], [0]),
                          ([4, 9], [0, 1], [1, 0]), ([4, 9, 5], [], [])):
        h.load_graph(ids, src, dst)
        assert h.call("get") == []
