"""CPU side of the BFS feature: pins tests/bfs_ref.py (the checker the GPU
tests compare against) to the reference's neighbors.at_hop / by_hop level
sets, and checks that the library and the binding expose mgx_bfs."""
import ctypes
import json
import os

import numpy as np
import pytest

from bfs_ref import bfs_ref, neighbors_coo, neighbors_expected_rows
from memgraph_amd import native

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "neighbors_e2e.json")

with open(GOLDEN) as _f:
    CASES = json.load(_f)


def test_fixture_has_the_seven_reference_cases():
    assert len(CASES) == 7
    assert sorted(c["procedure"] for c in CASES) == ["at_hop"] * 4 + ["by_hop"] * 3


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_bfs_ref_reproduces_reference_level_sets(case):
    nv, src, dst, source = neighbors_coo(case)
    ref = bfs_ref(nv, src, dst, source, directed=True, max_depth=case["distance"])
    got = neighbors_expected_rows(case, ref.hops)
    exp = [set(r) for r in case["expected"]]
    if case["procedure"] == "by_hop":
        assert len(got) == case["distance"]  # empty rows included
        assert got == exp
    else:
        assert sorted(map(sorted, got)) == sorted(map(sorted, exp))
    assert ref.hops[source] == 0 and ref.parent[source] == source
    assert ref.hops.max() <= case["distance"]


def test_bfs_ref_parents_scanned_and_depth_limit():
    # 0-1, 0-2, 1-3, 2-3, 3-4 undirected; 5 isolated.
    src, dst = [0, 0, 1, 2, 3], [1, 2, 3, 3, 4]
    r = bfs_ref(6, src, dst, 0)
    assert r.hops.tolist() == [0, 1, 1, 2, 3, -1]
    assert r.parent.tolist() == [0, 0, 0, 1, 3, -1]  # 3's parents are {1, 2}: min id
    assert r.frontier_sizes == [1, 2, 1, 1]
    assert (r.depth, r.reached) == (3, 5)
    assert r.entries_scanned == 2 + (2 + 2) + 3 + 1  # every expanded frontier's degrees
    r1 = bfs_ref(6, src, dst, 0, max_depth=1)
    assert r1.hops.tolist() == [0, 1, 1, -1, -1, -1]
    assert (r1.depth, r1.entries_scanned) == (1, 2)
    rd = bfs_ref(6, src, dst, 3, directed=True)
    assert rd.hops.tolist() == [-1, -1, -1, 0, 1, -1]


def test_library_exports_mgx_bfs():
    assert os.path.exists(native.LIB_PATH), "build first (__graft_entry__.build())"
    lib = ctypes.CDLL(native.LIB_PATH)
    assert hasattr(lib, "mgx_bfs")


def test_binding_exposes_bfs():
    assert hasattr(native.Native, "bfs")
    assert (native.BFS_AUTO, native.BFS_TOP_DOWN, native.BFS_BOTTOM_UP) == (0, 1, 2)
    assert ctypes.sizeof(native.BfsStats) == 56
    assert [n for n, _ in native.BfsStats._fields_] == [
        "depth", "reached", "entries_scanned", "top_down_levels", "bottom_up_levels",
        "bottom_up_mask", "ms"]


def test_level_sets_are_a_partition_of_reached():
    rng = np.random.default_rng(5)
    src, dst = rng.integers(0, 200, 500), rng.integers(0, 200, 500)
    r = bfs_ref(200, src, dst, 7)
    assert sum(r.frontier_sizes) == r.reached
    assert [int((r.hops == l).sum()) for l in range(r.depth + 1)] == r.frontier_sizes
