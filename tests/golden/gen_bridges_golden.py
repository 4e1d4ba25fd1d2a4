#!/usr/bin/env python3
"""Generate tests/golden/bridges_e2e.json from the reference's own bridges
tests: the three e2e cases (tests/mage/e2e/bridges_test/*/{input.cyp,test.yml})
and, as data only, the graph / expected-pair vectors of the unit tests in
src/mage/cpp/bridges_module/bridges_test.cpp (SmallTree,
HandmadeConnectedGraph1/2, HandmadeDisconnectedGraph, SimpleNeighborCycle,
NeighborCycle and the 100-cycle).

Run where the reference checkout exists (pass its root as argv[1]); the JSON
output is committed so no test reads the reference. Data only: node ids in
creation order, (from, to) edges in creation order, and the expected rows.
For an e2e case the expected rows are (from_id, to_id) in the edge's own
direction, as the YAML lists them (ORDER BY from_id, to_id); for a unit case
they are the unordered pairs its CheckBridges / ASSERT_EQ pins.

Every case is cross-checked at generation time against
tests/bridges_ref.py::bridges_dfs.
"""
import json
import os
import re
import sys

import yaml

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
import bridges_ref  # noqa: E402

EDGE_RE = re.compile(r"MERGE \(a:Node \{id: (\d+)\}\) MERGE \(b:Node \{id: (\d+)\}\) "
                     r"CREATE \(a\)-\[:\w+\]->\(b\)")
TEST_RE = re.compile(r"TEST\(Bridges, (\w+)\) \{(.*?)\n\}", re.S)
BUILD_RE = re.compile(r"BuildGraph\(\s*(\d+),\s*\{(.*?)\}\);", re.S)
CHECK_RE = re.compile(r"CheckBridges\(\s*bridges,\s*\{(.*?)\}\)\);", re.S)
PAIR_RE = re.compile(r"\{(\d+),\s*(\d+)\}")
UNIT = ("SmallTree", "HandmadeConnectedGraph1", "HandmadeConnectedGraph2",
        "HandmadeDisconnectedGraph", "SimpleNeighborCycle", "NeighborCycle", "Cycle")


def pairs_of(text):
    return [[int(a), int(b)] for a, b in PAIR_RE.findall(text)]


def unordered(rows):
    return sorted((min(a, b), max(a, b)) for a, b in rows)


def e2e_cases(root):
    suite = os.path.join(root, "tests", "mage", "e2e", "bridges_test")
    for name in sorted(os.listdir(suite)):
        d = os.path.join(suite, name)
        if not os.path.isdir(d):
            continue
        nodes, edges = [], []
        with open(os.path.join(d, "input.cyp")) as f:
            for line in f:
                m = EDGE_RE.search(line)
                if not m:
                    continue
                a, b = int(m.group(1)), int(m.group(2))
                for n in (a, b):  # MERGE creates in this order
                    if n not in nodes:
                        nodes.append(n)
                edges.append([a, b])
        with open(os.path.join(d, "test.yml")) as f:
            spec = yaml.safe_load(f)
        assert "bridges.get()" in spec["query"] and "ORDER BY from_id, to_id" in spec["query"]
        yield {"name": f"bridges_test/{name}", "kind": "e2e", "nodes": nodes, "edges": edges,
               "expected": [[r["from_id"], r["to_id"]] for r in spec["output"]],
               "origin": f"tests/mage/e2e/bridges_test/{name}"}


def unit_cases(root):
    path = os.path.join(root, "src", "mage", "cpp", "bridges_module", "bridges_test.cpp")
    with open(path) as f:
        bodies = dict(TEST_RE.findall(f.read()))
    for name in UNIT:
        body = bodies[name]
        if name == "Cycle":  # built by a loop: i -> (i + 1) % n, no bridges
            n = int(re.search(r"n = (\d+);", body).group(1))
            assert "(i + 1) % n" in body and "CheckBridges(bridges, {})" in body
            nv, edges, expected = n, [[i, (i + 1) % n] for i in range(n)], []
        else:
            m = BUILD_RE.search(body)
            nv, edges = int(m.group(1)), pairs_of(m.group(2))
            c = CHECK_RE.search(body)
            if c:
                expected = pairs_of(c.group(1))
            else:  # ASSERT_EQ on the count, and on the one bridge's edge id
                count = int(re.search(r"ASSERT_EQ\((\d+), bridges\.size\(\)\)", body).group(1))
                ids = [int(x) for x in re.findall(r"ASSERT_EQ\(bridges\[\d+\]\.id, (\d+)\)", body)]
                assert len(ids) == count
                expected = [edges[i] for i in ids]
        yield {"name": f"bridges_test.cpp/{name}", "kind": "unit", "nodes": list(range(nv)),
               "edges": edges, "expected": expected,
               "origin": f"src/mage/cpp/bridges_module/bridges_test.cpp TEST(Bridges, {name})"}


def main():
    root = sys.argv[1]
    cases = list(e2e_cases(root)) + list(unit_cases(root))
    for case in cases:
        dense = {n: i for i, n in enumerate(case["nodes"])}
        src = [dense[a] for a, _ in case["edges"]]
        dst = [dense[b] for _, b in case["edges"]]
        got = bridges_ref.bridges_dfs(len(dense), src, dst)
        exp = unordered((dense[a], dense[b]) for a, b in case["expected"])
        assert got == exp, (case["name"], got, exp)
        if case["kind"] == "e2e":  # the rows are edges in their own direction
            assert all(r in case["edges"] for r in case["expected"]), case["name"]
        print(f"ok {case['name']}: V={len(dense)} E={len(src)} bridges={len(exp)}")
    assert len(cases) == 10
    with open(os.path.join(HERE, "bridges_e2e.json"), "w") as f:
        json.dump(cases, f, indent=1)
    print(f"wrote {len(cases)} bridges fixtures")


if __name__ == "__main__":
    main()
