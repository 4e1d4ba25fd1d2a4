#!/usr/bin/env python3
"""Generate tests/golden/neighbors_e2e.json from the reference's own
neighbors e2e cases (tests/mage/e2e/neighbors_test/*/{input.cyp,test.yml}).

Run where the reference checkout exists (pass its root as argv[1], default
/root/reference); the JSON output is committed so no test reads the
reference. Data only: node names, (from, to, type) edges, the call's
arguments and the expected set of names per result row.

Every case is cross-checked at generation time: tests/bfs_ref.py on the COO
derived by the reference's direction rule reproduces the expected rows.
"""
import json
import os
import re
import sys

import yaml

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
from bfs_ref import bfs_ref, neighbors_coo, neighbors_expected_rows  # noqa: E402

EDGE_RE = re.compile(r"MERGE \(a:(\w+)\) MERGE \(b:(\w+)\) CREATE \(a\)-\[\w*:(\w+)\]->\(b\)")
CALL_RE = re.compile(r"MATCH \(\w+:(\w+)\)\s+CALL neighbors\.(\w+)\(\w+,\s*\[([^\]]*)\],\s*(\d+)\)")


def row_names(value):
    nodes = value if isinstance(value, list) else [value]
    return sorted(n["labels"][0] for n in nodes)


def main():
    root = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    suite = os.path.join(root, "tests", "mage", "e2e", "neighbors_test")
    cases = []
    for name in sorted(os.listdir(suite)):
        d = os.path.join(suite, name)
        if not os.path.isdir(d):
            continue
        nodes, edges = [], []
        with open(os.path.join(d, "input.cyp")) as f:
            for m in EDGE_RE.finditer(f.read()):
                a, b, t = m.groups()
                for n in (a, b):  # creation order
                    if n not in nodes:
                        nodes.append(n)
                edges.append([a, b, t])
        with open(os.path.join(d, "test.yml")) as f:
            spec = yaml.safe_load(f)
        m = CALL_RE.search(spec["query"])
        source, proc, raw_types, distance = m.groups()
        rel_types = [t.strip().strip("\"'") for t in raw_types.split(",")]
        if not raw_types.strip():
            rel_types = []
        case = {
            "name": f"neighbors_test/{name}",
            "nodes": nodes,
            "edges": edges,
            "source": source,
            "rel_types": rel_types,
            "distance": int(distance),
            "procedure": proc,
            "expected": [row_names(row["nodes"]) for row in (spec.get("output") or [])],
            "origin": f"tests/mage/e2e/neighbors_test/{name}",
        }
        nv, src, dst, s = neighbors_coo(case)
        got = neighbors_expected_rows(case, bfs_ref(nv, src, dst, s, directed=True,
                                                    max_depth=case["distance"]).hops)
        exp = [set(r) for r in case["expected"]]
        if proc == "by_hop":
            assert got == exp, (name, got, exp)
        else:  # at_hop rows are unordered
            assert sorted(map(sorted, got)) == sorted(map(sorted, exp)), (name, got, exp)
        cases.append(case)
        print(f"ok {case['name']}: V={nv} rows={len(exp)}")
    assert len(cases) == 7, len(cases)
    with open(os.path.join(HERE, "neighbors_e2e.json"), "w") as f:
        json.dump(cases, f, indent=1)
    print(f"wrote {len(cases)} neighbors fixtures")


if __name__ == "__main__":
    main()
