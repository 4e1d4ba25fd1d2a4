#!/usr/bin/env python3
"""Generate tests/golden/node_similarity_e2e.json from the reference's own
node_similarity e2e cases
(tests/mage/e2e/node_similarity_test/*/{input.cyp,test.yml}) whose query
calls jaccard* or overlap* (the cosine cases need node properties and are out
of scope).

Run where the reference checkout exists (pass its root as argv[1], default
/root/reference); the JSON output is committed so no test reads the
reference. Data only: node ids in creation order (the isolated nodes 6 and 7
included), (from, to) edges, the procedure, the two id lists of a pairwise
call and the expected rows or the expected exception text.

The YAML's exception text ("Incompatible lengths of given arguments") is an
older wording than the source's (node_similarity.hpp:129-131: "The node lists
must be the same length."); it is recorded as data, the tests assert the
source's message.

Every value case is cross-checked at generation time against
tests/similarity_ref.py. The YAML values are rounded to four places, so that
comparison (and the tests' comparison with these goldens) is at 1e-4 absolute.
"""
import json
import os
import re
import sys

import yaml

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
import similarity_ref  # noqa: E402

EDGE_RE = re.compile(r"MERGE \(a:Node \{id: (\d+)\}\) MERGE \(b:Node \{id: (\d+)\}\) "
                     r"CREATE \(a\)-\[:\w+\]->\(b\)")
NODE_RE = re.compile(r"^CREATE \(\w+:Node \{id: (\d+)\}\);", re.M)
# MATCH (m {id: K}) | MATCH (m) WHERE m.id = K | MATCH (m) WHERE m.id < K
MATCH_RE = re.compile(r"MATCH \((\w+)(?: \{id: (\d+)\})?\)(?:\s+WHERE \1\.id (=|<) (\d+))?"
                      r"\s+WITH collect\(\1\) as (\w+)")
CALL_RE = re.compile(r"CALL node_similarity\.(\w+)\(([^)]*)\)")
METRIC = {"jaccard": similarity_ref.JACCARD, "overlap": similarity_ref.OVERLAP}


def parse_graph(text):
    nodes, edges = [], []
    for line in text.splitlines():
        m = EDGE_RE.search(line)
        if m:
            a, b = int(m.group(1)), int(m.group(2))
            for n in (a, b):  # MERGE creates in this order
                if n not in nodes:
                    nodes.append(n)
            edges.append([a, b])
            continue
        m = NODE_RE.search(line)
        if m and int(m.group(1)) not in nodes:
            nodes.append(int(m.group(1)))
    return nodes, edges


def parse_lists(query, nodes):
    lists = {}
    for _var, prop_id, op, k, name in MATCH_RE.findall(query):
        if prop_id:
            lists[name] = [n for n in nodes if n == int(prop_id)]
        elif op == "=":
            lists[name] = [n for n in nodes if n == int(k)]
        elif op == "<":
            lists[name] = [n for n in nodes if n < int(k)]
        else:
            lists[name] = list(nodes)
    return lists


def main():
    root = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    suite = os.path.join(root, "tests", "mage", "e2e", "node_similarity_test")
    cases = []
    for name in sorted(os.listdir(suite)):
        d = os.path.join(suite, name)
        if not os.path.isdir(d):
            continue
        with open(os.path.join(d, "test.yml")) as f:
            spec = yaml.safe_load(f)
        m = CALL_RE.search(spec["query"])
        proc = m.group(1)
        if proc.split("_")[0] not in METRIC:
            continue
        with open(os.path.join(d, "input.cyp")) as f:
            nodes, edges = parse_graph(f.read())
        src = dst = None
        if proc.endswith("_pairwise"):
            lists = parse_lists(spec["query"], nodes)
            a, b = [x.strip() for x in m.group(2).split(",")]
            src, dst = lists[a], lists[b]
        expected = None
        if "output" in spec:
            expected = [[r["node1"], r["node2"], float(r["similarity"])]
                        for r in spec["output"]]
        case = {
            "name": f"node_similarity_test/{name}",
            "nodes": nodes,
            "edges": edges,
            "procedure": proc,
            "src": src,
            "dst": dst,
            "expected": expected,
            "exception_yaml": spec["exception"].strip() if "exception" in spec else None,
            "origin": f"tests/mage/e2e/node_similarity_test/{name}",
        }
        if expected is not None:
            dense = {n: i for i, n in enumerate(nodes)}
            nv = len(nodes)
            s = [dense[a] for a, _ in edges]
            t = [dense[b] for _, b in edges]
            metric = METRIC[proc.split("_")[0]]
            if src is None:
                sim = similarity_ref.all_pairs(nv, s, t, metric)
                got = [[nodes[i], nodes[j], sim[similarity_ref.pair_index(nv, i, j)]]
                       for i in range(nv) for j in range(i + 1, nv)]
            else:
                sim, _ = similarity_ref.pairs(nv, s, t, [dense[x] for x in src],
                                              [dense[x] for x in dst], metric)
                got = [[a, b, v] for a, b, v in zip(src, dst, sim)]
            assert len(got) == len(expected), (name, got, expected)
            for g, e in zip(got, expected):
                assert g[:2] == e[:2] and abs(g[2] - e[2]) <= 1e-4, (name, g, e)
        else:
            assert len(src) != len(dst), (name, src, dst)
        cases.append(case)
        print(f"ok {case['name']}: V={len(nodes)} E={len(edges)} {proc}")
    n_values = sum(c["expected"] is not None for c in cases)
    assert len(cases) == 12 and n_values == 10, (len(cases), n_values)
    with open(os.path.join(HERE, "node_similarity_e2e.json"), "w") as f:
        json.dump(cases, f, indent=1)
    print(f"wrote {len(cases)} node_similarity fixtures")


if __name__ == "__main__":
    main()
