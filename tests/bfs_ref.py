"""Plain numpy level-synchronous BFS over a COO: the checker for mgx_bfs.

Pinned to the reference's neighbors.at_hop / neighbors.by_hop level sets by
tests/test_bfs_cpu.py (fixture tests/golden/neighbors_e2e.json).
"""
from collections import namedtuple

import numpy as np

BfsRef = namedtuple("BfsRef", "hops parent frontier_sizes entries_scanned depth reached")


def adjacency(n_vertices, src, dst, directed):
    """CSR (row_ptr, col) of the traversal: from->to when directed, else every
    input edge twice (a self-loop gives two entries), as the symmetric CSR."""
    src = np.asarray(src, dtype=np.int64).reshape(-1)
    dst = np.asarray(dst, dtype=np.int64).reshape(-1)
    if not directed:
        src, dst = np.concatenate([src, dst]), np.concatenate([dst, src])
    order = np.lexsort((dst, src))
    src, dst = src[order], dst[order]
    row_ptr = np.zeros(n_vertices + 1, dtype=np.int64)
    np.add.at(row_ptr, src + 1, 1)
    return np.cumsum(row_ptr), dst


def bfs_ref(n_vertices, src, dst, source, directed=False, max_depth=-1):
    """hops (-1 = unreached or beyond max_depth), minimum-id parents
    (parent[source] = source, -1 where hops is -1), frontier size per level,
    and the CSR entries a top-down BFS examines: the degree sum of every
    frontier it expands (a frontier is expanded when it is non-empty and its
    level is below max_depth; the last one is expanded to learn it is last)."""
    row_ptr, col = adjacency(n_vertices, src, dst, directed)
    deg = np.diff(row_ptr)
    hops = np.full(n_vertices, -1, dtype=np.int64)
    parent = np.full(n_vertices, -1, dtype=np.int64)
    hops[source] = 0
    parent[source] = source
    frontier = np.array([source], dtype=np.int64)
    sizes = [1]
    scanned = 0
    level = 0
    while frontier.size and (max_depth < 0 or level < max_depth):
        scanned += int(deg[frontier].sum())
        # all (u, w) entries out of the frontier
        counts = deg[frontier]
        u = np.repeat(frontier, counts)
        starts = np.repeat(row_ptr[frontier], counts)
        within = np.arange(u.size, dtype=np.int64) - np.repeat(np.cumsum(counts) - counts, counts)
        w = col[starts + within]
        new = hops[w] < 0
        u, w = u[new], w[new]
        if w.size == 0:
            break
        best = np.full(n_vertices, np.iinfo(np.int64).max, dtype=np.int64)
        np.minimum.at(best, w, u)
        frontier = np.unique(w)
        hops[frontier] = level + 1
        parent[frontier] = best[frontier]
        sizes.append(int(frontier.size))
        level += 1
    return BfsRef(hops, parent, sizes, scanned, len(sizes) - 1, int((hops >= 0).sum()))


def level_sets(hops, max_level):
    """[{v : hops[v] == l} for l in 1..max_level]."""
    return [set(np.flatnonzero(hops == l).tolist()) for l in range(1, max_level + 1)]


def neighbors_coo(case):
    """Traversal COO of a neighbors_e2e.json case, by the reference's rule
    (neighbors.cpp:26-48): 'T>' follows from->to, '<T' follows to->from, a
    bare 'T' both, an empty list (or the empty type) all types both ways."""
    names = case["nodes"]
    idx = {n: i for i, n in enumerate(names)}
    rel_types = case["rel_types"] or [""]
    in_rels, out_rels = set(), set()
    for t in rel_types:
        if t.startswith("<"):
            in_rels.add(t[1:])
        elif t.endswith(">"):
            out_rels.add(t[:-1])
        else:
            in_rels.add(t)
            out_rels.add(t)
    src, dst = [], []
    for a, b, t in case["edges"]:
        if "" in out_rels or t in out_rels:
            src.append(idx[a])
            dst.append(idx[b])
        if "" in in_rels or t in in_rels:
            src.append(idx[b])
            dst.append(idx[a])
    return len(names), src, dst, idx[case["source"]]


def neighbors_expected_rows(case, hops):
    """Rows the reference procedure yields, as sets of names, from hops."""
    names = case["nodes"]
    d = case["distance"]
    sets = [{names[v] for v in s} for s in level_sets(hops, d)]
    if case["procedure"] == "by_hop":
        return sets  # exactly `distance` rows, empty ones included
    # at_hop: one row per node at level `distance`; nothing if a level before
    # it is empty (neighbors.cpp:89-91).
    return [{n} for n in sorted(sets[-1])] if d >= 1 and all(sets) else []
