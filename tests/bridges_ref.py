"""Independent restatements of bridge finding, for the CPU and GPU tests.

(a) bridges_dfs: the reference's algorithm restated (bridges.cpp:31-69): a
    low-link DFS over the undirected view that ignores the DFS parent by node
    id and keeps a candidate only when exactly one edge joins the unordered
    pair (GetEdgesBetweenNodes(from, to).size() == 1). Iterative, so a long
    path does not overflow the stack.
(b) forest_state: the level-synchronous formulation the library runs
    (memgraph_amd/csrc/bridges.hip, steps 1-7) in numpy with the same
    definitions: min-member roots, minimum-id parents one level up,
    ascending-id siblings, a global preorder, low/high over non-tree entries.
(c) bridges_bruteforce: delete one edge instance, count components.

All three return bridges as a sorted list of (u, v) with u < v.
"""
from collections import namedtuple

import numpy as np


def sym_csr(nv, src, dst):
    """Sorted symmetric CSR: every edge twice (a self-loop gives two entries)."""
    src = np.asarray(src, dtype=np.int64).reshape(-1)
    dst = np.asarray(dst, dtype=np.int64).reshape(-1)
    rows = np.concatenate([src, dst])
    cols = np.concatenate([dst, src])
    order = np.lexsort((cols, rows))
    rows, cols = rows[order], cols[order]
    rp = np.zeros(nv + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=nv), out=rp[1:])
    return rp, rows, cols


def pair_multiplicity(nv, src, dst):
    """{(min, max): number of edges joining that unordered pair}."""
    src = np.asarray(src, dtype=np.int64).reshape(-1)
    dst = np.asarray(dst, dtype=np.int64).reshape(-1)
    lo, hi = np.minimum(src, dst), np.maximum(src, dst)
    keys, counts = np.unique(lo * max(nv, 1) + hi, return_counts=True)
    return {(int(k // max(nv, 1)), int(k % max(nv, 1))): int(c) for k, c in zip(keys, counts)}


def bridges_dfs(nv, src, dst):
    rp, _, cols = sym_csr(nv, src, dst)
    rp, cols = rp.tolist(), cols.tolist()
    mult = pair_multiplicity(nv, src, dst)
    disc = [0] * nv
    low = [0] * nv
    counter = 0
    out = []
    for root in range(nv):
        if disc[root]:
            continue
        counter += 1
        disc[root] = low[root] = counter
        stack = [(root, root, rp[root])]
        while stack:
            node, par, j = stack[-1]
            if j < rp[node + 1]:
                stack[-1] = (node, par, j + 1)
                nxt = cols[j]
                if disc[nxt]:
                    if nxt != par and disc[nxt] < low[node]:
                        low[node] = disc[nxt]
                    continue
                counter += 1
                disc[nxt] = low[nxt] = counter
                stack.append((nxt, node, rp[nxt]))
            else:
                stack.pop()
                if node == root:
                    continue
                if low[node] < low[par]:
                    low[par] = low[node]
                if low[node] > disc[par]:
                    key = (min(node, par), max(node, par))
                    if mult[key] == 1:
                        out.append(key)
    return sorted(out)


def bridges_bruteforce(nv, src, dst):
    """Small graphs only: O(E^2)."""
    src = [int(x) for x in src]
    dst = [int(x) for x in dst]

    def components(skip):
        uf = list(range(nv))
        n = nv
        for i, (a, b) in enumerate(zip(src, dst)):
            if i == skip:
                continue
            while uf[a] != a:
                uf[a] = uf[uf[a]]
                a = uf[a]
            while uf[b] != b:
                uf[b] = uf[uf[b]]
                b = uf[b]
            if a != b:
                uf[a] = b
                n -= 1
        return n

    base = components(-1)
    out = set()
    for i in range(len(src)):
        if components(i) > base:
            out.add((min(src[i], dst[i]), max(src[i], dst[i])))
    return sorted(out)


ForestState = namedtuple("ForestState", "parent level pre nd low high bridges trees depth")
STATE_ARRAYS = ("parent", "level", "pre", "nd", "low", "high")


def _min_member_labels(nv, rows, cols):
    label = np.arange(nv, dtype=np.int64)
    while True:
        new = label.copy()
        np.minimum.at(new, rows, label[cols])
        while True:  # pointer jumping
            nxt = new[new]
            if np.array_equal(nxt, new):
                break
            new = nxt
        if np.array_equal(new, label):
            return label
        label = new


def _expand(rp, frontier):
    """CSR entry indices of the rows in `frontier`, and the row of each."""
    starts = rp[frontier]
    counts = rp[frontier + 1] - starts
    total = int(counts.sum())
    if total == 0:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    offs = np.cumsum(counts) - counts
    idx = np.repeat(starts - offs, counts) + np.arange(total)
    return idx, np.repeat(frontier, counts)


def forest_state(nv, src, dst):
    rp, rows, cols = sym_csr(nv, src, dst)
    ids = np.arange(nv, dtype=np.int64)
    # 1. forest: min-member roots, one multi-source BFS, minimum-id parents
    label = _min_member_labels(nv, rows, cols)
    roots = ids[label == ids]
    level = np.full(nv, -1, dtype=np.int64)
    parent = np.full(nv, np.iinfo(np.int64).max, dtype=np.int64)
    level[roots] = 0
    parent[roots] = roots
    frontier, depth = roots, 0
    levels = [roots]
    while True:
        idx, frm = _expand(rp, frontier)
        to = cols[idx]
        new = level[to] == -1
        if not new.any():
            break
        to, frm = to[new], frm[new]
        np.minimum.at(parent, to, frm)
        frontier = np.unique(to)
        depth += 1
        level[frontier] = depth
        levels.append(frontier)
    assert (level >= 0).all()
    # 2. child lists: non-roots stably sorted by parent (siblings ascending)
    nonroot = ids[parent != ids]
    child = nonroot[np.argsort(parent[nonroot], kind="stable")]
    cidx = np.zeros(nv, dtype=np.int64)
    cidx[child] = np.arange(len(child))
    child_ptr = np.searchsorted(parent[child], ids, side="left")
    # 3. subtree sizes, deepest level first
    nd = np.ones(nv, dtype=np.int64)
    for vs in levels[:0:-1]:
        np.add.at(nd, parent[vs], nd[vs])
    # 4. global preorder
    pre = np.zeros(nv, dtype=np.int64)
    pre[roots] = np.cumsum(nd[roots]) - nd[roots]
    s = np.cumsum(nd[child]) - nd[child]
    for vs in levels[1:]:
        p = parent[vs]
        pre[vs] = pre[p] + 1 + (s[cidx[vs]] - s[child_ptr[p]])
    assert np.array_equal(np.sort(pre), ids)
    # 5. local low/high: every entry but the one tree entry to the parent
    is_par = cols == parent[rows]
    npar = np.bincount(rows[is_par], minlength=nv)
    use = ~is_par | (npar[rows] >= 2)
    low, high = pre.copy(), pre.copy()
    np.minimum.at(low, rows[use], pre[cols[use]])
    np.maximum.at(high, rows[use], pre[cols[use]])
    # 6. fold bottom-up
    for vs in levels[:0:-1]:
        np.minimum.at(low, parent[vs], low[vs])
        np.maximum.at(high, parent[vs], high[vs])
    # 7. test
    is_bridge = (parent != ids) & (low >= pre) & (high < pre + nd)
    v = ids[is_bridge]
    p = parent[v]
    bridges = sorted(zip(np.minimum(p, v).tolist(), np.maximum(p, v).tolist()))
    return ForestState(parent, level, pre, nd, low, high, bridges, len(roots), depth)


def random_multigraphs(n=300, seed=20):
    """(nv, src, dst) with V in 2..40 and E <= 2V; self-loops, duplicate and
    antiparallel edges injected. Seeded: the CPU and the GPU tests see the
    same graphs."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        nv = int(rng.integers(2, 41))
        ne = int(rng.integers(0, nv + nv // 2 + 1))
        src = rng.integers(0, nv, ne).tolist()
        dst = rng.integers(0, nv, ne).tolist()
        for _ in range(int(rng.integers(0, 4))):
            if len(src) >= 2 * nv:
                break
            kind = int(rng.integers(0, 3))
            if kind == 0 or not src:
                x = int(rng.integers(0, nv))
                src.append(x)
                dst.append(x)
            else:
                i = int(rng.integers(0, len(src)))
                a, b = (src[i], dst[i]) if kind == 1 else (dst[i], src[i])
                src.append(a)
                dst.append(b)
        assert len(src) <= 2 * nv
        out.append((nv, src, dst))
    return out
