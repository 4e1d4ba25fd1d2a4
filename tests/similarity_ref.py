"""Plain-Python restatement of the reference's node similarity
(src/mage/cpp/node_similarity_module/algorithms/node_similarity.hpp), with
sets. TEST INFRASTRUCTURE: the expected value of every similarity test.

  neighbor_sets   GetNeighbors, :107-121: the set of `to` ids of a node's
                  out-relationships (a std::set, so multi-edges count once
                  and a self-loop puts the node in its own set).
  jaccard         JaccardFunc, :43-52: |A & B| / (double)|A | B|, 0.0 when
                  the union is empty.
  overlap         OverlapFunc, :59-68: |A & B| / min(|A|, |B|), 0.0 when
                  that minimum is 0.
  pairs           CalculateSimilarityPairwise, :126-158: list order.
  all_pairs       CalculateSimilarityCartesian, :163-200: node1 over the
                  scan, node2 over the scan, a pair skipped when node1 ==
                  node2 or (node2, node1) was already emitted, so for
                  scan-order ids 0..V-1 it is row-major i < j and pair (i, j)
                  sits at i*(2V-i-1)/2 + (j-i-1).
The quotient is one IEEE double division of two integers, which Python's
int / int also is (correctly rounded), so values are bit-identical.
"""
import numpy as np

JACCARD = 0
OVERLAP = 1


def neighbor_sets(nv, src, dst):
    sets = [set() for _ in range(nv)]
    for s, d in zip(np.asarray(src).tolist(), np.asarray(dst).tolist()):
        sets[s].add(d)  # :117-119
    return sets


def jaccard(a, b):
    union = len(a | b)  # :47
    if union == 0:  # :48-50
        return 0.0
    return len(a & b) / union  # :51


def overlap(a, b):
    denominator = min(len(a), len(b))  # :63
    if denominator == 0:  # :64-66 (an integer below 1e-9 is 0)
        return 0.0
    return len(a & b) / denominator  # :67


def similarity(a, b, metric):
    if metric == JACCARD:
        return jaccard(a, b)
    if metric == OVERLAP:
        return overlap(a, b)
    raise ValueError(metric)


def pairs_from_sets(sets, u, v, metric):
    sim = np.zeros(len(u), dtype=np.float64)
    common = np.zeros(len(u), dtype=np.int64)
    for k, (a, b) in enumerate(zip(np.asarray(u).tolist(), np.asarray(v).tolist())):
        sim[k] = similarity(sets[a], sets[b], metric)  # :143-155
        common[k] = len(sets[a] & sets[b])
    return sim, common


def pairs(nv, src, dst, u, v, metric):
    """(sim, common) for the listed pairs, in list order."""
    if len(u) != len(v):
        raise ValueError("The node lists must be the same length.")  # :129-131
    return pairs_from_sets(neighbor_sets(nv, src, dst), u, v, metric)


def pair_index(nv, i, j):
    return i * (2 * nv - i - 1) // 2 + (j - i - 1)


def all_pairs(nv, src, dst, metric):
    """sim[V(V-1)/2], zeros included, row-major i < j (:168-198)."""
    sets = neighbor_sets(nv, src, dst)
    out = np.zeros(nv * (nv - 1) // 2, dtype=np.float64)
    k = 0
    for i in range(nv):
        for j in range(i + 1, nv):
            out[k] = similarity(sets[i], sets[j], metric)
            k += 1
    return out
