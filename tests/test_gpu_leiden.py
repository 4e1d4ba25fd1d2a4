"""GPU tests for leiden_community_detection.

The reference leiden is randomized (random_device-seeded shuffle in
MoveNodesFast and minstd draws in MergeNodesSubset), so parity follows the
DESIGN.md statistical bar: partition equality (canonicalized, per level) on
trajectory-stable golden graphs where repeated reference runs agree, and
partition QUALITY (CPM objective, community counts) within the reference's
run distribution elsewhere. The reference core (ref_leiden in
oracle/_ref/libref_online.so) provides the comparison runs; they are
recorded in tests/golden/leiden_reference.json (tests/golden_replay.py says
how to re-record), so the tests run where oracle/_ref cannot be built."""
import ctypes
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from memgraph_amd.native import BUILD_SYM_CSR, BUILD_WEIGHTED, Native  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from golden_replay import GoldenReplay  # noqa: E402

pytestmark = pytest.mark.gpu

I64 = ctypes.c_int64
P64 = ctypes.POINTER(ctypes.c_int64)
PD = ctypes.POINTER(ctypes.c_double)
CAP = 16


class RefLeiden:
    """The reference core: recorded runs, or the live library when
    re-recording them."""

    def __init__(self):
        self.golden = GoldenReplay("leiden_reference")
        if not self.golden.recording:
            return
        path = os.path.join(REPO, "oracle", "_ref", "libref_online.so")
        self.lib = ctypes.CDLL(path)
        self.lib.ref_leiden.argtypes = [I64, I64, P64, P64, PD, ctypes.c_double,
                                        ctypes.c_double, ctypes.c_double, I64, I64,
                                        P64, P64]

    def run(self, V, src, dst, weights=None, gamma=1.0, theta=0.01, resolution=0.01,
            max_iterations=(1 << 62)):
        args = dict(V=V, src=src, dst=dst, weights=weights, gamma=gamma, theta=theta,
                    resolution=resolution, max_iterations=max_iterations)
        hier, lv = self.golden.call({"run": args, "cap": CAP}, lambda: self._run(**args))
        return np.asarray(hier, dtype=np.int64), np.asarray(lv, dtype=np.int64)

    def _run(self, V, src, dst, weights, gamma, theta, resolution, max_iterations):
        src = np.ascontiguousarray(src, dtype=np.int64)
        dst = np.ascontiguousarray(dst, dtype=np.int64)
        w = np.ascontiguousarray(weights if weights is not None else [],
                                 dtype=np.float64)
        hier = np.full(V * CAP, -1, dtype=np.int64)
        lv = np.zeros(V, dtype=np.int64)
        self.lib.ref_leiden(I64(V), I64(len(src)), src.ctypes.data_as(P64),
                            dst.ctypes.data_as(P64),
                            w.ctypes.data_as(PD) if weights is not None else None,
                            gamma, theta, resolution, I64(max_iterations), I64(CAP),
                            hier.ctypes.data_as(P64), lv.ctypes.data_as(P64))
        return hier.reshape(V, CAP), lv


@pytest.fixture(scope="module")
def nat():
    n = Native()
    if n.device_count() == 0:
        pytest.skip("no HIP device")
    return n


@pytest.fixture(scope="module")
def ctx(nat):
    c = nat.init(0)
    yield c
    nat.destroy(c)


@pytest.fixture(scope="module")
def ref():
    return RefLeiden()


def canonical_partition(labels):
    """labels -> canonical tuple (first-occurrence renumbering)."""
    remap = {}
    out = []
    for l in labels:
        if l not in remap:
            remap[l] = len(remap)
        out.append(remap[l])
    return tuple(out)


def top_partition(hier, levels):
    return canonical_partition([hier[v][levels[v] - 1] for v in range(len(levels))])


# two triangles + bridge
V6 = 6
SRC6 = [0, 1, 2, 3, 4, 5, 2]
DST6 = [1, 2, 0, 4, 5, 3, 3]


def test_leiden_golden_partition(nat, ctx, ref):
    """On the golden graph the reference's partition is trajectory-stable
    across its own random runs; ours must equal it (canonicalized)."""
    parts = set()
    for _ in range(8):
        h, lv = ref.run(V6, SRC6, DST6)
        if (lv < 0).any():
            continue
        assert (lv > 0).all()
        parts.add(top_partition(h, lv))
    assert len(parts) == 1, f"reference unstable on golden graph: {parts}"

    g = nat.graph_from_coo(ctx, SRC6, DST6, V6, flags=BUILD_SYM_CSR)
    gh, glv = nat.leiden(ctx, g, V6, seed=3, cap=CAP)
    assert (glv > 0).all()
    assert top_partition(gh, glv) in parts, (top_partition(gh, glv), parts)
    # triangles end up together
    p = top_partition(gh, glv)
    assert p[0] == p[1] == p[2]
    assert p[3] == p[4] == p[5]
    assert p[0] != p[3]
    nat.graph_destroy(ctx, g)


def _cpm_quality(V, src, dst, labels, gamma_norm):
    """CPM objective: sum over unique undirected edges inside communities of
    w minus gamma * sum_c |c|(|c|-1)/2 (the objective MoveNodesFast
    locally optimizes, reference leiden.cpp:88-101)."""
    seen = set()
    intra = 0.0
    for s, d in zip(src, dst):
        key = (min(s, d), max(s, d))
        if key in seen:
            continue
        seen.add(key)
        if labels[s] == labels[d] and s != d:
            intra += 1.0
    sizes = {}
    for l in labels:
        sizes[l] = sizes.get(l, 0) + 1
    pen = sum(n * (n - 1) / 2 for n in sizes.values())
    return intra - gamma_norm * pen


def test_leiden_quality_random(nat, ctx, ref):
    """Planted-partition graph (8 dense clusters, sparse bridges): CPM finds
    the planted structure robustly in both implementations, so community
    count and CPM quality must sit inside the reference's run spread. A
    uniform random graph is NOT used here: on those, even the reference's
    own runs swing between 3 and 40 communities and sometimes end in its
    "No communities detected." error path (observed via ref_leiden), so no
    cross-implementation bound is meaningful."""
    rng = np.random.RandomState(9)
    K, M = 8, 15          # 8 clusters of 15 nodes
    V = K * M
    src, dst = [], []
    for k in range(K):
        base = k * M
        for i in range(M):
            for j in range(i + 1, M):
                if rng.rand() < 0.5:
                    src.append(base + i)
                    dst.append(base + j)
    for _ in range(20):   # sparse inter-cluster bridges
        a, b = rng.randint(0, V), rng.randint(0, V)
        if a // M != b // M:
            src.append(a)
            dst.append(b)
    uniq = {(min(s, d), max(s, d)) for s, d in zip(src, dst)}
    gamma_norm = 1.0 / sum(1.0 for _ in uniq)

    ref_q = []
    ref_k = []
    for _ in range(10):
        h, lv = ref.run(V, src, dst)
        if (lv <= 0).any():
            continue  # reference-error run (leiden.cpp:585-586)
        labels = [h[v][lv[v] - 1] for v in range(V)]
        ref_q.append(_cpm_quality(V, src, dst, labels, gamma_norm))
        ref_k.append(len(set(labels)))
    assert len(ref_q) >= 3, "reference errored on most planted-partition runs"

    g = nat.graph_from_coo(ctx, src, dst, V, flags=BUILD_SYM_CSR)
    gh, glv = nat.leiden(ctx, g, V, seed=7, cap=CAP)
    assert (glv > 0).all()
    labels = [gh[v][glv[v] - 1] for v in range(V)]
    q = _cpm_quality(V, src, dst, labels, gamma_norm)
    k = len(set(labels))
    spread = max(ref_q) - min(ref_q) + 1e-9
    assert q >= min(ref_q) - max(3 * spread, 0.05 * abs(min(ref_q)) + 1e-6), \
        (q, ref_q)
    assert min(ref_k) - 2 <= k <= max(ref_k) + 2, (k, ref_k)
    nat.graph_destroy(ctx, g)


def test_leiden_weighted(nat, ctx, ref):
    """Weighted golden: heavier triangle edges dominate the bridge."""
    w = [5.0, 5.0, 5.0, 5.0, 5.0, 5.0, 0.5]
    h, lv = ref.run(V6, SRC6, DST6, weights=w)
    if (lv < 0).any():
        pytest.skip("reference errored on the weighted golden run")
    expected = top_partition(h, lv)
    g = nat.graph_from_coo(ctx, SRC6, DST6, V6, weights=w,
                           flags=BUILD_SYM_CSR | BUILD_WEIGHTED)
    gh, glv = nat.leiden(ctx, g, V6, seed=5, cap=CAP)
    assert top_partition(gh, glv) == expected
    nat.graph_destroy(ctx, g)


def test_leiden_module_registration():
    """leiden_community_detection.so registers the reference's exact
    procedures (leiden_community_detection_module.cpp:108-160)."""
    import json
    import subprocess
    mockdir = os.path.join(os.path.dirname(__file__), "mock")
    script = (
        "import sys, json\n"
        f"sys.path.insert(0, {mockdir!r})\n"
        "from harness import ModuleHost\n"
        "h = ModuleHost('leiden_community_detection')\n"
        "print(json.dumps(h.procedures()))\n")
    out = subprocess.run([sys.executable, "-c", script], capture_output=True,
                         text=True)
    assert out.returncode == 0, out.stderr
    procs = json.loads(out.stdout)
    assert procs["get"]["args"] == [
        ["weight_property", "string"], ["gamma", "float"], ["theta", "float"],
        ["resolution_parameter", "float"], ["number_of_iterations", "int"]]
    assert procs["get"]["results"] == [
        ["node", "node"], ["community_id", "int"], ["communities", "list"]]
    assert procs["get_subgraph"]["args"][:2] == [
        ["subgraph_nodes", "list"], ["subgraph_relationships", "list"]]


def test_leiden_module_scenario(nat):
    """The real .so end-to-end on the golden graph through the mock host."""
    import subprocess
    mockdir = os.path.join(os.path.dirname(__file__), "mock")
    script = (
        "import sys, ctypes, os\n"
        f"sys.path.insert(0, {mockdir!r})\n"
        "os.environ['MGX_LEIDEN_SEED'] = '11'\n"
        "from harness import ModuleHost\n"
        "h = ModuleHost('leiden_community_detection')\n"
        "h.load_graph([0,1,2,3,4,5], [0,1,2,3,4,5,2], [1,2,0,4,5,3,3])\n"
        "rows = h.call('get')\n"
        "assert len(rows) == 6, rows\n"
        "h.mock.mock_result_list_len.restype = ctypes.c_int64\n"
        "cids = [h.row_int(i, 'community_id') for i in rows]\n"
        "lens = [h.mock.mock_result_list_len(ctypes.c_int64(i), b'communities')\n"
        "        for i in rows]\n"
        "assert all(l >= 1 for l in lens), lens\n"
        "assert cids[0] == cids[1] == cids[2]\n"
        "assert cids[3] == cids[4] == cids[5]\n"
        "assert cids[0] != cids[3]\n"
        "print('LEIDEN_MODULE_OK')\n")
    out = subprocess.run([sys.executable, "-c", script], capture_output=True,
                         text=True)
    assert out.returncode == 0, out.stderr + out.stdout
    assert "LEIDEN_MODULE_OK" in out.stdout
