"""Persistent device state of the online modules (mgx_dev_array, mgx_online.h).

Their arrays start at 2^20, 2^16, 64, 256 and 4096 elements, so no other test
of these modules, on graphs of 6 to a few dozen vertices, ever grows one with
live contents. mgx_test_state_hook shrinks every first capacity; each module's
smallest scenario of its own test file (set on the 6-node graph, an update
that adds a vertex and an edge, get) must then give what it gives with the
default capacities, and a forced allocation failure (mgx_test_scope_hook, as in
test_gpu_scope_leaks.py) anywhere in it must report out-of-memory, leave no
scope-owned block behind, leave no persistent block behind after a reset, and
leave the module able to reproduce the kept result from `set`.

First capacities 1 and 6: from 1 the arrays of 6 slots hold 8, so the seventh
vertex fits, while the 60 walks of pagerank_online (64) grow at the update;
from 6 the slot arrays hold 6 and the seventh vertex grows every one of them.

What "the same result" means per module:
  pagerank_online  exact: ranks are integer counts over RNG streams keyed by
                   seed, walk and generation, divided by their sum.
  katz_online      exact: two default runs with a reset between were
                   bit-identical on the parent commit.
  LabelRankT       label equality, the bar of test_gpu_lrt.py.

Scope allocations per scenario with the first capacity at 1, i.e. the first k
that gets through minus one, as measured: pagerank_online 33, katz_online 51,
LabelRankT 165 (the loop's cap is 500). Persistent blocks held after a
scenario: 8, 13 and 6.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from memgraph_amd.native import (BUILD_IN_CSR, BUILD_NO_PERM, BUILD_OUT_CSR,  # noqa: E402
                                 BUILD_SYM_CSR, ERR_OUT_OF_MEMORY, MgxError, Native)

pytestmark = pytest.mark.gpu

K_CAP = 500
MODULES = ["pronline", "konline", "lrt"]

# test_gpu_pronline.py / test_gpu_konline.py: the reference e2e graph, then 4->6
E2E_SRC = [0, 1, 2, 3, 3, 3]
E2E_DST = [1, 2, 0, 3, 4, 5]
# test_gpu_lrt.py: two triangles and a bridge, then vertex 6 tied to vertex 0
LRT_SRC = [0, 1, 2, 3, 4, 5, 2]
LRT_DST = [1, 2, 0, 4, 5, 3, 3]


@pytest.fixture(scope="module")
def nat():
    n = Native()
    if n.device_count() == 0:
        pytest.skip("no HIP device")
    return n


@pytest.fixture(scope="module")
def world(nat):
    """The context and each module's two graphs, built once: building a graph
    allocates through scopes too, so it stays outside the armed stretch."""
    ctx = nat.init(0)
    six, seven = list(range(6)), list(range(7))
    graphs = {
        "pronline": (nat.graph_from_coo(ctx, E2E_SRC, E2E_DST, 6, flags=BUILD_OUT_CSR),
                     nat.graph_from_coo(ctx, E2E_SRC + [4], E2E_DST + [6], 7,
                                        flags=BUILD_OUT_CSR)),
        "konline": (nat.graph_from_coo(ctx, E2E_SRC, E2E_DST, 6,
                                       flags=BUILD_IN_CSR | BUILD_OUT_CSR | BUILD_NO_PERM),
                    nat.graph_from_coo(ctx, E2E_SRC + [4], E2E_DST + [6], 7,
                                       flags=BUILD_IN_CSR | BUILD_OUT_CSR | BUILD_NO_PERM)),
        "lrt": (nat.graph_from_coo(ctx, LRT_SRC, LRT_DST, 6, flags=BUILD_SYM_CSR),
                nat.graph_from_coo(ctx, LRT_SRC + [6, 0], LRT_DST + [0, 6], 7,
                                   flags=BUILD_SYM_CSR)),
    }

    def pronline():
        g, g2 = graphs["pronline"]
        a = nat.pronline_set(ctx, g, six, R=10, eps=0.2, seed=21)
        b = nat.pronline_update(ctx, g2, seven, cv=[6], ce=[(4, 6)])
        c, consistent = nat.pronline_get(ctx, seven)
        return a, b, c, np.array([consistent, *nat.pronline_stats(ctx)])

    def konline():
        g, g2 = graphs["konline"]
        a = nat.konline_set(ctx, g, six)
        b = nat.konline_update(ctx, g2, seven, cv=[6], ce=[(4, 6)])
        c, consistent = nat.konline_get(ctx, seven)
        return a, b, c, np.array([consistent, nat.konline_iterations()])

    def lrt():
        g, g2 = graphs["lrt"]
        a = nat.lrt_set(ctx, g, six)
        b = nat.lrt_update(ctx, g2, seven, mv=[6], me=[(6, 0), (0, 6)])
        c, ran = nat.lrt_get(ctx, g2, seven)
        return a, b, c, np.array([ran])

    def reset_all():
        nat.pronline_reset(ctx)
        nat.konline_reset(ctx)
        nat.lrt_reset(ctx)

    reset_all()
    assert nat.test_state_hook(-1) == 0
    kept = {}
    for name, run in (("pronline", pronline), ("konline", konline), ("lrt", lrt)):
        kept[name] = run()  # default capacities
        assert nat.test_state_hook(-1) > 0, f"{name} holds no persistent block after a run"
        reset_all()
        assert nat.test_state_hook(-1) == 0, f"{name}: blocks left after reset"
    yield {"reset_all": reset_all, "kept": kept,
           "run": {"pronline": pronline, "konline": konline, "lrt": lrt}}
    nat.test_scope_hook(-1)
    nat.test_state_hook(-1)
    reset_all()
    for pair in graphs.values():
        for g in pair:
            nat.graph_destroy(ctx, g)
    nat.destroy(ctx)


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("first_cap", [1, 6])
@pytest.mark.parametrize("name", MODULES)
def test_growth_equals_no_growth(nat, world, name, first_cap):
    world["reset_all"]()
    assert nat.test_state_hook(first_cap) == 0
    try:
        got = world["run"][name]()
    finally:
        held = nat.test_state_hook(-1)
    print(f"{name}: first capacity {first_cap}, {held} persistent blocks after the scenario")
    assert same(got, world["kept"][name]), (name, first_cap, got, world["kept"][name])
    assert nat.test_scope_hook(-1) == 0, "scope blocks outstanding after a clean run"


@pytest.mark.parametrize("name", MODULES)
def test_failed_allocation_leaves_nothing_behind(nat, world, name):
    run, kept, reset_all = world["run"][name], world["kept"][name], world["reset_all"]
    k = 1
    while True:
        assert k < K_CAP, f"{name}: still failing at allocation {k}"
        reset_all()
        assert nat.test_state_hook(1) == 0
        nat.test_scope_hook(k)
        try:
            got, status = run(), 0
        except MgxError as e:
            got, status = None, e.status
        outstanding = nat.test_scope_hook(-1)  # also disarms
        if status == 0:
            break
        assert status == ERR_OUT_OF_MEMORY, (name, k, status)
        assert outstanding == 0, f"{name}: {outstanding} blocks left after failing allocation {k}"
        reset_all()
        assert nat.test_state_hook(-1) == 0, f"{name}: persistent blocks left after allocation {k}"
        assert same(run(), kept), f"{name}: result changed after failing allocation {k}"
        assert nat.test_scope_hook(-1) == 0
        k += 1
    print(f"{name}: {k - 1} scope allocations per scenario")
    assert k > 1, f"{name}: the hook never fired"
    assert outstanding == 0
    assert same(got, kept)
    reset_all()
    assert nat.test_state_hook(-1) == 0


def test_reset_of_all_modules_frees_every_persistent_block(nat, world):
    for name in MODULES:
        world["run"][name]()
    assert nat.test_state_hook(-1) > 0
    world["reset_all"]()
    assert nat.test_state_hook(-1) == 0
    assert nat.test_scope_hook(-1) == 0
