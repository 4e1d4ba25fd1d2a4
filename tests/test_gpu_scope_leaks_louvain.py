"""Louvain's error paths release their device buffers: the seventh stateless
entry point under the allocation-failure loop of test_gpu_scope_leaks.py, on
that file's 317-vertex graph and with its checks (every failing call reports
out-of-memory, leaves no scope-owned block behind and leaves the context able
to reproduce the un-armed result exactly; the cap on k is that file's 500).

Louvain does not write to the graph. It only grows the context's col/w arenas,
which stay consistent when that fails: pointer and size are cleared before the
re-allocation. The graph's weights are integers, so every fp64 sum is exact and
the result is reproducible bit for bit.

Per the CPU oracle the graph takes two phases: 317 vertices in 4 sweeps with
the star's centre (300 neighbours) on the hub-pool path, one coarsening, then
3 vertices in 2 sweeps. So the level sweeps, the renumbering, the coarsening
and the hand-over of a coarse level all fail in turn.

Scope allocations per call, as measured: 59.
"""
import numpy as np
import pytest

import test_gpu_scope_leaks as base
from test_gpu_scope_leaks import nat, world  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu


def test_louvain_failed_allocation_leaves_nothing_behind(nat, world, monkeypatch):  # noqa: F811
    ctx, g, V = world

    def louvain():
        comm, n = nat.louvain(ctx, g, V)
        return comm, np.array([n])

    ids, sizes = np.unique(louvain()[0], return_counts=True)
    assert dict(zip(ids.tolist(), sizes.tolist())) == {-1: 4, 0: 6, 1: 6, 2: 301}, \
        "the CPU oracle's partition of this graph"
    monkeypatch.setattr(base, "calls", lambda *_: {"louvain": louvain})
    base.test_failed_allocation_leaves_nothing_behind(nat, world, "louvain")
