"""The bench.py contract itself, exercised at a small scale on the GPU box:
one JSON line with the required fields, value consistent with ms_per_step,
parity check against the oracle enabled (--full), and the plain run's
--dump-outputs checked against the oracle."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

RESULT_KEYS = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step",
               "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config",
               "csr_build_ms", "roofline")


def run_bench(*extra):
    out = subprocess.run(
        [sys.executable, os.path.join(REPO, "bench.py"), "--scale", "16", "--steps", "3",
         "--warmup", "1", *extra],
        capture_output=True, text=True, cwd=REPO, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0])


def test_bench_contract_small():
    d = run_bench("--full", "--cpu-baseline", "0", "--check", "1")
    for key in RESULT_KEYS:
        assert key in d, key
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1
    assert d["unit"] == "edges/s"
    E = d["config"]["edges"]
    assert abs(d["value"] - E / (d["ms_per_step"] / 1e3)) / d["value"] < 1e-6
    assert d["roofline"]["bound"] == "hbm" and d["roofline"]["peak"] == 8000.0
    assert d["parity_linf_vs_oracle"] <= 1e-6


def test_bench_plain_run_dumps_outputs(oracle, tmp_path):
    """A plain run keeps the result line's fields, leaves the --full legs out,
    and --dump-outputs writes the rank vector after warmup+steps sweeps."""
    d = run_bench("--gpus", "1", "--dump-outputs", str(tmp_path))
    for key in RESULT_KEYS:
        assert key in d, key
    assert d["metric"] == "edges/s PageRank" and d["unit"] == "edges/s"
    assert d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1
    E = d["config"]["edges"]
    assert abs(d["value"] - E / (d["ms_per_step"] / 1e3)) / d["value"] < 1e-6
    assert d["cpu_baseline"] is None and "parity_linf_vs_oracle" not in d

    assert sorted(os.listdir(tmp_path)) == ["rank.npy"]
    got = np.load(tmp_path / "rank.npy")
    V = d["config"]["vertices"]
    assert got.dtype == np.float64 and got.shape == (V,)
    src, dst = oracle.gen_rmat(16, E, seed=1)
    exp, _ = oracle.pagerank(V, src, dst, max_iterations=4, eps=0.0)
    assert np.abs(got - exp).max() <= 1e-6


def test_bench_check_needs_full():
    out = subprocess.run(
        [sys.executable, os.path.join(REPO, "bench.py"), "--scale", "16", "--steps", "3",
         "--warmup", "1", "--check", "1"],
        capture_output=True, text=True, cwd=REPO, timeout=300)
    assert out.returncode == 2 and "--full" in out.stderr
