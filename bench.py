#!/usr/bin/env python3
"""Benchmark driver (contract: one JSON line from rank 0).

Workload (BASELINE.json metric): PageRank, fixed iterations, on RMAT-26
(V=2^26, E=2^30, Graph500 .57/.19/.19/.05, seed 1, multi-edges kept),
generated ON DEVICE, CSR resident in HBM before the timed region. A "step"
is one full PageRank iteration sweep. `value` = E_total * steps / t(steps),
edges/s aggregated over all ranks; t = max over ranks between barriers.

N>1 (launched by torch.distributed.run): one process per GPU; vertex-range
sharded in-CSR, ncclAllGather of owned rank/contrib slices per iteration
over xGMI (RCCL inside libmgx_analytics; torch.distributed gloo is used
ONLY to bootstrap the ncclUniqueId and for wall-clock barriers — no torch
in the compute path). Scaling is "strong": fixed RMAT-26 total work.

A plain run (`--gpus 1 --steps N --warmup W`) does only what the headline
figure needs: build the graph, warm up, time the N sweeps, print the result
line. Everything else the benchmark can measure or check sits behind
`--full` (off by default): the CPU baseline, the `--check` parity run
against the oracle, and the throwaway graph build that primes the allocator
so that `csr_build_ms` is the steady-state COO->CSR time (without it
`csr_build_ms` is the cold first build).

--dump-outputs DIR: after the timed steps, write what a caller of the timed
path receives after its last step, the normalized rank vector, as
DIR/rank.npy (float64). Above DUMP_MAX_ELEMS vertices a fixed seeded sample
of rows is written instead, so that two builds run with the same arguments
can be compared output for output.

cpu_baseline (--full): the reference's own ParallelIterativePageRank
compiled from the reference sources (oracle/_ref, kind "reference"; falls
back to the oracle restatement, kind "port", if _ref wasn't built), timed on
the host cores on a bounded sample (default RMAT-22, 6 iterations, one thread
per core, or OMP_NUM_THREADS where that is set lower), scaled to edges/s.
Rank 0, N=1 only.

roofline: dominant kernel = the fused SpMV sweep; algorithmic bytes per
launch = E*8 + V*20; achieved = bytes / avg sweep launch time
measured live with HIP events on the library's own stream. traffic comes
from profiles/traffic.json when a rocprofv3 --pmc pass has been recorded
for this workload (see profiles/README.md), else null.
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

HBM_PEAK = 8.0e12  # B/s, MI355X spec (MI355X_MICROARCH.md)
DUMP_MAX_ELEMS = 1 << 22  # rows written by --dump-outputs (f64: 32 MiB)
DUMP_SAMPLE_SEED = 20240229


def parse_args():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--scale", type=int, default=26)
    p.add_argument("--edge-factor", type=int, default=16)
    p.add_argument("--damping", type=float, default=0.85)
    p.add_argument("--seed", type=int, default=1)
    p.add_argument("--full", action="store_true",
                   help="also run everything beyond the headline figure: the CPU "
                        "baseline, --check, and the allocator-priming throwaway "
                        "graph build behind the steady-state csr_build_ms")
    p.add_argument("--dump-outputs", metavar="DIR", default=None,
                   help="write the rank vector the timed path produced in its "
                        "last step to DIR/rank.npy (seeded row sample when large)")
    p.add_argument("--cpu-baseline", type=int, default=1,
                   help="with --full: time the CPU baseline leg (0 turns it off)")
    p.add_argument("--cpu-sample-scale", type=int, default=22)
    p.add_argument("--cpu-sample-iters", type=int, default=6)
    p.add_argument("--check", type=int, default=0,
                   help="with --full: verify the first steps against the oracle "
                        "(small scales)")
    p.add_argument("--algo", default="pagerank",
                   choices=["pagerank", "wcc", "katz", "louvain"],
                   help="pagerank is the contract workload; the others are "
                        "secondary evidence lines (BASELINE.md configs 3-4)")
    p.add_argument("--gen", default="rmat", choices=["rmat", "uniform"],
                   help="secondary-line graph generator; uniform bounds "
                        "deg_max so Katz runs in its CONVERGENT regime "
                        "(VERDICT r01 weak #4: at RMAT-24 the reference's "
                        "divergent-gamma regime converges in one sweep)")
    p.add_argument("--katz-alpha", type=float, default=0.2)
    p.add_argument("--katz-eps", type=float, default=1e-2)
    args = p.parse_args()
    if args.check and not args.full:
        p.error("--check is part of the full run: pass --full with it")
    return args


def run_secondary(args):
    """Secondary algorithms: whole-call runtime on
    an RMAT graph, N=1 only. Emits one JSON line; not the contract metric."""
    import numpy as np  # noqa: F401
    from memgraph_amd.native import (BUILD_IN_CSR, BUILD_SYM_CSR, BUILD_WEIGHTED,
                                     Native)
    nat = Native()
    if nat.device_count() == 0:
        print(json.dumps({"error": "no HIP device"}))
        sys.exit(1)
    ctx = nat.init(0)
    # config 3/4 defaults: wcc/katz on RMAT-24; louvain on RMAT-22 — at
    # RMAT-24-weighted the grappolo break rule (modularity gain < 1e-6 per
    # Jacobi sweep, parallelLouvainMethod.cpp:251) admits thousands of
    # tiny-gain sweeps on the coarse levels (the reference's own CPU code
    # crawls the same way there).
    default_scale = 22 if args.algo == "louvain" else 24
    scale = args.scale if args.scale != 26 else default_scale
    V = 1 << scale
    E = args.edge_factor * V
    flags = {"wcc": BUILD_SYM_CSR, "katz": BUILD_IN_CSR,
             "louvain": BUILD_SYM_CSR | BUILD_WEIGHTED}[args.algo]
    if args.gen == "uniform":
        g = nat.graph_uniform(ctx, V, E, seed=args.seed, flags=flags)
    else:
        g = nat.graph_rmat(ctx, scale, E, seed=args.seed, flags=flags)
    reps = max(args.steps // 10, 1)
    extra = {}
    # one untimed warm call, then timed repetitions of the whole call
    for phase in ("warm", "timed"):
        if phase == "timed":
            nat.sync(ctx)
            t0 = time.perf_counter()
        for _ in range(1 if phase == "warm" else reps):
            if args.algo == "wcc":
                _, n = nat.wcc(ctx, g, V)
                extra["components"] = int(n)
            elif args.algo == "katz":
                _, iters = nat.katz(ctx, g, V, alpha=args.katz_alpha,
                                    epsilon=args.katz_eps)
                extra["iterations"] = int(iters)
            else:
                _, n = nat.louvain(ctx, g, V)
                extra["communities"] = int(n)
        if phase == "timed":
            nat.sync(ctx)
            t1 = time.perf_counter()
    secs = (t1 - t0) / reps
    out = {
        "metric": f"{args.algo} runtime",
        "value": secs * 1e3,
        "unit": "ms",
        "n_gpus": 1,
        "steps": reps,
        "warmup": 1,
        "ms_per_step": secs * 1e3,
        "higher_is_better": False,
        "scaling": "strong",
        "vs_baseline": None,
        "dtype": "f64" if args.algo == "katz" else "int32/f64",
        "data": "synthetic",
        "config": {"workload": f"{'RMAT' if args.gen == 'rmat' else 'UNIFORM'}-{scale} {args.algo}", "scale": scale,
                   "vertices": V, "edges": E, "seed": args.seed,
                   "parallelism": "single"},
        "edges_per_s": E / secs,
        "csr_build_ms": nat.graph_build_ms(g),
        **extra,
    }
    print(json.dumps(out))
    nat.graph_destroy(ctx, g)
    nat.destroy(ctx)


def cpu_baseline_leg(args):
    """Bounded reference-CPU sample, scaled to edges/s."""
    import numpy as np  # noqa: F401
    from memgraph_amd import rmat

    scale = args.cpu_sample_scale
    iters = args.cpu_sample_iters
    n_edges = args.edge_factor * (1 << scale)
    src, dst = rmat.gen_rmat(scale, n_edges, seed=args.seed)
    cores = os.cpu_count() or 1
    omp = os.environ.get("OMP_NUM_THREADS", "")
    if omp.isdigit() and 0 < int(omp) < cores:
        cores = int(omp)
    kind = None
    try:
        from oracle import Reference
        ref = Reference()
        _, secs = ref.pagerank_timed(1 << scale, src, dst, iterations=iters,
                                     damping=args.damping, n_threads=cores)
        kind = "reference"
    except OSError:
        from oracle import Oracle
        orc = Oracle()
        _, secs = orc.pagerank_timed(1 << scale, src, dst, iterations=iters,
                                     damping=args.damping, n_threads=cores)
        kind = "port"
    value = n_edges * iters / secs
    return {
        "value": value,
        "unit": "edges/s",
        "cores": cores,
        "kind": kind,
        "sample": f"RMAT-{scale} ({n_edges} edges), {iters} iterations, "
                  f"{cores} threads, {secs:.1f}s",
    }


def read_traffic(workload):
    path = os.path.join(REPO, "profiles", "traffic.json")
    if not os.path.exists(path):
        return None
    with open(path) as f:
        data = json.load(f)
    entry = data.get(workload)
    return entry.get("bytes_per_launch") if entry else None


def dump_outputs(outdir, rank_vec):
    """DIR/rank.npy: the whole rank vector, or above DUMP_MAX_ELEMS rows a
    sample at fixed seeded row indices (sorted, distinct)."""
    import numpy as np
    n = len(rank_vec)
    if n > DUMP_MAX_ELEMS:
        rng = np.random.default_rng(DUMP_SAMPLE_SEED)
        idx = np.unique(rng.integers(0, n, size=DUMP_MAX_ELEMS))
        rank_vec = rank_vec[idx]
    os.makedirs(outdir, exist_ok=True)
    np.save(os.path.join(outdir, "rank.npy"),
            np.ascontiguousarray(rank_vec, dtype=np.float64))


def main():
    args = parse_args()
    if args.algo != "pagerank":
        run_secondary(args)
        return
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", str(args.gpus)))
    local_rank = int(os.environ.get("LOCAL_RANK", str(rank)))
    n_gpus = max(world, args.gpus)

    from memgraph_amd.native import BUILD_IN_CSR, Native
    from memgraph_amd.sharding import shard_range

    dist = None
    if n_gpus > 1:
        import torch.distributed as dist_mod
        dist = dist_mod
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29501")
        dist.init_process_group("gloo", rank=rank, world_size=world)

    nat = Native()
    if nat.device_count() == 0:
        print(json.dumps({"error": "no HIP device"}))
        sys.exit(1)
    ctx = nat.init(local_rank)

    V = 1 << args.scale
    E = args.edge_factor * V

    if n_gpus > 1:
        uid = nat.comm_unique_id() if rank == 0 else None
        box = [uid]
        dist.broadcast_object_list(box, src=0)
        nat.comm_init(ctx, rank, world, box[0])
        row_begin, row_end = shard_range(V, world, rank)
        g = nat.graph_rmat_sharded(ctx, args.scale, E, row_begin, row_end, seed=args.seed)
        run = nat.pagerank_start_dist(ctx, g, row_begin, row_end, damping=args.damping)
    else:
        # Warm build (--full): the first large hipMallocs stall the stream
        # inside the build's event bracket (observed 0.3-1.7 s spread); a
        # throwaway build primes the allocator so the reported CSR-build
        # time is the actual device COO->CSR work.
        if args.full:
            g = nat.graph_rmat(ctx, args.scale, E, seed=args.seed, flags=BUILD_IN_CSR)
            nat.graph_destroy(ctx, g)
        g = nat.graph_rmat(ctx, args.scale, E, seed=args.seed, flags=BUILD_IN_CSR)
        run = nat.pagerank_start(ctx, g, damping=args.damping)
    csr_build_ms = nat.graph_build_ms(g)

    # Warmup (untimed), then flush the sweep-timing accumulator.
    if args.warmup > 0:
        nat.pagerank_iterate(run, args.warmup)
    nat.sync(ctx)
    sweep_ms0, launches0 = nat.pagerank_timing(run)

    # Timed region: barrier + sync on both sides, EXACTLY `steps` sweeps.
    if dist:
        dist.barrier()
    nat.sync(ctx)
    t0 = time.perf_counter()
    nat.pagerank_iterate(run, args.steps)
    nat.sync(ctx)
    if dist:
        dist.barrier()
    t1 = time.perf_counter()
    elapsed = t1 - t0
    if dist:
        import torch
        t = torch.tensor([elapsed], dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t[0])

    sweep_ms1, launches1 = nat.pagerank_timing(run)
    sweep_launches = launches1 - launches0
    sweep_ms_avg = (sweep_ms1 - sweep_ms0) / max(sweep_launches, 1)

    # The rank vector leaves the device only where something reads it.
    check = args.full and args.check and rank == 0 and n_gpus == 1
    dump = args.dump_outputs is not None and rank == 0
    got = nat.pagerank_finish(run, V, want_rank=check or dump)
    if dump:
        dump_outputs(args.dump_outputs, got)

    check_note = None
    if check:
        import numpy as np
        from oracle import Oracle
        orc = Oracle()
        src, dst = orc.gen_rmat(args.scale, E, seed=args.seed)
        exp, _ = orc.pagerank(V, src, dst, max_iterations=args.warmup + args.steps,
                              eps=0.0)
        check_note = float(np.abs(got - exp).max())
        assert check_note <= 1e-6, f"parity check failed: {check_note}"

    value = E * args.steps / elapsed  # whole-job edges/s, all ranks

    # Roofline for the dominant kernel on THIS rank (rank 0 reports).
    if n_gpus > 1:
        local_rows = shard_range(V, world, rank)[1] - shard_range(V, world, rank)[0]
        local_edges = nat.lib.mgx_graph_local_edges(g)  # exact owned edges
        algo_bytes = local_edges * 8 + local_rows * 20
    else:
        algo_bytes = E * 8 + V * 20
    achieved = algo_bytes / (sweep_ms_avg / 1e3) if sweep_ms_avg > 0 else 0.0
    workload = f"RMAT-{args.scale} PageRank ({args.steps} iters)"
    traffic = read_traffic(workload) if rank == 0 else None

    result = {
        "metric": "edges/s PageRank",
        "value": value,
        "unit": "edges/s",
        "n_gpus": n_gpus,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": elapsed * 1e3 / args.steps,
        "higher_is_better": True,
        "scaling": "strong",
        "vs_baseline": None,
        "dtype": "f32",
        "data": "synthetic",
        "config": {
            "workload": workload,
            "scale": args.scale,
            "vertices": V,
            "edges": E,
            "damping": args.damping,
            "seed": args.seed,
            "accumulation": "f64-per-row",
            "parallelism": f"vertex-range shard x{n_gpus}" if n_gpus > 1 else "single",
        },
        "csr_build_ms": csr_build_ms,
        "roofline": {
            "bound": "hbm",
            "achieved": achieved / 1e9,  # GB/s
            "peak": HBM_PEAK / 1e9,
            "unit": "GB/s",
            "frac": achieved / HBM_PEAK,
            "traffic": traffic,
        },
    }
    if rank == 0:
        if args.full and n_gpus == 1 and args.cpu_baseline:
            result["cpu_baseline"] = cpu_baseline_leg(args)
        else:
            result["cpu_baseline"] = None
        if check_note is not None:
            result["parity_linf_vs_oracle"] = check_note
        print(json.dumps(result))

    nat.graph_destroy(ctx, g)
    nat.destroy(ctx)
    if dist:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
