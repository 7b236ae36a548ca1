#!/usr/bin/env python3
"""Flagship benchmark: FULL place+route wall-clock to feasibility on the
bitcoin_miner-scale synthetic config (BASELINE.json config 5), 1-8 MI355X.

A step = one COMPLETE place-and-route flow on a fixed synthetic netlist of
the named scale: GPU SA placement anneal (timing-driven, batched-move
CDNA4 kernels; strip-sharded over RCCL for N>1), PathFinder routing on the
HBM-resident rr graph to ZERO overused nodes with all sinks reached
(selective reroute + partial rip-up; occ all-reduce per iteration for
N>1), and STA-driven criticalities each iteration. The metric is the
reference's headline: place+route wall-clock at the reported
wirelength/critical-path. Setup (netlist synthesis, rr-graph build, one-
time graph upload) is untimed — the rr graph is the fixed device model.

N>1 is STRONG scaling: the same flow partitioned across GPUs.

A plain run does only what the headline figure needs: setup, warmup, the
timed flows, the optional output dump, the result line. --full is where
any further measurement belongs (none at present).

Launch (driver contract):
  python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]
  # N>1: python -m torch.distributed.run --nnodes=1 --nproc-per-node N \
  #        --master-addr 127.0.0.1 bench.py --gpus N ...
"""
import argparse
import gc
import json
import os
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent))

import numpy as np

# --dump-outputs writes at most this much in all (the limit is 64 MB);
# an array over its share is cut to a fixed, seeded sample of its entries
DUMP_BUDGET_BYTES = 48 << 20


def flow_outputs(flow):
    """What a caller of the timed flow receives, as two sets of named
    arrays: (exact, routed).

    exact — the same bits in every run with the same arguments: the
    placement (block coordinates, sub-tile slots, final bb and timing
    costs) and the routing verdict [success, overused nodes].

    routed — what the router produced: occupancy per rr node, routed
    delay per sink, and [wirelength, critical path (s), iterations]. The
    benched router lets the concurrent nets of a launch see each other's
    congestion through unordered atomics, so these differ in detail from
    run to run on identical inputs and are compared with a tolerance (see
    docs/MEASUREMENTS.md for the measured spread). The CPU engines have
    no device router: there only the summary is written."""
    pl = flow["place"]
    exact = {
        "place_x": np.asarray(pl.x, dtype=np.float32),
        "place_y": np.asarray(pl.y, dtype=np.float32),
        "place_slot": np.asarray(pl.slot, dtype=np.float32),
        "place_cost": np.array([pl.bb_cost, pl.td_cost], dtype=np.float64),
        "route_verdict": np.array(
            [float(flow["success"]), float(flow["route"]["overused"])],
            dtype=np.float64),
    }
    routed = {
        "route_summary": np.array(
            [float(flow["wirelength"]), float(flow["cpd"]),
             float(flow["route"]["iters"])], dtype=np.float64),
    }
    router = flow.get("router")
    if router is not None:
        routed["node_occ"] = router.t_occ.cpu().numpy().astype(np.float32)
        routed["sink_delay"] = router.t_sink_delay.cpu().numpy().astype(
            np.float32)
    return exact, routed


def dump_outputs(dirname, arrays, budget=DUMP_BUDGET_BYTES):
    d = Path(dirname)
    d.mkdir(parents=True, exist_ok=True)
    share = budget // len(arrays)
    for name, a in arrays.items():
        a = np.ascontiguousarray(a).reshape(-1)
        keep = share // a.itemsize
        if a.size > keep:
            idx = np.random.default_rng(0).choice(a.size, keep, replace=False)
            a = a[np.sort(idx)]
        np.save(d / f"{name}.npy", a)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=1,
                    help="number of timed complete place+route flows")
    ap.add_argument("--warmup", type=int, default=1,
                    help="untimed warmup flows (same work)")
    ap.add_argument("--config", type=str, default="bitcoin_miner",
                    help="named arch scale (BASELINE configs)")
    ap.add_argument("--fill", type=float, default=0.6)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--max-iters", type=int, default=80)
    ap.add_argument("--inner-num", type=float, default=1.0)
    ap.add_argument("--verbose", action="store_true")
    ap.add_argument("--dump-outputs", type=str, default=None, metavar="DIR",
                    help="after the timed flows, write the outputs of the "
                         "last one: DIR/<name>.npy for those that are "
                         "bit-identical from run to run (placement, its "
                         "costs, routing verdict), DIR/routed/<name>.npy for "
                         "the router's (occupancy, sink delays, summary), "
                         "which vary slightly between runs")
    ap.add_argument("--full", action="store_true",
                    help="also run the measurements that the headline "
                         "figure does not need (none at present)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    import torch
    from parallel_eda_amd.arch.archdef import get_arch
    from parallel_eda_amd.io.synth import synth_netlist, spec_for_arch
    from parallel_eda_amd.parallel.dist import init_dist
    from parallel_eda_amd import rrgraph

    rank, ws, local = init_dist()
    assert ws == args.gpus or ws == 1, f"WORLD_SIZE {ws} != --gpus {args.gpus}"
    use_gpu = torch.cuda.is_available()
    device = f"cuda:{local}" if use_gpu else "cpu"
    if use_gpu:
        torch.cuda.set_device(device)
    else:
        # CPU fallback exercises the exact distributed launch path (gloo)
        # with the oracle engines; headline numbers require MI355X.
        print("bench: no GPU — CPU-oracle fallback (not a headline number)",
              file=sys.stderr, flush=True)

    def log(*a):
        if rank == 0 and args.verbose:
            print(*a, file=sys.stderr, flush=True)

    # ---- setup (untimed): netlist + device model ----
    t_setup = time.perf_counter()
    arch = get_arch(args.config)
    nl = synth_netlist(spec_for_arch(arch, fill=args.fill, seed=args.seed))
    g = rrgraph.build_rr_graph(arch)
    dev_graph = None
    if use_gpu:
        from parallel_eda_amd.route.gpu_router import DevGraph
        dev_graph = DevGraph(g, arch, device)
    log(f"setup {time.perf_counter()-t_setup:.1f}s: {nl.num_blocks} blocks, "
        f"{nl.num_nets} nets, {nl.num_conns} conns; rr {g.num_nodes} nodes "
        f"{g.num_edges} edges")

    dist = None
    if ws > 1:
        import torch.distributed as dist

    def barrier_sync():
        if dist is not None:
            dist.barrier()
        if use_gpu:
            torch.cuda.synchronize(device)

    def one_flow(seed):
        if use_gpu:
            from parallel_eda_amd.parallel.full_flow import run_flow_gpu
            return run_flow_gpu(nl, arch, g, dev_graph=dev_graph, rank=rank,
                                world_size=ws, device=device, seed=seed,
                                max_route_iters=args.max_iters,
                                incremental=True, verbose=args.verbose,
                                inner_num=args.inner_num)
        from parallel_eda_amd.parallel.full_flow import run_flow_dist
        return run_flow_dist(nl, arch, rank=rank, world_size=ws, seed=seed,
                             max_route_iters=args.max_iters,
                             incremental=True, verbose=args.verbose)

    # A flow's result carries its live GpuRouter (tens of GiB of search
    # scratch at bitcoin scale), so only the most recent one is kept, and
    # it is dropped — and its memory handed back to the device, which the
    # router's scratch planner sizes itself against — before the next
    # flow starts. Every flow therefore sees the same free memory.
    last = None

    # The release runs inside the timed region, so a step pays for it;
    # release_s (printed with --verbose) says how much.
    release_s = 0.0

    def next_flow():
        nonlocal last, release_s
        t_rel = time.perf_counter()
        last = None
        if use_gpu:
            gc.collect()
            torch.cuda.empty_cache()
        release_s += time.perf_counter() - t_rel
        last = one_flow(args.seed)

    for w in range(args.warmup):
        t0 = time.perf_counter()
        next_flow()
        barrier_sync()
        log(f"warmup {w}: {time.perf_counter()-t0:.1f}s "
            f"success={last['success']}"
            f" wl={last['wirelength']} cpd={last['cpd']*1e9:.2f}ns "
            f"iters={last['route']['iters']} phases={last.get('phase_s')}")

    barrier_sync()
    t0 = time.perf_counter()
    feasible = True
    for k in range(args.steps):
        next_flow()
        feasible = feasible and bool(last["success"])
        log(f"step {k}: success={last['success']} wl={last['wirelength']} "
            f"cpd={last['cpd']*1e9:.2f}ns iters={last['route']['iters']} "
            f"phases={last.get('phase_s')} prof={last['route'].get('prof')} "
            f"rprof={getattr(last.get('router'), 'prof', None)}")
    barrier_sync()
    elapsed = time.perf_counter() - t0
    log(f"release between flows: {release_s:.2f}s over "
        f"{args.warmup + args.steps} flows")
    if dist is not None:
        from parallel_eda_amd.parallel.dist import allreduce_
        t = torch.tensor([elapsed], device=device if use_gpu else "cpu")
        allreduce_(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())

    sec_per_flow = elapsed / args.steps
    if rank == 0 and args.dump_outputs:
        exact, routed = flow_outputs(last)
        dump_outputs(args.dump_outputs, exact, DUMP_BUDGET_BYTES // 2)
        dump_outputs(Path(args.dump_outputs) / "routed", routed,
                     DUMP_BUDGET_BYTES // 2)
    if rank == 0:
        out = {
            "metric": "place+route wall-clock to feasibility (s/flow; "
                      "bitcoin_miner-scale synthetic on stratixiv-like "
                      "fabric)" if args.config == "bitcoin_miner" else
                      f"place+route wall-clock to feasibility (s/flow; "
                      f"{args.config}-scale synthetic)",
            "value": round(sec_per_flow, 3),
            "unit": "s",
            "n_gpus": args.gpus,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(sec_per_flow * 1000.0, 1),
            "higher_is_better": False,
            "scaling": "strong",
            "vs_baseline": None,
            "dtype": "fp32" if use_gpu else "fp32-cpu-fallback",
            "data": "synthetic (no network: synthetic netlist of the named "
                    "scale, random seed %d; placement computed in the timed "
                    "flow)" % args.seed,
            "feasible": feasible,
            "config": {
                "model": args.config,
                "arch": arch.name,
                "grid": f"{arch.nx}x{arch.ny}", "W": arch.W,
                "rr_nodes": g.num_nodes, "rr_edges": int(g.num_edges),
                "blocks": int(nl.num_blocks),
                "nets": int(nl.num_nets), "conns": int(nl.num_conns),
                "global_batch": int(nl.num_conns), "seq_len": 0,
                "parallelism": f"strip-sharded SA + spatial-partition "
                               f"routing x{args.gpus} GPUs, RCCL occ "
                               f"all-reduce per iteration",
                "route_iterations": int(last["route"]["iters"]),
                "final_overused": int(last["route"]["overused"]),
                "wirelength": int(last["wirelength"]),
                "crit_path_ns": round(last["cpd"] * 1e9, 3),
                "phase_s": {k2: round(v, 2)
                            for k2, v in last.get("phase_s", {}).items()},
            },
        }
        print(json.dumps(out))
    if dist is not None:
        dist.destroy_process_group()
    return 0 if feasible else 1


if __name__ == "__main__":
    sys.exit(main())
