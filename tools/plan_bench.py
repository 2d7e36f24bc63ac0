#!/usr/bin/env python3
"""Throughput of PlanningWorld.plan_batch_device (mpg_plan_batch) on one GPU.

Workload: cfg5 -- the cfg3 world (Panda + 10 boxes), every row from
scenes.PLAN_START to scenes.PLAN_GOALS[--goal] ("far"), range 0.1, the rows'
sampler seeds derived from --seed, starts and goals device-resident.
PLAN_START itself touches a box of the scene: plan() resamples it
(random_sample_nearby), plan_batch reports it, so the rows start at the first
collision-free state of the same perturbation ladder (ratio (k + 1) / 1000 of
the joint range, k = 0, 1, ..., drawn with default_rng(--seed)).  Reports, per
Q:

  plans/s of the whole call (a host clock around it; the call ends with a
    stream synchronise), best of --reps, counting every row and solved rows
  the success rate, the mean and maximum rounds of a row -- a row's growTree
    calls: iterations + nodes added - 1 when solved, which its iterations and
    tree sizes give exactly -- and the rounds of the call (the slowest row's,
    rounded up to check_every)
  the split of one profiled call between the collide passes (the world's
    profile hooks: cull / bucket / narrow) and everything else (propose,
    commit, launch gaps, the host's reads of the active count)
  with --cadence: the Q rows again with each check_every of the list

One JSON line per Q (and per cadence).  Usage:
  python tools/plan_bench.py [--rows 1 64 1024 4096] [--cadence 1 8 64]

The per-round split into propose, collide, commit and gaps comes from a kernel
trace, taken in a run of its own (tracing slows the host):
  rocprofv3 --kernel-trace --output-format csv -d DIR -o trace -- \
      python tools/plan_bench.py --rows 1024 --reps 1 --no-profile
  python tools/plan_bench.py --trace DIR/trace_kernel_trace.csv[.gz]
--trace needs no GPU: it takes the last mpg_plan_batch call of the trace (from
its rrt_gather_kernel to its rrt_path_kernel), counts the rounds (propose
launches) and prints, per round, the time in rrt_propose_kernel, in the
collide pass's kernels, in rrt_commit_kernel, in everything else, and the
gaps (the call's span minus the time some kernel ran).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


COLLIDE_KERNELS = ("cull_kernel", "range_sum_kernel", "range_scan_kernel", "scatter_kernel", "narrow_kernel",
                   "closed_form_kernel")


def trace_split(path):
    """The per-round split of the last plan_batch call in a rocprofv3 kernel-trace CSV."""
    import csv
    import gzip
    with (gzip.open(path, "rt") if path.endswith(".gz") else open(path)) as fh:
        ks = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(fh))
    first = max(i for i, k in enumerate(ks) if "rrt_gather_kernel" in k[2])
    last = max(i for i, k in enumerate(ks) if "rrt_path_kernel" in k[2])
    call = ks[first:last + 1]
    rounds = sum("rrt_propose_kernel" in k[2] for k in call)
    ns = {"propose": 0, "collide": 0, "commit": 0, "other_kernels": 0}
    per_kernel = {}
    for s, e, name in call:
        key = ("propose" if "rrt_propose_kernel" in name else "commit" if "rrt_commit_kernel" in name else
               "collide" if any(c in name for c in COLLIDE_KERNELS) else "other_kernels")
        ns[key] += e - s
        if key == "collide":
            c = next(c for c in COLLIDE_KERNELS if c in name)
            per_kernel[c] = per_kernel.get(c, 0) + e - s
    span = call[-1][1] - call[0][0]
    us = lambda v: round(v / 1e3 / max(rounds, 1), 2)  # noqa: E731
    out = {"bench": "plan_batch_trace", "rounds": rounds, "call_span_ms": round(span / 1e6, 3),
           "us_per_round": {**{k: us(v) for k, v in ns.items()}, "gaps": us(span - sum(ns.values())), "span": us(span)},
           "collide_kernels_us_per_round": {k: us(v) for k, v in per_kernel.items()}}
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trace", default=None, help="a rocprofv3 kernel-trace CSV: print its per-round split and exit")
    ap.add_argument("--rows", type=int, nargs="+", default=[1, 64, 1024, 4096])
    ap.add_argument("--goal", default="far")
    ap.add_argument("--range", type=float, default=0.1)
    ap.add_argument("--max-rounds", type=int, default=20000)
    ap.add_argument("--max-nodes", type=int, default=2048)
    ap.add_argument("--max-waypoints", type=int, default=512)
    ap.add_argument("--check-every", type=int, default=8)
    ap.add_argument("--cadence", type=int, nargs="*", default=[])
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-profile", action="store_true")
    args = ap.parse_args()
    if args.trace:
        trace_split(args.trace)
        return
    import torch
    from mplib_amd import scenes
    import build_hash

    w, art = scenes.world(3)
    lib_hash = build_hash.build_hash(build_hash.LIB)
    stream = torch.cuda.current_stream().cuda_stream
    lim = scenes.joint_limits(art)
    ratio = (np.arange(1001)[:, None] + 1) / 1000.0
    cand = np.array(scenes.PLAN_START) + (lim[:, 1] - lim[:, 0]) * ratio * np.random.default_rng(args.seed).uniform(
        -1.0, 1.0, size=(1001, 7))
    cand = np.vstack([np.array(scenes.PLAN_START)[None], np.clip(cand, lim[:, 0], lim[:, 1])])
    first_free = int(np.flatnonzero(w.collide_batch(cand)[0] == 0)[0])
    start_state = cand[first_free]

    def run(Q, check_every, profile):
        s = torch.from_numpy(np.tile(start_state, (Q, 1))).cuda()
        g = torch.from_numpy(np.tile(np.array(scenes.PLAN_GOALS[args.goal]), (Q, 1))).cuda()
        path = torch.zeros(Q, args.max_waypoints, 7, dtype=torch.float64, device="cuda")
        cnt = torch.zeros(Q, dtype=torch.int32, device="cuda")
        st = torch.zeros(Q, dtype=torch.uint8, device="cuda")
        it = torch.zeros(Q, dtype=torch.int32, device="cuda")
        sz = torch.zeros(Q, 2, dtype=torch.int32, device="cuda")

        def call():
            w.plan_batch_device(s.data_ptr(), g.data_ptr(), Q, 1, path.data_ptr(), cnt.data_ptr(), st.data_ptr(),
                                it.data_ptr(), sz.data_ptr(), 0, stream, range=args.range, max_rounds=args.max_rounds,
                                max_nodes=args.max_nodes, max_waypoints=args.max_waypoints, seed=args.seed,
                                check_every=check_every)

        call()  # warm up: workspaces, code objects
        torch.cuda.synchronize()
        best = None
        for _ in range(args.reps):
            t0 = time.perf_counter()
            call()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        stv, itv, szv = st.cpu().numpy(), it.cpu().numpy(), sz.cpu().numpy()
        solved = stv == 1
        rounds = itv + szv.sum(axis=1) - 2 - solved  # one start root, one goal root
        call_rounds = -(-int(rounds.max()) // check_every) * check_every
        out = {
            "bench": "plan_batch", "world": "cfg5 cfg3-scene PLAN_START -> " + args.goal, "Q": Q, "range": args.range,
            "start_ladder_step": first_free, "check_every": check_every, "max_rounds": args.max_rounds,
            "max_nodes": args.max_nodes, "status_counts": {str(k): int(v) for k, v in zip(*np.unique(stv, return_counts=True))},
            "lib_hash": lib_hash, "total_ms": round(best * 1e3, 3), "plans_per_s": round(Q / best, 1),
            "solved_plans_per_s": round(float(solved.sum()) / best, 1), "success_rate": round(float(solved.mean()), 4),
            "mean_rounds": round(float(rounds.mean()), 1), "max_rounds_of_a_row": int(rounds.max()),
            "call_rounds": call_rounds, "us_per_round": round(best * 1e6 / max(call_rounds, 1), 1),
            "mean_iterations": round(float(itv.mean()), 1), "max_tree": int(szv.max()),
            "mean_waypoints": round(float(cnt.cpu().numpy()[solved].mean()), 1) if solved.any() else 0.0,
        }
        if profile:
            w.profile_enable(True)
            t0 = time.perf_counter()
            call()
            torch.cuda.synchronize()
            prof_ms = (time.perf_counter() - t0) * 1e3
            prof = w.profile_read()
            w.profile_enable(False)
            collide_ms = sum(v[0] for v in prof.values())
            out.update({"profiled_call_ms": round(prof_ms, 3), "collide_ms": round(collide_ms, 3),
                        "collide_us_per_round": round(collide_ms * 1e3 / max(call_rounds, 1), 1),
                        "collide_stages_ms": {str(k): round(v[0], 3) for k, v in prof.items()}})
        print(json.dumps(out), flush=True)

    for Q in args.rows:
        run(Q, args.check_every, not args.no_profile)
    for ce in args.cadence:
        run(max(args.rows), ce, False)


if __name__ == "__main__":
    main()
