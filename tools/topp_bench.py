#!/usr/bin/env python3
"""Throughput of DeviceWorld.topp_batch_device (mpg_topp_batch) on one GPU.

Workload: the "walk" family of recipe T (tests/topp_cases.py) scaled to 64
waypoints -- row r is the cumulative sum of default_rng(r).normal(0, 0.05,
(64, 7)) -- under the Panda's velocity and acceleration limits, everything
device-resident, the defaults (grid_per_segment 8: N = 504 gridpoints per row,
step 0.1, at most 256 samples).  Reports, per row count:

  rows/s of the whole call (HIP events around it, best of --reps after a
    warm-up call)
  the mean duration and sample count, the rows that are not MPG_TOPP_OK
  topp_row / topp_sample of the same header (csrc/mpg_topp.h, built for the
    host by tests/native/topp_host.cpp) on one thread over the first
    --host-rows rows, scaled to the batch, and whether its durations are the
    device's bit for bit

The split between topp_row_kernel and topp_sample_kernel comes from a kernel
trace of a run of its own (rocprofv3 --kernel-trace --stats -- python
tools/topp_bench.py --rows 1024).  One JSON line per row count.
Usage: python tools/topp_bench.py [--rows 1024 16384]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

WAYPOINTS = 64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[1 << 10, 1 << 14])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-rows", type=int, default=256)
    args = ap.parse_args()
    import torch
    from mplib_amd.batch import DeviceWorld
    import build_hash
    import topp_cases as T
    import worlds as Wd

    dw = DeviceWorld(Wd.desc_arrays(Wd.oracle_world(3)))
    lib_hash = build_hash.build_hash(build_hash.LIB)
    for n in args.rows:
        path = np.stack([np.cumsum(np.random.default_rng(r).normal(0.0, 0.05, size=(WAYPOINTS, 7)), axis=0)
                         for r in range(n)])
        cnt = np.full(n, WAYPOINTS, np.int32)
        p, c = torch.from_numpy(path).cuda(), torch.from_numpy(cnt).cuda()
        stream = torch.cuda.current_stream().cuda_stream
        out = dw.topp_batch_device(p, c, T.VMAX, T.AMAX, stream=stream)  # warm up: workspace, code objects
        torch.cuda.synchronize()
        total_ms = None
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            dw.topp_batch_device(p, c, T.VMAX, T.AMAX, out=out, stream=stream)
            b.record()
            torch.cuda.synchronize()
            ms = a.elapsed_time(b)
            total_ms = ms if total_ms is None else min(total_ms, ms)
        ns, dur, st = (t.cpu().numpy() for t in out[4:7])
        n_host = min(args.host_rows, n)
        T.host_topp(path[:1], cnt[:1])  # builds the shim
        t0 = time.perf_counter()
        host = T.host_topp(path[:n_host], cnt[:n_host])
        host_s = (time.perf_counter() - t0) * n / n_host
        print(json.dumps({
            "bench": "topp_batch", "rows": n, "waypoints": WAYPOINTS, "grid": T.grid_size(WAYPOINTS),
            "lib_hash": lib_hash, "total_ms": round(total_ms, 3), "rows_per_s": round(n / total_ms * 1e3),
            "mean_duration_s": round(float(dur.mean()), 3), "mean_samples": round(float(ns.mean()), 1),
            "rows_not_ok": int((st != T.OK).sum()),
            "host_topp_row_s_one_thread": round(host_s, 4), "host_rows_timed": n_host,
            "host_durations_equal": bool(np.array_equal(host["duration"], dur[:n_host])),
            "speedup_vs_host": round(host_s * 1e3 / total_ms, 1),
        }), flush=True)


if __name__ == "__main__":
    main()
