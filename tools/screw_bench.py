#!/usr/bin/env python3
"""Throughput of PlanningWorld.plan_screw_batch_device (mpg_screw_batch) on one GPU.

Workload: recipe S of tests/screw_cases.py scaled to N rows in the cfg3 world
(Panda + 10 boxes): q_start uniform in 0.6 x the joint limits, the goal the
start pose of panda_hand rotated in the world by 0.05 .. 0.5 rad and translated
by 0.02 .. 0.15 m, everything device-resident, max_waypoints = 64.  Reports,
per N:

  rows/s of the whole call (HIP events around it, best of --reps)
  the split between screw_kernel (+ the fold) and the collide pass over the
    padded path (the world's profile hooks give the collide pass's cull /
    bucket / narrow time; the rest of the call is the screw kernels)
  the mean and maximum waypoint count and the share of VALID rows
  screw_row of the same header (csrc/mpg_screw.h, built for the host by
    tests/native/screw_host.cpp) on one thread over the first --host-rows rows,
    scaled to the batch

One JSON line per N.  Usage: python tools/screw_bench.py [--rows 1024 16384]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

LINK = "panda_hand"
MAX_WAYPOINTS = 64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[1 << 10, 1 << 14])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-rows", type=int, default=2048)
    args = ap.parse_args()
    import torch
    from mplib_amd import _capi as C
    from mplib_amd import scenes
    import build_hash
    import screw_cases as S

    w, art = scenes.world(3)
    li = w.ik_link_index(LINK)
    lim = scenes.joint_limits(art)
    lib_hash = build_hash.build_hash(build_hash.LIB)
    info = C.WorldInfo()
    h = ctypes.c_void_p(w.device_handle())
    C.check(C.lib().mpg_world_get_info(h, ctypes.byref(info)), "info")
    for n in args.rows:
        rng = np.random.default_rng(2025)
        q0 = rng.uniform(0.6 * lim[:, 0], 0.6 * lim[:, 1], size=(n, 7))
        axis = S.random_unit(rng, n)
        angle = rng.uniform(0.05, 0.5, size=n)
        shift = S.random_unit(rng, n) * rng.uniform(0.02, 0.15, size=(n, 1))
        poses = np.zeros((n, info.n_links, 7))
        C.check(C.lib().mpg_fk_batch(h, q0.ctypes.data, n, poses.ctypes.data, C.MPG_MEM_HOST, None), "fk")
        goal = np.stack([S.moved_pose(poses[i, li], axis[i], angle[i], shift[i]) for i in range(n)])
        g = torch.from_numpy(goal).cuda()
        s0 = torch.from_numpy(q0).cuda()
        path = torch.zeros(n, MAX_WAYPOINTS, 7, dtype=torch.float64, device="cuda")
        cnt = torch.zeros(n, dtype=torch.int32, device="cuda")
        st = torch.zeros(n, dtype=torch.uint8, device="cuda")
        hit = torch.zeros(n, dtype=torch.int32, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream

        def call():
            w.plan_screw_batch_device(li, g.data_ptr(), s0.data_ptr(), n, path.data_ptr(), cnt.data_ptr(),
                                      st.data_ptr(), hit.data_ptr(), stream, max_waypoints=MAX_WAYPOINTS)

        call()  # warm up: workspaces, code objects
        torch.cuda.synchronize()
        total_ms = None
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            call()
            b.record()
            torch.cuda.synchronize()
            ms = a.elapsed_time(b)
            total_ms = ms if total_ms is None else min(total_ms, ms)
        stv, cv = st.cpu().numpy(), cnt.cpu().numpy()
        w.profile_enable(True)
        call()
        torch.cuda.synchronize()
        prof = w.profile_read()
        w.profile_enable(False)
        collide_ms = sum(v[0] for v in prof.values())
        n_host = min(args.host_rows, n)
        S.host_header_rows(goal[:1], q0[:1], max_waypoints=MAX_WAYPOINTS)  # builds the shim
        t0 = time.perf_counter()
        hp, hc, hs = S.host_header_rows(goal[:n_host], q0[:n_host], max_waypoints=MAX_WAYPOINTS)
        host_s = (time.perf_counter() - t0) * n / n_host
        print(json.dumps({
            "bench": "screw_batch", "world": "cfg3 panda_10boxes", "rows": n, "max_waypoints": MAX_WAYPOINTS,
            "lib_hash": lib_hash, "total_ms": round(total_ms, 3), "rows_per_s": round(n / total_ms * 1e3),
            "collide_ms": round(collide_ms, 3), "screw_ms": round(total_ms - collide_ms, 3),
            "collide_share": round(collide_ms / total_ms, 3), "mean_waypoints": round(float(cv.mean()), 2),
            "max_waypoints_used": int(cv.max()), "reached": round(float((stv & 1).astype(bool).mean()), 4),
            "valid_rows": round(float(((stv & 3) == 3).mean()), 4),
            "host_screw_row_s_one_thread": round(host_s, 4), "host_rows_timed": n_host,
            "host_counts_equal": bool((hc == cv[:n_host]).all()),
            "speedup_vs_host": round(host_s * 1e3 / total_ms, 1),
        }), flush=True)


if __name__ == "__main__":
    main()
