#!/usr/bin/env python3
"""Throughput of PlanningWorld.ik_batch_device (mpg_ik_batch) on one GPU.

Workload: M goal poses x 20 seeds in the cfg3 world (Panda + 10 boxes), the
goals the FK of states uniform in 0.8 x the joint limits, the seeds drawn on
the device, everything device-resident.  Reports, per M:

  rows/s and goals/s of the whole call (HIP events around it, best of --reps)
  the split between the IK kernels and the collide pass (the world's profile
    hooks give the collide pass's cull / bucket / narrow time; the rest of the
    call is the IK kernels)
  the mean iterations per row and the share of rows converged / valid
  the same call with row claiming disabled (max_waves so large that every row
    has a lane of its own)
  the host compute_IK_CLIK on one thread over the first --host-rows rows of the
    same batch (the same seeds, read back), scaled to the batch

One JSON line per M.  Usage: python tools/ik_bench.py [--goals 1024 16384]
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

SEEDS = 20
START = np.array([0.0, 0.2, 0.0, -1.8, 0.0, 2.0, 0.8])
LINK = "panda_hand"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--goals", type=int, nargs="+", default=[1 << 10, 1 << 14])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-rows", type=int, default=2000)
    args = ap.parse_args()
    import torch
    from mplib_amd import scenes
    import build_hash

    w, art = scenes.world(3)
    pin = art.get_pinocchio_model()
    li = w.ik_link_index(LINK)
    lim = scenes.joint_limits(art)
    lib_hash = build_hash.build_hash(build_hash.LIB)
    for M in args.goals:
        rows = M * SEEDS
        q_goal = np.random.default_rng(5).uniform(0.8 * lim[:, 0], 0.8 * lim[:, 1], size=(M, 7))
        pose = np.stack([w.fk_link_pose(q, li) for q in q_goal]) if M <= 4096 else None
        if pose is None:  # large M: the goals' FK through the batched call
            import ctypes
            from mplib_amd import _capi as C
            info = C.WorldInfo()
            h = ctypes.c_void_p(w.device_handle())
            C.check(C.lib().mpg_world_get_info(h, ctypes.byref(info)), "info")
            out = np.zeros((M, info.n_links, 7))
            C.check(C.lib().mpg_fk_batch(h, q_goal.ctypes.data, M, out.ctypes.data, C.MPG_MEM_HOST, None), "fk")
            pose = np.ascontiguousarray(out[:, li])
        g = torch.from_numpy(pose).cuda()
        s0 = torch.from_numpy(START.copy()).cuda()
        q = torch.zeros(rows, 7, dtype=torch.float64, device="cuda")
        st = torch.zeros(rows, dtype=torch.uint8, device="cuda")
        it = torch.zeros(rows, dtype=torch.int32, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream

        def call(max_waves=0, max_iter=1000):
            w.ik_batch_device(li, g.data_ptr(), M, SEEDS, 0, s0.data_ptr(), q.data_ptr(), st.data_ptr(), 0,
                              it.data_ptr(), stream, seed=1, max_waves=max_waves, max_iter=max_iter)

        def timed(**kw):
            best = None
            for _ in range(args.reps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                call(**kw)
                b.record()
                torch.cuda.synchronize()
                ms = a.elapsed_time(b)
                best = ms if best is None else min(best, ms)
            return best

        call()  # warm up: workspaces, code objects
        torch.cuda.synchronize()
        total_ms = timed()
        stv, itv = st.cpu().numpy(), it.cpu().numpy()
        w.profile_enable(True)
        call()
        torch.cuda.synchronize()
        prof = w.profile_read()
        w.profile_enable(False)
        collide_ms = sum(v[0] for v in prof.values())
        no_claim_ms = timed(max_waves=(rows + 63) // 64)
        # the host CLIK on the same seeds: max_iter = 0 returns them
        call(max_iter=0)
        torch.cuda.synchronize()
        seeds = q.cpu().numpy()
        n_host = min(args.host_rows, rows)
        t0 = time.perf_counter()
        ok = 0
        for r in range(n_host):
            _, s, _ = pin.compute_IK_CLIK(8, list(pose[r // SEEDS]), list(seeds[r]) + [0.0, 0.0])
            ok += bool(s)
        host_s = (time.perf_counter() - t0) * rows / n_host
        print(json.dumps({
            "bench": "ik_batch", "world": "cfg3 panda_10boxes", "goals": M, "seeds": SEEDS, "rows": rows,
            "lib_hash": lib_hash, "total_ms": round(total_ms, 3), "rows_per_s": round(rows / total_ms * 1e3),
            "goals_per_s": round(M / total_ms * 1e3), "collide_ms": round(collide_ms, 3),
            "ik_ms": round(total_ms - collide_ms, 3), "mean_iters": round(float(itv.mean()), 1),
            "max_iters": int(itv.max()), "converged": round(float((stv & 1).astype(bool).mean()), 4),
            "valid_rows": round(float(((stv & 15) == 15).mean()), 4),
            "goals_with_solution": round(float(((stv & 15) == 15).reshape(M, SEEDS).any(axis=1).mean()), 4),
            "no_claim_ms": round(no_claim_ms, 3), "claim_speedup": round(no_claim_ms / total_ms, 3),
            "host_clik_s_one_thread": round(host_s, 2), "host_rows_timed": n_host,
            "host_converged": round(ok / n_host, 4), "speedup_vs_host": round(host_s * 1e3 / total_ms, 1),
        }), flush=True)


if __name__ == "__main__":
    main()
