#!/usr/bin/env python3
"""Throughput of a world with movable scene objects ("Movable
scene objects"): cfg3 at 2^20 device-resident states with red_cube, blue_cube,
box0 and box3 movable, timed with

  per_row   one pose set per configuration (4 x 7 x 8 = 224 B of poses next to
            the 56 B of joint values of a row),
  shared    one pose set for the batch,
  parked    all four objects far away (the cull's far test drops them),

against the static cfg3 world in the same process.  Prints one JSON line with
the configs/s of each and the three ratios to the static world.

--queries times instead the two planner-facing queries on the movable world,
device-resident inputs and outputs, at the world's current poses and with one
pose set per row (seconds per call, median of --steps):

  distance    distance_batch_device at 2^18 states,
  motion      mpg_check_motion_batch(_free) at 2^16 edges (q_to = q_from +
              N(0, 0.3) clipped to the limits, the default longest valid
              segment), one pose set per edge,

each also with a per-row array that repeats the current poses (the same work
as the current-pose call plus the pose traffic alone), and the host-memory
Python calls (distance_batch, check_motion_batch) with
and without object_poses, which add the copies over the host link.
--current-only skips the per-row variants (a library without them).

    python tools/movable_bench.py [--n 1048576] [--steps 10] [--warmup 3]
    python tools/movable_bench.py --queries [--current-only]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]
import torch  # noqa: E402
from mplib_amd import scenes  # noqa: E402

MOVABLE = ["red_cube", "blue_cube", "box0", "box3"]


def poses(n, seed=2024):
    """Positions over the robot's workspace, uniform random orientations."""
    rng = np.random.default_rng(seed)
    P = np.zeros((n, len(MOVABLE), 7))
    P[:, :, :3] = rng.uniform([-0.3, -0.4, 0.0], [0.6, 0.4, 0.9], size=(n, len(MOVABLE), 3))
    qt = rng.normal(size=(n, len(MOVABLE), 4))
    P[:, :, 3:] = qt / np.linalg.norm(qt, axis=2, keepdims=True)
    return P


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in ev])) * 1e-3


def queries(args):
    """distance at 2^18 states and motion validation at 2^16 edges: current
    poses against one pose set per row."""
    from mplib_amd import _capi as C
    nd, ne = 1 << 18, 1 << 16
    dev = torch.device("cuda", 0)
    wm, art = scenes.world(3)
    for name in MOVABLE:
        wm.set_normal_object_movable(name)
    qh = scenes.sample_states(art, nd, scenes.CFG_SEED[3])
    lim = scenes.joint_limits(art)
    q0h = qh[:ne]
    q1h = np.clip(q0h + np.random.default_rng(17).normal(scale=0.3, size=q0h.shape), lim[:, 0], lim[:, 1])
    Ph = poses(nd)
    cur = np.array([list(wm.get_normal_object(name).get_pose()) for name in MOVABLE], dtype=np.float64)
    same = np.ascontiguousarray(np.broadcast_to(cur, (nd,) + cur.shape))  # every row: the current poses
    q, q0, q1, P, S = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (qh, q0h, q1h, Ph, same))
    d = [torch.zeros(nd, dtype=torch.float64, device=dev) for _ in range(2)]
    p = [torch.zeros(nd, dtype=torch.int32, device=dev) for _ in range(2)]
    valid = torch.zeros(ne, dtype=torch.uint8, device=dev)
    first, segs = (torch.zeros(ne, dtype=torch.int32, device=dev) for _ in range(2))
    s = torch.cuda.current_stream().cuda_stream
    so2, extent = wm.get_motion_space()
    L, h, vp = C.lib(), ctypes.c_void_p(wm.device_handle()), ctypes.c_void_p

    def distance(rows, P=P):
        kw = dict(object_poses_ptr=P.data_ptr(), object_pose_rows=rows) if rows else {}
        return lambda: wm.distance_batch_device(q.data_ptr(), nd, d[0].data_ptr(), p[0].data_ptr(), d[1].data_ptr(),
                                                p[1].data_ptr(), stream=s, **kw)

    def motion(rows, P=P):
        tail = (ne, so2, 0.01 * extent, vp(valid.data_ptr()), vp(first.data_ptr()), vp(segs.data_ptr()),
                C.MPG_MEM_DEVICE, vp(s))
        if rows:
            return lambda: C.check(L.mpg_check_motion_batch_free(h, vp(q0.data_ptr()), vp(q1.data_ptr()),
                                                                 vp(P.data_ptr()), rows, *tail))
        return lambda: C.check(L.mpg_check_motion_batch(h, vp(q0.data_ptr()), vp(q1.data_ptr()), *tail))

    op = {name: Ph[:, k] for k, name in enumerate(MOVABLE)}
    ope = {name: Ph[:ne, k] for k, name in enumerate(MOVABLE)}
    runs = [("distance_current", distance(0)), ("motion_current", motion(0)),
            ("distance_host_current", lambda: wm.distance_batch(qh)),
            ("motion_host_current", lambda: wm.check_motion_batch(q0h, q1h))]
    if not args.current_only:
        runs += [("distance_per_row_same", distance(nd, S)), ("motion_per_row_same", motion(ne, S)),
                 ("distance_per_row", distance(nd)), ("motion_per_row", motion(ne)),
                 ("distance_host_per_row", lambda: wm.distance_batch(qh, object_poses=op)),
                 ("motion_host_per_row", lambda: wm.check_motion_batch(q0h, q1h, object_poses=ope))]
    out = {"states": nd, "edges": ne, "steps": args.steps, "unit": "s per call (median)",
           "pose_bytes_per_row": len(MOVABLE) * 7 * 8}
    for key, fn in runs:
        out[key] = timed(fn, args.steps, args.warmup)
        if key.startswith("motion") and "host" not in key:
            out[key + "_states"] = int(segs.sum().item())
            out[key + "_valid_rate"] = float(valid.float().mean().item())
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--queries", action="store_true", help="time distance and motion validation instead")
    ap.add_argument("--current-only", action="store_true", help="with --queries: no per-row variants")
    args = ap.parse_args()
    if args.queries:
        return queries(args)
    n = args.n
    dev = torch.device("cuda", 0)
    ws, art = scenes.world(3)
    wm, _ = scenes.world(3)
    for name in MOVABLE:
        wm.set_normal_object_movable(name)
    q = torch.from_numpy(scenes.sample_states(art, n, scenes.CFG_SEED[3])).to(dev)
    P = poses(n)
    per_row = torch.from_numpy(P).to(dev)
    shared = torch.from_numpy(P[0].copy()).to(dev)
    park = P[0].copy()
    park[:, :3] = (0.0, 0.0, -10.0)
    parked = torch.from_numpy(park).to(dev)
    flags = torch.zeros(n, dtype=torch.uint8, device=dev)
    masks = torch.zeros((n, ws.get_mask_words()), dtype=torch.int32, device=dev)
    s = torch.cuda.current_stream().cuda_stream

    def run(w, pose=None, rows=0):
        return lambda: w.collide_batch_device(q.data_ptr(), n, flags.data_ptr(), masks.data_ptr(), s,
                                              pose.data_ptr() if pose is not None else 0, rows)

    out = {"n": n, "steps": args.steps, "unit": "configs/s", "pose_bytes_per_row": len(MOVABLE) * 7 * 8,
           "q_bytes_per_row": int(q.shape[1]) * 8}
    rate = {}
    for key, fn in (("static", run(ws)), ("per_row", run(wm, per_row, n)), ("shared", run(wm, shared, 1)),
                    ("parked", run(wm, parked, 1))):
        rate[key] = n / timed(fn, args.steps, args.warmup)
        out[key] = rate[key]
        out[key + "_collision_rate"] = float(flags.float().mean().item())
    for key in ("per_row", "shared", "parked"):
        out[key + "_over_static"] = rate[key] / rate["static"]
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
