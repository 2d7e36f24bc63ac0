"""Batched state-validity checking through the C ABI (include/mpgpu.h).

``DeviceWorld`` owns one immutable device snapshot (``mpg_world``) built from
a plain-array world description and evaluates ``collide()`` /
``collideFull()`` for a whole batch of joint configurations in one launch.
Inputs may be host numpy arrays (copied through staging buffers) or device
tensors (any object exposing ``data_ptr()``, e.g. a torch tensor on the
world's device; the launch is enqueued on the given stream and not
synchronised).  A descriptor may hold free frames (``link_parent`` =
``_capi.LINK_FREE``): the poses of the movable objects on them are inputs --
``set_free_poses`` and ``collide_batch(..., free_pose=...)``.

Reference semantics: ``flags[i] == PlanningWorld.collide()`` after
``set_qpos_all(q[i])`` (src/planning_world.h:248-250, cpp:250-262), and bit p
of ``pair_mask[i]`` is set iff pair p is in ``collide_full()``'s result
(src/planning_world.cpp:484-490, ACM-filtered by :265-274).
"""
from __future__ import annotations

import ctypes
from typing import Dict, Optional

import numpy as np

from . import _capi as C

_DESC_INT_FIELDS = ["joint_type", "joint_parent", "joint_q_source", "link_parent", "geom_type",
                    "geom_vertex_start", "geom_vertex_count", "moving_link", "moving_geom", "static_geom",
                    "pair_a", "pair_b"]
_DESC_F64_FIELDS = ["joint_axis", "joint_placement", "joint_q_const", "link_placement", "geom_param",
                    "vertices", "moving_offset", "static_transform"]


class DeviceWorld:
    """An ``mpg_world`` snapshot on one device."""

    def __init__(self, arrays: Dict[str, np.ndarray], device: int = 0, gjk_tolerance: float = 1e-6,
                 gjk_solver: int = C.GJK_LIBCCD):
        L = C.lib()
        self._keep = []

        def ip(name):
            a = np.ascontiguousarray(np.asarray(arrays[name], dtype=np.int32).reshape(-1))
            if a.size == 0:
                a = np.zeros(1, np.int32)
            self._keep.append(a)
            return a.ctypes.data_as(C._I32P)

        def fp(name):
            a = np.ascontiguousarray(np.asarray(arrays[name], dtype=np.float64).reshape(-1))
            if a.size == 0:
                a = np.zeros(1, np.float64)
            self._keep.append(a)
            return a.ctypes.data_as(C._F64P)

        d = C.WorldDesc()
        d.n_joints = len(arrays["joint_type"])
        d.dof = int(arrays["dof"])
        d.n_links = len(arrays["link_parent"])
        d.n_geoms = len(arrays["geom_type"])
        d.n_vertices = int(np.asarray(arrays["vertices"]).size // 3)
        d.n_moving = len(arrays["moving_link"])
        d.n_static = len(arrays["static_geom"])
        d.n_pairs = len(arrays["pair_a"])
        for f in _DESC_INT_FIELDS:
            setattr(d, f, ip(f))
        for f in _DESC_F64_FIELDS:
            setattr(d, f, fp(f))
        al = np.ascontiguousarray(np.asarray(arrays["pair_allowed"], dtype=np.uint8).reshape(-1))
        if al.size == 0:
            al = np.zeros(1, np.uint8)
        self._keep.append(al)
        d.pair_allowed = al.ctypes.data_as(C._U8P)
        d.gjk_tolerance = gjk_tolerance
        d.gjk_solver = int(gjk_solver)
        leaves = np.ascontiguousarray(np.asarray(arrays.get("octree_leaf", np.zeros(0)), dtype=np.float64).reshape(-1))
        d.n_octree_leaves = leaves.size // 6
        if leaves.size == 0:
            leaves = np.zeros(6)
        self._keep.append(leaves)
        d.octree_leaf = leaves.ctypes.data_as(C._F64P)
        tris = np.ascontiguousarray(np.asarray(arrays.get("mesh_triangle", np.zeros(0)), dtype=np.int32).reshape(-1))
        d.n_mesh_triangles = tris.size // 3
        if tris.size == 0:
            tris = np.zeros(3, np.int32)
        self._keep.append(tris)
        d.mesh_triangle = tris.ctypes.data_as(C._I32P)
        faces = np.ascontiguousarray(np.asarray(arrays.get("convex_face", np.zeros(0)), dtype=np.int32).reshape(-1))
        d.n_convex_face_ints = faces.size
        if faces.size == 0:
            faces = np.zeros(1, np.int32)
        self._keep.append(faces)
        d.convex_face = faces.ctypes.data_as(C._I32P)
        for f in ("joint_lower", "joint_upper"):  # optional: NULL = unbounded
            if f in arrays and arrays[f] is not None:
                a = np.ascontiguousarray(np.asarray(arrays[f], dtype=np.float64).reshape(-1))
                self._keep.append(a)
                setattr(d, f, a.ctypes.data_as(C._F64P))
        h = ctypes.c_void_p()
        C.check(L.mpg_world_create(ctypes.byref(d), device, ctypes.byref(h)), "mpg_world_create")
        self._keep = []
        self._h = h
        info = C.WorldInfo()
        C.check(L.mpg_world_get_info(h, ctypes.byref(info)), "mpg_world_get_info")
        self.n_pairs = info.n_pairs
        self.mask_words = info.mask_words
        self.dof = info.dof
        self.n_links = info.n_links
        self.device = info.device
        self.block_size = info.block_size
        nf, far = ctypes.c_int32(0), ctypes.c_double(0.0)
        C.check(L.mpg_world_get_free_info(h, ctypes.byref(nf), ctypes.byref(far), None), "mpg_world_get_free_info")
        self.n_free = nf.value          # free frames: the trailing user links (movable objects)
        self.far_radius = far.value     # the cull's far-test radius (0 without free frames)

    def close(self):
        if getattr(self, "_h", None):
            C.lib().mpg_world_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    def set_small_batch_max(self, n: int):
        """Host batches of at most n configurations take the one-launch latency path (0 disables)."""
        C.check(C.lib().mpg_set_small_batch_max(self._h, int(n)), "mpg_set_small_batch_max")

    def cull_grid_info(self) -> dict:
        """The cull's lookup grids (mpg_cull_grid_info): ``objects`` (moving
        object ids), ``partners`` per object, ``box`` [objects, 6] (lo, hi),
        ``cells``, ``cell_edge`` and ``built`` (the first bulk call builds them)."""
        n, cells, built = ctypes.c_int32(0), ctypes.c_int64(0), ctypes.c_int32(0)
        edge = ctypes.c_double(0.0)
        L = C.lib()
        C.check(L.mpg_cull_grid_info(self._h, ctypes.byref(n), ctypes.byref(cells), ctypes.byref(built),
                                     ctypes.byref(edge), 0, None, None, None), "mpg_cull_grid_info")
        obj = np.zeros(n.value, np.int32)
        part = np.zeros(n.value, np.int32)
        box = np.zeros((n.value, 6))
        C.check(L.mpg_cull_grid_info(self._h, None, None, None, None, n.value, obj.ctypes.data_as(ctypes.c_void_p),
                                     part.ctypes.data_as(ctypes.c_void_p), box.ctypes.data_as(ctypes.c_void_p)),
                "mpg_cull_grid_info")
        return dict(objects=obj, partners=part, box=box, cells=cells.value, cell_edge=edge.value, built=bool(built.value))

    def task_plan_info(self, stream: Optional[int] = None) -> dict:
        """The narrow-phase task list of the last bulk collide call on
        ``stream`` (mpg_debug_task_plan; synchronises the stream): ``tasks``,
        ``task_size`` (first level), ``levels`` in use and ``candidates``."""
        t, c = ctypes.c_int64(0), ctypes.c_int64(0)
        ts, lv = ctypes.c_int32(0), ctypes.c_int32(0)
        C.check(C.lib().mpg_debug_task_plan(self._h, ctypes.c_void_p(stream or 0), ctypes.byref(t), ctypes.byref(ts),
                                            ctypes.byref(lv), ctypes.byref(c)), "mpg_debug_task_plan")
        return dict(tasks=t.value, task_size=ts.value, levels=lv.value, candidates=c.value)

    def release_stream(self, stream: int):
        """Drop the workspace / side stream kept for a caller stream (call before destroying it)."""
        C.check(C.lib().mpg_release_stream(self._h, ctypes.c_void_p(int(stream))), "mpg_release_stream")

    # ------------------------------------------------------------------
    def collide_batch(self, q, flags=None, pair_mask=None, stream: Optional[int] = None, free_pose=None):
        """Host path (numpy): returns (flags[n] u8, pair_mask[n, W] u32).
        Device path (tensors with data_ptr()): fills the given device buffers
        on ``stream`` and returns them without synchronising.
        ``free_pose``: the free frames' poses for this call, ``[n, n_free, 7]``
        (one set per configuration) or ``[n_free, 7]`` (shared), in the same
        memory as ``q`` (mpg_collide_batch_free); None: the current poses."""
        if hasattr(q, "data_ptr"):
            n = q.shape[0] if q.dim() > 1 else q.numel() // self.dof
            if flags is None:
                raise ValueError("device path needs preallocated flags (and optionally pair_mask)")
            mk = ctypes.c_void_p(pair_mask.data_ptr() if pair_mask is not None else 0)
            if free_pose is not None:
                rows = self._free_rows(free_pose.numel(), n)
                C.check(C.lib().mpg_collide_batch_free(self._h, ctypes.c_void_p(q.data_ptr()),
                                                       ctypes.c_void_p(free_pose.data_ptr()), rows, n,
                                                       ctypes.c_void_p(flags.data_ptr()), mk, C.MPG_MEM_DEVICE,
                                                       ctypes.c_void_p(stream or 0)), "mpg_collide_batch_free")
                return flags, pair_mask
            C.check(C.lib().mpg_collide_batch(self._h, ctypes.c_void_p(q.data_ptr()), n,
                                              ctypes.c_void_p(flags.data_ptr()), mk,
                                              C.MPG_MEM_DEVICE, ctypes.c_void_p(stream or 0)), "mpg_collide_batch")
            return flags, pair_mask
        qa = np.ascontiguousarray(np.asarray(q, dtype=np.float64)).reshape(-1, self.dof)
        n = qa.shape[0]
        fl = np.zeros(n, np.uint8)
        pm = np.zeros((n, self.mask_words), np.uint32)
        if free_pose is not None:
            fp = np.ascontiguousarray(np.asarray(free_pose, dtype=np.float64))
            rows = self._free_rows(fp.size, n)
            C.check(C.lib().mpg_collide_batch_free(self._h, qa.ctypes.data_as(ctypes.c_void_p),
                                                   fp.ctypes.data_as(ctypes.c_void_p), rows, n,
                                                   fl.ctypes.data_as(ctypes.c_void_p), pm.ctypes.data_as(ctypes.c_void_p),
                                                   C.MPG_MEM_HOST, ctypes.c_void_p(stream or 0)),
                    "mpg_collide_batch_free")
            return fl, pm
        C.check(C.lib().mpg_collide_batch(self._h, qa.ctypes.data_as(ctypes.c_void_p), n,
                                          fl.ctypes.data_as(ctypes.c_void_p), pm.ctypes.data_as(ctypes.c_void_p),
                                          C.MPG_MEM_HOST, ctypes.c_void_p(stream or 0)), "mpg_collide_batch")
        return fl, pm

    def _free_rows(self, size: int, n: int) -> int:
        per = self.n_free * 7
        if per == 0:
            raise ValueError("the world has no free frames")
        if size == per:
            return 1
        if size == per * n:
            return n
        raise ValueError(f"free_pose must hold [{self.n_free}, 7] or [{n}, {self.n_free}, 7] values")

    def set_free_poses(self, pose7):
        """Replace the world's current free poses, ``[n_free, 7]`` (p, wxyz):
        every entry point uses them afterwards; nothing is rebuilt.  Not
        concurrent with other calls on this world (mpg_world_set_free_poses)."""
        p = np.ascontiguousarray(np.asarray(pose7, dtype=np.float64))
        if p.size != self.n_free * 7 or self.n_free == 0:
            raise ValueError(f"pose7 must hold [{self.n_free}, 7] values (the world's free frames)")
        C.check(C.lib().mpg_world_set_free_poses(self._h, p.ctypes.data_as(ctypes.c_void_p)),
                "mpg_world_set_free_poses")

    def free_poses(self) -> np.ndarray:
        """The current free poses, ``[n_free, 7]``."""
        out = np.zeros((self.n_free, 7))
        C.check(C.lib().mpg_world_get_free_info(self._h, None, None, out.ctypes.data_as(ctypes.c_void_p)),
                "mpg_world_get_free_info")
        return out

    def debug_collide_pairs(self, geom_a: int, geom_b: int, Ta, Tb) -> np.ndarray:
        """Narrow phase only: fcl::collide(geometry geom_a at Ta[i], geom_b at
        Tb[i]) (SE3 rows of 12 doubles) -> uint8 hits (mpg_debug_collide_pairs)."""
        A = np.ascontiguousarray(Ta, dtype=np.float64).reshape(-1, 12)
        B = np.ascontiguousarray(Tb, dtype=np.float64).reshape(-1, 12)
        n = len(A)
        hit = np.zeros(n, np.uint8)
        C.check(C.lib().mpg_debug_collide_pairs(self._h, int(geom_a), int(geom_b), n, A.ctypes.data_as(ctypes.c_void_p),
                                                B.ctypes.data_as(ctypes.c_void_p), hit.ctypes.data_as(ctypes.c_void_p)),
                "mpg_debug_collide_pairs")
        return hit

    def fk_batch(self, q) -> np.ndarray:
        """[n, n_links, 7] link poses (p, wxyz) -- getLinkPose for every user link."""
        qa = np.ascontiguousarray(np.asarray(q, dtype=np.float64)).reshape(-1, self.dof)
        n = qa.shape[0]
        out = np.zeros((n, self.n_links, 7))
        C.check(C.lib().mpg_fk_batch(self._h, qa.ctypes.data_as(ctypes.c_void_p), n,
                                     out.ctypes.data_as(ctypes.c_void_p), C.MPG_MEM_HOST, None), "mpg_fk_batch")
        return out

    def ik_batch(self, link: int, goal_poses, *, start_qpos=None, q_init=None, n_init_qpos: int = 20, mask=None,
                 seed: int = 0, eps: float = 1e-5, max_iter: int = 1000, dt: float = 0.1, damp: float = 1e-12,
                 threshold: float = 1e-3, max_waves: int = 0, out=None, stream: Optional[int] = None):
        """Planner.IK's loop for every goal pose of world link ``link`` in one
        call (mpg_ik_batch): per (goal, seed) row the closed-loop IK, the
        joint-limit wrap, ``collide()`` and the distance_6D threshold.
        Host path (numpy ``goal_poses`` (7,) / [M, 7]; ``q_init`` [M, S, dof]
        or None: ``n_init_qpos`` seeds per goal drawn on the device, seed 0 =
        ``start_qpos``): returns (q [M, S, dof], status [M, S] u8 of
        ``_capi.MPG_IK_*`` bits, err [M, S, 6], iters [M, S] i32).
        Device path (tensors with data_ptr(); ``q_init`` [M, S, dof] or None
        with ``n_init_qpos``): ``out`` = (q, status, err or None, iters or
        None) preallocated tensors, filled on ``stream`` without
        synchronising and returned.  ``mask`` is always a host array."""
        o = C.IkOptions(eps, int(max_iter), dt, damp, threshold, None, int(seed), int(max_waves))
        mk = None
        if mask is not None:
            mk = np.ascontiguousarray(np.asarray(mask, dtype=bool).reshape(-1)).astype(np.uint8)
            if mk.size != self.dof:
                raise ValueError(f"mask must hold {self.dof} values")
            o.mask = mk.ctypes.data
        P = ctypes.c_void_p
        if hasattr(goal_poses, "data_ptr"):
            M = goal_poses.numel() // 7
            S = int(n_init_qpos) if q_init is None else (q_init.numel() // max(self.dof, 1)) // max(M, 1)
            if out is None:
                raise ValueError("device path needs out=(q, status, err, iters) preallocated")
            q, status, err, iters = out
            ptr = lambda t: P(t.data_ptr() if t is not None else 0)  # noqa: E731
            C.check(C.lib().mpg_ik_batch(self._h, int(link), ptr(goal_poses), M, S, ptr(q_init), ptr(start_qpos),
                                         ctypes.byref(o), ptr(q), ptr(status), ptr(err), ptr(iters), C.MPG_MEM_DEVICE,
                                         P(stream or 0)), "mpg_ik_batch")
            return out
        g = np.ascontiguousarray(np.asarray(goal_poses, dtype=np.float64)).reshape(-1, 7)
        M = g.shape[0]
        qi = qs = None
        S = int(n_init_qpos)
        if q_init is not None:
            qi = np.ascontiguousarray(np.asarray(q_init, dtype=np.float64))
            if M == 0 or qi.size % (M * max(self.dof, 1)):
                raise ValueError(f"q_init must be [{M}, S, {self.dof}]")
            S = qi.size // (M * max(self.dof, 1))
        if start_qpos is not None:
            qs = np.ascontiguousarray(np.asarray(start_qpos, dtype=np.float64).reshape(-1))
            if qs.size != self.dof:
                raise ValueError(f"start_qpos must hold {self.dof} values")
        q = np.zeros((M, S, self.dof))
        status = np.zeros((M, S), np.uint8)
        err = np.zeros((M, S, 6))
        iters = np.zeros((M, S), np.int32)
        hp = lambda a: P(a.ctypes.data if a is not None else 0)  # noqa: E731
        C.check(C.lib().mpg_ik_batch(self._h, int(link), hp(g), M, S, hp(qi), hp(qs), ctypes.byref(o), hp(q),
                                     hp(status), hp(err), hp(iters), C.MPG_MEM_HOST, P(stream or 0)), "mpg_ik_batch")
        return q, status, err, iters

    def screw_batch(self, link: int, goal_poses, start_qpos, *, qpos_step: float = 0.1, max_waypoints: int = 64,
                    first_hit: bool = True, out=None, stream: Optional[int] = None):
        """Planner.plan_screw's loop for every (goal pose, start state) row of
        world link ``link`` in one call (mpg_screw_batch): the joint-space
        waypoints of the straight-line screw motion, then one ``collide()``
        pass over them.
        Host path (numpy ``goal_poses`` (7,) / [n, 7]; ``start_qpos`` (dof,)
        for every row, or [n, dof]): returns (path [n, max_waypoints, dof],
        n_waypoints [n] i32, status [n] u8 of ``_capi.MPG_SCREW_*`` bits,
        first_hit [n] i32 or None).  The slots of ``path`` past a row's count
        repeat its last waypoint.
        Device path (tensors with data_ptr(); ``goal_poses`` [n, 7],
        ``start_qpos`` [n, dof]): ``out`` = (path, n_waypoints, status,
        first_hit or None) preallocated tensors, filled on ``stream`` without
        synchronising and returned."""
        o = C.ScrewOptions(float(qpos_step), int(max_waypoints))
        P = ctypes.c_void_p
        if hasattr(goal_poses, "data_ptr"):
            n = goal_poses.numel() // 7
            if out is None:
                raise ValueError("device path needs out=(path, n_waypoints, status, first_hit) preallocated")
            if start_qpos.numel() != n * self.dof:
                raise ValueError(f"start_qpos must be [{n}, {self.dof}]")
            path, count, status, hit = out
            ptr = lambda t: P(t.data_ptr() if t is not None else 0)  # noqa: E731
            C.check(C.lib().mpg_screw_batch(self._h, int(link), ptr(goal_poses), ptr(start_qpos), n, ctypes.byref(o),
                                            ptr(path), ptr(count), ptr(status), ptr(hit), C.MPG_MEM_DEVICE,
                                            P(stream or 0)), "mpg_screw_batch")
            return out
        g = np.ascontiguousarray(np.asarray(goal_poses, dtype=np.float64)).reshape(-1, 7)
        n = g.shape[0]
        qs = np.asarray(start_qpos, dtype=np.float64)
        if qs.ndim == 1 and qs.size == self.dof:
            qs = np.broadcast_to(qs, (n, self.dof))
        if qs.shape != (n, self.dof):
            raise ValueError(f"start_qpos must be ({self.dof},) or [{n}, {self.dof}]")
        qs = np.ascontiguousarray(qs)
        mw = max(int(max_waypoints), 0)
        path = np.zeros((n, mw, self.dof))
        count = np.zeros(n, np.int32)
        status = np.zeros(n, np.uint8)
        hit = np.full(n, -1, np.int32) if first_hit else None
        hp = lambda a: P(a.ctypes.data if a is not None else 0)  # noqa: E731
        C.check(C.lib().mpg_screw_batch(self._h, int(link), hp(g), hp(qs), n, ctypes.byref(o), hp(path), hp(count),
                                        hp(status), hp(hit), C.MPG_MEM_HOST, P(stream or 0)), "mpg_screw_batch")
        return path, count, status, hit

    def plan_batch(self, start_qpos, goal_qpos, *, range: float = 0.0, max_rounds: int = 20000, max_nodes: int = 2048,
                   max_waypoints: int = 256, seed: int = 0, row_seed=None, check_every: int = 8, so2_mask: int = 0,
                   out=None, stream: Optional[int] = None):
        """Planner.plan's RRTConnect for every (start state, goal states) row
        in one call (mpg_plan_batch): the rows advance in lockstep, one
        growTree per row and round, all their motion states in one
        ``collide()`` pass per round.  ``so2_mask``: bit d marks state slot d
        as an SO2 (continuous) joint; the other slots use the descriptor's
        joint limits.
        Host path (numpy ``start_qpos`` (dof,) for every row, or [Q, dof];
        ``goal_qpos`` [Q, dof] or [Q, G, dof]; ``row_seed`` [Q] uint64 or
        None): returns (path [Q, max_waypoints, dof], n_waypoints [Q] i32,
        status [Q] u8 of ``_capi.MPG_PLAN_*`` bits, iterations [Q] i32,
        tree_sizes [Q, 2] i32).  The slots of ``path`` past a row's count
        repeat its last waypoint.
        Device path (tensors with data_ptr(); ``start_qpos`` [Q, dof],
        ``goal_qpos`` [Q, G, dof]): ``out`` = (path, n_waypoints, status,
        iterations or None, tree_sizes or None) preallocated tensors, filled
        on ``stream`` and returned.  The host decides when to stop, so the
        call synchronises ``stream`` once per ``check_every`` rounds and once
        at the end."""
        o = C.PlanOptions(float(range), int(max_rounds), int(max_nodes), int(max_waypoints), int(check_every),
                          int(seed), int(so2_mask))
        P = ctypes.c_void_p
        dof = max(self.dof, 1)
        if hasattr(start_qpos, "data_ptr"):
            Q = start_qpos.numel() // dof
            if out is None:
                raise ValueError("device path needs out=(path, n_waypoints, status, iterations, tree_sizes) preallocated")
            if Q == 0 or goal_qpos.numel() % (Q * dof):
                raise ValueError(f"goal_qpos must be [{Q}, G, {self.dof}]")
            G = goal_qpos.numel() // (Q * dof)
            path, count, status, iters, sizes = out
            ptr = lambda t: P(t.data_ptr() if t is not None else 0)  # noqa: E731
            C.check(C.lib().mpg_plan_batch(self._h, ptr(start_qpos), ptr(goal_qpos), Q, G, ptr(row_seed),
                                           ctypes.byref(o), ptr(path), ptr(count), ptr(status), ptr(iters), ptr(sizes),
                                           C.MPG_MEM_DEVICE, P(stream or 0)), "mpg_plan_batch")
            return out
        g = np.asarray(goal_qpos, dtype=np.float64)
        if g.ndim == 2:
            g = g[:, None, :]
        if g.ndim != 3 or g.shape[2] != self.dof:
            raise ValueError(f"goal_qpos must be [Q, {self.dof}] or [Q, G, {self.dof}]")
        g = np.ascontiguousarray(g)
        Q, G = g.shape[0], g.shape[1]
        qs = np.asarray(start_qpos, dtype=np.float64)
        if qs.ndim == 1 and qs.size == self.dof:
            qs = np.broadcast_to(qs, (Q, self.dof))
        if qs.shape != (Q, self.dof):
            raise ValueError(f"start_qpos must be ({self.dof},) or [{Q}, {self.dof}]")
        qs = np.ascontiguousarray(qs)
        rs = None
        if row_seed is not None:
            rs = np.ascontiguousarray(np.asarray(row_seed, dtype=np.uint64).reshape(-1))
            if rs.size != Q:
                raise ValueError(f"row_seed must hold {Q} values")
        path = np.zeros((Q, max(int(max_waypoints), 0), self.dof))
        count = np.zeros(Q, np.int32)
        status = np.zeros(Q, np.uint8)
        iters = np.zeros(Q, np.int32)
        sizes = np.zeros((Q, 2), np.int32)
        hp = lambda a: P(a.ctypes.data if a is not None else 0)  # noqa: E731
        C.check(C.lib().mpg_plan_batch(self._h, hp(qs), hp(g), Q, G, hp(rs), ctypes.byref(o), hp(path), hp(count),
                                       hp(status), hp(iters), hp(sizes), C.MPG_MEM_HOST, P(stream or 0)),
                "mpg_plan_batch")
        return path, count, status, iters, sizes

    def _topp_sizes(self, max_waypoints, grid_per_segment, min_grid, max_samples):
        """Refuses what would size the outputs wrongly; returns Ncap."""
        if not 2 <= int(max_waypoints) <= 4096:
            raise ValueError("max_waypoints outside [2, 4096]")
        if not 1 <= int(grid_per_segment) <= 64 or not 2 <= int(min_grid) <= 65536:
            raise ValueError("grid_per_segment outside [1, 64] or min_grid outside [2, 65536]")
        if not 1 <= int(max_samples) <= 65536:
            raise ValueError("max_samples outside [1, 65536]")
        return max(int(min_grid), int(grid_per_segment) * (int(max_waypoints) - 1))

    def topp_batch(self, path, n_waypoints, vel_limits, acc_limits, *, step: float = 0.1, grid_per_segment: int = 8,
                   min_grid: int = 100, max_samples: int = 256, return_grid: bool = False,
                   stream: Optional[int] = None):
        """Planner.TOPP for every row of ``path`` [rows, max_waypoints, dof]
        (numpy; the layout screw_batch / plan_batch return, ``n_waypoints``
        [rows] the rows' counts) in one call (mpg_topp_batch): a cubic spline
        through the waypoints, TOPP-RA under ``vel_limits`` / ``acc_limits``
        [dof], samples every ``step``.  Returns (times [rows, max_samples],
        position, velocity, acceleration [rows, max_samples, dof], n_samples
        [rows] i32, duration [rows], status [rows] u8 of ``_capi.MPG_TOPP_*``
        bits) and, with ``return_grid``, (grid_x, grid_t) [rows, Ncap + 1]: the
        profile sdot^2 and the time at the gridpoints.  Sample slots past a
        row's n_samples repeat its last sample."""
        p = np.ascontiguousarray(np.asarray(path, dtype=np.float64))
        if p.ndim != 3 or p.shape[2] != self.dof:
            raise ValueError(f"path must be [rows, max_waypoints, {self.dof}]")
        rows, mw = p.shape[0], p.shape[1]
        cnt = np.ascontiguousarray(np.asarray(n_waypoints, dtype=np.int32).reshape(-1))
        if cnt.size != rows:
            raise ValueError(f"n_waypoints must hold {rows} values")
        ncap = self._topp_sizes(mw, grid_per_segment, min_grid, max_samples)
        vel, acc = self._topp_limits(vel_limits, acc_limits)
        o = C.ToppOptions(float(step), int(grid_per_segment), int(min_grid), int(max_samples))
        ms = int(max_samples)
        times = np.zeros((rows, ms))
        pos, velo, accel = (np.zeros((rows, ms, self.dof)) for _ in range(3))
        ns = np.zeros(rows, np.int32)
        dur = np.zeros(rows)
        status = np.zeros(rows, np.uint8)
        gx, gt = (np.zeros((rows, ncap + 1)), np.zeros((rows, ncap + 1))) if return_grid else (None, None)
        P = ctypes.c_void_p
        hp = lambda a: P(a.ctypes.data if a is not None else 0)  # noqa: E731
        C.check(C.lib().mpg_topp_batch(self._h, hp(p), hp(cnt), rows, mw, hp(vel), hp(acc), ctypes.byref(o), hp(times),
                                       hp(pos), hp(velo), hp(accel), hp(ns), hp(dur), hp(status), hp(gx), hp(gt),
                                       C.MPG_MEM_HOST, P(stream or 0)), "mpg_topp_batch")
        out = (times, pos, velo, accel, ns, dur, status)
        return out + (gx, gt) if return_grid else out

    def _topp_limits(self, vel_limits, acc_limits):
        vel = np.ascontiguousarray(np.asarray(vel_limits, dtype=np.float64).reshape(-1))
        acc = np.ascontiguousarray(np.asarray(acc_limits, dtype=np.float64).reshape(-1))
        if vel.size != self.dof or acc.size != self.dof:
            raise ValueError(f"vel_limits and acc_limits must hold {self.dof} values")
        return vel, acc

    def topp_batch_device(self, path, n_waypoints, vel_limits, acc_limits, *, step: float = 0.1,
                          grid_per_segment: int = 8, min_grid: int = 100, max_samples: int = 256,
                          return_grid: bool = False, out=None, stream: Optional[int] = None):
        """``topp_batch`` on torch tensors of the world's device: ``path``
        [rows, max_waypoints, dof] float64 and ``n_waypoints`` [rows] int32 as
        ``screw_batch`` / ``plan_batch`` left them (``vel_limits`` /
        ``acc_limits`` stay host arrays).  Everything is enqueued on ``stream``
        and nothing synchronises.  ``out``: topp_batch's tuple as preallocated
        tensors (with the two grids when ``return_grid``), else they are
        allocated with torch.  Returns the tuple."""
        import torch

        if path.dim() != 3 or path.shape[2] != self.dof or not path.is_contiguous():
            raise ValueError(f"path must be a contiguous [rows, max_waypoints, {self.dof}] tensor")
        rows, mw = int(path.shape[0]), int(path.shape[1])
        if n_waypoints.numel() != rows or n_waypoints.dtype != torch.int32:
            raise ValueError(f"n_waypoints must hold {rows} int32 values")
        ncap = self._topp_sizes(mw, grid_per_segment, min_grid, max_samples)
        vel, acc = self._topp_limits(vel_limits, acc_limits)
        o = C.ToppOptions(float(step), int(grid_per_segment), int(min_grid), int(max_samples))
        ms = int(max_samples)
        if out is None:
            f64 = dict(dtype=torch.float64, device=path.device)
            out = (torch.empty((rows, ms), **f64), torch.empty((rows, ms, self.dof), **f64),
                   torch.empty((rows, ms, self.dof), **f64), torch.empty((rows, ms, self.dof), **f64),
                   torch.empty(rows, dtype=torch.int32, device=path.device), torch.empty(rows, **f64),
                   torch.empty(rows, dtype=torch.uint8, device=path.device))
            if return_grid:
                out = out + (torch.empty((rows, ncap + 1), **f64), torch.empty((rows, ncap + 1), **f64))
        if len(out) != (9 if return_grid else 7):
            raise ValueError("out must hold topp_batch's tensors")
        P = ctypes.c_void_p
        ptr = lambda t: P(t.data_ptr() if t is not None else 0)  # noqa: E731
        hp = lambda a: P(a.ctypes.data)  # noqa: E731
        gx, gt = (out[7], out[8]) if return_grid else (None, None)
        C.check(C.lib().mpg_topp_batch(self._h, ptr(path), ptr(n_waypoints), rows, mw, hp(vel), hp(acc), ctypes.byref(o),
                                       *(ptr(t) for t in out[:7]), ptr(gx), ptr(gt), C.MPG_MEM_DEVICE, P(stream or 0)),
                "mpg_topp_batch")
        return out


def device_sincos(x, device: int = 0):
    xa = np.ascontiguousarray(np.asarray(x, dtype=np.float64).reshape(-1))
    s = np.zeros_like(xa)
    c = np.zeros_like(xa)
    C.check(C.lib().mpg_debug_sincos(xa.ctypes.data_as(ctypes.c_void_p), xa.size, s.ctypes.data_as(ctypes.c_void_p),
                                     c.ctypes.data_as(ctypes.c_void_p), device), "mpg_debug_sincos")
    return s, c


def collide_batch_multi(worlds, q):
    """One host batch over several DeviceWorlds (built from the same
    descriptor, one per GPU): mpg_collide_batch_multi checks contiguous shards
    concurrently.  Returns (flags[n] u8, pair_mask[n, W] u32)."""
    worlds = list(worlds)
    if not worlds:
        raise ValueError("no worlds")
    w0 = worlds[0]
    q = np.ascontiguousarray(q, dtype=np.float64).reshape(-1, w0.dof)
    n = q.shape[0]
    flags = np.zeros(n, np.uint8)
    masks = np.zeros((n, w0.mask_words), np.uint32)
    hs = (ctypes.c_void_p * len(worlds))(*[w.handle for w in worlds])
    C.check(C.lib().mpg_collide_batch_multi(hs, len(worlds), q.ctypes.data, n, flags.ctypes.data, masks.ctypes.data),
            "mpg_collide_batch_multi")
    return flags, masks


def shard_range_c(n: int, k: int, parts: int):
    """mpg_shard_range: (start, count) of part k of n configurations."""
    start, count = ctypes.c_int64(), ctypes.c_int64()
    C.check(C.lib().mpg_shard_range(int(n), int(k), int(parts), ctypes.byref(start), ctypes.byref(count)),
            "mpg_shard_range")
    return start.value, count.value


def collide_batch_multi_device(worlds, qs, flags, masks=None, streams=None, gather_flags=None, gather_masks=None):
    """mpg_collide_batch_multi_device: shard k already on worlds[k]'s device
    (torch tensors or raw device pointers via .data_ptr()): qs[k] [count, dof]
    float64, flags[k] [count] uint8, masks[k] [count, W] int32/uint32 or None;
    streams[k] a stream handle (int) or None.  gather_flags / gather_masks:
    tensors on worlds[0]'s device receiving every shard in order.  Enqueues
    only (no synchronisation)."""
    worlds = list(worlds)
    k = len(worlds)
    handle = lambda w: w.handle if hasattr(w, "handle") else w.device_handle()  # noqa: E731  (DeviceWorld / PlanningWorld)
    if not (len(qs) == len(flags) == k) or (masks is not None and len(masks) != k):
        raise ValueError("one q / flags (/ masks) buffer per world")
    P = ctypes.c_void_p
    ptr = lambda t: P(t.data_ptr() if t is not None else 0)  # noqa: E731
    hs = (P * k)(*[handle(w) for w in worlds])
    qa = (P * k)(*[ptr(t) for t in qs])
    fa = (P * k)(*[ptr(t) for t in flags])
    ma = (P * k)(*[ptr(t) for t in masks]) if masks is not None else None
    sa = (P * k)(*[P(int(s or 0)) for s in streams]) if streams is not None else None
    counts = (ctypes.c_int64 * k)(*[int(t.shape[0]) for t in qs])
    C.check(C.lib().mpg_collide_batch_multi_device(hs, k, qa, counts, fa, ma, sa, ptr(gather_flags),
                                                   ptr(gather_masks)), "mpg_collide_batch_multi_device")
