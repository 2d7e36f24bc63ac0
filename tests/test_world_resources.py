"""The buffers, streams and events an mpg_world owns (mplib_amd/csrc/mpg_devbuf.h,
mpg_world.h): they grow in place while the world is used, per-stream state is
evicted and rebuilt, and a destroyed world gives everything back.

Two worlds: the cfg3 world with the four movable objects of
test_movable_objects (free frames: free_stage, Workspace::links, Dist::links /
fp, Motion::fp / row_of) and the plain cfg3 world (latency server, latency
path, host pipeline).  Every result is compared bit for bit with a fresh world
that sees only that one call, or with the CPU oracle.
"""
import ctypes
import functools

import numpy as np
import pytest

import worlds as Wd
from mplib_amd import _capi as C
from mplib_amd import pymp, scenes
from mplib_amd.batch import DeviceWorld
from test_movable_objects import MOVABLE, art, free_desc, gen_poses, movable_world
from test_movable_queries import poses_of

pytestmark = pytest.mark.gpu

KINDS = ("free", "static")
ROWS = (3, 200, 1500, 5000, 3)  # server / latency path / host pipeline at small_batch_max 1024, then small again
EDGES = (5, 200, 5)
HOST_ROWS = (3, 200, 3)  # fk, IK, screw: their host staging grows once, then is reused while larger than needed
HAND = "panda_hand"
N_MAX = max(ROWS)


# ---------------------------------------------------------------------------
# inputs, worlds, buffers
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def inputs(kind):
    """(q [N_MAX, 7], P [N_MAX, 4, 7] or None)."""
    if kind == "free":
        out = (Wd.sample_q(art(), N_MAX, 11), gen_poses(N_MAX))
    else:
        out = (scenes.sample_states(scenes.world(3)[1], N_MAX, 616), None)
    for a in out:
        if a is not None:
            a.setflags(write=False)
    return out


def make(kind):
    return movable_world()[0] if kind == "free" else scenes.world(3)[0]


@functools.lru_cache(maxsize=None)
def long_lived(kind):
    """The one world of a kind that every growth test below keeps using."""
    return make(kind)


def ptr(a):
    if a is None:
        return None
    return ctypes.c_void_p(a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data)


def addr(a):
    return 0 if a is None else a.data_ptr()


def place(a, dev):
    """A contiguous numpy array, or its copy in device memory."""
    if a is None:
        return None
    a = np.ascontiguousarray(a)
    if not dev:
        return a
    import torch
    return torch.from_numpy(a if a.flags.writeable else a.copy()).cuda()


def zeros(shape, dtype, dev):
    """(uint32 device arrays are int32 tensors: the bits are what is compared)"""
    if not dev:
        return np.zeros(shape, dtype)
    import torch
    name = {"uint32": "int32", "bool": "uint8"}.get(np.dtype(dtype).name, np.dtype(dtype).name)
    return torch.zeros(shape, dtype=getattr(torch, name), device="cuda")


def back(outs, dev, dtypes):
    if dev:
        import torch
        torch.cuda.synchronize()
        outs = [o.cpu().numpy() for o in outs]
    return [o.view(dt) if o.dtype != np.dtype(dt) else o for o, dt in zip(outs, dtypes)]


def pose_rows(kind, n, shared=False):
    """(pose array or None, free_rows) for the first n rows; the shared set is
    row 1 (under row 0 an object stands in the robot's base: no valid edge)."""
    P = inputs(kind)[1]
    if P is None:
        return None, 0
    return (P[1], 1) if shared else (P[:n], n)


# ---------------------------------------------------------------------------
# one call of each family: host buffers (dev=False) or device buffers
# ---------------------------------------------------------------------------
def collide(w, kind, n, dev):
    q = inputs(kind)[0][:n]
    P, rows = pose_rows(kind, n)
    if not dev:
        return list(w.collide_batch(q, object_poses=poses_of(P) if rows else None))
    tq, tp = place(q, True), place(P, True)
    fl, mk = zeros(n, np.uint8, True), zeros((n, w.get_mask_words()), np.uint32, True)
    w.collide_batch_device(tq.data_ptr(), n, fl.data_ptr(), mk.data_ptr(), 0, addr(tp), rows)
    return back([fl, mk], True, (np.uint8, np.uint32))


def contacts(w, kind, n, dev):
    q = inputs(kind)[0][:n]
    P, rows = pose_rows(kind, n)
    n_pairs, W = len(w.get_collision_pair_info()), w.get_mask_words()
    tq, tp = place(q, dev), place(P, dev)
    outs = [zeros(n, np.uint8, dev), zeros((n, W), np.uint32, dev), zeros((n, n_pairs), np.float64, dev),
            zeros((n, n_pairs, 3), np.float64, dev), zeros((n, n_pairs, 3), np.float64, dev)]
    C.check(C.lib().mpg_collide_contacts_free(ctypes.c_void_p(w.device_handle()), ptr(tq), ptr(tp), rows, n, 0,
                                              *[ptr(o) for o in outs], C.MPG_MEM_DEVICE if dev else C.MPG_MEM_HOST,
                                              None), "mpg_collide_contacts_free")
    return back(outs, dev, (np.uint8, np.uint32, np.float64, np.float64, np.float64))


def distance(w, kind, n, dev, signed):
    q = inputs(kind)[0][:n]
    P, rows = pose_rows(kind, n)
    req = pymp.fcl.DistanceRequest(enable_signed_distance=True, enable_nearest_points=True) if signed else None
    if not dev:
        return list(w.distance_batch(q, request=req, nearest_points=signed, object_poses=poses_of(P) if rows else None))
    tq, tp = place(q, True), place(P, True)
    ds, ps, do, po = (zeros(n, dt, True) for dt in (np.float64, np.int32, np.float64, np.int32))
    pts = [zeros((n, 6), np.float64, True) for _ in range(2)] if signed else [None, None]
    w.distance_batch_device(tq.data_ptr(), n, ds.data_ptr(), ps.data_ptr(), do.data_ptr(), po.data_ptr(),
                            addr(pts[0]), addr(pts[1]), 0, req, addr(tp), rows)
    outs = [ds, ps, do, po] + (pts if signed else [])
    return back(outs, True, (np.float64, np.int32, np.float64, np.int32, np.float64, np.float64))


def motion(w, kind, n, dev, shared):
    """n edges from row e towards row N_MAX - 1 - e (a fifth of the way: inside the limits)."""
    q = inputs(kind)[0]
    q_from = q[:n]
    q_to = 0.8 * q_from + 0.2 * q[::-1][:n]
    P, rows = pose_rows(kind, n, shared)
    if not dev:
        v, f, s = w.check_motion_batch(q_from, q_to, object_poses=poses_of(P) if rows else None)
        return [np.asarray(v, bool), f, s]
    so2, extent = w.get_motion_space()
    ta, tb, tp = place(q_from, True), place(q_to, True), place(P, True)
    outs = [zeros(n, np.uint8, True), zeros(n, np.int32, True), zeros(n, np.int32, True)]
    C.check(C.lib().mpg_check_motion_batch_free(ctypes.c_void_p(w.device_handle()), ptr(ta), ptr(tb), ptr(tp), rows, n,
                                                so2, 0.01 * extent, *[ptr(o) for o in outs], C.MPG_MEM_DEVICE, None),
            "mpg_check_motion_batch_free")
    v, f, s = back(outs, True, (np.uint8, np.int32, np.int32))
    return [v.astype(bool), f, s]


def fk_rows(w, q):
    """mpg_fk_batch on host buffers: [len(q), n_links, 7]."""
    q = np.ascontiguousarray(q)
    info = C.WorldInfo()
    h = ctypes.c_void_p(w.device_handle())
    C.check(C.lib().mpg_world_get_info(h, ctypes.byref(info)), "mpg_world_get_info")
    out = np.zeros((len(q), info.n_links, 7))
    C.check(C.lib().mpg_fk_batch(h, ptr(q), len(q), ptr(out), C.MPG_MEM_HOST, None), "mpg_fk_batch")
    return out


def fk(w, kind, n):
    """Host buffers, as ik and screw below: what grows is the staging (their
    device-buffer calls are tested in test_ik_batch.py and test_screw_batch.py)."""
    return [fk_rows(w, inputs(kind)[0][:n])]


@functools.lru_cache(maxsize=None)
def hand_goals(kind):
    """[max(HOST_ROWS), 7]: the hand's pose a tenth of the way from row i to row N_MAX - 1 - i."""
    n = max(HOST_ROWS)
    q = inputs(kind)[0]
    w = make(kind)
    goals = np.ascontiguousarray(fk_rows(w, 0.9 * q[:n] + 0.1 * q[::-1][:n])[:, w.ik_link_index(HAND)])
    goals.setflags(write=False)
    return goals


def ik(w, kind, n):
    """One seed per goal, given (nothing is sampled), 5 iterations."""
    q0 = inputs(kind)[0][:n].reshape(n, 1, -1)
    return list(w.ik_batch(HAND, hand_goals(kind)[:n], q_init=q0, max_iter=5))


def screw(w, kind, n):
    return list(w.plan_screw_batch(HAND, hand_goals(kind)[:n], inputs(kind)[0][:n], max_waypoints=8))


def equal(got, want, msg):
    assert len(got) == len(want), msg
    for k, (g, r) in enumerate(zip(got, want)):
        np.testing.assert_array_equal(np.asarray(g).reshape(np.asarray(r).shape), r, err_msg=f"{msg}, output {k}")


def grow_and_compare(kind, call, sizes, what):
    """`call(world, n, dev)` on the long-lived world at each size, host then
    device buffers, against a fresh world's host-buffer call of that size."""
    w = long_lived(kind)
    ref = {}
    for n in sizes:
        if n not in ref:
            fresh = make(kind)
            ref[n] = call(fresh, n, False)
            del fresh  # a PlanningWorld destroys its mpg_world with its last reference
        for dev in (False, True):
            equal(call(w, n, dev), ref[n], f"{what}, {kind} world, n = {n}, {'device' if dev else 'host'} buffers")
    return ref


# ---------------------------------------------------------------------------
# growth in place
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_collide_buffers_grow_in_place(kind):
    """collide_batch at 3, 200, 1500, 5000 and 3 rows again on one world: each
    staging buffer and workspace is replaced at least twice, then reused while
    larger than needed.  The static world's answer is also the oracle's."""
    ref = grow_and_compare(kind, lambda w, n, dev: collide(w, kind, n, dev), ROWS, "collide_batch")
    assert 0 < int(ref[N_MAX][0].sum()) < N_MAX
    if kind == "static":
        equal(ref[N_MAX], Wd.oracle_world(3).collide_batch(inputs(kind)[0], nthreads=16), "fresh world vs oracle")


@pytest.mark.parametrize("kind", KINDS)
def test_contact_buffers_grow_in_place(kind):
    ref = grow_and_compare(kind, lambda w, n, dev: contacts(w, kind, n, dev), ROWS, "contacts")
    assert ref[N_MAX][2].any()  # some pair penetrates


@pytest.mark.parametrize("kind", KINDS)
def test_distance_buffers_grow_in_place(kind):
    """distance_batch plain at 3, 200, 1500, 3 rows and signed with nearest
    points at 3, 64, 3 rows (the EPA is the expensive part)."""
    ref = grow_and_compare(kind, lambda w, n, dev: distance(w, kind, n, dev, False), (3, 200, 1500, 3), "distance_batch")
    assert np.isfinite(ref[1500][0]).all()
    ref = grow_and_compare(kind, lambda w, n, dev: distance(w, kind, n, dev, True), (3, 64, 3), "signed distance_batch")
    assert int((ref[64][0] < 0).sum() + (ref[64][2] < 0).sum()) > 0  # a penetration depth was measured


@pytest.mark.parametrize("kind", KINDS)
def test_motion_buffers_grow_in_place(kind):
    """check_motion_batch at 5, 200 and 5 edges, with shared poses and (the
    free-frame world) with per-edge poses.  (The oracle finds 86 of the 200
    edges valid under the shared pose set.)"""
    for shared in (True, False) if kind == "free" else (True,):
        ref = grow_and_compare(kind, lambda w, n, dev: motion(w, kind, n, dev, shared), EDGES,
                               f"check_motion_batch ({'shared' if shared else 'per-edge'} poses)")
        assert 0 < int(ref[200][0].sum()) < 200


def grow_host(kind, call, what):
    """`call(world, kind, n)` on the long-lived world at HOST_ROWS, against a fresh world's call of that size."""
    w = long_lived(kind)
    ref = {}
    for n in HOST_ROWS:
        if n not in ref:
            fresh = make(kind)
            ref[n] = call(fresh, kind, n)
            del fresh
        equal(call(w, kind, n), ref[n], f"{what}, {kind} world, n = {n}")
    return ref


@pytest.mark.parametrize("kind", KINDS)
def test_fk_buffers_grow_in_place(kind):
    ref = grow_host(kind, fk, "fk_batch")
    assert np.abs(np.linalg.norm(ref[200][0][..., 3:], axis=-1) - 1.0).max() < 1e-9  # poses, not zeros


@pytest.mark.parametrize("kind", KINDS)
def test_ik_buffers_grow_in_place(kind):
    """(q, status, err, iters) of 3, 200 and 3 rows, at most 5 iterations each."""
    ref = grow_host(kind, ik, "ik_batch")
    q, status, err, iters = ref[200]
    assert q.shape == (200, 1, 7) and np.isfinite(q).all()
    assert (iters <= 5).all() and (iters > 0).any()  # the loop ran


@pytest.mark.parametrize("kind", KINDS)
def test_screw_buffers_grow_in_place(kind):
    """(path, n_waypoints, status, first_hit) of 3, 200 and 3 rows with max_waypoints = 8."""
    ref = grow_host(kind, screw, "plan_screw_batch")
    path, count, status, hit = ref[200]
    assert path.shape == (200, 8, 7) and np.isfinite(path).all()
    assert ((count >= 0) & (count <= 8)).all() and (count > 1).any()  # the loop ran


# ---------------------------------------------------------------------------
# per-stream state: eviction, rebuild, release
# ---------------------------------------------------------------------------
def test_stream_state_is_evicted_and_rebuilt():
    """collide_batch on device buffers, 64 rows, on 34 streams in turn (two
    more than the 32 whose state a world keeps), again on the first one (its
    workspace was evicted), and again on one after release_stream: the
    oracle's answer every time."""
    import torch
    ow = Wd.oracle_world(3)
    w = DeviceWorld(Wd.desc_arrays(ow))
    q = Wd.sample_q(ow.art, 64, 23)
    fo, mo = ow.collide_batch(q)
    assert 0 < int(fo.sum()) < len(q)
    tq = torch.from_numpy(q).cuda()
    streams = [torch.cuda.Stream() for _ in range(34)]
    torch.cuda.synchronize()

    def run(s):
        fl = torch.full((len(q),), 7, dtype=torch.uint8, device="cuda")
        mk = torch.full((len(q), w.mask_words), -1, dtype=torch.int32, device="cuda")
        s.wait_stream(torch.cuda.current_stream())  # the fills above
        w.collide_batch(tq, fl, mk, stream=s.cuda_stream)
        s.synchronize()
        np.testing.assert_array_equal(fl.cpu().numpy(), fo)
        np.testing.assert_array_equal(mk.cpu().numpy().view(np.uint32), mo)

    for s in streams:
        run(s)
    run(streams[0])
    w.release_stream(streams[5].cuda_stream)
    run(streams[5])
    w.release_stream(streams[5].cuda_stream)
    w.release_stream(streams[5].cuda_stream)  # nothing kept for it: a no-op
    w.close()


# ---------------------------------------------------------------------------
# create, use, destroy
# ---------------------------------------------------------------------------
def use_every_family(w, q, P):
    """One small host-buffer call per family on a DeviceWorld."""
    L, h, n = C.lib(), w.handle, len(q)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    q = np.ascontiguousarray(q)
    flags, _ = w.collide_batch(q, free_pose=P)
    w.fk_batch(q)
    fp, rows = (vp(P), len(P)) if P is not None else (None, 0)
    fl, mk = np.zeros(n, np.uint8), np.zeros((n, w.mask_words), np.uint32)
    depth, normal, pos = np.zeros((n, w.n_pairs)), np.zeros((n, w.n_pairs, 3)), np.zeros((n, w.n_pairs, 3))
    C.check(L.mpg_collide_contacts_free(h, vp(q), fp, rows, n, 0, vp(fl), vp(mk), vp(depth), vp(normal), vp(pos),
                                        C.MPG_MEM_HOST, None), "mpg_collide_contacts_free")
    np.testing.assert_array_equal(fl, flags)
    req = C.DistanceRequest(C.MPG_DISTANCE_SIGNED, 1e-6)
    ds, ps, do, po = np.zeros(n), np.zeros(n, np.int32), np.zeros(n), np.zeros(n, np.int32)
    C.check(L.mpg_distance_batch_free(h, vp(q), fp, rows, n, 0, ctypes.byref(req), vp(ds), vp(ps), None, vp(do), vp(po),
                                      None, C.MPG_MEM_HOST, None), "mpg_distance_batch_free")
    q_to = np.ascontiguousarray(0.8 * q + 0.2 * q[::-1])
    v, f, s = np.zeros(n, np.uint8), np.zeros(n, np.int32), np.zeros(n, np.int32)
    C.check(L.mpg_check_motion_batch_free(h, vp(q), vp(q_to), fp, rows, n, 0, 0.5, vp(v), vp(f), vp(s), C.MPG_MEM_HOST,
                                          None), "mpg_check_motion_batch_free")
    return flags


def test_destroyed_worlds_give_their_memory_back():
    """22 cycles of: build the free-frame and the static world, one small host
    call per family on each, close().  The device's free memory after cycle
    22 is not below the reading after cycle 2 by more than one cycle's
    footprint (read inside cycle 3 while its worlds live): a buffer leaked
    per cycle would show as about twenty footprints.  The margin is one
    footprint because other allocations of the process may settle during the
    first cycles.  numpy inputs: torch's caching allocator holds nothing.
    (Measured: a footprint of 48 MiB, and the readings after cycles 2..22
    all equal.  Creating a world takes 0.44 s, so the 44 of them take 20 s.)"""
    import torch
    ow = Wd.oracle_world(3)
    descs = (free_desc(ow, MOVABLE), Wd.desc_arrays(ow))
    n = 40
    qs = [inputs(kind)[0][:n] for kind in KINDS]
    Ps = (np.ascontiguousarray(inputs("free")[1][:n]), None)
    want = ow.collide_batch(qs[1])[0]
    free_after, alive = {}, None
    for cycle in range(1, 23):
        worlds = [DeviceWorld(d) for d in descs]
        flags = [use_every_family(w, q, P) for w, q, P in zip(worlds, qs, Ps)]
        np.testing.assert_array_equal(flags[1], want)
        if cycle == 3:
            torch.cuda.synchronize()
            alive = torch.cuda.mem_get_info()[0]
        for w in worlds:
            w.close()
        torch.cuda.synchronize()
        free_after[cycle] = torch.cuda.mem_get_info()[0]
    footprint = free_after[2] - alive
    later = [free_after[c] for c in range(2, 23)]
    print(f"free after cycle 2: {free_after[2]}, after cycle 22: {free_after[22]}, one cycle's footprint: {footprint}, "
          f"spread of the readings after cycles 2..22: {max(later) - min(later)}")
    assert footprint > 0
    assert free_after[22] >= free_after[2] - footprint, (free_after, footprint)
