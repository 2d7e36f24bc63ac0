"""GPU: mpg_screw_batch (PlanningWorld.plan_screw_batch / plan_screw_batch_device,
DeviceWorld.screw_batch, mplib_amd.planner.plan_screw) against the numpy
restatement of planner.py's plan_screw, the host build of the header the kernel
runs, the world's own collide_batch and the CPU oracle.  Inputs and references:
tests/screw_cases.py."""
import ctypes
import functools

import numpy as np
import pytest

import ik_cases as K
import screw_cases as S
import worlds as Wd
from mplib_amd import _capi as C
from mplib_amd import planner as P
from mplib_amd import scenes

pytestmark = pytest.mark.gpu

LINK = "panda_hand"
END_BITS = 0xFF & ~C.MPG_SCREW_COLLISION_FREE


@functools.lru_cache(maxsize=None)
def world_art(cfg=3):
    return scenes.world(cfg)


def world(cfg=3):
    return world_art(cfg)[0]


@functools.lru_cache(maxsize=None)
def device_s(max_waypoints=64, qpos_step=0.1):
    """Recipe S through the host path of the cfg3 world: (path, n_waypoints, status, first_hit)."""
    q0, goal = S.recipe_s()
    out = world().plan_screw_batch(LINK, goal, q0, max_waypoints=max_waypoints, qpos_step=qpos_step)
    return K._ro(*out)


@functools.lru_cache(maxsize=None)
def header_s(max_waypoints=64):
    q0, goal = S.recipe_s()
    return K._ro(*S.host_header_rows(goal, q0, max_waypoints=max_waypoints))


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_path_parity_well_conditioned(n):
    """Test 1 on the first n rows whose sigma_min(J) stays >= 1e-2 along the
    path (row counts at the wave edges): status and count equal np_plan_screw's,
    max|dq| <= 1e-9 (operation order ~1e-16 times kappa(J J^T) <= 1e4 |J|^2,
    summed over at most 24 steps).  Against the host build of mpg_screw.h:
    status and n_waypoints equal, the path within 1e-9.  It is not bit-equal on
    every row: sin and cos are the same code on both sides, but the exponential
    coordinates take one acos, and the device's differs from the host libm's
    in the last place on some arguments.  Measured: 63 of these 65 rows
    are bit-equal, the other two differ by at most 1.1e-15; the rows that take
    no acos (test_small_rotation_is_dropped) are bit-equal.  max|dq| against
    the reference: 7.8e-14."""
    q0, goal = S.recipe_s()
    idx = np.flatnonzero(S.well_rows())[:n]
    path, cnt, st, _ = world().plan_screw_batch(LINK, goal[idx], q0[idx])
    differ, dmax = S.compare_paths(st, cnt, path, rows=idx)
    print("well rows n=%d: differ %d, max|dq| %.3g" % (n, differ.sum(), dmax.max()))
    assert not differ.any()
    assert dmax.max() <= 1e-9
    hp, hc, hs = header_s()
    np.testing.assert_array_equal(cnt, hc[idx])
    np.testing.assert_array_equal(st & END_BITS, hs[idx])
    same = (path == hp[idx]).all(axis=(1, 2))
    print("bit-equal to the host build: %d of %d rows, max difference %.3g" % (same.sum(), n, np.abs(path - hp[idx]).max()))
    assert np.abs(path - hp[idx]).max() <= 1e-9


def test_path_parity_all_rows():
    """Test 1 on all 256 rows of recipe S, max_waypoints = 512 (the longest
    reference path has 262 waypoints): the bounds of test_screw_host.py.  The
    reference's own two-run figure over all 256 rows: no status or count
    differs (see there).  Measured: no row differs, max|dq| 7.8e-14 on the
    well-conditioned rows and 8.5e-8 over all; 236 of the 256 rows are
    bit-equal to the host build of the header, 14 of the other 20 differ from
    waypoint 1 on (see test_path_parity_well_conditioned)."""
    path, cnt, st, _ = device_s(512)
    rst, _, _, sig, _ = S.reference_s()
    well = sig >= S.WELL
    differ, dmax = S.compare_paths(st, cnt, path)
    print("all rows: differ %d (well %d), max|dq| well %.3g all %.3g"
          % (differ.sum(), differ[well].sum(), dmax[well].max(), dmax.max()))
    assert not differ[well].any()
    assert dmax[well].max() <= 1e-9
    assert differ.sum() <= 8
    assert not differ[rst == S.REACHED].any()
    hp, hc, hs = header_s(512)
    np.testing.assert_array_equal(cnt[well], hc[well])
    same = (path == hp).all(axis=(1, 2))
    d1 = np.abs(path[:, 1] - hp[:, 1]).max(axis=1)
    print("bit-equal to the host build: %d of %d well rows (%d of all); rows that differ at waypoint 1 already: %d of %d"
          % (same[well].sum(), well.sum(), same.sum(), ((d1 > 0) & ~same).sum(), (~same).sum()))
    assert np.abs(path[well] - hp[well]).max() <= 1e-9


def test_collision_fold():
    """Test 2, cfg3: the COLLISION_FREE bit and first_hit against the world's
    collide_batch of the returned waypoints, and those flags against the CPU
    oracle's."""
    path, cnt, st, hit = device_s()
    w = world()
    n, mw, dof = path.shape
    flags, _ = w.collide_batch(path.reshape(-1, dof))
    flags = flags.reshape(n, mw)
    want_hit = np.full(n, -1, np.int32)
    for i in range(n):
        nz = np.flatnonzero(flags[i, 1:cnt[i]])
        if len(nz):
            want_hit[i] = nz[0] + 1
    np.testing.assert_array_equal((st & C.MPG_SCREW_COLLISION_FREE) != 0, want_hit < 0)
    np.testing.assert_array_equal(hit, want_hit)
    oflags, _ = Wd.oracle_world(3).collide_batch(path.reshape(-1, dof))
    np.testing.assert_array_equal(flags.reshape(-1) != 0, oflags != 0)
    valid = (st & C.MPG_SCREW_VALID) == C.MPG_SCREW_VALID
    print("fold: colliding rows %d, first hit after waypoint 1: %d, starts in collision %d, valid %d"
          % ((want_hit >= 0).sum(), (want_hit > 1).sum(), (flags[:, 0] != 0).sum(), valid.sum()))
    assert (want_hit >= 0).sum() >= 10
    assert (want_hit > 1).sum() >= 3
    assert valid.sum() >= 150
    # waypoint 0 is not checked: a start in collision alone does not clear the bit
    alone = (flags[:, 0] != 0) & (want_hit < 0)
    assert alone.any() and ((st[alone] & C.MPG_SCREW_COLLISION_FREE) != 0).all()


def test_padding():
    """Test 3: the slots past count repeat waypoint count - 1 bit for bit."""
    path, cnt, st, _ = device_s()
    q0, _ = S.recipe_s()
    for i in range(len(cnt)):
        assert 1 <= cnt[i] <= path.shape[1]
        np.testing.assert_array_equal(path[i, cnt[i]:], np.broadcast_to(path[i, cnt[i] - 1], path[i, cnt[i]:].shape))
    np.testing.assert_array_equal(path[:, 0], q0)
    assert all(bin(int(s) & END_BITS).count("1") == 1 for s in st)


def test_max_waypoints_4():
    """Test 4.  A row needs more than four waypoints when the default run
    stores more than four, or stores four and then tries a fifth state (it
    ends STALLED or at a LIMIT there): the cap is checked right after the
    fourth waypoint is stored."""
    path, cnt, st, _ = device_s()
    p4, c4, s4, _ = device_s(4)
    more = (cnt > 4) | ((cnt == 4) & ((st & C.MPG_SCREW_REACHED) == 0))
    assert more.sum() >= 100 and (~more).sum() >= 10
    assert ((s4[more] & C.MPG_SCREW_TRUNCATED) != 0).all() and ((s4[more] & C.MPG_SCREW_REACHED) == 0).all()
    assert (c4[more] == 4).all()
    np.testing.assert_array_equal(p4[more], path[more][:, :4])
    np.testing.assert_array_equal(s4[~more] & END_BITS, st[~more] & END_BITS)
    np.testing.assert_array_equal(c4[~more], cnt[~more])
    np.testing.assert_array_equal(p4[~more], path[~more][:, :4])


def gantry_desc():
    """The Panda's descriptor with the kinematics of its seven arm joints
    replaced: PZ, RX, RY, RZ, PX, PY, RX, each 0.1 m above the last along z with
    an identity rotation, panda_hand 0.1 m above joint 7.  At q = 0 the hand's
    rotation is exactly the identity and its position exactly on the z axis, so
    a goal's rotation about z does not touch the translation of goal *
    link_pose^-1 -- in general it does, by rounding at least."""
    d = dict(Wd.desc_arrays(K.oracle_world()))
    types = [6, 0, 1, 2, 4, 5, 0]
    jt, ax = list(d["joint_type"]), list(d["joint_axis"])
    pl, lo, hi = list(d["joint_placement"]), list(d["joint_lower"]), list(d["joint_upper"])
    for j, s in enumerate(d["joint_q_source"]):
        if s < 0:
            continue
        jt[j] = types[s]
        ax[3 * j:3 * j + 3] = [1.0, 0.0, 0.0]
        pl[12 * j:12 * j + 12] = [1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0, 0, 0, 0.1]
        lo[j], hi[j] = -10.0, 10.0
    lp = list(d["link_placement"])
    lp[12 * K.HAND:12 * K.HAND + 12] = [1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0, 0, 0, 0.1]
    d.update(joint_type=jt, joint_axis=ax, joint_placement=pl, joint_lower=lo, joint_upper=hi, link_placement=lp)
    return d


def test_hand_made_rows():
    """Test 5: a goal rotated by exactly pi, a start just inside joint 4's
    upper limit moving toward it, and a start with a finger outside its limit."""
    w = world()
    lim = K.limits()
    li = w.ik_link_index(LINK)
    q0 = np.array([0.0, 0.2, 0.0, -1.8, 0.0, 2.0, 0.8])
    start = w.fk_link_pose(q0, li)
    # a goal rotated by exactly pi: ROT_PI, one waypoint
    goal = S.moved_pose(start, np.array([0.0, 0.0, 1.0]), np.pi, np.zeros(3))
    path, cnt, st, hit = w.plan_screw_batch(LINK, goal, q0)
    assert st[0] & END_BITS == C.MPG_SCREW_ROT_PI and cnt[0] == 1 and hit[0] == -1
    np.testing.assert_array_equal(path[0], np.broadcast_to(q0, path[0].shape))
    # 0.02 rad inside joint 4's upper limit, moving toward it: J dq of a pure joint 4 motion as the goal
    q1 = q0.copy()
    q1[3] = lim[3, 1] - 0.02
    q2 = q1.copy()
    q2[3] = lim[3, 1] + 0.3
    path, cnt, st, _ = w.plan_screw_batch(LINK, w.fk_link_pose(q2, li), q1, qpos_step=0.005)
    assert st[0] & END_BITS == C.MPG_SCREW_LIMIT and 3 <= cnt[0] <= 8
    assert (np.diff(path[0, :cnt[0], 3]) > 0).all()
    assert (path[0, :cnt[0], 3] <= lim[3, 1] + 1e-3).all()
    # a finger outside its limit: the fingers are constants of this world's
    # state, not dof slots, so no bit changes (plan_screw itself tests all nine
    # joints of its qpos and fails there)
    art = world_art()[1]
    near = S.moved_pose(start, np.array([0.0, 0.0, 1.0]), 0.1, np.array([0.03, 0.0, 0.02]))
    ref = w.plan_screw_batch(LINK, near, q0)
    keep = np.array(art.get_qpos())
    try:
        art.set_qpos(np.concatenate([q0, [0.05, 0.05]]), True)
        got = w.plan_screw_batch(LINK, near, q0)
    finally:
        art.set_qpos(keep, True)
    assert ref[2][0] & END_BITS == C.MPG_SCREW_REACHED
    np.testing.assert_array_equal(got[2] & END_BITS, ref[2] & END_BITS)
    np.testing.assert_array_equal(got[0], ref[0])


def test_small_rotation_is_dropped():
    """Test 5, second row: a goal translated by 0.1 m and rotated by 1e-3 rad
    gives the same path, bit for bit, as the pure translation.  On the gantry
    (gantry_desc) through DeviceWorld, where the two relative transforms have
    the same translation exactly; a rotation of 1e-2 rad is not dropped."""
    from mplib_amd.batch import DeviceWorld
    d = gantry_desc()
    dw = DeviceWorld(d)
    q0 = np.zeros(7)
    t = np.array([0.06, -0.048, 0.8 + 0.064])  # the hand starts at (0, 0, 0.8): a shift of 0.1 m

    def goal(angle):
        return np.concatenate([t, [np.cos(angle / 2), 0.0, 0.0, np.sin(angle / 2)]])
    goals = np.stack([goal(0.0), goal(1e-3), goal(1e-2)])
    path, cnt, st, _ = dw.screw_batch(K.HAND, goals, q0, qpos_step=0.02)
    dw.close()
    assert (st & END_BITS == C.MPG_SCREW_REACHED).all()
    assert cnt[0] == cnt[1] and cnt[0] >= 5
    np.testing.assert_array_equal(path[1], path[0])
    assert np.abs(path[2, cnt[2] - 1] - path[0, cnt[0] - 1]).max() > 1e-3
    # and the host build of the header agrees bit for bit
    hp, hc, hs = S.host_header_rows(goals, np.broadcast_to(q0, (3, 7)), qpos_step=0.02, desc=d)
    np.testing.assert_array_equal(cnt, hc)
    np.testing.assert_array_equal(path[:2], hp[:2])  # no acos on these two rows
    print("gantry, 1e-2 rad row against the host build: max difference %.3g" % np.abs(path[2] - hp[2]).max())
    assert np.abs(path[2] - hp[2]).max() <= 1e-9


def test_smaller_step():
    """Test 6: qpos_step = 0.02 on 32 rows: more waypoints, and on the rows
    that reach at both steps the final distance_6D to the goal is no larger."""
    q0, goal = S.recipe_s()
    idx = np.flatnonzero(S.well_rows())[:32]
    w = world()
    li = w.ik_link_index(LINK)
    a = w.plan_screw_batch(LINK, goal[idx], q0[idx], max_waypoints=512)
    b = w.plan_screw_batch(LINK, goal[idx], q0[idx], qpos_step=0.02, max_waypoints=512)
    both = ((a[2] & C.MPG_SCREW_REACHED) != 0) & ((b[2] & C.MPG_SCREW_REACHED) != 0)
    assert both.sum() >= 16
    assert (b[1][both] > a[1][both]).all()
    for k in np.flatnonzero(both):
        da = K.np_distance_6d(goal[idx[k]], w.fk_link_pose(a[0][k, a[1][k] - 1], li))
        db = K.np_distance_6d(goal[idx[k]], w.fk_link_pose(b[0][k, b[1][k] - 1], li))
        assert db <= da, (k, da, db)


def test_device_path_and_streams():
    """Test 7: torch tensors on two streams at once equal the host path bit
    for bit; DeviceWorld over the C ABI with first_hit = NULL."""
    import torch
    from mplib_amd.batch import DeviceWorld
    q0, goal = S.recipe_s()
    w = world()
    li = w.ik_link_index(LINK)
    ref = device_s()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = []
    for k, (a, b) in enumerate(((0, 96), (96, 256))):
        n = b - a
        with torch.cuda.stream(streams[k]):
            g = torch.from_numpy(goal[a:b].copy()).cuda()
            s0 = torch.from_numpy(q0[a:b].copy()).cuda()
            o = (torch.zeros(n, 64, 7, dtype=torch.float64, device="cuda"),
                 torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(n, dtype=torch.uint8, device="cuda"),
                 torch.zeros(n, dtype=torch.int32, device="cuda"))
        streams[k].synchronize()  # the inputs are in place; the calls below only enqueue
        outs.append((g, s0, o))
    for k in range(2):
        g, s0, o = outs[k]
        w.plan_screw_batch_device(li, g.data_ptr(), s0.data_ptr(), g.shape[0], o[0].data_ptr(), o[1].data_ptr(),
                                  o[2].data_ptr(), o[3].data_ptr(), streams[k].cuda_stream)
    torch.cuda.synchronize()
    for k, (a, b) in enumerate(((0, 96), (96, 256))):
        for x, y in zip(outs[k][2], ref):
            np.testing.assert_array_equal(x.cpu().numpy(), y[a:b])
    # the C ABI on another descriptor of the same world, first_hit = NULL
    dw = DeviceWorld(Wd.desc_arrays(Wd.oracle_world(3)))
    with torch.cuda.stream(streams[0]):
        g = torch.from_numpy(goal[:80].copy()).cuda()
        s0 = torch.from_numpy(q0[:80].copy()).cuda()
        o = (torch.zeros(80, 64, 7, dtype=torch.float64, device="cuda"), torch.zeros(80, dtype=torch.int32, device="cuda"),
             torch.zeros(80, dtype=torch.uint8, device="cuda"), None)
    streams[0].synchronize()
    dw.screw_batch(K.HAND, g, s0, out=o, stream=streams[0].cuda_stream)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(o[1].cpu().numpy(), ref[1][:80])
    np.testing.assert_array_equal(o[2].cpu().numpy(), ref[2][:80])
    np.testing.assert_allclose(o[0].cpu().numpy(), ref[0][:80], rtol=0, atol=1e-9)
    path, cnt, st, hit = dw.screw_batch(K.HAND, goal[:80], q0[:80], first_hit=False)
    assert hit is None
    np.testing.assert_array_equal(st, ref[2][:80])
    dw.close()


def test_continuous_joint(tmp_path_factory):
    """Test 8: panda_joint7 continuous (the model test_ik_batch.py builds).
    The continuous joint's slot has no limits and is not wrapped: starts near
    +-pi cross it.  Against np_plan_screw on that model's own PinocchioModel:
    the bounds of test 1 on the rows whose sigma_min stays >= 1e-2."""
    from test_ik_batch import continuous_model
    w, art = continuous_model(str(tmp_path_factory.mktemp("screw_urdf")))
    pin = art.get_pinocchio_model()
    assert pin.get_joint_types()[6].startswith("JointModelRUB")
    lim = S.limits9().copy()
    lim[6] = [-np.inf, np.inf]
    rng = np.random.default_rng(41)
    n = 48
    q0 = rng.uniform(0.6 * lim[:7, 0].clip(-3, 3), 0.6 * lim[:7, 1].clip(-3, 3), size=(n, 7))
    q0[:, 6] = np.where(rng.random(n) < 0.5, 1, -1) * rng.uniform(2.9, 3.3, n)  # near and beyond +-pi

    def fk(q7):
        pin.compute_forward_kinematics(list(q7) + [0.0, 0.0])
        return np.asarray(pin.get_link_pose(K.HAND))

    start = np.stack([fk(q) for q in q0])
    axis = S.random_unit(rng, n)
    shift = S.random_unit(rng, n) * rng.uniform(0.02, 0.15, size=(n, 1))
    goal = np.stack([S.moved_pose(start[i], axis[i], rng.uniform(0.05, 0.5), shift[i]) for i in range(n)])
    path, cnt, st, _ = w.plan_screw_batch(LINK, goal, q0, max_waypoints=512)
    checked, worst, crossed = 0, 0.0, 0
    for i in range(n):
        rst, rpath, sig, _ = S.np_plan_screw(goal[i], q0[i], pin=pin, fk=fk, lim=lim)
        if sig < S.WELL:
            continue
        checked += 1
        assert st[i] & END_BITS == rst and cnt[i] == len(rpath), (i, st[i], rst, cnt[i], len(rpath))
        worst = max(worst, np.abs(path[i, :cnt[i]] - rpath).max())
        crossed += bool(np.abs(rpath[:, 6]).max() > np.pi)
    print("continuous joint: %d rows checked, max|dq| %.3g, beyond +-pi on %d" % (checked, worst, crossed))
    assert checked >= 24 and crossed >= 8
    assert worst <= 1e-9


def test_facade_and_argument_errors():
    """Test 9."""
    w = world()
    art = world_art()[1]
    q0, goal = S.recipe_s()
    path, cnt, st, hit = device_s()
    valid = (st & C.MPG_SCREW_VALID) == C.MPG_SCREW_VALID
    ok, bad = int(np.flatnonzero(valid)[0]), int(np.flatnonzero(hit > 0)[0])
    lim_row = int(np.flatnonzero((st & C.MPG_SCREW_LIMIT) != 0)[0])
    keep = np.array(art.get_qpos())
    r = P.plan_screw(w, LINK, goal[ok], q0[ok])
    assert r["status"] == "Success"
    np.testing.assert_array_equal(r["path"], path[ok, :cnt[ok]])
    r = P.plan_screw(w, LINK, goal[bad], q0[bad])
    assert r["status"] == "screw plan failed" and "COLLISION at waypoint %d" % hit[bad] in r["reason"]
    r = P.plan_screw(w, LINK, goal[lim_row], q0[lim_row])
    assert r["status"] == "screw plan failed" and "LIMIT" in r["reason"]
    both = P.plan_screw(w, LINK, goal[[ok, bad]], q0[[ok, bad]])
    assert [b["status"] for b in both] == ["Success", "screw plan failed"]
    np.testing.assert_array_equal(np.array(art.get_qpos()), keep)
    # a (dof,) start is broadcast
    one = w.plan_screw_batch(LINK, goal[[ok, ok]], q0[ok])
    np.testing.assert_array_equal(one[0][1], path[ok])
    # refusals
    with pytest.raises(NotImplementedError, match="six joints"):
        w.plan_screw_batch("panda_link3", goal[:1], q0[:1])
    with pytest.raises(ValueError):
        w.plan_screw_batch("no_such_link", goal[:1], q0[:1])
    with pytest.raises(ValueError, match="out of range"):
        w.plan_screw_batch(99, goal[:1], q0[:1])
    g = goal[:1].copy()
    g[0, 3:] *= 1.001
    with pytest.raises(ValueError, match="unit norm"):
        w.plan_screw_batch(LINK, g, q0[:1])
    g = goal[:1].copy()
    g[0, 1] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        w.plan_screw_batch(LINK, g, q0[:1])
    s = q0[:1].copy()
    s[0, 2] = np.inf
    with pytest.raises(ValueError, match="non-finite"):
        w.plan_screw_batch(LINK, goal[:1], s)
    for mw in (1, 4097):
        with pytest.raises(ValueError, match="max_waypoints"):
            w.plan_screw_batch(LINK, goal[:1], q0[:1], max_waypoints=mw)
    for step in (0.0, -0.1):
        with pytest.raises(ValueError, match="qpos_step"):
            w.plan_screw_batch(LINK, goal[:1], q0[:1], qpos_step=step)
    # the C ABI's own checks of the same options
    h = ctypes.c_void_p(w.device_handle())
    for o in (C.ScrewOptions(0.1, 1), C.ScrewOptions(0.1, 4097), C.ScrewOptions(0.0, 64)):
        assert C.lib().mpg_screw_batch(h, w.ik_link_index(LINK), None, None, 0, ctypes.byref(o), None, None, None, None,
                                       C.MPG_MEM_HOST, None) == C.MPG_E_INVALID
    out = w.plan_screw_batch(LINK, np.zeros((0, 7)), np.zeros((0, 7)))
    assert out[0].shape == (0, 64, 7) and out[1].shape == (0,)


def test_free_frame_link_refused():
    from test_movable_objects import movable_world
    w = movable_world()[0]
    h = ctypes.c_void_p(w.device_handle())
    info = C.WorldInfo()
    C.check(C.lib().mpg_world_get_info(h, ctypes.byref(info)), "info")
    q0, goal = S.recipe_s()
    with pytest.raises(ValueError, match="free frame"):
        w.plan_screw_batch(info.n_links - 1, goal[:1], q0[:1])
    # the robot's links of that world work, at the movable objects' current poses
    path, cnt, st, hit = w.plan_screw_batch(LINK, goal[:16], q0[:16])
    flags, _ = w.collide_batch(path.reshape(-1, 7))
    flags = flags.reshape(16, -1)
    for i in range(16):
        assert bool(st[i] & C.MPG_SCREW_COLLISION_FREE) == (not flags[i, 1:cnt[i]].any())
