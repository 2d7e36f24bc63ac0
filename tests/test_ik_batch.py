"""GPU: mpg_ik_batch (PlanningWorld.ik_batch / ik_batch_device, DeviceWorld.ik_batch,
mplib_amd.planner.ik) against the host compute_IK_CLIK, the CPU oracle's FK of
the answers, and numpy restatements of planner.py's limit check and
distance_6D.  Inputs and references: tests/ik_cases.py."""
import ctypes
import functools
import os

import numpy as np
import pytest

import ik_cases as K
from mplib_amd import _capi as C
from mplib_amd import planner as P
from mplib_amd import scenes

pytestmark = pytest.mark.gpu

LINK = "panda_hand"
START = np.array([0.0, 0.2, 0.0, -1.8, 0.0, 2.0, 0.8])


@functools.lru_cache(maxsize=None)
def world(cfg=2):
    return scenes.world(cfg)[0]


def run(pose, q0, cfg=2, **kw):
    """One goal per row: (q [n, 7], status [n], err [n, 6], iters [n])."""
    n = len(pose)
    q, st, err, it = world(cfg).ik_batch(LINK, pose, q_init=np.asarray(q0).reshape(n, 1, 7), **kw)
    return q[:, 0], st[:, 0], err[:, 0], it[:, 0]


def assert_reaches_goal(q, st, rows=None, kind="A", goal_q=None):
    """Every CONVERGED row's CPU FK is at its goal: within 2 eps in position and
    in max|dR| (the error is measured in the parent joint's frame; the hand
    frame sits < 0.25 m from that joint, so the link's position error is at
    most eps (1 + 0.25) plus rounding)."""
    conv = (st & C.MPG_IK_CONVERGED) != 0
    if not conv.any():
        return conv
    idx = np.flatnonzero(conv)
    rows = idx if rows is None else np.asarray(rows)[idx]
    dp, dR = K.fk_residual(q[idx], goal_q=goal_q, kind=kind, rows=rows)
    assert dp.max() <= 2 * K.EPS and dR.max() <= 2 * K.EPS, (dp.max(), dR.max())
    return conv


@pytest.mark.parametrize("n", [1, 63, 64, 65, 256])
def test_one_step(n):
    """Test 1.  The device against compute_IK_CLIK(maxIter=1) on the recipe A
    rows with sigma_min(J) >= 1e-2, max|dq| <= 1e-9: operation order (~1e-16)
    times kappa(J J^T) <= 4e4, plus the device's acos, a few ulp of an angle,
    times |J^+| dt <= 10.  Row counts at the wave edges.
    Two-run check of the reference on these rows: see test_ik_host.py (at most
    4.3e-13 on the 231 well-conditioned rows)."""
    _, pose, q0 = K.recipe("A")
    well = K.sigma_min("A") >= 1e-2
    idx = np.flatnonzero(well)[:n] if n < 200 else np.arange(n)
    ref = K.wrapped_reference("A", 1)[0][idx]
    q, st, _, it = run(pose[idx], q0[idx], max_iter=1)
    d = np.abs(q - ref).max(axis=1)[well[idx]]
    print("one step n=%d: max|dq| %.3g" % (n, d.max()))
    assert (it <= 1).all()
    assert d.max() <= 1e-9


def test_near_rows_full_run():
    """Test 2, recipe A.  Two-run check of the reference on these rows: 256 /
    256 converge, no status differs, median max|dq| 6.3e-14, 1 row above 1e-6
    (1.3e-5).  iters is compared with mpg_ik.h's own count on the host
    (compute_IK_CLIK does not return one)."""
    _, pose, q0 = K.recipe("A")
    ref_q, ref_ok, ref_err = K.wrapped_reference("A")
    _, _, _, host_it = K.host_header_rows(pose, q0)
    q, st, err, it = run(pose, q0)
    assert ((st & C.MPG_IK_CONVERGED) != 0).all() and ((st & C.MPG_IK_SINGULAR) == 0).all()
    assert np.abs(it.astype(int) - host_it).max() <= 1
    d = np.abs(q - ref_q).max(axis=1)
    print("near rows: max|dq| %.3g, rows over 1e-6: %d, iters %d..%d, max|derr| %.3g"
          % (d.max(), (d > 1e-6).sum(), it.min(), it.max(), np.abs(err - ref_err).max()))
    assert (d > 1e-6).sum() <= 2
    assert_reaches_goal(q, st)
    assert (np.linalg.norm(err, axis=1) < K.EPS).all()
    assert np.abs(err - ref_err).max() <= 1e-9


def test_uniform_rows():
    """Test 3, recipe B: 15 % of these rows end in another basin under a 1e-13
    perturbation of the reference itself, so no row-wise comparison of q.
    Every CONVERGED row reaches its goal by the CPU FK; the CONVERGED bit
    differs from the host's on at most 13 of 256 rows (5 %).  Two-run check of
    the reference on these rows: 255 and 254 of 256 converge, 3 statuses differ,
    35 rows (14 %) end more than 1e-6 apart."""
    _, pose, q0 = K.recipe("B")
    _, ref_ok, _ = K.host_reference("B")
    q, st, _, it = run(pose, q0)
    conv = assert_reaches_goal(q, st, kind="B")
    print("uniform rows: converged %d (host %d), bits differ on %d, mean iters %.0f"
          % (conv.sum(), ref_ok.sum(), (conv != ref_ok).sum(), it.mean()))
    assert conv.sum() >= 200
    assert (conv != ref_ok).sum() <= 13


def test_row_claiming():
    """Test 4: 1000 recipe A rows on two waves (every lane claims ~8 rows)
    against the full grid: a row's result does not depend on the lane that ran
    it -- q, status and iters equal bit for bit."""
    q_goal, pose, q0 = K.recipe("A", 1000, 77)
    a = run(pose, q0, max_waves=2)
    b = run(pose, q0, max_waves=0)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)
    conv = assert_reaches_goal(a[0], a[1], goal_q=q_goal)
    assert conv.sum() >= 990


def test_goal_seed_mapping_and_sampling():
    """Test 5: 3 goals x 7 seeds drawn on the device."""
    q_goal, pose, _ = K.recipe("A")
    lim = K.limits()
    w = world()
    mask = np.zeros(7, bool)
    mask[5] = True
    for mk in (None, mask):
        q, st, _, it = w.ik_batch(LINK, pose[:3], start_qpos=START, n_init_qpos=7, seed=11, max_iter=0, mask=mk)
        assert q.shape == (3, 7, 7) and (it == 0).all()
        for g in range(3):
            np.testing.assert_array_equal(q[g, 0], START)
            for r in range(1, 7):
                want = P.sample_uniform(lim[:, 0], lim[:, 1], 1, 11, offset=g * 7 + r)[0]
                if mk is not None:
                    want[mk] = START[mk]
                np.testing.assert_array_equal(q[g, r], want)
    # the same call with the default max_iter: each row's residual against its own goal g
    q, st, _, _ = w.ik_batch(LINK, pose[:3], start_qpos=START, n_init_qpos=7, seed=11)
    for g in range(3):
        conv = assert_reaches_goal(q[g], st[g], rows=np.full(7, g))
        assert conv.sum() >= 2, (g, st[g])


def test_mask():
    """Test 6: a masked joint never moves; with two joints free and damp = 1e-6
    the pivots are at least damp, so no row is SINGULAR."""
    _, pose, q0 = K.recipe("A")
    mask = np.zeros(7, bool)
    mask[0] = True
    q, st, _, _ = run(pose[:64], q0[:64], mask=mask)
    np.testing.assert_array_equal(q[:, 0], q0[:64, 0])
    assert (np.abs(q[:, 1:] - q0[:64, 1:]).max(axis=1) > 0).all()
    two = np.ones(7, bool)
    two[[1, 3]] = False
    q, st, err, it = run(pose[:64], q0[:64], mask=two, damp=1e-6)
    assert np.isfinite(q).all() and np.isfinite(err).all()
    np.testing.assert_array_equal(q[:, two], q0[:64][:, two])
    assert ((st & C.MPG_IK_SINGULAR) == 0).all()


def fk_batch(w, q):
    n = len(q)
    info = C.WorldInfo()
    h = ctypes.c_void_p(w.device_handle())
    C.check(C.lib().mpg_world_get_info(h, ctypes.byref(info)), "info")
    out = np.zeros((n, info.n_links, 7))
    q = np.ascontiguousarray(q)
    C.check(C.lib().mpg_fk_batch(h, q.ctypes.data, n, out.ctypes.data, C.MPG_MEM_HOST, None), "mpg_fk_batch")
    return out


def test_filter_bits():
    """Test 7: the cfg3 world, the recipe B goals x 8 seeds drawn on the device."""
    _, pose, _ = K.recipe("B")
    lim = K.limits()
    w = world(3)
    q, st, _, _ = w.ik_batch(LINK, pose, start_qpos=START, n_init_qpos=8, seed=3)
    rows = q.reshape(-1, 7)
    s = st.reshape(-1)
    flags, _ = w.collide_batch(rows)
    np.testing.assert_array_equal((s & C.MPG_IK_COLLISION_FREE) != 0, flags == 0)
    rev = np.ones(7, bool)
    wrapped, fail = K.np_check_joint_limit(rows, lim[:, 0], lim[:, 1], rev)
    np.testing.assert_array_equal(wrapped, rows)  # q_out holds wrapped values: wrapping them again is the identity
    np.testing.assert_array_equal((s & C.MPG_IK_IN_LIMITS) != 0, ~fail.any(axis=1))
    hand = fk_batch(w, rows)[:, K.HAND]
    goal = np.repeat(pose, 8, axis=0)
    dist = np.array([K.np_distance_6d(goal[i], hand[i]) for i in range(len(rows))])
    np.testing.assert_array_equal((s & C.MPG_IK_WITHIN_THRESHOLD) != 0, dist < 1e-3)
    valid = (st & C.MPG_IK_VALID) == C.MPG_IK_VALID
    print("filter bits: valid rows %d of %d, goals with one %d of %d, colliding rows %d, out of limits %d"
          % (valid.sum(), valid.size, valid.any(axis=1).sum(), len(pose), (flags != 0).sum(), fail.any(axis=1).sum()))
    assert valid.any() and (flags != 0).any()
    # the wrap itself: max_iter = 0 from starts shifted by +-2 pi and beyond hi
    rng = np.random.default_rng(8)
    q0 = rng.uniform(lim[:, 0], lim[:, 1], size=(64, 7))
    q0[:16] += K.TWO_PI
    q0[16:32] -= K.TWO_PI
    q0[32:48, 3] = lim[3, 1] + rng.uniform(0.01, 0.5, 16)
    q1, s1, _, _ = run(pose[:64], q0, cfg=3, max_iter=0)
    want, fail = K.np_check_joint_limit(q0, lim[:, 0], lim[:, 1], rev)
    assert K.ulp_diff(q1, want).max() <= 4
    np.testing.assert_array_equal((s1 & C.MPG_IK_IN_LIMITS) != 0, ~fail.any(axis=1))
    assert fail[32:48].any(axis=1).all() and not fail[:32].any()


def test_facade_and_argument_errors():
    """Test 8a: planner.ik's return convention, and the refusals."""
    q_goal, pose, _ = K.recipe("A")
    w = world()
    s, goals = P.ik(w, LINK, pose[0], START, n_init_qpos=20)
    assert s == "Success" and len(goals) >= 1
    G = np.asarray(goals)
    dp, dR = K.fk_residual(G, rows=np.zeros(len(G), int))
    assert dp.max() <= 2 * K.EPS and dR.max() <= 2 * K.EPS
    for i in range(len(G)):
        for j in range(i):
            assert np.linalg.norm(G[i] - G[j]) >= 0.1
    s1, best = P.ik(w, LINK, pose[0], START, return_closest=True)
    assert s1 == "Success" and best.shape == (7,)
    assert np.linalg.norm(best - START) <= min(np.linalg.norm(g - START) for g in G) + 1e-12
    far = pose[0].copy()
    far[:3] = [3.0, 0.0, 0.5]
    assert P.ik(w, LINK, far, START) == ("IK Failed! Cannot find valid solution.", None)
    both = P.ik(w, LINK, np.stack([pose[0], far]), START)
    assert both[0][0] == "Success" and both[1] == ("IK Failed! Cannot find valid solution.", None)
    np.testing.assert_array_equal(np.asarray(both[0][1]), G)
    # refusals
    with pytest.raises(ValueError):
        w.ik_batch("no_such_link", pose[:1], start_qpos=START)
    with pytest.raises(ValueError, match="out of range"):
        w.ik_batch(99, pose[:1], start_qpos=START)
    with pytest.raises(ValueError, match="max_iter"):
        w.ik_batch(LINK, pose[:1], start_qpos=START, max_iter=100001)
    with pytest.raises(ValueError, match="max_iter"):
        w.ik_batch(LINK, pose[:1], start_qpos=START, max_iter=-1)
    bad = pose[:1].copy()
    bad[0, 1] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        w.ik_batch(LINK, bad, start_qpos=START)
    bad = pose[:1].copy()
    bad[0, 3:] *= 1.001
    with pytest.raises(ValueError, match="unit norm"):
        w.ik_batch(LINK, bad, start_qpos=START)
    with pytest.raises(ValueError, match="both NULL"):
        w.ik_batch(LINK, pose[:1])


def test_free_frame_link_refused():
    from test_movable_objects import movable_world
    w = movable_world()[0]
    h = ctypes.c_void_p(w.device_handle())
    info = C.WorldInfo()
    C.check(C.lib().mpg_world_get_info(h, ctypes.byref(info)), "info")
    _, pose, _ = K.recipe("A")
    with pytest.raises(ValueError, match="free frame"):
        w.ik_batch(info.n_links - 1, pose[:1], start_qpos=START)
    # and the robot's links of that world work, at the movable objects' current poses
    q, st, _, _ = w.ik_batch(LINK, pose[:8], start_qpos=START, n_init_qpos=4, seed=1)
    flags, _ = w.collide_batch(q.reshape(-1, 7))
    np.testing.assert_array_equal((st.reshape(-1) & C.MPG_IK_COLLISION_FREE) != 0, flags == 0)


def test_device_path_and_streams():
    """Test 8b: device buffers on a non-default stream equal the host path bit
    for bit; two streams with different goals are independent."""
    import torch
    _, pose, q0 = K.recipe("B")
    w = world(3)
    li = w.ik_link_index(LINK)
    host = [run(pose[:96], q0[:96], cfg=3), run(pose[96:224], q0[96:224], cfg=3)]
    host_seeded = w.ik_batch(LINK, pose[:16], start_qpos=START, n_init_qpos=5, seed=9)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = []
    for k, (a, b) in enumerate(((0, 96), (96, 224))):
        n = b - a
        with torch.cuda.stream(streams[k]):
            g = torch.from_numpy(pose[a:b].copy()).cuda()
            qi = torch.from_numpy(q0[a:b].copy()).cuda()
            o = (torch.zeros(n, 7, dtype=torch.float64, device="cuda"), torch.zeros(n, dtype=torch.uint8, device="cuda"),
                 torch.zeros(n, 6, dtype=torch.float64, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda"))
        streams[k].synchronize()  # the inputs are in place; the calls below only enqueue
        outs.append((g, qi, o))
    for k in range(2):
        g, qi, o = outs[k]
        w.ik_batch_device(li, g.data_ptr(), g.shape[0], 1, qi.data_ptr(), 0, o[0].data_ptr(), o[1].data_ptr(),
                          o[2].data_ptr(), o[3].data_ptr(), streams[k].cuda_stream)
    torch.cuda.synchronize()
    for k in range(2):
        for x, y in zip(outs[k][2], host[k]):
            np.testing.assert_array_equal(x.cpu().numpy(), y)
    # seeds drawn on the device, device-resident start
    with torch.cuda.stream(streams[0]):
        g = torch.from_numpy(pose[:16].copy()).cuda()
        s0 = torch.from_numpy(START.copy()).cuda()
        o = (torch.zeros(80, 7, dtype=torch.float64, device="cuda"), torch.zeros(80, dtype=torch.uint8, device="cuda"))
    streams[0].synchronize()
    w.ik_batch_device(li, g.data_ptr(), 16, 5, 0, s0.data_ptr(), o[0].data_ptr(), o[1].data_ptr(), 0, 0,
                      streams[0].cuda_stream, seed=9)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(o[0].cpu().numpy().reshape(16, 5, 7), host_seeded[0])
    np.testing.assert_array_equal(o[1].cpu().numpy().reshape(16, 5), host_seeded[1])


def test_device_world_c_abi():
    """DeviceWorld.ik_batch (mplib_amd/batch.py) over the C ABI agrees with PlanningWorld.ik_batch
    (two descriptors of the same robot, built by the oracle and by pymp)."""
    import worlds as Wd
    from mplib_amd.batch import DeviceWorld
    _, pose, q0 = K.recipe("A")
    dw = DeviceWorld(Wd.desc_arrays(K.oracle_world()))
    q, st, err, it = dw.ik_batch(K.HAND, pose[:32], q_init=q0[:32].reshape(32, 1, 7))
    ref = run(pose[:32], q0[:32])
    np.testing.assert_array_equal(st[:, 0], ref[1])
    np.testing.assert_allclose(q[:, 0], ref[0], rtol=0, atol=1e-9)
    np.testing.assert_allclose(err[:, 0], ref[2], rtol=0, atol=1e-9)
    assert np.abs(it[:, 0].astype(int) - ref[3]).max() <= 1
    dw.close()


@functools.lru_cache(maxsize=None)
def continuous_model(tmp):
    """panda.urdf with panda_joint7 continuous, written to tmp; the loader
    resolves mesh files against the URDF's directory (an absolute file name
    included), so the mesh tree is linked next to the copy."""
    from mplib_amd import pymp
    src = open(os.path.join(scenes.PANDA_DIR, "panda.urdf")).read()
    os.symlink(os.path.join(scenes.PANDA_DIR, "franka_description"), os.path.join(tmp, "franka_description"))
    old = '<joint name="panda_joint7" type="revolute">'
    assert old in src
    src = src.replace(old, '<joint name="panda_joint7" type="continuous">')
    urdf = os.path.join(tmp, "panda_continuous.urdf")
    open(urdf, "w").write(src)
    art = pymp.articulation.ArticulatedModel(urdf, os.path.join(scenes.PANDA_DIR, "panda.srdf"), [0, 0, -9.81],
                                             scenes.PANDA_JOINTS, scenes.PANDA_LINKS, verbose=False, convex=True)
    art.set_move_group(LINK)
    return pymp.planning_world.PlanningWorld([art], ["panda"], [], []), art


def test_continuous_joint(tmp_path_factory):
    """Test 9: tests 1 and 2 at 64 rows with panda_joint7 continuous: the
    answers come back as atan2 values inside [-pi, pi]; the reference and the
    FK of the answers are that model's own (compute_IK_CLIK,
    compute_forward_kinematics)."""
    w, art = continuous_model(str(tmp_path_factory.mktemp("ik_urdf")))
    pin = art.get_pinocchio_model()
    assert pin.get_joint_types()[6].startswith("JointModelRUB")
    lim = K.limits()
    rng = np.random.default_rng(31)
    q_goal = rng.uniform(0.8 * lim[:, 0], 0.8 * lim[:, 1], size=(64, 7))
    q_goal[:, 6] = rng.uniform(-3.1, 3.1, 64)
    q0 = np.clip(q_goal + rng.normal(scale=0.2, size=(64, 7)), lim[:, 0], lim[:, 1])
    q0[:, 6] = q_goal[:, 6] + rng.normal(scale=0.2, size=64)  # may leave [-pi, pi]: the answer is wrapped by atan2

    def fk(q7):
        pin.compute_forward_kinematics(list(q7) + [0.0, 0.0])
        return np.asarray(pin.get_link_pose(K.HAND))

    pose = np.stack([fk(q) for q in q_goal])
    for max_iter, tol, over in ((1, 1e-9, 0), (1000, 1e-6, 2)):
        ref = np.zeros((64, 7))
        ok = np.zeros(64, bool)
        sig = np.zeros(64)
        for i in range(64):
            r, ok[i], _ = pin.compute_IK_CLIK(K.HAND, list(pose[i]), list(q0[i]) + [0.0, 0.0], [], maxIter=max_iter)
            ref[i] = np.asarray(r)[:7]
            pin.compute_full_jacobian(list(q0[i]) + [0.0, 0.0])
            sig[i] = np.linalg.svd(np.asarray(pin.get_link_jacobian(K.HAND, True))[:, :7], compute_uv=False).min()
        # step 2 wraps joints 1-6 into their limits; the continuous joint has none
        wlo, whi = lim[:, 0].copy(), lim[:, 1].copy()
        wlo[6], whi[6] = -np.inf, np.inf
        ref = K.np_check_joint_limit(ref, wlo, whi, np.ones(7, bool))[0]
        q, st, _, _ = w.ik_batch(LINK, pose, q_init=q0.reshape(64, 1, 7), max_iter=max_iter)
        q, st = q[:, 0], st[:, 0]
        assert (np.abs(q[:, 6]) <= np.pi).all()
        d = np.abs(q - ref)
        d[:, 6] = np.minimum(d[:, 6], np.abs(d[:, 6] - K.TWO_PI))  # the same angle either side of +-pi
        d = d.max(axis=1)
        rows = sig >= 1e-2 if max_iter == 1 else np.ones(64, bool)
        print("continuous joint, max_iter %d: max|dq| %.3g on %d rows" % (max_iter, d[rows].max(), rows.sum()))
        assert (d[rows] > tol).sum() <= over
        if max_iter > 1:
            assert ok.all() and ((st & C.MPG_IK_CONVERGED) != 0).all()
            got = np.stack([fk(x) for x in q])
            assert np.linalg.norm(got[:, :3] - pose[:, :3], axis=1).max() <= 2 * K.EPS
            dq = np.minimum(np.abs(got[:, 3:] - pose[:, 3:]).max(axis=1), np.abs(got[:, 3:] + pose[:, 3:]).max(axis=1))
            assert dq.max() <= 2 * K.EPS
