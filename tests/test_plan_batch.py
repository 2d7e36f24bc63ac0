"""GPU: mpg_plan_batch (PlanningWorld.plan_batch / plan_batch_device,
DeviceWorld.plan_batch, mplib_amd.planner.plan_batch / plan_to_pose_batch)
against the host models of tests/rrt_cases.py -- the numpy restatement of the
algorithm and the host build of the header the kernels run, both with the CPU
oracle as state validity.  Every comparison of outputs is exact: the
arithmetic has no library call, and the device's collision flags are the
oracle's (the project's standing invariant), so a row that differs in one bit
is a bug."""
import functools

import numpy as np
import pytest

import rrt_cases as R
import worlds as Wd
import zoo
from mplib_amd import _capi as C
from mplib_amd import planner as P
from mplib_amd import scenes

pytestmark = pytest.mark.gpu

NAMES = ("path", "n_waypoints", "status", "iterations", "tree_sizes")
KW = dict(range=R.RANGE, max_rounds=R.MAX_ROUNDS, max_nodes=R.MAX_NODES, max_waypoints=R.MAX_WAYPOINTS)


def assert_same(got, want, rows=None):
    for name, a, b in zip(NAMES, got, want):
        np.testing.assert_array_equal(a, b if rows is None else b[rows], err_msg=name)


@functools.lru_cache(maxsize=None)
def world_art(cfg=3):
    return scenes.world(cfg)


def world():
    return world_art()[0]


def model(start, goal, seeds, **kw):
    """The host build of the header with the oracle as validity."""
    lo, hi = R.limits()
    return R.host_plan_batch(lo, hi, start, goal, seeds, R.oracle_valid, **kw)


@functools.lru_cache(maxsize=None)
def device_r():
    """Recipe R and its extra row as one 65-row batch through the host path."""
    start, goal, seeds = R.recipe_r()
    return R._ro(*world().plan_batch(start, goal, row_seed=seeds, **KW))


def test_status_bits_and_limits_are_the_models():
    lo, hi = R.limits()
    lim = scenes.joint_limits(scenes.panda())
    np.testing.assert_array_equal(lim[:, 0], lo)
    np.testing.assert_array_equal(lim[:, 1], hi)
    assert (C.MPG_PLAN_SOLVED, C.MPG_PLAN_START_INVALID, C.MPG_PLAN_GOAL_INVALID, C.MPG_PLAN_ROUNDS_EXHAUSTED,
            C.MPG_PLAN_NODES_EXHAUSTED, C.MPG_PLAN_TRUNCATED) == (1, 2, 4, 8, 16, 32)
    assert (P.PLAN_SOLVED, P.PLAN_TRUNCATED) == (R.SOLVED, R.TRUNCATED)


@pytest.mark.parametrize("Q", [1, 3, 65])
def test_first_rows_equal_the_model(Q):
    """Test 1: the first Q rows of recipe R (65: with its extra row) as one
    batch; every output bit-equal to the numpy model and to the host build of
    the header.  The device's flags on the returned waypoints are the
    oracle's."""
    start, goal, seeds = R.recipe_r()
    got = device_r() if Q == R.N_BATCH else world().plan_batch(start[:Q], goal[:Q], row_seed=seeds[:Q], **KW)
    assert_same(got, R.reference_r(), slice(0, Q))
    assert_same(got, R.header_r(), slice(0, Q))
    path, cnt = got[0], got[1]
    pts = np.concatenate([path[r, :max(cnt[r], 1)] for r in range(Q)])
    flags, _ = world().collide_batch(pts)
    np.testing.assert_array_equal(flags != 0, R.oracle_valid(pts) != 0)


def test_large_trees():
    """Test 2: the rows of recipe R whose trees pass 256 nodes -- more nodes
    than the scan has threads, so every thread takes several and the reduction
    sees ties broken by index -- planned as a batch of their own."""
    start, goal, seeds = R.recipe_r()
    ref = R.reference_r()
    idx = np.flatnonzero(ref[4][:R.N_ROWS].max(axis=1) > 256)
    assert len(idx) >= 1
    got = world().plan_batch(start[idx], goal[idx], row_seed=seeds[idx], **KW)
    assert_same(got, ref, idx)
    assert (got[4].max(axis=1) > 256).all()
    print("rows past 256 nodes: %d, largest tree %d" % (len(idx), got[4].max()))


@pytest.mark.parametrize("opts,status", [(dict(max_nodes=8), R.NODES_EXHAUSTED), (dict(max_rounds=5), R.ROUNDS_EXHAUSTED),
                                         (dict(max_waypoints=2), R.SOLVED | R.TRUNCATED)])
def test_limits(opts, status):
    """Test 3: max_nodes = 8, max_rounds = 5 and max_waypoints = 2, each on
    three rows it ends, equal to the model."""
    start, goal, seeds = R.recipe_r()
    ref = R.reference_r()
    if "max_waypoints" in opts:
        idx = np.flatnonzero((ref[2] == R.SOLVED) & (ref[1] > 2))[:3]
    else:
        idx = np.flatnonzero(ref[4][:R.N_ROWS].max(axis=1) > 256)[:3]
    kw = dict(KW, **opts)
    got = world().plan_batch(start[idx], goal[idx], row_seed=seeds[idx], **kw)
    mkw = {("range_" if k == "range" else k): v for k, v in kw.items()}
    assert_same(got, model(start[idx], goal[idx], seeds[idx], **mkw))
    assert (got[2] == status).all() and (got[1] == 0).all()


def test_invalid_rows_in_a_mixed_batch():
    """Test 4: a colliding start, a colliding only goal, a start outside the
    bounds and two solvable rows in one batch."""
    start, goal, seeds = R.recipe_r()
    lo, hi = R.limits()
    bad = np.array(Wd.KAT_COLLIDING)
    out = start[0].copy()
    out[0] = hi[0] + 0.5
    s = np.array([bad, start[0], out, start[1], start[2]])
    g = np.array([goal[0], bad, goal[0], goal[1], goal[2]])
    sd = seeds[[0, 0, 0, 1, 2]]
    got = world().plan_batch(s, g, row_seed=sd, **KW)
    assert_same(got, model(s, g, sd))
    assert list(got[2][:3]) == [R.START_INVALID, R.GOAL_INVALID, R.START_INVALID]
    solo = world().plan_batch(s[3:], g[3:], row_seed=sd[3:], **KW)
    for a, b in zip(got, solo):
        np.testing.assert_array_equal(a[3:], b)
    assert_same(solo, R.reference_r(), [1, 2])


def test_rows_do_not_depend_on_the_batch():
    """Test 5a: three rows alone, inside the 65-row batch and in permuted
    order give identical outputs (explicit row seeds)."""
    start, goal, seeds = R.recipe_r()
    hard = np.flatnonzero(R.reference_r()[4][:R.N_ROWS].max(axis=1) > 256)
    idx = np.array([0, int(hard[0]), 7])
    alone = [world().plan_batch(start[[i]], goal[[i]], row_seed=seeds[[i]], **KW) for i in idx]
    perm = world().plan_batch(start[idx[::-1]], goal[idx[::-1]], row_seed=seeds[idx[::-1]], **KW)
    batch = device_r()
    for k, i in enumerate(idx):
        for name, a, b, c in zip(NAMES, alone[k], batch, perm):
            np.testing.assert_array_equal(a[0], b[i], err_msg=name)
            np.testing.assert_array_equal(a[0], c[len(idx) - 1 - k], err_msg=name)


@pytest.mark.parametrize("check_every", [1, 8, 1000])
def test_check_every_changes_nothing(check_every):
    """Test 5b: how often the host looks at the count of unfinished rows."""
    start, goal, seeds = R.recipe_r()
    got = world().plan_batch(start[:3], goal[:3], row_seed=seeds[:3], check_every=check_every, **KW)
    assert_same(got, R.reference_r(), slice(0, 3))


def test_device_path_equals_host_path():
    """Test 6: torch tensors on a non-default stream (plan_batch_device, and
    DeviceWorld over the C ABI with iterations = tree_sizes = NULL) equal the
    host path."""
    import torch
    from mplib_amd.batch import DeviceWorld
    start, goal, seeds = R.recipe_r()
    n = 9
    ref = device_r()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        s = torch.from_numpy(start[:n].copy()).cuda()
        g = torch.from_numpy(goal[:n].copy()).cuda()
        sd = torch.from_numpy(seeds[:n].copy().view(np.int64)).cuda()
        o = (torch.zeros(n, R.MAX_WAYPOINTS, 7, dtype=torch.float64, device="cuda"),
             torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(n, dtype=torch.uint8, device="cuda"),
             torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(n, 2, dtype=torch.int32, device="cuda"))
    st.synchronize()
    world().plan_batch_device(s.data_ptr(), g.data_ptr(), n, 1, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(),
                              o[3].data_ptr(), o[4].data_ptr(), sd.data_ptr(), st.cuda_stream, **KW)
    torch.cuda.synchronize()
    for name, x, y in zip(NAMES, o, ref):
        np.testing.assert_array_equal(x.cpu().numpy(), y[:n], err_msg=name)
    dw = DeviceWorld(Wd.desc_arrays(Wd.oracle_world(3)))
    o2 = (torch.zeros_like(o[0]), torch.zeros_like(o[1]), torch.zeros_like(o[2]), None, None)
    dw.plan_batch(s, g.reshape(n, 1, 7), row_seed=sd, out=o2, stream=st.cuda_stream, **KW)
    torch.cuda.synchronize()
    for name, x, y in zip(NAMES[:3], o2, ref):
        np.testing.assert_array_equal(x.cpu().numpy(), y[:n], err_msg=name)
    host = dw.plan_batch(start[:n], goal[:n], row_seed=seeds[:n], **KW)
    assert_same(host, ref, slice(0, n))


def test_goal_lists():
    """Test 7: G = 2.  [free, free] ends at one of the two goals; [colliding,
    free] plans to the second.  Both equal the model."""
    start, goal, seeds = R.recipe_r()
    bad = np.array(Wd.KAT_COLLIDING)
    s = start[[1, 0, 5]]
    g = np.array([[goal[1], goal[2]], [bad, goal[0]], [goal[6], goal[5]]])
    got = world().plan_batch(s, g, row_seed=seeds[:3], **KW)
    assert_same(got, model(s, g, seeds[:3]))
    path, cnt, st, _, sz = got
    assert (st == R.SOLVED).all()
    assert list(sz[:, 1] >= 1) == [True] * 3
    for r in range(3):
        end = path[r, cnt[r] - 1]
        assert any(np.array_equal(end, x) for x in g[r])
    np.testing.assert_array_equal(path[1, cnt[1] - 1], goal[0])


def test_continuous_joint_wraps(tmp_path_factory):
    """Test 8: zoo's "ikc" chain (8 joints, three continuous: the smallest
    world with one).  The world's SO2 bits are the continuous columns; a pair
    whose first continuous value goes from 3.0 to -3.0 crosses +-pi, and every
    output equals the model."""
    c = zoo.case(tmp_path_factory.mktemp("plan_ikc"), "ikc")
    w, _ = zoo.product_world(c)
    assert w.get_motion_space()[0] == c.so2_mask and c.so2_mask != 0
    col = int(np.flatnonzero(c.cont)[0])

    def valid(q):
        return (c.ow.collide_batch(q)[0] != 0).astype(np.uint8)

    q = c.sample(64, 5)
    q = q[valid(q) == 0]
    a, b = q[:16].copy(), q[16:32].copy()
    a[:, col], b[:, col] = 3.0, -3.0
    keep = (valid(a) == 0) & (valid(b) == 0)
    a, b = a[keep][:4], b[keep][:4]
    assert len(a) == 4
    seeds = np.array([21, 22, 23, 24], np.uint64)
    kw = dict(max_rounds=1500, max_nodes=512, max_waypoints=128)
    got = w.plan_batch(a, b, range=0.3, row_seed=seeds, **kw)
    want = R.host_plan_batch(c.lim[:, 0], c.lim[:, 1], a, b, seeds, valid, range_=0.3, so2_mask=c.so2_mask, **kw)
    assert_same(got, want)
    assert_same(got, R.np_plan_batch(c.lim[:, 0], c.lim[:, 1], a, b, seeds, valid, range_=0.3, so2_mask=c.so2_mask, **kw))
    path, cnt, st, _, _ = got
    assert (st == R.SOLVED).all() and got[3].max() > 50  # one row samples the SO2 slots many times
    for r in np.flatnonzero(st == R.SOLVED):
        p = path[r, :cnt[r]]
        assert (np.abs(p[:, col]) <= np.pi).all()
        assert np.abs(np.diff(p[:, col])).max() > 6.0  # over the seam, not 6 rad round


def test_planner_level_calls():
    """Test 9: planner.plan_batch's dictionaries; plan_to_pose_batch reaches,
    for each solved row, a state whose link pose is within the IK threshold of
    the goal pose."""
    start, goal, seeds = R.recipe_r()
    w = world()
    out = P.plan_batch(w, start[0], np.array([goal[0], Wd.KAT_COLLIDING]), row_seed=seeds[[0, 0]], **KW)
    ref = R.reference_r()
    assert out[0]["status"] == "Success"
    np.testing.assert_array_equal(out[0]["path"], ref[0][0, :ref[1][0]])
    assert out[1] == {"status": "plan failed", "reason": "GOAL_INVALID"}
    assert P.plan_reason(R.SOLVED | R.TRUNCATED) == "TRUNCATED"
    assert P.plan_reason(R.START_INVALID | R.GOAL_INVALID) == "START_INVALID, GOAL_INVALID"
    link = "panda_hand"
    li = w.ik_link_index(link)
    poses = np.array([w.fk_link_pose(goal[i], li) for i in range(4)])
    res = P.plan_to_pose_batch(w, link, poses, start[0], max_goals=2, **KW)
    assert len(res) == 4
    solved = [r for r in res if r["status"] == "Success"]
    assert len(solved) >= 2
    for pose, r in zip(poses, res):
        if r["status"] != "Success":
            continue
        np.testing.assert_array_equal(r["path"][0], start[0])
        end = np.array(w.fk_link_pose(r["path"][-1], li))
        assert P.distance_6d(pose[:3], pose[3:], end[:3], end[3:]) <= 1e-3
