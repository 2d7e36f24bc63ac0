"""GPU: every joint kind and tree shape through the device paths (tests/zoo.py).

ZOO (all twelve joint kinds, four branch joints, fixed joints, URDF-borne
spheres and a cylinder) in the model's own orders and in permuted user orders
with a move group that ends mid-tree, its cut-down MINI that fits the resident
latency server, and the 20-joint LONG chain, against the
CPU oracle -- exactly (flags, every mask word, pose doubles) for FK, the bulk
pipeline, link-pose input, the latency path and motion validation, within the
existing one-step / path bounds for IK and screw planning.  The oracle's own
FK conventions for these robots are pinned by test_joint_kinds.py.
"""
import ctypes
import os

import numpy as np
import pytest

import ik_cases as K
import screw_cases as S
import worlds as Wd
import zoo as Z
from mplib_amd import _capi as C
from mplib_amd import pymp
from mplib_amd.batch import DeviceWorld

pytestmark = pytest.mark.gpu

NTHREADS = min(16, os.cpu_count() or 1)
_DW, _PW, _REF = {}, {}, {}


@pytest.fixture(scope="module")
def zdir(tmp_path_factory):
    return tmp_path_factory.mktemp("zoo")


def dw(c):
    """The C-ABI world of a case, built from the oracle's descriptor."""
    if c.name not in _DW:
        _DW[c.name] = DeviceWorld(Wd.desc_arrays(c.ow))
    return _DW[c.name]


def pw(c):
    """The product world of a case (its own loader)."""
    if c.name not in _PW:
        _PW[c.name] = Z.product_world(c)
    return _PW[c.name][0]


def oracle_collide(c, n, seed):
    """(q, flags, masks): a batch with one row in eight at +-60 rad in the
    rotating joints, and the oracle's answer (computed once per batch)."""
    key = (c.name, n, seed)
    if key not in _REF:
        q = c.sample(n, seed, far=n // 8)
        f, m = c.ow.collide_batch(q, nthreads=NTHREADS)
        for a in (q, f, m):
            a.setflags(write=False)
        _REF[key] = (q, f, m)
    return _REF[key]


def assert_both_outcomes(c, f, m):
    """A condition on the inputs (the oracle's output): the batch has hits and
    free rows, and a self pair and a robot-scene pair with both outcomes."""
    ns = c.ow.n_self_pairs
    assert 0.05 <= f.mean() <= 0.95, (c.name, f.mean())
    assert any(Z.hit_and_free(m, p) for p in range(ns))
    assert any(Z.hit_and_free(m, p) for p in range(ns, len(c.ow.pairs)))


def collide_link_poses(d, poses):
    n = len(poses)
    poses = np.ascontiguousarray(poses, dtype=np.float64)
    fl = np.zeros(n, np.uint8)
    pm = np.zeros((n, d.mask_words), np.uint32)
    C.check(C.lib().mpg_collide_link_poses(d.handle, poses.ctypes.data_as(ctypes.c_void_p), n,
                                           fl.ctypes.data_as(ctypes.c_void_p), pm.ctypes.data_as(ctypes.c_void_p),
                                           C.MPG_MEM_HOST, None), "mpg_collide_link_poses")
    return fl, pm


# ------------------------------------------------------------------------ FK
@pytest.mark.parametrize("n", [1, 63, 65, 1000])
@pytest.mark.parametrize("name", Z.CASE_NAMES)
def test_fk_equals_oracle(zdir, name, n):
    """mpg_fk_batch on every link, a quarter of the rows with the rotating
    joints (continuous ones too) at +-60 rad; through the product world's own
    model (fk_link_pose, and PinocchioModel.compute_forward_kinematics on the
    whole user qpos) on three rows of the 63-row batch."""
    c = Z.case(zdir, name)
    q = c.sample(n, 50 + n, far=(n + 3) // 4)
    want = c.ow.fk_batch(q)[0]
    np.testing.assert_array_equal(dw(c).fk_batch(q), want)
    if n == 63:
        w = pw(c)
        pin = _PW[c.name][1].get_pinocchio_model()
        ua = c.art
        slot = [ua.user_vidx[ua.user_joint_names.index(j)] for j in c.mg_names]
        for i in (0, 31, 62):
            full = np.array(c.full_qpos())  # the host model's own FK: the whole user qpos, constants included
            full[slot] = q[i]
            pin.compute_forward_kinematics(list(full))
            for l in range(len(c.link_list())):
                np.testing.assert_array_equal(w.fk_link_pose(q[i], l), want[i, l])
                np.testing.assert_array_equal(pin.get_link_pose(l), want[i, l])
        pin.compute_forward_kinematics(c.full_qpos())  # the shared model back at the articulation's qpos


# ---------------------------------------------------------------- bulk pipeline
@pytest.mark.parametrize("n", [1, 65, 4096])
@pytest.mark.parametrize("name", Z.CASE_NAMES)
def test_bulk_collide_equals_oracle(zdir, name, n):
    """The two-phase pipeline (fp32 cull with spilled frame saves and folded
    constant joints, narrow phase) through the product world, through the C ABI
    on the oracle's descriptor, and with the oracle's link poses as input."""
    c = Z.case(zdir, name)
    q, fo, mo = oracle_collide(c, n, 60 + n)
    if n > 1:
        assert_both_outcomes(c, fo, mo)
    if n == 4096 and name in ("zoo", "zoo_perm"):  # the narrow phase decides about each URDF sphere and the cylinder
        for link in ("l7", "l12", "l9"):
            assert any(Z.hit_and_free(mo, p) for p in c.curved_pairs(link)), link
    w, d = pw(c), dw(c)
    assert [(i[3], i[4]) for i in w.get_collision_pair_info()] == c.ow.pair_names()
    w.set_small_batch_max(0)
    d.set_small_batch_max(0)
    for f, m in (w.collide_batch(q), d.collide_batch(q), collide_link_poses(d, c.ow.fk_batch(q)[0])):
        np.testing.assert_array_equal(f, fo)
        np.testing.assert_array_equal(m, mo)


# ----------------------------------------------------------------- latency path
LAT_N = (1, 4, 64, 65, 200, 300)


@pytest.mark.parametrize("host_sc", [64, 0])
@pytest.mark.parametrize("server", [1, 0])
@pytest.mark.parametrize("name", Z.CASE_NAMES)
def test_latency_path_equals_oracle(zdir, name, server, host_sc, monkeypatch):
    """Host batches of 1, 4, 64, 65, 200 and 300 states through the one-launch
    latency path of a fresh world, with the host sin/cos limit at its default
    (64 states) and at 0.  The path a batch takes (mpg_collide_host.h):
    ZOO, zoo_perm, MINI (dof <= 16, chains <= 12): up to the host limit the
      sin/cos come from the host and the kernel reads the pair records
      (rec_side_tf; 1 and 4 states travel in the kernel arguments); above it
      and up to 256 states the kernel computes sin/cos inline and walks the
      staged joint table (stage_lat_joints, chain_oMi_lat) -- at 65 and 200
      states by default, at every size up to 256 with the host limit at 0;
      300 states take small_sincos_kernel and the generic FK.
    LONG (dof 20, chains of 20): no records and no inline sin/cos; up to the
      host limit host sin/cos with the generic FK, above it (every size with
      the limit at 0) small_sincos_kernel with the generic FK.
    The resident server, where it is on and the world fits it (MINI; ZOO
    holds more joints and objects than its LDS; LONG never), takes every
    batch of at most 32 states first.  The world exposes the server's state
    and counts; nothing exposes which kernel instance ran, so the list above
    is read from the host code and not asserted."""
    monkeypatch.setenv("MPG_SMALL_SERVER", str(server))
    monkeypatch.setenv("MPG_SMALL_SERVER_MAX", "32")
    monkeypatch.setenv("MPG_SMALL_HOST_SC", str(host_sc))
    c = Z.case(zdir, name)
    q, fo, mo = oracle_collide(c, 300, 70)
    assert_both_outcomes(c, fo, mo)
    for w in (Z.product_world(c)[0], DeviceWorld(Wd.desc_arrays(c.ow))):
        w.set_small_batch_max(1024)
        for n in LAT_N:
            for i in range(0, 128 if n <= 64 else 300, n):
                f, m = w.collide_batch(q[i:i + n])
                np.testing.assert_array_equal(f, fo[i:i + n])
                np.testing.assert_array_equal(m, mo[i:i + n])
        if isinstance(w, DeviceWorld):
            w.close()
            continue
        st = w.latency_server_stats()
        assert st["fallbacks"] == 0, st
        if name == "long" or not server:
            assert st["state"] == "unused" and st["served"] == 0, st
        elif name == "mini" or st["state"] != "unused":
            assert st["state"] == "in_use" and st["served"] == 128 + 32 and st["starts"] >= 1, st


# ------------------------------------------------------------ motion validation
def _motion_edges(c):
    """600 random edges + 257 hand-made ones on the continuous columns."""
    rng = np.random.default_rng(81)
    n = 600
    q_from = c.sample(n, 82)
    q_to = q_from + rng.normal(scale=rng.choice([0.02, 0.3, 1.0], size=(n, 1)), size=(n, c.dof))
    q_to = np.clip(q_to, c.lim[:, 0], c.lim[:, 1])
    cols = np.flatnonzero(c.cont)
    base = c.sample(257, 83)
    a, b = base.copy(), base.copy()
    pi = np.pi
    ends = [(0.0, pi), (pi, 0.0), (0.0, -pi),                                   # |delta| exactly pi
            (0.0, pi + 1e-12), (0.0, pi - 1e-12), (0.0, -pi - 1e-12), (0.0, -pi + 1e-12),
            (pi + 1e-12, 0.0), (-pi + 1e-12, 0.0), (-0.5, pi - 0.5),
            (3.0, -3.0), (-3.0, 3.0),                                           # through +-pi, wrapped
            (2.5, -2.0), (-2.9, 1.0), (1.0, 1.0)]
    for r in range(257):
        col = cols[r % len(cols)]
        lo, hi = ends[(r // len(cols)) % len(ends)]
        if r % 5 == 0:  # the edge's only motion is in this continuous joint
            a[r, col], b[r, col] = lo, hi
        elif r % 5 == 1:  # zero-length edge
            a[r, col] = b[r, col] = lo
        else:
            b[r] = np.clip(base[r] + rng.normal(scale=0.1, size=c.dof), c.lim[:, 0], c.lim[:, 1])
            a[r, col], b[r, col] = lo, hi
    assert (a[0] != b[0]).sum() == 1 and (a[1] == b[1]).all()
    return np.concatenate([a[:100], q_from, a[100:]]), np.concatenate([b[:100], q_to, b[100:]])


@pytest.mark.parametrize("name", Z.CASE_NAMES)
def test_check_motion_batch_with_continuous_joints(zdir, name):
    """check_motion_batch against zoo.motion_reference with so2_mask != 0:
    857 edges (they straddle the 256-thread blocks), among them continuous
    columns with |delta| exactly pi, pi +- 1e-12 in both directions, edges
    through +-pi that interpolate the short way and wrap, zero-length edges
    and edges that move one continuous joint only."""
    c = Z.case(zdir, name)
    w = pw(c)
    so2, extent = w.get_motion_space()
    assert so2 == c.so2_mask and so2 != 0 and abs(extent - c.extent) < 1e-12
    assert [i for i in range(c.dof) if (so2 >> i) & 1] == list(np.flatnonzero(c.cont))
    if name == "long":
        assert so2 >> 16
    q_from, q_to = _motion_edges(c)
    assert len(q_from) == 257 + 600
    rv, rf, rs = Z.motion_reference(q_from, q_to, 0.01 * extent, so2, c.ow, nthreads=NTHREADS)
    valid, first, segs = w.check_motion_batch(q_from, q_to)
    np.testing.assert_array_equal(segs, rs)
    np.testing.assert_array_equal(valid, rv)
    np.testing.assert_array_equal(first, rf)
    assert 0 < rv.sum() < len(rv) and rs.max() > 4


# --------------------------------------------------------------- IK and screw
IK_LINK = {"zoo": "tip", "long": "l11", "ikc": "l8"}


@pytest.mark.parametrize("name", ["zoo", "long", "ikc"])
def test_ik_one_step(zdir, name):
    """ik_batch, max_iter = 1, n = 1 and 65, against the host compute_IK_CLIK
    on rows with sigma_min(J) >= 1e-2: max |dq| <= 1e-9 (test_ik_batch.py's
    one-step bound).  zoo/tip has 7 joints above it, long/l11 11 of 20, ikc/l8
    all 8; between them the chains hold every joint kind.
    Measured max |dq| at n = 65: zoo 8.9e-16, long 4.4e-16, ikc 4.4e-16."""
    c = Z.case(zdir, name)
    w = pw(c)
    pin = _PW[c.name][1].get_pinocchio_model()
    li = c.link_list().index(IK_LINK[name])
    rng = np.random.default_rng(32)
    q_goal = rng.uniform(0.8 * c.lim[:, 0], 0.8 * c.lim[:, 1], size=(128, c.dof))
    q0 = np.clip(q_goal + rng.normal(scale=0.2, size=q_goal.shape), c.lim[:, 0], c.lim[:, 1])
    pose = np.ascontiguousarray(c.ow.fk_batch(q_goal)[0][:, li])
    ref, smin = np.zeros_like(q0), np.zeros(len(q0))
    for i in range(len(q0)):
        ref[i] = np.asarray(pin.compute_IK_CLIK(li, list(pose[i]), list(q0[i]), [], maxIter=1)[0])
        pin.compute_full_jacobian(list(q0[i]))
        smin[i] = np.linalg.svd(np.asarray(pin.get_link_jacobian(li, True)), compute_uv=False).min()
    lo, hi = np.where(c.cont, -np.inf, c.lim[:, 0]), np.where(c.cont, np.inf, c.lim[:, 1])
    ref = K.np_check_joint_limit(ref, lo, hi, c.rot)[0]
    well = np.flatnonzero(smin >= 1e-2)
    assert len(well) >= 65
    for n in (1, 65):
        idx = well[:n]
        q, st, _, it = w.ik_batch(IK_LINK[name], pose[idx], q_init=q0[idx].reshape(n, 1, c.dof), max_iter=1)
        d = np.abs(q[:, 0] - ref[idx]).max()
        print("%s one step n=%d: max|dq| %.3g" % (name, n, d))
        assert (it <= 1).all() and np.abs(ref[idx] - q0[idx]).max() > 1e-3
        assert d <= 1e-9


@pytest.mark.parametrize("name", ["zoo", "long", "ikc"])
def test_screw_paths(zdir, name):
    """plan_screw_batch, n = 1 and 65, against screw_cases.np_plan_screw on
    the rows whose sigma_min(J) stays >= 1e-2 along the path: status and
    waypoint count equal, max |dq| <= 1e-9 (test_screw_batch.py's bound).
    Measured max |dq| at n = 65: zoo 7.3e-15, long 6.6e-16, ikc 8.9e-16."""
    c = Z.case(zdir, name)
    w = pw(c)
    pin = _PW[c.name][1].get_pinocchio_model()
    li = c.link_list().index(IK_LINK[name])
    rng = np.random.default_rng(41)
    n = 96
    q0 = rng.uniform(0.6 * c.lim[:, 0], 0.6 * c.lim[:, 1], size=(n, c.dof))
    axis, angle = S.random_unit(rng, n), rng.uniform(0.05, 0.5, size=n)
    shift = S.random_unit(rng, n) * rng.uniform(0.02, 0.15, size=(n, 1))
    start = c.ow.fk_batch(q0)[0][:, li]
    goal = np.stack([S.moved_pose(start[i], axis[i], angle[i], shift[i]) for i in range(n)])
    lim = np.array([l[0] for l in pin.get_joint_limits(True) if l])
    ref = [S.np_plan_screw(goal[i], q0[i], pin=pin, fk=lambda q: c.ow.fk_batch(q[None])[0][0, li], lim=lim, pad=(),
                           link=li) for i in range(n)]
    well = np.flatnonzero([r[2] >= S.WELL and len(r[1]) <= 64 for r in ref])
    assert len(well) >= 65 and sum(ref[i][0] == S.REACHED for i in well) >= 5
    for k in (1, 65):
        idx = well[:k]
        path, cnt, st, _ = w.plan_screw_batch(IK_LINK[name], goal[idx], q0[idx])
        d = 0.0
        for r, i in enumerate(idx):
            assert (int(st[r]) & ~S.COLLISION_FREE) == ref[i][0] and cnt[r] == len(ref[i][1]), (i, st[r], cnt[r])
            d = max(d, np.abs(path[r][:cnt[r]] - ref[i][1]).max())
        print("%s screw n=%d: max|dq| %.3g" % (name, k, d))
        assert d <= 1e-9


def test_chains_beyond_the_ik_limit_are_refused(zdir):
    """LONG's last link has 20 joints above it: ik_batch and plan_screw_batch
    raise NotImplementedError naming the 15-joint limit, and the world still
    answers the next valid calls as the oracle does -- a fresh world, so the
    65 rows take the latency path and then, with the small-batch limit at 0,
    the bulk pipeline, whatever ran before this test."""
    c = Z.case(zdir, "long")
    w = Z.product_world(c)[0]
    q, fo, mo = oracle_collide(c, 65, 90)
    pose = np.ascontiguousarray(c.ow.fk_batch(q[:2])[0][:, c.link_list().index("l20")])
    with pytest.raises(NotImplementedError, match="15 joints"):
        w.ik_batch("l20", pose, q_init=q[:2].reshape(2, 1, c.dof), max_iter=1)
    with pytest.raises(NotImplementedError, match="15 joints"):
        w.plan_screw_batch("l20", pose, q[:2])
    for limit in (1024, 0):
        w.set_small_batch_max(limit)
        f, m = w.collide_batch(q)
        np.testing.assert_array_equal(f, fo)
        np.testing.assert_array_equal(m, mo)
    li = c.link_list().index("l15")  # exactly 15 joints above: accepted
    pose = np.ascontiguousarray(c.ow.fk_batch(q[:2])[0][:, li])
    _, st, _, _ = w.ik_batch("l15", pose, q_init=q[:2].reshape(2, 1, c.dof), max_iter=1000)
    assert ((st & C.MPG_IK_CONVERGED) != 0).all()


# -------------------------------------------------------------------- planner
def test_device_checker_plans_the_oracle_path(zdir):
    """RRTConnect on the permuted ZOO (two continuous joints in the move
    group), one seed: the device checker plans the oracle checker's path bit
    for bit, and every state and edge of it is valid by the oracle (edges by
    zoo.motion_reference).  On the CPU the query takes 245 iterations and
    2463 state checks."""
    c = Z.case(zdir, "zoo_perm")

    def oracle_checker(states):
        return c.ow.collide_batch(states)[0] == 0

    q = c.sample(400, 5)
    free = q[oracle_checker(q)]
    start, goal = free[27], free[28]
    dev = pymp.ompl.OMPLPlanner(Z.product_world(c)[0])
    ref = pymp.ompl.OMPLPlanner(Z.product_world(c)[0], state_validity_checker=oracle_checker)
    so2 = ref.get_state_space()[2]
    assert [bool(s) for s in so2] == list(c.cont)
    pymp.set_global_seed(0)
    s1, p1 = dev.plan(start, [goal], range=0.5, time=20.0)
    pymp.set_global_seed(0)
    s2, p2 = ref.plan(start, [goal], range=0.5, time=20.0)
    assert s1 == s2 == "Exact solution"
    assert np.array_equal(p1, p2) and len(p1) > 10
    assert np.array_equal(p1[0], start) and np.array_equal(p1[-1], goal)
    assert oracle_checker(p1).all()
    valid, _, _ = Z.motion_reference(p1[:-1], p1[1:], ref.get_state_space()[5], c.so2_mask, c.ow)
    assert valid.all()
