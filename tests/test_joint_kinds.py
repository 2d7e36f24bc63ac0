"""CPU: every joint kind and tree shape, not only the Panda's (tests/zoo.py).

The oracle's forward kinematics against an independent numpy evaluator of the
URDF, the product's host loader against the oracle's, and the product's FK
copies that compile for the host (mpg_fk.h, the fp32 cull's bp_fk with its
frame saves and constant-joint folding, mpg_ik.h's step, kinjac.cpp's
Jacobians) on ZOO in two orderings and on the 20-joint LONG chain.  No device.
"""
import numpy as np
import pytest

import worlds as Wd
import zoo as Z
from oracle import model as M
from test_broadphase import MARGIN, _check
from test_host_fk import host_fk


@pytest.fixture(scope="module")
def zdir(tmp_path_factory):
    return tmp_path_factory.mktemp("zoo")


def test_inputs_cover_what_they_are_for(zdir):
    """Conditions on the inputs, asserted on oracle-side data: the joint kinds,
    the cull's save slots, chain lengths, dof and the collision rates."""
    zoo, perm, long_, mini = (Z.case(zdir, n) for n in Z.CASE_NAMES)
    pin = zoo.art.pin
    kinds = {pin.names[j]: pin.joint_type_name(j) for j in range(1, len(pin.joints))}
    assert kinds == Z.ZOO_KINDS
    assert sorted({kinds[n] for n in zoo.mg_names}) == Z.ALL_KINDS and len(Z.ALL_KINDS) == 12
    assert zoo.dof == 16 and perm.dof == 11 and long_.dof == 20 and mini.dof == 12
    mpin = mini.art.pin  # one joint of each kind, the third frame save spills
    assert sorted(mpin.joint_type_name(j) for j in range(1, len(mpin.joints))) == Z.ALL_KINDS
    assert Z.save_slots(Wd.desc_arrays(mini.ow)["joint_parent"]) == 3
    # the joints outside the permuted move group are non-zero constants: X, Y and unaligned revolutes among them
    assert sorted(perm.const) == sorted(set(kinds) - set(perm.mg_names)) and all(perm.const.values())
    assert {kinds[n] for n in perm.const} >= {"JointModelRUBX", "JointModelRY", "JointModelRUBY",
                                              "JointModelRevoluteUnaligned"}
    assert perm.mg_names != sorted(perm.mg_names, key=pin.names.index)  # the user order is not the model's
    for c in (zoo, perm):
        d = Wd.desc_arrays(c.ow)
        # frame saves of the fp32 cull (bp_build): two live in registers, the third and fourth spill
        assert Z.save_slots(d["joint_parent"]) >= 4
        assert max(len(pin.supports(f.parent)) for f in pin.frames) - 1 == 7
    dl = Wd.desc_arrays(long_.ow)
    assert Z.save_slots(dl["joint_parent"]) == 0
    chain = [len(long_.art.pin.supports(long_.art.pin.frames[f].parent)) - 1 for f in long_.art.link_frames]
    assert max(chain) == 20 and chain[long_.link_list().index("l11")] == 11
    assert long_.so2_mask >> 16 and long_.ow.W >= 7 and zoo.ow.W > 1
    for c in (zoo, perm, long_, mini):
        q = c.sample(1000, 3)
        f, m = c.ow.collide_batch(q, nthreads=4)
        ns = c.ow.n_self_pairs
        assert 0.05 <= f.mean() <= 0.95, (c.name, f.mean())
        assert any(Z.hit_and_free(m, p) for p in range(ns))
        assert any(Z.hit_and_free(m, p) for p in range(ns, len(c.ow.pairs)))
    # the URDF-borne spheres and the cylinder are collision objects of the oracle's world, and the narrow
    # phase decides about each of them: one of its pairs is hit in one row and free in another
    geoms = [type(o.geom).__name__ for o in zoo.art.objects]
    assert geoms.count("SphereGeom") == 2 and geoms.count("CylinderGeom") == 1
    for c in (zoo, perm):
        _, m = c.ow.collide_batch(c.sample(4096, 4), nthreads=4)
        for link in ("l7", "l12", "l9"):
            assert len(c.curved_pairs(link)) > 10 and any(Z.hit_and_free(m, p) for p in c.curved_pairs(link)), link


@pytest.mark.parametrize("name", Z.CASE_NAMES)
def test_oracle_fk_matches_independent_fk(zdir, name):
    """The oracle's link poses against ref_fk (numpy, Rodrigues, rpy as
    Rz Ry Rx) on 180 in-limit rows and 20 rows with angles in +-60 rad, every
    link, positions and rotation matrices (the oracle's rebuilt from its
    quaternion).  Tolerance 1e-12: the two differ in summation order only; a
    convention error (rpy order, axis normalisation, the sign of 0 0 -1) is
    1e-3 or more.  Measured maxima (position m, rotation entry):
    zoo 5.8e-16, 2.6e-15; zoo_perm 9.2e-16, 1.6e-15; long 1.3e-15, 2.7e-15;
    mini 4.4e-16, 1.6e-15."""
    c = Z.case(zdir, name)
    q = c.sample(200, 21, far=20)
    poses, _ = c.ow.fk_batch(q)
    dp = dR = 0.0
    for i in range(len(q)):
        ref = Z.ref_fk(c.urdf, c.q_by_name(q[i]))
        for k, link in enumerate(c.link_list()):
            T = ref(link)
            R = np.array(M.quat_to_mat(*poses[i, k, 3:])).reshape(3, 3)
            dp = max(dp, np.abs(T[:3, 3] - poses[i, k, :3]).max())
            dR = max(dR, np.abs(T[:3, :3] - R).max())
    print(f"{name}: oracle vs ref_fk max |dp| {dp:.2e} m, max |dR| {dR:.2e}")
    assert dp < 1e-12 and dR < 1e-12, (dp, dR)


@pytest.mark.parametrize("name", Z.CASE_NAMES)
def test_host_loader_equals_oracle(zdir, name):
    """The product's model of the URDF (ingest.cpp, kin.cpp) against the
    oracle's, exactly: joint names, types, parents and limits in the model's
    order, the user orders, the move group, the collision objects' links, the
    pair table and the motion space.  The joint axes and placements, the
    q sources and constants and the link placements have no host accessor:
    the Jacobian test below pins the geometry of every case to ref_fk, and the
    q sources and constants are pinned on the device, through the exact FK and
    collide comparisons of test_joint_kinds_gpu.py."""
    c = Z.case(zdir, name)
    w, art = Z.product_world(c)
    pin, opin = art.get_pinocchio_model(), c.art.pin
    assert pin.get_joint_names(False) == opin.names
    assert pin.get_joint_types(False)[1:] == [opin.joint_type_name(j) for j in range(1, len(opin.joints))]
    assert pin.get_parents(False)[1:] == [j.parent for j in opin.joints[1:]]
    assert pin.get_joint_dims(False)[1:] == [j.nv for j in opin.joints[1:]]
    assert pin.get_link_names(False) == opin.link_names()
    assert pin.get_joint_names(True) == c.art.user_joint_names
    assert pin.get_link_names(True) == c.art.user_link_names
    assert pin.get_joint_ids(True) == c.art.user_vidx and pin.get_joint_dims(True) == c.art.user_nv
    lims = [l[0] for l in pin.get_joint_limits(True) if l]
    np.testing.assert_array_equal(np.array(lims), c.art.joint_limits())
    assert [n for n in art.get_move_group_joint_names() if n != "universe"] == c.mg_names
    assert art.get_qpos_dim() == c.dof and w.get_state_dim() == c.dof
    np.testing.assert_array_equal(art.get_qpos(), c.full_qpos())
    fcl = art.get_fcl_model()
    assert fcl.get_collision_link_names() == [o.link for o in c.art.objects]
    assert [tuple(p) for p in fcl.get_collision_pairs()] == c.art.pairs
    info = w.get_collision_pair_info()
    assert [(i[3], i[4]) for i in info] == c.ow.pair_names()
    assert not any(i[5] for i in info) and w.get_mask_words() == c.ow.W
    so2, extent = w.get_motion_space()
    assert so2 == c.so2_mask and so2 != 0
    assert [n for i, n in enumerate(c.mg_names) if (so2 >> i) & 1] == \
        [n for n in c.mg_names if n.startswith(("j_c",)) or (name == "long" and int(n[1:]) % 7 in (3, 6))]
    assert abs(extent - c.extent) < 1e-12


@pytest.mark.parametrize("name", Z.CASE_NAMES)
def test_host_fk_equals_oracle(zdir, name):
    """mpg_fk.h compiled for the host: bit for bit the oracle's link poses."""
    c = Z.case(zdir, name)
    q = c.sample(2000, 22, far=200)
    np.testing.assert_array_equal(host_fk(Wd.desc_arrays(c.ow), q), c.ow.fk_batch(q)[0])


def _reach(c):
    """The robot's largest object-to-joint distance: an object's points lie
    within |its placement in the joint frame| + its bounding radius of the
    joint frame the cull carries it on (for a folded constant joint, of the
    nearest moving ancestor: the placements in between are added)."""
    art, pin = c.art, c.art.pin
    moving = {art.user_joints[i] for i in art.move_group}
    out = 0.0
    for o, l in zip(art.objects, art.obj_user_link):
        f = pin.frames[art.link_frames[l]]
        T, j = M.se3_mul(f.placement, o.origin), f.parent
        d = float(np.linalg.norm(T[1]))
        while j > 0 and j not in moving:
            d += float(np.linalg.norm(pin.joints[j].placement[1]))
            j = pin.joints[j].parent
        g = o.geom
        r = (0.5 * float(np.linalg.norm(g.side)) if isinstance(g, M.BoxGeom) else
             g.radius if isinstance(g, M.SphereGeom) else float(np.hypot(g.radius, 0.5 * g.lz)))
        out = max(out, d + r)
    return out


@pytest.mark.parametrize("name", Z.CASE_NAMES)
def test_fp32_cull_fk_within_margin(zdir, name):
    """bp_fk (every revolute and prismatic kind in fp32, the spilled frame
    saves, the folded constant joints) against the oracle on 20 000 in-limit
    rows and 2 000 rows with revolute and continuous values in +-60 rad: the
    three bounds of test_broadphase.py, the combined one with this robot's
    largest object-to-joint distance in place of the Panda's 0.3 m.
    Measured (dR, dRq, dp m; reach m): zoo 6.2e-7, 1.1e-6, 3.9e-7; 0.31.
    zoo_perm 5.3e-7, 1.1e-6, 4.0e-7; 0.86.  long 6.3e-7, 1.3e-6, 6.4e-7; 0.10.
    mini 4.6e-7, 8.5e-7, 2.7e-7; 0.31."""
    c = Z.case(zdir, name)
    dR, dRq, dp = _check(c.sample(22000, 23, far=2000), c.ow)
    reach = _reach(c)
    print(f"{name}: fp32 cull FK dR {dR:.2e} dRq {dRq:.2e} dp {dp:.2e} m, reach {reach:.3f} m")
    assert dp < MARGIN / 20, dp
    assert dR < 2e-5 and dRq < 2e-5, (dR, dRq)
    assert dp + reach * 3 ** 0.5 * dRq < MARGIN / 10


# ---------------------------------------------------------------- Jacobians, IK step
IK_LINKS = {"zoo": ["tip", "l13", "l7", "l14", "l9", "l12"], "long": ["l11", "l15"], "ikc": ["l8"],
            "mini": ["tip", "l13", "l7", "l8b", "l12"]}
IK_LINKS["zoo_perm"] = IK_LINKS["zoo"]


@pytest.mark.parametrize("name", Z.CASE_NAMES + ["ikc"])
def test_link_jacobians_match_finite_differences(zdir, name):
    """kinjac.cpp's WORLD and LOCAL link Jacobians on the product loader's
    model, for one link of every subtree, against central differences
    (h = 1e-6) of ref_fk; atol 1e-7 as in test_pinocchio_ik.py.  Every joint
    of the whole user qpos is a column -- in zoo_perm the permuted order and
    the joints outside the move group too -- so this pins the loader's joint
    axes, placements, parents and link placements for every case without a
    device (the product's own FK, compute_forward_kinematics, runs on one)."""
    c = Z.case(zdir, name)
    _, art = Z.product_world(c)
    pin = art.get_pinocchio_model()
    ua = c.art
    names = [n for n in ua.user_joint_names if n != "universe"]
    col = [ua.user_vidx[ua.user_joint_names.index(n)] for n in names]
    assert sorted(col) == list(range(len(names))) == sorted(pin.get_joint_ids(True)[-len(names):])
    lim = np.where(np.abs(ua.joint_limits()) > 3.1415, np.sign(ua.joint_limits()) * np.pi, ua.joint_limits())
    rng = np.random.default_rng(31)
    h = 1e-6

    def pose(vals, link):
        T = Z.ref_fk(c.urdf, dict(zip(names, vals)))(link)
        return T[:3, :3], T[:3, 3]

    for link in IK_LINKS[name]:
        li = c.link_list().index(link)
        for _ in range(2):
            q = rng.uniform(lim[:, 0], lim[:, 1])
            full = np.zeros(len(names))
            full[col] = q
            pin.compute_full_jacobian(list(full))
            Jw, Jl = pin.get_link_jacobian(li, False), pin.get_link_jacobian(li, True)
            R, p = pose(q, link)
            for j in range(len(names)):
                dq = np.zeros(len(names))
                dq[j] = h
                (Rp, pp), (Rm, pm) = pose(q + dq, link), pose(q - dq, link)
                dp = (pp - pm) / (2 * h)
                W = (Rp - Rm) / (2 * h) @ R.T
                w = np.array([W[2, 1] - W[1, 2], W[0, 2] - W[2, 0], W[1, 0] - W[0, 1]]) / 2
                msg = f"{link} {names[j]}"
                np.testing.assert_allclose(Jw[3:, col[j]], w, atol=1e-7, err_msg=msg)
                np.testing.assert_allclose(Jw[:3, col[j]], dp - np.cross(w, p), atol=1e-7, err_msg=msg)
                np.testing.assert_allclose(Jl[:3, col[j]], R.T @ dp, atol=1e-7, err_msg=msg)
                np.testing.assert_allclose(Jl[3:, col[j]], R.T @ w, atol=1e-7, err_msg=msg)


@pytest.mark.parametrize("name,link", [("zoo", "tip"), ("long", "l11"), ("ikc", "l8")])
def test_ik_header_one_step_matches_compute_ik_clik(zdir, name, link):
    """mpg_ik.h's ik_fk / ik_update compiled for the host, one step from 128
    starts, against the host compute_IK_CLIK (whose Jacobians the test above
    pins to ref_fk) on the rows with sigma_min(J) >= 1e-2: max |dq| <= 1e-9,
    test_ik_host.py's one-step bound (the Jacobian columns the header leaves
    are not reachable from outside it; a wrong column moves the step by 1e-3
    or more).  zoo/tip: 7 joints above, five kinds (RX, RY, RZ, unaligned
    revolute and prismatic); long/l11: 11 joints above, all seven LONG kinds,
    continuous joints whose values are integrated and never wrapped; ikc/l8:
    the other five kinds (PX, PZ, RUBX, RUBZ, unaligned continuous) and RX, RY, RZ.
    Measured max |dq|: zoo/tip 8.9e-16, long/l11 1.1e-16, ikc/l8 0 (bit-equal), 128 of 128 rows each."""
    import ik_cases as K
    c = Z.case(zdir, name)
    _, art = Z.product_world(c)
    pin = art.get_pinocchio_model()
    li = c.link_list().index(link)
    rng = np.random.default_rng(32)
    q_goal = rng.uniform(0.8 * c.lim[:, 0], 0.8 * c.lim[:, 1], size=(128, c.dof))
    q0 = np.clip(q_goal + rng.normal(scale=0.2, size=q_goal.shape), c.lim[:, 0], c.lim[:, 1])
    pose = np.ascontiguousarray(c.ow.fk_batch(q_goal)[0][:, li])
    ref = np.zeros_like(q0)
    smin = np.zeros(len(q0))
    for i in range(len(q0)):
        ref[i] = np.asarray(pin.compute_IK_CLIK(li, list(pose[i]), list(q0[i]), [], maxIter=1)[0])
        pin.compute_full_jacobian(list(q0[i]))
        smin[i] = np.linalg.svd(np.asarray(pin.get_link_jacobian(li, True)), compute_uv=False).min()
    d = Wd.desc_arrays(c.ow)
    lo = np.where(c.cont, -np.inf, c.lim[:, 0])
    hi = np.where(c.cont, np.inf, c.lim[:, 1])
    ref = K.np_check_joint_limit(ref, lo, hi, c.rot)[0]
    q, _, _, it = K.host_header_rows(pose, q0, max_iter=1, desc=d, link=li)
    well = smin >= 1e-2
    dq = np.abs(q - ref).max(axis=1)
    print(f"{name}/{link}: rows {int(well.sum())} max|dq| {dq[well].max():.2e} (all rows {dq.max():.2e})")
    assert well.sum() >= 32 and (it <= 1).all()
    assert np.abs(ref - q0).max() > 1e-3  # the step moved
    assert dq[well].max() <= 1e-9
