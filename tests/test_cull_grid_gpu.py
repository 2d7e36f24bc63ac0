"""The cull's lookup grids on the device: flags and pair masks of the bulk
path (set_small_batch_max(0): cull_kernel) equal the oracle's wherever the
lookups replace the moving-static sphere tests, and wherever they must not.
"""
import ctypes
import functools
import os

import numpy as np
import pytest

import oracle
from oracle import model as M
import worlds as Wd

gpu = pytest.mark.gpu
NTHREADS = min(16, os.cpu_count() or 1)


@functools.lru_cache(maxsize=None)
def ow3():
    return Wd.oracle_world(3)


@functools.lru_cache(maxsize=None)
def ref3():
    """q and the oracle's answer for 4096 cfg3 rows (computed once, read-only)."""
    q = Wd.sample_q(ow3().art, 4096, 31)
    f, m = ow3().collide_batch(q, nthreads=NTHREADS)
    for a in (q, f, m):
        a.setflags(write=False)
    return q, f, m


def bulk_world(ow):
    from mplib_amd.batch import DeviceWorld
    d = DeviceWorld(Wd.desc_arrays(ow))
    d.set_small_batch_max(0)
    return d


def check(d, q, fo, mo):
    f, m = d.collide_batch(np.ascontiguousarray(q))
    np.testing.assert_array_equal(f, fo)
    np.testing.assert_array_equal(m, mo)


def grids(d, at_least=1, built=True):
    """mpg_cull_grid_info of world d: at least so many objects have a grid, and
    the words are built (or not yet); returns the record."""
    g = d.cull_grid_info()
    assert len(g["objects"]) >= at_least and g["cells"] > 0 and 0.02 <= g["cell_edge"] <= 0.0801, g
    assert g["cells"] <= 1 << 19 and g["partners"].min() >= 6 and g["partners"].max() <= 32, g
    assert g["built"] == built, g
    return g


@gpu
@pytest.mark.parametrize("n", [1, 63, 65, 4096])
def test_cfg3_sizes(n):
    q, fo, mo = ref3()
    assert 0 < int(fo.sum()) < len(fo)
    d = bulk_world(ow3())
    grids(d, 6, built=False)
    check(d, q[:n], fo[:n], mo[:n])
    grids(d, 6)


@gpu
def test_centres_next_to_the_grid_box_faces():
    """link2's centre rides a sphere about the fixed origin of joints 1 and 2,
    so it touches the faces of its grid box (the cube about that sphere): rows
    that put it within a cell of the +-x and +-y faces, and boxes right
    there."""
    import test_cull_grid as TG
    import test_support_height as SH
    art = Wd.panda_articulation()
    m = next(i for i, o in enumerate(art.objects) if o.link == "panda_link2")
    probe = oracle.OracleWorld(art, scene=Wd.boxes_scene())
    gi = lambda g: next(i for i, gg in enumerate(probe.geoms) if gg is g)  # noqa: E731
    c_loc = SH._sides(probe)[gi(art.objects[m].geom)][0]
    cen = [np.zeros(3)] * len(art.objects)
    cen[m] = c_loc
    lo, hi = TG.reach_boxes(probe, cen)
    rng = np.random.default_rng(5)
    q = Wd.sample_q(art, 2048, 6)
    q[:, 0] = rng.choice([0.0, np.pi / 2, -np.pi / 2, 2.8], len(q)) + rng.uniform(-0.05, 0.05, len(q))
    q[:, 1] = rng.choice([-1.0, 1.0], len(q)) * rng.uniform(1.35, 1.76, len(q))
    _, objT = probe.fk_batch(q)
    c = objT[:, m, :9].reshape(-1, 3, 3) @ c_loc + objT[:, m, 9:]
    gap = np.minimum(c[:, :2] - lo[m][:2], hi[m][:2] - c[:, :2]).min(axis=1)
    assert gap.min() >= 0.0 and int((gap < 0.04).sum()) >= 50, (float(gap.min()), int((gap < 0.04).sum()))
    r = float(hi[m][0] - lo[m][0]) / 2
    o = (lo[m] + hi[m]) / 2
    at = [(sx * (r + 0.12), sy * 0.05) for sx in (1, -1) for sy in (1, -1)] + [(sx * 0.05, sy * (r + 0.12)) for sy in (1, -1) for sx in (1, -1)]
    scene = [(f"face{k}", M.BoxGeom((0.06, 0.06, 0.3)), (list(M.IDENT[0]), [float(o[0] + dx), float(o[1] + dy), float(o[2])]))
             for k, (dx, dy) in enumerate(at)]  # eight: enough partners for link2 to have a grid
    ow = oracle.OracleWorld(art, scene=scene)
    fo, mo = ow.collide_batch(q, nthreads=NTHREADS)
    names = ow.pair_names()
    hits = sum(int(((mo[:, p >> 5] >> np.uint32(p & 31)) & 1).sum()) for p, pn in enumerate(names) if pn[1].startswith("face"))
    assert hits > 0
    d = bulk_world(ow)
    check(d, q, fo, mo)
    g = grids(d)
    k = list(g["objects"]).index(m)  # link2 has a grid; the rows against the box the library made
    lo_p, hi_p = g["box"][k, :3], g["box"][k, 3:]
    cf = c.astype(np.float32).astype(np.float64)
    gap = np.minimum(cf[:, :2] - lo_p[:2], hi_p[:2] - cf[:, :2]).min(axis=1)
    assert gap.min() >= 0.0 and int((gap < g["cell_edge"]).sum()) >= 50, (float(gap.min()), int((gap < g["cell_edge"]).sum()))


@gpu
def test_33_statics_some_objects_keep_the_loop():
    """cfg3's boxes and 23 small ones inside the arm's reach: the far links
    have more than 32 static partners the reach ball does not exclude."""
    rng = np.random.default_rng(33)
    scene = Wd.boxes_scene()
    for k in range(23):
        side = rng.uniform(0.02, 0.08, size=3)
        pos = rng.uniform([-0.5, -0.5, 0.1], [0.6, 0.5, 0.9])
        scene.append((f"extra{k}", M.BoxGeom(tuple(float(s) for s in side)), (list(M.IDENT[0]), [float(v) for v in pos])))
    assert len(scene) == 33
    ow = oracle.OracleWorld(Wd.panda_articulation(), scene=scene, allowed=[("panda_link0", "table")])
    q = Wd.sample_q(ow.art, 2048, 34)
    fo, mo = ow.collide_batch(q, nthreads=NTHREADS)
    assert 0 < int(fo.sum()) < len(fo)
    d = bulk_world(ow)
    check(d, q, fo, mo)
    g = grids(d)
    partners = [sum(1 for p, pr in enumerate(ow.pairs) if pr[0] == oracle.KIND_ROBOT and pr[1] == m and
                    pr[2] == oracle.KIND_SCENE and frozenset((pr[4], pr[5])) not in ow.allowed)
                for m in range(len(ow.art.objects))]
    assert max(partners) == 33
    assert len(g["objects"]) < sum(1 for k in partners if k >= 6)  # some object kept the loop


@gpu
def test_movable_objects_world():
    """A world with free frames answers joint-value rows through link poses,
    so it has no grid at all; the shared rows of tests/test_movable_objects.py
    with per-row poses, and the same world asked without poses."""
    import test_movable_objects as TM
    from mplib_amd.batch import DeviceWorld
    q, P, fo, mo = TM.shared()
    g = DeviceWorld(TM.free_desc(ow3(), TM.MOVABLE)).cull_grid_info()
    assert len(g["objects"]) == 0 and g["cells"] == 0 and not g["built"], g
    wm, _ = TM.movable_world()
    wm.set_small_batch_max(0)
    f, m = wm.collide_batch(q, object_poses={name: P[:, k] for k, name in enumerate(TM.MOVABLE)})
    np.testing.assert_array_equal(f, fo)
    np.testing.assert_array_equal(m, mo)
    f0, m0 = ow3().collide_batch(q, nthreads=NTHREADS)
    f, m = wm.collide_batch(q)  # the objects where the scene put them: cfg3
    np.testing.assert_array_equal(f, f0)
    np.testing.assert_array_equal(m, m0)


@gpu
def test_prismatic_joint_beyond_its_bound():
    """The Panda on a 0.3 m rail (small enough for the grids): rows with the
    rail value far outside its limits are evaluated with every pair."""
    from mplib_amd import scenes
    from test_multi_art import RAIL_AT, RAIL_JOINTS, rail_panda_urdf
    urdf = rail_panda_urdf(0.0, 0.3)
    scene = []
    for name, side, pos in scenes._boxes():
        p = [RAIL_AT[0] + 0.2 + pos[0], RAIL_AT[1] + pos[1], RAIL_AT[2] + pos[2]]
        scene.append((name, M.BoxGeom(tuple(float(x) for x in side)), (list(M.IDENT[0]), [float(x) for x in p])))
    oart = M.Articulation(urdf, os.path.join(Wd.panda_dir(), "panda.srdf"), Wd.PANDA_LINKS, RAIL_JOINTS, convex=True,
                          move_group="panda_hand")
    ow = oracle.OracleWorld(oart, scene=scene, allowed=[("panda_link0", "table")])
    lim = oart.joint_limits()[:8]
    rng = np.random.default_rng(8)
    q = rng.uniform(lim[:, 0], lim[:, 1], size=(2048, 8))
    q[1024:, 0] = rng.choice([-1.0, 1.0], 1024) * rng.uniform(0.5, 4.0, 1024)  # forced rows
    fo, mo = ow.collide_batch(q, nthreads=NTHREADS)
    assert 0 < int(fo[:1024].sum()) < 1024
    d = bulk_world(ow)
    check(d, q, fo, mo)
    grids(d, 6)


@gpu
def test_link_pose_input_is_unchanged():
    from mplib_amd import _capi as C
    q, fo, mo = ref3()
    d = bulk_world(ow3())
    n = 2048
    poses = np.ascontiguousarray(d.fk_batch(np.ascontiguousarray(q[:n])))
    fl = np.zeros(n, np.uint8)
    pm = np.zeros((n, d.mask_words), np.uint32)
    C.check(C.lib().mpg_collide_link_poses(d.handle, poses.ctypes.data_as(ctypes.c_void_p), n,
                                           fl.ctypes.data_as(ctypes.c_void_p), pm.ctypes.data_as(ctypes.c_void_p),
                                           C.MPG_MEM_HOST, None), "mpg_collide_link_poses")
    np.testing.assert_array_equal(fl, fo[:n])
    np.testing.assert_array_equal(pm, mo[:n])


@gpu
def test_two_worlds_each_use_their_own_table():
    """cfg3 and the eight rotated statics of tests/test_cull_grid.py alive at
    once, calls interleaved; both have grids, of different sizes."""
    import test_cull_grid as TG
    q, fo, mo = ref3()
    orot = TG.rotated_statics_world()
    fr, mr = orot.collide_batch(q[:2048], nthreads=NTHREADS)
    assert 0 < int(fr.sum()) < len(fr)
    a, b = bulk_world(ow3()), bulk_world(orot)
    for _ in range(2):
        check(a, q[:2048], fo[:2048], mo[:2048])
        check(b, q[:2048], fr, mr)
    ga, gb = grids(a, 6), grids(b, 6)
    assert ga["cells"] != gb["cells"] or not np.array_equal(ga["partners"], gb["partners"])


@gpu
@pytest.mark.parametrize("name", [3, "rotated"])
def test_library_boxes_hold_every_centre(name):
    """The boxes mpg_world_create made (mpg_cull_grid_info) hold the fp32
    centre of every gridded object in 10^5 sampled configurations (fp64 FK)."""
    import test_cull_grid as TG
    ow, _, _, _, cen = TG.world_grid(name)
    g = grids(bulk_world(ow), 6, built=False)
    _, objT = ow.fk_batch(Wd.sample_q(ow.art, 100000, 5))
    for k, m in enumerate(g["objects"]):
        c = (objT[:, m, :9].reshape(-1, 3, 3) @ cen[m] + objT[:, m, 9:]).astype(np.float32).astype(np.float64)
        assert np.all(c >= g["box"][k, :3]) and np.all(c < g["box"][k, 3:]), (name, int(m))


@gpu
def test_first_bulk_call_after_latency_calls():
    """The grids are built by the first bulk launch, not by world creation or
    the latency path."""
    from mplib_amd.batch import DeviceWorld
    q, fo, mo = ref3()
    d = DeviceWorld(Wd.desc_arrays(ow3()))
    grids(d, 6, built=False)
    for k in range(20):
        f, m = d.collide_batch(np.ascontiguousarray(q[8 * k:8 * k + 8]))
        np.testing.assert_array_equal(f, fo[8 * k:8 * k + 8])
        np.testing.assert_array_equal(m, mo[8 * k:8 * k + 8])
    grids(d, 6, built=False)
    d.set_small_batch_max(0)
    check(d, q, fo, mo)
    grids(d, 6)
    check(d, q[:65], fo[:65], mo[:65])
