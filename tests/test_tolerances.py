"""CollisionRequest.gjk_tolerance and DistanceRequest.distance_tolerance off
their default of 1e-6: the oracle honours the request's tolerance, and the
device equals it on every path the tolerance reaches (the pipeline, the
one-launch small_kernel, the latency server, octree leaves, mesh triangles,
contacts, GST_INDEP's own GJK, the distance kernels and the Python surface).

What pins the oracle here.  The reference tree vendors neither FCL nor libccd,
so there is no reference run to compare the oracle's use of the tolerance
with.  It is pinned by citation (FCL 0.7.0: fcl::collide copies
request.gjk_tolerance into GJKSolver_libccd::collision_tolerance, which
GJKCollide stores as ccd.mpr_tolerance, and into GJKSolver_indep::
gjk_tolerance; oracle/collide_oracle.c orc_world.gjk_tolerance) and by the
properties that follow from the algorithms alone:

* libccd MPR: a larger tolerance ends refinePortal at the same or an earlier
  iteration of the same portal sequence, always with "no intersection", so
  hits(T_big) is a subset of hits(T_small): MPR never gains a pair bit.
* FCL's own GJK reports Inside once its ray is shorter than the tolerance, so
  a larger tolerance gains bits (shapes up to gjk_tolerance apart).
* The batch minimum of the distance entry point equals the brute-force
  minimum over the pairs at every tolerance.

Every "teeth" count below (how many oracle bits or values differ from the
oracle's own default-tolerance run on the same rows) is a condition on the
inputs, measured on the CPU and asserted from the oracle alone: a device that
ignored, clamped or mis-converted the tolerance fails the comparison on
exactly those bits."""
import ctypes
import os

import numpy as np
import pytest

import worlds as Wd

NTHREADS = min(16, os.cpu_count() or 1)
DEFAULT = 1e-6
# rows of Wd.sample_q(art, n, seed): seed 9001 + cfg (libccd) / 9101 + cfg
# (GST_INDEP); the point-cloud world counts as cfg 6 (worlds.oracle_world)
WORLDS = {2: (2, 4096), 3: (3, 4096), 4: (4, 4096),
          7: (7, 8192),         # 4096 rows lose 13 bits at 1e-2, 8192 lose 28 (all on mesh triangles)
          "cloud": (6, 4096)}   # the floor cloud: 64 lost at 1e-2, 31 of them on octree leaves
_BASE, _ORACLE, _REF = {}, {}, {}


def _base(name):
    if name not in _BASE:
        _BASE[name] = Wd.oracle_cloud_world("floor") if name == "cloud" else Wd.oracle_world(name)
    return _BASE[name]


def _oracle(name, tol=DEFAULT, solver="libccd"):
    """The world `name` with CollisionRequest(gjk_tolerance=tol, gjk_solver_type=solver)."""
    import oracle
    key = (name, tol, solver)
    if key not in _ORACLE:
        b = _base(name)
        _ORACLE[key] = oracle.OracleWorld(b.art, scene=b.scene, attached=b.attached,
                                          allowed=[tuple(p) for p in b.allowed], gjk_solver=solver, gjk_tolerance=tol)
    return _ORACLE[key]


def _rows(name, solver="libccd"):
    cfg, n = WORLDS[name]
    return Wd.sample_q(_base(name).art, n, (9101 if solver == "indep" else 9001) + cfg)


def _collide_ref(name, tol, solver="libccd"):
    """(q, flags, masks) of the oracle at `tol`, computed once and read-only."""
    key = (name, tol, solver)
    if key not in _REF:
        q = _rows(name, solver)
        f, m = _oracle(name, tol, solver).collide_batch(q, nthreads=NTHREADS)
        for a in (q, f, m):
            a.setflags(write=False)
        _REF[key] = (q, f, m)
    return _REF[key]


def _pair_bits(m, n_pairs):
    return np.stack([(m[:, p >> 5] >> (p & 31)) & 1 for p in range(n_pairs)], 1).astype(bool)


def _count(m):
    return int(np.unpackbits(np.ascontiguousarray(m).view(np.uint8)).sum())


def _teeth_first(name, tol, solver="libccd"):
    """Row order with the rows whose oracle masks differ from the default-
    tolerance run first (stable), so that short batches carry them."""
    _, _, m = _collide_ref(name, tol, solver)
    _, _, m0 = _collide_ref(name, DEFAULT, solver)
    return np.argsort(~(m != m0).any(1), kind="stable")


# ------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("name", [2, 3, 4, 7, "cloud"])
def test_mpr_never_gains_a_bit_and_loses_some(name):
    """hits(T_big) is a subset of hits(T_small) along 1e-9 -> 1e-6 -> 1e-3 ->
    1e-2, and at 1e-2 at least 20 pair bits of the default run are gone
    (measured: cfg2 32, cfg3 77, cfg4 118 on 4096 rows; cfg7 28 on 8192 rows
    -- 4096 rows lose 13 --, all of them mesh-triangle MPR against the scene
    boxes; the floor cloud 64 on 4096 rows, 31 of them octree-leaf MPR).  For
    cfg7 and the cloud the 20 are asked of those pairs alone, so the GPU
    tests below have teeth on the mesh and octree paths."""
    chain = [1e-9, DEFAULT, 1e-3, 1e-2]
    masks = [_collide_ref(name, t)[2] for t in chain]
    for small, big, t in zip(masks, masks[1:], chain[1:]):
        assert _count(big & ~small) == 0, ("gained at", t)
    ow = _base(name)
    lost = _pair_bits(masks[1], len(ow.pairs)) & ~_pair_bits(masks[3], len(ow.pairs))
    if name == 7:  # (mesh link, scene box): shapeTriangleIntersect's MPR
        lost = lost[:, ow.n_self_pairs:]
    elif name == "cloud":  # (link, cloud): the leaf boxes' MPR
        lost = lost[:, [k for k, (_, b) in enumerate(ow.pair_names()) if b == "scene_pcd"]]
    print(name, "bits lost at 1e-2:", int(lost.sum()))
    assert lost.sum() >= 20


def _brute_force_distance(ow, q, signed, tol):
    """min over the non-allowed pairs of fcl::distance, in pair order with
    strict '<', per group (PlanningWorld::distanceSelf / distanceOthers)."""
    import oracle
    _, objT = ow.fk_batch(q)
    scene_T = [np.asarray(oracle._se3_flat(s[2]), np.float64) for s in ow.scene]
    n = len(q)
    best = np.full((n, 2), np.finfo(np.float64).max)
    arg = np.full((n, 2), -1, np.int32)
    allowed = [frozenset((p[4], p[5])) in ow.allowed for p in ow.pairs]
    for i in range(n):
        for p, (ka, ia, kb, ib, _, _) in enumerate(ow.pairs):
            if allowed[p]:
                continue
            side = []
            for k, j in ((ka, ia), (kb, ib)):  # cfg3 / cfg4: robot and scene objects only
                side.append((ow._w.obj_geom[j], objT[i, j]) if k == 0 else (ow._w.scene_geom[j], scene_T[j]))
            d, _, _ = Wd.distance_pair_ex(ow, side[0][0], side[0][1], side[1][0], side[1][1], signed=signed,
                                          distance_tolerance=tol)
            g = 0 if p < ow.n_self_pairs else 1
            if d < best[i, g]:
                best[i, g], arg[i, g] = d, p
    return best, arg


@pytest.mark.parametrize("signed", [False, True])
@pytest.mark.parametrize("tol", [1e-4, 1e-2])
@pytest.mark.parametrize("cfg", [3, 4])
def test_oracle_distance_minimum_at_loose_tolerances(cfg, tol, signed):
    """Whatever the batch entry point skips (a bounding-sphere lower bound
    against the running minimum holds only up to the solver's error, which
    grows with the tolerance), its value and argmin pair equal the brute-force
    minimum of the single-pair entry point bit for bit."""
    ow = _base(cfg)
    q = _rows(cfg)[:64]
    ds, ps, _, do, po, _ = ow.distance_batch_ex(q, signed=signed, distance_tolerance=tol)
    best, arg = _brute_force_distance(ow, q, signed, tol)
    np.testing.assert_array_equal(ds, best[:, 0])
    np.testing.assert_array_equal(do, best[:, 1])
    np.testing.assert_array_equal(ps, arg[:, 0])
    np.testing.assert_array_equal(po, arg[:, 1])


@pytest.mark.parametrize("bad", [0.0, -1e-6, float("nan")])
def test_world_create_rejects_a_bad_gjk_tolerance(bad):
    """mpg_world_create validates before touching a device: MPG_E_INVALID
    (ValueError through _capi.check) for a tolerance that is not > 0."""
    from mplib_amd.batch import DeviceWorld
    with pytest.raises(ValueError, match="gjk_tolerance must be > 0"):
        DeviceWorld(Wd.desc_arrays(_base(3)), gjk_tolerance=bad)
    import oracle
    with pytest.raises(ValueError):
        oracle.OracleWorld(_base(3).art, gjk_tolerance=bad)


# ------------------------------------------------------------------------ GPU
def _device(name, tol=DEFAULT, solver="libccd"):
    from mplib_amd import _capi as C
    from mplib_amd.batch import DeviceWorld
    return DeviceWorld(Wd.desc_arrays(_oracle(name, tol, solver)), gjk_tolerance=tol,
                       gjk_solver=C.GJK_INDEP if solver == "indep" else C.GJK_LIBCCD)


def _server_stats(dw):
    from mplib_amd import _capi as C
    served, starts, fallbacks = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
    state = ctypes.c_int32(0)
    C.check(C.lib().mpg_latency_server_stats(dw.handle, ctypes.byref(served), ctypes.byref(starts),
                                             ctypes.byref(fallbacks), ctypes.byref(state)), "mpg_latency_server_stats")
    return dict(served=served.value, starts=starts.value, fallbacks=fallbacks.value, state=state.value)


def _check_collide(dw, q, fo, mo):
    f, m = dw.collide_batch(q)
    np.testing.assert_array_equal(f, fo)
    np.testing.assert_array_equal(m, mo)


@pytest.mark.gpu
@pytest.mark.parametrize("tol", [1e-9, 1e-3, 1e-2])
@pytest.mark.parametrize("name", [3, 4, 7, "cloud"])
def test_device_collide_libccd_tolerance(name, tol, monkeypatch):
    """libccd worlds at a non-default gjk_tolerance: every flag and pair bit
    of the oracle at the same tolerance, on the pipeline (all rows), the
    one-launch path (the first 512 rows, then the 512 that hold every row
    whose oracle masks differ from the default-tolerance run) and small
    batches of 1, 7 and 32 rows, those rows first -- the latency server where
    the world is eligible for it (cfg3, cfg4: served, never fallen back; a
    world with mesh or octree pairs never starts one and runs them as one
    launch).

    Teeth, oracle bits lost against 1e-6: at 1e-2 cfg3 77, cfg4 118, cfg7 28
    (mesh triangles), cloud 64 (31 on octree leaves); at 1e-3 cfg3 4, cfg4 8,
    cfg7 1, cloud 2.  At 1e-9 the oracle's masks equal the default run's, so
    that case cannot tell a device that ignores the tolerance from a correct
    one; it catches a tolerance that is clamped from below, flushed to zero or
    lost in a conversion (MPR would then run to its iteration cap or stop on
    another iteration), and a world whose creation or margins break on a tiny
    value."""
    monkeypatch.setenv("MPG_SMALL_SERVER", "1")
    monkeypatch.setenv("MPG_SMALL_SERVER_MAX", "32")
    q, fo, mo = _collide_ref(name, tol)
    if tol == 1e-2:  # a condition on the inputs, not on the device
        assert (mo != _collide_ref(name, DEFAULT)[2]).any()
    order = _teeth_first(name, tol)
    dw = _device(name, tol)
    try:
        dw.set_small_batch_max(0)
        _check_collide(dw, q, fo, mo)
        dw.set_small_batch_max(1024)
        _check_collide(dw, q[:512], fo[:512], mo[:512])
        head = order[:512]  # and the 512 rows that hold every differing row
        _check_collide(dw, q[head], fo[head], mo[head])
        for lo, hi in ((0, 1), (1, 8), (8, 40)):
            rows = order[lo:hi]
            _check_collide(dw, q[rows], fo[rows], mo[rows])
        st = _server_stats(dw)
        if name in (3, 4):
            assert st["state"] == 1 and st["served"] == 3 and st["fallbacks"] == 0, st
        else:
            assert st == dict(served=0, starts=0, fallbacks=0, state=0), st
    finally:
        dw.close()


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", [3, 4])
def test_device_contacts_at_a_loose_tolerance(cfg):
    """mpg_collide_contacts at gjk_tolerance 1e-2 on 256 rows: flags and masks
    equal, and libccd's MPR penetration (depth, normal, position) of every
    reported pair equals the oracle's at the same tolerance within 1e-9, zero
    elsewhere -- compared as test_gpu_parity.test_contacts_match_oracle
    compares at the default.  Teeth, the oracle's contacts at 1e-2 against its
    own at 1e-6 on these rows: cfg3 95 hits, 4 hits lost, 89 depths that
    differ by more than 1e-9 (up to 9.3 cm); cfg4 90, 9 and 88 (2.9 cm)."""
    from mplib_amd import _capi as C
    tol = 1e-2
    ow = _oracle(cfg, tol)
    q = _rows(cfg)[:256]
    n, P = len(q), len(ow.pairs)
    hit, rd, rn, rp = ow.contact_batch(q)
    fo, mo = ow.collide_batch(q)
    hit0, rd0, _, _ = _oracle(cfg, DEFAULT).contact_batch(q)
    h = hit.astype(bool)
    both = h & hit0.astype(bool)
    print(cfg, "contacts:", int(h.sum()), "hits lost vs 1e-6:", int((hit0.astype(bool) & ~h).sum()),
          "depths that differ by more than 1e-9:", int((np.abs(rd - rd0)[both] > 1e-9).sum()))
    assert h.sum() > 50 and (np.abs(rd - rd0)[both] > 1e-9).sum() >= 20
    dw = _device(cfg, tol)
    try:
        flags = np.zeros(n, np.uint8)
        masks = np.zeros((n, dw.mask_words), np.uint32)
        depth, normal, pos = np.zeros((n, P)), np.zeros((n, P, 3)), np.zeros((n, P, 3))
        v = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
        C.check(C.lib().mpg_collide_contacts(dw.handle, v(np.ascontiguousarray(q)), n, 0, v(flags), v(masks), v(depth),
                                             v(normal), v(pos), C.MPG_MEM_HOST, None), "mpg_collide_contacts")
    finally:
        dw.close()
    np.testing.assert_array_equal(flags, fo)
    np.testing.assert_array_equal(masks, mo)
    np.testing.assert_allclose(depth[h], rd[h], atol=1e-9)
    np.testing.assert_allclose(normal[h], rn[h], atol=1e-9)
    np.testing.assert_allclose(pos[h], rp[h], atol=1e-9)
    assert not depth[~h].any() and not normal[~h].any()


@pytest.mark.gpu
@pytest.mark.parametrize("tol", [1e-3, 1e-2, 5e-2])
@pytest.mark.parametrize("cfg", [3, 4])
def test_device_collide_gjk_indep_tolerance(cfg, tol):
    """GST_INDEP worlds (FCL's own GJK on the CF_GJK pairs) at a non-default
    gjk_tolerance: every bit of the oracle's on the pipeline (4096 rows) and
    the one-launch path (the first 512 rows, then 512 with the differing rows
    first).  GJK reports
    Inside for shapes up to gjk_tolerance apart, so 5e-2 lies above the libccd
    false-hit reach the cull of such a world used to stop at: the margins
    follow the tolerance (mpg_abi_world.h "culling margins").

    Teeth, oracle bits against 1e-6 (gained / lost): cfg3 23 / 48, 110 / 273,
    997 / 570; cfg4 8 / 27, 55 / 199, 563 / 460 at 1e-3, 1e-2, 5e-2."""
    q, fo, mo = _collide_ref(cfg, tol, "indep")
    m0 = _collide_ref(cfg, DEFAULT, "indep")[2]
    print(cfg, tol, "gained", _count(mo & ~m0), "lost", _count(m0 & ~mo))
    if tol == 5e-2:
        assert _count(mo & ~m0) >= 100
    head = _teeth_first(cfg, tol, "indep")[:512]
    dw = _device(cfg, tol, "indep")
    try:
        dw.set_small_batch_max(0)
        f, m = dw.collide_batch(q)
        print("pipeline: wrong bits", _count(m ^ mo), "of them missing", _count(mo & ~m))
        np.testing.assert_array_equal(f, fo)
        np.testing.assert_array_equal(m, mo)
        dw.set_small_batch_max(1024)
        for rows in (np.arange(512), head):
            f, m = dw.collide_batch(q[rows])
            print("one launch: wrong bits", _count(m ^ mo[rows]), "of them missing", _count(mo[rows] & ~m))
            np.testing.assert_array_equal(f, fo[rows])
            np.testing.assert_array_equal(m, mo[rows])
    finally:
        dw.close()


def _distance_req(dw, q, n_self, flags, tol, points):
    from mplib_amd import _capi as C
    n = len(q)
    req = C.DistanceRequest(flags=flags | (C.MPG_DISTANCE_NEAREST_POINTS if points else 0), distance_tolerance=tol)
    ds, do = np.zeros(n), np.zeros(n)
    ps, po = np.zeros(n, np.int32), np.zeros(n, np.int32)
    qs, qo = np.zeros((n, 6)), np.zeros((n, 6))
    v = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    rc = C.lib().mpg_distance_batch_req(dw.handle, v(np.ascontiguousarray(q)), n, n_self, ctypes.byref(req), v(ds), v(ps),
                                        v(qs), v(do), v(po), v(qo), C.MPG_MEM_HOST, None)
    return rc, (ds, ps, qs, do, po, qo)


@pytest.mark.gpu
@pytest.mark.parametrize("tol", [1e-9, 1e-4, 1e-2])
@pytest.mark.parametrize("variant", ["libccd", "libccd_signed", "indep"])
@pytest.mark.parametrize("cfg", [3, 4])
def test_device_distance_tolerance(cfg, variant, tol):
    """mpg_distance_batch_req at a non-default distance_tolerance, 1024 rows,
    with and without nearest points: distances, argmin pairs and points equal
    to the oracle's at the same tolerance (assert_array_equal, as the
    default-tolerance tests).  libccd unsigned, libccd signed (EPA; the rows
    past the lane's 96-vertex polytope would take distance_redo_kernel: these
    batches have none, the oracle's largest polytope is printed) and
    GST_INDEP unsigned.

    Teeth, self-distance values of the oracle that differ from its 1e-6 run
    (others group in brackets): libccd, signed or not, cfg3 152 (37) at 1e-4,
    872 (360) at 1e-2, 3 (4) at 1e-9; cfg4 126 (200), 885 (860), 1 (5);
    GST_INDEP cfg3 127 (80), 976 (883), 0 (1); cfg4 130 (335), 989 (901),
    0 (1).  At least 50 are asserted for tolerances >= 1e-4."""
    from mplib_amd import _capi as C
    solver = "indep" if variant == "indep" else "libccd"
    signed = variant == "libccd_signed"
    ow = _oracle(cfg, DEFAULT, solver)
    q = _rows(cfg)[:1024]
    flags = C.MPG_DISTANCE_GJK_INDEP if solver == "indep" else C.MPG_DISTANCE_SIGNED if signed else 0
    kw = dict(signed=signed, indep=solver == "indep")
    base = ow.distance_batch_ex(q, **kw)
    dw = _device(cfg, DEFAULT, solver)
    try:
        for points in (False, True):
            ow.epa_stats()
            ref = ow.distance_batch_ex(q, nearest_points=points, distance_tolerance=tol, **kw)
            if signed:
                print("largest EPA polytope:", ow.epa_stats()[0], "(redo rows need > 96)")
            differ = int((ref[0] != base[0]).sum())
            print(cfg, variant, tol, points, "self distances that differ from the 1e-6 run:", differ,
                  "others:", int((ref[3] != base[3]).sum()))
            if tol >= 1e-4:
                assert differ >= 50
            rc, got = _distance_req(dw, q, ow.n_self_pairs, flags, tol, points)
            C.check(rc, "mpg_distance_batch_req")
            for g, r in zip(got, ref):
                np.testing.assert_array_equal(g, r)
    finally:
        dw.close()


@pytest.mark.gpu
def test_distance_request_rejects_a_bad_tolerance():
    """mpg_distance_batch_req needs a world before it reads the request, so
    this check runs on a device: MPG_E_INVALID for a negative or NaN
    distance_tolerance, and the outputs stay untouched."""
    from mplib_amd import _capi as C
    ow = _base(3)
    dw = _device(3)
    try:
        for bad in (-1e-6, float("nan")):
            rc, got = _distance_req(dw, _rows(3)[:4], ow.n_self_pairs, 0, bad, False)
            assert rc == C.MPG_E_INVALID
            assert "distance_tolerance" in C.lib().mpg_last_error().decode()
            assert not any(a.any() for a in got)
    finally:
        dw.close()


@pytest.mark.gpu
def test_tolerances_through_the_python_api():
    """PlanningWorld on the cfg3 product world, 48 rows: collide_full with
    CollisionRequest(gjk_tolerance=1e-2) row by row equals the oracle at 1e-2,
    a default request the oracle at 1e-6, then 1e-2 again (the snapshot key
    holds the tolerance: a rebuild and a return); distance_batch with
    DistanceRequest(distance_tolerance=1e-4) -- not the default request's
    fast path -- equals the oracle at 1e-4, and a default request afterwards
    the oracle at 1e-6.  The rows start with those whose oracle masks differ
    between the two tolerances."""
    from mplib_amd import pymp, scenes
    w, _ = scenes.world(3)
    q_all, _, m_loose = _collide_ref(3, 1e-2)
    m_default = _collide_ref(3, DEFAULT)[2]
    rows = _teeth_first(3, 1e-2)[:48]
    q = np.ascontiguousarray(q_all[rows])
    assert ((m_loose != m_default).any(1)[rows]).sum() >= 20
    ow = _base(3)
    names = [(i[3], i[4]) for i in w.get_collision_pair_info()]
    assert names == ow.pair_names()
    for tol, masks in ((1e-2, m_loose), (DEFAULT, m_default), (1e-2, m_loose)):
        req = pymp.fcl.CollisionRequest() if tol == DEFAULT else pymp.fcl.CollisionRequest(gjk_tolerance=tol)
        for i, r in enumerate(rows):
            w.set_qpos_all(list(q[i]))
            got = sorted((c.link_name1, c.link_name2) for c in w.collide_full(req))
            assert got == sorted(ow.decode(masks[r])), (tol, i)
    loose = ow.distance_batch_ex(q, distance_tolerance=1e-4)
    default = ow.distance_batch_ex(q)
    assert (loose[0] != default[0]).any() or (loose[3] != default[3]).any()
    ds, ps, do, po, _, _ = w.distance_batch(q, request=pymp.fcl.DistanceRequest(distance_tolerance=1e-4))
    for g, r in ((ds, loose[0]), (ps, loose[1]), (do, loose[3]), (po, loose[4])):
        np.testing.assert_array_equal(g, r)
    ds, ps, do, po = w.distance_batch(q, request=pymp.fcl.DistanceRequest())
    for g, r in ((ds, default[0]), (ps, default[1]), (do, default[3]), (po, default[4])):
        np.testing.assert_array_equal(g, r)
