"""The cull's fused pair test and the item list of its sincos pass, on the host.

1. ``bp_sat_support_separated`` (mpg_broadphase.h: the pair's frame formed once,
   the 15 SAT axes, then the support-height axes on the same values) decides
   what ``fobb_separated || bp_support_separated`` decides, for every
   non-allowed pair of the cfg2, cfg3 and cfg4 worlds on the oracle's fp64
   poses of ``sample_q(art, 16384, 1)`` -- with a table on both sides (a box
   takes the table of its eight corners), on either side alone and on neither.
2. ``bp_sincos_items`` gives every (compacted configuration, revolute source)
   to exactly one thread of the block, and ``revolute_sources`` lists what the
   joint-by-joint loop it replaces wrote.
"""
import ctypes
import os

import numpy as np
import pytest

import oracle
from oracle import model as M
import worlds as Wd
from native import host_shim

_FP = ctypes.POINTER(ctypes.c_float)
_DP = ctypes.POINTER(ctypes.c_double)
_IP = ctypes.POINTER(ctypes.c_int)
_lib = None

# the device's cull margin for worlds with MPR pairs and the support axes' pad
# (tests/test_support_height.py)
MARGIN = np.float32(0.018581 * 1.001 + 1e-5)
SH_MARGIN = np.float32(float(MARGIN) + 4e-6 * 4.0)
N, SEED = 16384, 1


def lib():
    global _lib
    if _lib is None:
        _lib = host_shim._build(os.path.join(os.path.dirname(host_shim.__file__), "cull_fused.cpp"),
                                "mplib_amd_cull_fused")
        _lib.cf_floats.restype = ctypes.c_int
        _lib.cf_rev_sources.restype = ctypes.c_int
        _lib.cf_sincos_items.restype = ctypes.c_long
    return _lib


def _side_of(g):
    """(centre, extents, table) of a geometry as bp_build / bp_build_support
    record a hull; a box is the hull of its corners."""
    if isinstance(g, M.ConvexGeom):
        V = np.ascontiguousarray(g.vertices, np.float64)
    else:
        assert isinstance(g, M.BoxGeom), "replay world with an unexpected geometry"
        V = np.array([[sx * g.side[0], sy * g.side[1], sz * g.side[2]]
                      for sx in (-.5, .5) for sy in (-.5, .5) for sz in (-.5, .5)])
    c = np.zeros(3)
    e = np.zeros(3, np.float32)
    lib().cf_obb(V.ctypes.data_as(_DP), len(V), c.ctypes.data_as(_DP), e.ctypes.data_as(_FP))
    tab = np.zeros(lib().cf_floats(), np.float32)
    lib().cf_table(V.ctypes.data_as(_DP), len(V), c.ctypes.data_as(_DP), tab.ctypes.data_as(_FP))
    return c, e, tab


MODES = {"both": (True, True), "a_only": (True, False), "b_only": (False, True), "neither": (False, False)}


@pytest.mark.parametrize("cfg", [3, 2, 4])
def test_fused_decision_equals_sat_or_support(cfg):
    ow = Wd.oracle_world(cfg)
    q = Wd.sample_q(ow.art, N, SEED)
    _, objT = ow.fk_batch(q)
    sides = [_side_of(g) for g in ow.geoms]
    gi = lambda g: next(i for i, gg in enumerate(ow.geoms) if gg is g)  # noqa: E731
    obj_g = [gi(o.geom) for o in ow.art.objects]
    scene_g = [gi(s[1]) for s in ow.scene]

    def side(kind, idx):
        if kind == oracle.KIND_ROBOT:
            return sides[obj_g[idx]], np.ascontiguousarray(objT[:, idx, :])
        assert kind == oracle.KIND_SCENE
        T = np.asarray(list(ow.scene[idx][2][0]) + list(ow.scene[idx][2][1]), np.float64)
        return sides[scene_g[idx]], np.ascontiguousarray(np.broadcast_to(T, (N, 12)))

    tot = {m: np.zeros(4, np.int64) for m in MODES}
    pairs = 0
    for pr in ow.pairs:
        if frozenset((pr[4], pr[5])) in ow.allowed:
            continue
        pairs += 1
        (ca, ea, ta), Ta = side(pr[0], pr[1])
        (cb, eb, tb), Tb = side(pr[2], pr[3])
        for m, (ua, ub) in MODES.items():
            lib().cf_compare(ca.ctypes.data_as(_DP), ea.ctypes.data_as(_FP), ta.ctypes.data_as(_FP) if ua else None,
                             Ta.ctypes.data_as(_DP), cb.ctypes.data_as(_DP), eb.ctypes.data_as(_FP),
                             tb.ctypes.data_as(_FP) if ub else None, Tb.ctypes.data_as(_DP), ctypes.c_long(N),
                             ctypes.c_float(MARGIN), ctypes.c_float(SH_MARGIN),
                             tot[m].ctypes.data_as(ctypes.POINTER(ctypes.c_longlong)))
    assert pairs > 0
    for m, t in tot.items():
        differ, by_sat, by_support, kept = (int(v) for v in t)
        print(f"cfg{cfg} {m}: {pairs} pairs x {N} poses, SAT separates {by_sat}, support axes {by_support}, "
              f"kept {kept}, decisions that differ {differ}")
        assert by_sat + by_support + kept == pairs * N
        assert by_sat > 0 and kept > 0 and (by_support > 0 or m == "neither")  # every branch of the decision is taken
        assert differ == 0
    # the tables matter: with both they separate more than with none
    assert tot["both"][2] > tot["neither"][2]


# revolute (aligned, unaligned, continuous), prismatic and fixed joints
_RX, _RU, _PX, _PU, _RUBZ = 0, 3, 4, 7, 10


def _joint_table(dof):
    """A joint table with dof move-group slots taken by joints of mixed kinds in
    a scrambled slot order, fixed joints (source -1) between them, and the last
    revolute slot driven by two joints."""
    kinds = [_RX, _PX, _RU, _RUBZ, _PU]
    rng = np.random.default_rng(dof)
    slots = rng.permutation(dof)
    jt, js = [], []
    for i, s in enumerate(slots):
        jt.append(kinds[i % len(kinds)] if dof > 1 else _RX)
        js.append(int(s))
        if i % 3 == 1:
            jt.append(_RX)  # a joint outside the move group
            js.append(-1)
    rev = [s for t, s in zip(jt, js) if s >= 0 and t in (_RX, _RU, _RUBZ)]
    jt.append(_RX)  # a second joint on an already listed slot
    js.append(rev[-1])
    return np.array(jt, np.int32), np.array(js, np.int32)


@pytest.mark.parametrize("block", [64, 128, 256])
@pytest.mark.parametrize("dof", [1, 7, 16])
def test_sincos_items_visit_each_element_once(dof, block):
    jt, js = _joint_table(dof)
    out = np.zeros(len(jt), np.int32)
    n_rev = lib().cf_rev_sources(jt.ctypes.data_as(_IP), js.ctypes.data_as(_IP), len(jt), out.ctypes.data_as(_IP))
    src = out[:n_rev]
    # the plain loop: every joint in order, its slot if revolute and in the group
    plain = [int(s) for t, s in zip(jt, js) if s >= 0 and (t <= _RU or t >= 8)]
    assert sorted(set(plain)) == sorted(src.tolist()) and len(set(src.tolist())) == n_rev
    assert list(dict.fromkeys(plain)) == src.tolist()  # joint order, each slot once
    assert 0 < n_rev <= dof and (dof == 1 or n_rev < dof)
    for total in (0, 1, block - 1, block):
        visits = np.zeros(max(total * n_rev, 1), np.int32)
        bad = lib().cf_sincos_items(block, total, n_rev, visits.ctypes.data_as(_IP))
        assert bad == 0
        want = np.zeros_like(visits)
        for k in range(total):       # the plain loop over (configuration, revolute source)
            for r in range(n_rev):
                want[k * n_rev + r] += 1
        np.testing.assert_array_equal(visits, want)


def test_sincos_items_without_revolute_joints():
    jt, js = np.array([_PX, _RX], np.int32), np.array([0, -1], np.int32)
    out = np.zeros(2, np.int32)
    assert lib().cf_rev_sources(jt.ctypes.data_as(_IP), js.ctypes.data_as(_IP), 2, out.ctypes.data_as(_IP)) == 0
    visits = np.zeros(1, np.int32)
    assert lib().cf_sincos_items(256, 256, 0, visits.ctypes.data_as(_IP)) == 0 and visits[0] == 0
