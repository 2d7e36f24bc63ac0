"""The cull's support-height tables and axes (mpg_broadphase.h), on the host.

1. ``bp_support_height`` is an upper bound of the exact fp64 support height of
   every Panda hull and of the cone / UV-sphere hulls of worlds.py.
2. Replay of the cull's two pair tests (the product's ``fobb_separated``, then
   ``bp_support_separated``) on the oracle's fp64 poses of the cfg3, cfg2 and
   cfg4 worlds: no pair the oracle reports as hit is dropped, and on cfg3 the
   support-height axes remove at least a quarter of the OBB survivors.
"""
import ctypes
import functools
import os
import zlib

import numpy as np
import pytest

import oracle
from oracle import model as M
import worlds as Wd
from native import host_shim

_FP = ctypes.POINTER(ctypes.c_float)
_DP = ctypes.POINTER(ctypes.c_double)
_lib = None

# the device's cull margin for worlds with MPR pairs (mpg_abi_world.h: libccd's
# false-hit reach, widened) and the support axes' pad kFp32CullRel * X, with
# X = 4 m above the coordinate bound of these worlds (reach 1.2 m, statics
# within 1 m, radii below 0.6 m)
MARGIN = np.float32(0.018581 * 1.001 + 1e-5)
SH_MARGIN = np.float32(float(MARGIN) + 4e-6 * 4.0)


def lib():
    global _lib
    if _lib is None:
        _lib = host_shim._build(os.path.join(os.path.dirname(host_shim.__file__), "support_height.cpp"),
                                "mplib_amd_support_height")
        _lib.sh_floats.restype = ctypes.c_int
        _lib.sh_k.restype = ctypes.c_int
    return _lib


def table_of(V):
    """(table, centre, extents) of hull V as the snapshot builds them."""
    V = np.ascontiguousarray(V, np.float64)
    c = np.zeros(3)
    e = np.zeros(3, np.float32)
    lib().sh_obb(V.ctypes.data_as(_DP), len(V), c.ctypes.data_as(_DP), e.ctypes.data_as(_FP))
    tab = np.zeros(lib().sh_floats(), np.float32)
    lib().sh_table(V.ctypes.data_as(_DP), len(V), c.ctypes.data_as(_DP), tab.ctypes.data_as(_FP))
    return tab, c, e


def heights(tab, dirs):
    dirs = np.ascontiguousarray(dirs, np.float32)
    out = np.zeros(len(dirs), np.float32)
    lib().sh_height(tab.ctypes.data_as(_FP), dirs.ctypes.data_as(_FP), ctypes.c_long(len(dirs)), out.ctypes.data_as(_FP))
    return out


def exact_heights(V, c, dirs):
    D = np.asarray(dirs, np.float32).astype(np.float64)
    out = np.full(len(D), -np.inf)
    P = np.asarray(V, np.float64) - c
    for k in range(0, len(P), 256):
        out = np.maximum(out, (D @ P[k:k + 256].T).max(axis=1))
    return out


@functools.lru_cache(maxsize=None)
def _hulls():
    art = Wd.panda_articulation()
    seen, out = [], []
    for o in art.objects:
        if isinstance(o.geom, M.ConvexGeom) and not any(o.geom is g for g in seen):
            seen.append(o.geom)
            out.append((o.link, o.geom.vertices))
    out.append(("cone_hull", Wd.cone_hull().vertices))
    out.append(("uv_sphere_hull", Wd.uv_sphere_hull().vertices))
    return out


def _grid_dirs():
    """Directions exactly on cell corners, cell edges, face edges and the axes."""
    K = lib().sh_k()
    g = -1.0 + 2.0 * np.arange(K + 1) / K            # cell corners along one ratio
    mid = -1.0 + 2.0 * (np.arange(4 * K + 1)) / (4 * K)  # corners and points inside the edges
    dirs = []
    for f in range(3):
        for sgn in (1.0, -1.0):
            for u in mid:
                for v in g:                            # on the cell edges v = const (corners included)
                    for (a, b) in ((u, v), (v, u)):
                        d = np.zeros(3)
                        d[f], d[(f + 1) % 3], d[(f + 2) % 3] = sgn, a, b
                        dirs.append(d)
            for u in mid:                              # the face's own edges (ties between faces)
                for e1 in (-1.0, 1.0):
                    for (a, b) in ((u, e1), (e1, u)):
                        d = np.zeros(3)
                        d[f], d[(f + 1) % 3], d[(f + 2) % 3] = sgn, a, b
                        dirs.append(d)
    dirs += [s * np.eye(3)[k] for k in range(3) for s in (1.0, -1.0)]
    D = np.asarray(dirs)
    return np.concatenate([D, 0.37 * D, 11.0 * D])     # other lengths: h is positively homogeneous


@pytest.mark.parametrize("name,V", _hulls(), ids=[h[0] for h in _hulls()])
def test_support_height_is_an_upper_bound(name, V):
    tab, c, _ = table_of(V)
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    rand = rng.normal(size=(100000, 3)) * rng.uniform(0.05, 20.0, size=(100000, 1))
    for what, dirs in (("random", rand), ("grid", _grid_dirs())):
        dirs = dirs.astype(np.float32)
        h = heights(tab, dirs).astype(np.float64)
        ex = exact_heights(V, c, dirs)
        bad = np.flatnonzero(~(h >= ex))
        assert bad.size == 0, (name, what, bad.size, float((ex - h).max()))
    # and not a loose one: within 2 % of the hull's radius on average
    r = np.linalg.norm(np.asarray(V) - c, axis=1).max()
    u = (rand / np.linalg.norm(rand, axis=1, keepdims=True)).astype(np.float32)
    assert float(np.mean(heights(tab, u) - exact_heights(V, c, u))) < 0.02 * r


def _sides(ow):
    """Per geometry of ow: (centre, extents, table or None) as bp_build /
    bp_build_support record them."""
    out = []
    for g in ow.geoms:
        if isinstance(g, M.ConvexGeom):
            tab, c, e = table_of(g.vertices)
            out.append((c, e, tab))
        elif isinstance(g, M.BoxGeom):
            V = np.array([[sx * g.side[0], sy * g.side[1], sz * g.side[2]]
                          for sx in (-.5, .5) for sy in (-.5, .5) for sz in (-.5, .5)])
            _, c, e = table_of(V)
            out.append((c, e, None))
        else:
            raise AssertionError("replay world with an unexpected geometry")
    return out


_REPLAY = {}


def replay(cfg):
    """(OBB survivors, survivors of the support axes, hits, hits dropped) over
    every non-allowed pair of world cfg on sample_q(art, 16384, 1)."""
    if cfg in _REPLAY:
        return _REPLAY[cfg]
    ow = Wd.oracle_world(cfg)
    q = Wd.sample_q(ow.art, 16384, 1)
    n = len(q)
    _, masks = ow.collide_batch(q, nthreads=min(8, os.cpu_count() or 1))
    _, objT = ow.fk_batch(q)
    sides = _sides(ow)
    gi = lambda g: next(i for i, gg in enumerate(ow.geoms) if gg is g)  # noqa: E731
    obj_g = [gi(o.geom) for o in ow.art.objects]
    scene_g = [gi(s[1]) for s in ow.scene]

    def side(kind, idx):
        if kind == oracle.KIND_ROBOT:
            return sides[obj_g[idx]], np.ascontiguousarray(objT[:, idx, :])
        assert kind == oracle.KIND_SCENE
        T = np.asarray(list(ow.scene[idx][2][0]) + list(ow.scene[idx][2][1]), np.float64)
        return sides[scene_g[idx]], np.ascontiguousarray(np.broadcast_to(T, (n, 12)))

    fp = lambda a: a.ctypes.data_as(_FP) if a is not None else None  # noqa: E731
    tot = np.zeros(4, np.int64)
    for p, pr in enumerate(ow.pairs):
        if frozenset((pr[4], pr[5])) in ow.allowed:
            continue
        (ca, ea, ta), Ta = side(pr[0], pr[1])
        (cb, eb, tb), Tb = side(pr[2], pr[3])
        out = np.zeros(n, np.uint8)
        lib().sh_replay(ca.ctypes.data_as(_DP), fp(ea), fp(ta), Ta.ctypes.data_as(_DP), cb.ctypes.data_as(_DP), fp(eb),
                        fp(tb), Tb.ctypes.data_as(_DP), ctypes.c_long(n), ctypes.c_float(MARGIN),
                        ctypes.c_float(SH_MARGIN), out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)))
        hit = ((masks[:, p >> 5] >> np.uint32(p & 31)) & 1).astype(bool)
        tot += (int((out >= 1).sum()), int((out == 2).sum()), int(hit.sum()), int((hit & (out != 2)).sum()))
    _REPLAY[cfg] = tuple(int(v) for v in tot)
    return _REPLAY[cfg]


@pytest.mark.parametrize("cfg", [3, 2, 4])
def test_replay_drops_no_hit(cfg):
    obb, kept, hits, dropped = replay(cfg)
    print(f"cfg{cfg}: OBB survivors {obb}, after the support axes {kept} "
          f"(removed {100.0 * (obb - kept) / obb:.1f} %), hits {hits}, hits dropped {dropped}")
    assert hits > 0 and dropped == 0


def test_replay_cfg3_removes_a_quarter():
    obb, kept, _, _ = replay(3)
    frac = (obb - kept) / obb
    print(f"cfg3: the support axes remove {100.0 * frac:.1f} % of the OBB survivors")
    assert frac >= 0.25
