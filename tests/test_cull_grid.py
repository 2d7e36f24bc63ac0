"""The cull's lookup grids (mpg_broadphase.h bp_grid_*), on the host.

1. Soundness of the bits: for points all over the grids -- random ones, points
   a few fp32 ulps either side of cell faces, the box's own faces and corners
   -- every partner the product's fp32 sphere test keeps, and every partner
   whose fp64 sphere-OBB distance is within radius + margin, has its bit in
   the word the cull's index arithmetic picks.  cfg3's statics and the rotated
   statics of tests/test_cull_support_axes.py.
2. The boxes (the chain-length reach argument of world creation, restated
   here) hold every object centre of 10^5 sampled configurations (fp64 FK).
3. Replay on the oracle's fp64 poses of sample_q(art, 16384, 1), cfg3, cfg4
   (no grid there: four partners per object) and the rotated statics:
   sphere test -> SAT -> support axes against lookup -> SAT -> support axes.
   No oracle hit is dropped, no sphere keep is missing from the lookup,
   and the lookup's final candidates exceed the sphere path's by at most 1 %.
4. Budget and fallback decisions depend on the inputs alone; 6 and 32
   partners get a grid, 5, 33 and 0 do not.

The builder also runs as a program of its own (tests/native/cull_grid.cpp with
-DCULL_GRID_MAIN) under ASan and UBSan.
"""
import ctypes
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import oracle
from oracle import model as M
import worlds as Wd
from native import host_shim
import test_support_height as SH
from test_cull_support_axes import rotated_scene_world

_FP = ctypes.POINTER(ctypes.c_float)
_DP = ctypes.POINTER(ctypes.c_double)
_IP = ctypes.POINTER(ctypes.c_int)
_UP = ctypes.POINTER(ctypes.c_uint32)
MARGIN = SH.MARGIN            # the device's cull margin of these worlds
X = 4.0                       # above their coordinate bound (test_support_height.py)
BUDGET = 1 << 19
_SRC = os.path.join(os.path.dirname(host_shim.__file__), "cull_grid.cpp")
_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = host_shim._build(_SRC, "mplib_amd_cull_grid")
        _lib.grid_new.restype = ctypes.c_void_p
        _lib.grid_h.restype = ctypes.c_double
        _lib.grid_cell_pad.restype = ctypes.c_double
        _lib.grid_cells.restype = ctypes.c_longlong
        _lib.grid_hash.restype = ctypes.c_ulonglong
        _lib.grid_widen.restype = ctypes.c_float
        for f in (_lib.grid_free, _lib.grid_h, _lib.grid_cell_pad, _lib.grid_cells, _lib.grid_hash):
            f.argtypes = [ctypes.c_void_p]
        _lib.grid_slot.argtypes = [ctypes.c_void_p, ctypes.c_int]
        _lib.grid_dims.argtypes = [ctypes.c_void_p, ctypes.c_int, _IP, _FP]
        _lib.grid_lookup.argtypes = [ctypes.c_void_p, ctypes.c_int, _FP, ctypes.c_long, _UP, _IP]
        _lib.grid_sphere.argtypes = [ctypes.c_void_p, ctypes.c_int, _FP, ctypes.c_long, ctypes.c_float, _UP]
        _lib.grid_widen.argtypes = [ctypes.c_double]
    return _lib


class Grid:
    def __init__(self, lo, hi, r, partners, sobj, budget=BUDGET):
        lo, hi, r = (np.ascontiguousarray(a, np.float64) for a in (lo, hi, r))
        npart = np.asarray([len(p) for p in partners], np.int32)
        sid = np.asarray([s for p in partners for s in p] + [0], np.int32)
        self.sobj = np.ascontiguousarray(sobj, np.float32)
        self.partners = partners
        self.r = r
        self._free = lib().grid_free
        self.h = lib().grid_new(len(r), lo.ctypes.data_as(_DP), hi.ctypes.data_as(_DP), r.ctypes.data_as(_DP),
                                npart.ctypes.data_as(_IP), sid.ctypes.data_as(_IP), len(self.sobj),
                                self.sobj.ctypes.data_as(_FP), ctypes.c_double(X), ctypes.c_double(float(MARGIN)),
                                ctypes.c_longlong(budget))

    def __del__(self):
        self._free(self.h)

    def slot(self, cand):
        return lib().grid_slot(self.h, cand)

    def dims(self, slot):
        n = np.zeros(3, np.int32)
        o = np.zeros(3, np.float32)
        lib().grid_dims(self.h, slot, n.ctypes.data_as(_IP), o.ctypes.data_as(_FP))
        return n, o

    def lookup(self, slot, c):
        c = np.ascontiguousarray(c, np.float32)
        out = np.zeros(len(c), np.uint32)
        cell = np.zeros(len(c), np.int32)
        lib().grid_lookup(self.h, slot, c.ctypes.data_as(_FP), len(c), out.ctypes.data_as(_UP), cell.ctypes.data_as(_IP))
        return out, cell

    def sphere(self, slot, c):
        c = np.ascontiguousarray(c, np.float32)
        out = np.zeros(len(c), np.uint32)
        lib().grid_sphere(self.h, slot, c.ctypes.data_as(_FP), len(c), ctypes.c_float(MARGIN), out.ctypes.data_as(_UP))
        return out


def static_records(ow, sides):
    """The cull's fp32 static records (BS_C, BS_R, BS_E) as bp_build makes them."""
    gi = lambda g: next(i for i, gg in enumerate(ow.geoms) if gg is g)  # noqa: E731
    rec = np.zeros((len(ow.scene), 16), np.float32)
    for s, (_, g, T) in enumerate(ow.scene):
        c, e, _ = sides[gi(g)]
        R = np.asarray(T[0], np.float64).reshape(3, 3)
        rec[s, 0:3] = (R @ c + np.asarray(T[1])).astype(np.float32)
        rec[s, 3:12] = R.reshape(-1).astype(np.float32)
        rec[s, 12:15] = e
    return rec


def reach_boxes(ow, centres):
    """Per moving object the cube its OBB centre cannot leave: around the
    first chain joint's origin, half edge = the chain's placement lengths and
    prismatic travels from there plus the centre's offset in its joint frame
    (mpg_abi_world.h's reach ball without the object's radius)."""
    d = Wd.desc_arrays(ow)
    jp = np.asarray(d["joint_placement"], np.float64).reshape(-1, 12)
    lp = np.asarray(d["link_placement"], np.float64).reshape(-1, 12)
    mo = np.asarray(d["moving_offset"], np.float64).reshape(-1, 12)
    travel = np.zeros(len(jp))
    for j, t in enumerate(d["joint_type"]):
        if 4 <= t <= 7:
            if d["joint_q_source"][j] >= 0:
                travel[j] = max(abs(d["joint_lower"][j]), abs(d["joint_upper"][j]))
            else:
                travel[j] = abs(d["joint_q_const"][j])
    lo, hi = [], []
    for m, l in enumerate(d["moving_link"]):
        a = mo[m, :9].reshape(3, 3) @ centres[m] + mo[m, 9:]
        b = lp[l, :9].reshape(3, 3) @ a + lp[l, 9:]
        chain, j = [], d["link_parent"][l]
        while j > 0:
            chain.append(j - 1)
            j = d["joint_parent"][j - 1]
        chain.reverse()
        if not chain:
            c, rc = b, 0.0
        else:
            c = jp[chain[0], 9:]
            rc = travel[chain[0]] + np.linalg.norm(b) + sum(np.linalg.norm(jp[j, 9:]) + travel[j] for j in chain[1:])
        pad = rc * 1e-9 + 4e-6 * X + 1e-6
        lo.append(c - rc - pad)
        hi.append(c + rc + pad)
    return np.asarray(lo), np.asarray(hi)


def rotated_statics_world():
    """The rotated boxes and the cone hull of tests/test_cull_support_axes.py
    and three more rotated boxes: eight statics, enough partners for a grid."""
    base = rotated_scene_world()
    rng = np.random.default_rng(2025)
    scene = list(base.scene)
    for k in range(3):
        side = rng.uniform(0.03, 0.3, size=3)
        pos = rng.uniform([0.2, -0.5, 0.05], [0.7, 0.5, 0.8])
        w, x, y, z = Wd.random_quat(rng)
        scene.append((f"rbox{4 + k}", M.BoxGeom(tuple(float(s) for s in side)),
                      (M.quat_to_mat(w, x, y, z), [float(v) for v in pos])))
    return oracle.OracleWorld(base.art, scene=scene)


@functools.lru_cache(maxsize=None)
def world_grid(name):
    """(oracle world, sides, Grid over its moving objects with every
    non-allowed moving-static pair as a partner, pair index per (object, bit))."""
    ow = rotated_statics_world() if name == "rotated" else Wd.oracle_world(name)
    sides = SH._sides(ow)
    gi = lambda g: next(i for i, gg in enumerate(ow.geoms) if gg is g)  # noqa: E731
    objs = ow.art.objects
    cen = [sides[gi(o.geom)][0] for o in objs]
    rad = [float(lib().grid_widen(float(np.linalg.norm(np.asarray(o.geom.vertices) - sides[gi(o.geom)][0], axis=1).max())))
           for o in objs]
    partners = [[] for _ in objs]
    pair_of = [[] for _ in objs]
    for p, pr in enumerate(ow.pairs):
        if frozenset((pr[4], pr[5])) in ow.allowed:
            continue
        if pr[0] == oracle.KIND_ROBOT and pr[2] == oracle.KIND_SCENE:
            partners[pr[1]].append(pr[3])
            pair_of[pr[1]].append(p)
    lo, hi = reach_boxes(ow, cen)
    return ow, sides, Grid(lo, hi, rad, partners, static_records(ow, sides)), pair_of, cen


def exact_dist(rec, pts):
    """fp64 distance of points to the OBB of one fp32 static record."""
    r = rec.astype(np.float64)
    t = (pts.astype(np.float64) - r[0:3]) @ r[3:12].reshape(3, 3)
    return np.linalg.norm(np.maximum(np.abs(t) - r[12:15], 0.0), axis=1)


def face_points(rng, n, o, h, count):
    """Points whose coordinates sit within a few fp32 ulps of cell faces (the
    box's own faces and corners included)."""
    pts = np.zeros((count, 3), np.float32)
    for k in range(3):
        i = rng.integers(0, n[k] + 1, size=count)
        i[: count // 8] = rng.choice([0, n[k]], size=count // 8)  # the box's faces; all three: corners
        v = (np.float64(o[k]) + i * h).astype(np.float32)
        for _ in range(3):
            step = rng.integers(-1, 2, size=count)
            v = np.where(step < 0, np.nextafter(v, np.float32(-np.inf)), np.where(step > 0, np.nextafter(v, np.float32(np.inf)), v))
        free = rng.random(count) < 0.5  # half the coordinates anywhere in the box
        pts[:, k] = np.where(free, (o[k] + rng.random(count) * n[k] * h).astype(np.float32), v)
    return pts


@pytest.mark.parametrize("name", [3, "rotated"])
def test_bits_are_sound(name):
    ow, _, G, _, _ = world_grid(name)
    rng = np.random.default_rng(11)
    h = lib().grid_h(G.h)
    total = 0
    slots = [(m, G.slot(m)) for m in range(len(G.partners)) if G.slot(m) >= 0]
    assert len(slots) >= 6
    per = 1_000_000 // len(slots) // 2
    for m, s in slots:
        n, o = G.dims(s)
        rand = (o + rng.random((per, 3)) * n * h * 1.02 - 0.01 * n * h).astype(np.float32)
        for pts in (rand, face_points(rng, n, o, h, per)):
            look, _ = G.lookup(s, pts)
            kept = G.sphere(s, pts)
            assert int(np.count_nonzero(kept & ~look)) == 0, (name, m)
            for k, sid in enumerate(G.partners[m]):
                near = exact_dist(G.sobj[sid], pts) <= G.r[m] + float(MARGIN)
                assert not np.any(near & (((look >> np.uint32(k)) & 1) == 0)), (name, m, k)
            total += len(pts)
    assert total >= 900_000


@pytest.mark.parametrize("cfg", [3, "rotated"])
def test_boxes_hold_every_centre(cfg):
    """The boxes of this file's restatement (the replay below runs on them);
    the library's own boxes are checked in tests/test_cull_grid_gpu.py."""
    ow, _, G, _, cen = world_grid(cfg)
    q = Wd.sample_q(ow.art, 100000, 5)
    _, objT = ow.fk_batch(q)
    for m in range(len(cen)):
        s = G.slot(m)
        assert s >= 0, (cfg, m)
        T = objT[:, m, :]
        c = (T[:, :9].reshape(-1, 3, 3) @ cen[m] + T[:, 9:]).astype(np.float32)
        _, cell = G.lookup(s, c)
        assert int((cell < 0).sum()) == 0, (cfg, m)


_REPLAY = {}


def replay(cfg):
    if cfg in _REPLAY:
        return _REPLAY[cfg]
    ow, sides, G, pair_of, cen = world_grid(cfg)
    q = Wd.sample_q(ow.art, 16384, 1)
    n = len(q)
    _, masks = ow.collide_batch(q, nthreads=min(8, os.cpu_count() or 1))
    _, objT = ow.fk_batch(q)
    gi = lambda g: next(i for i, gg in enumerate(ow.geoms) if gg is g)  # noqa: E731
    obj_g = [gi(o.geom) for o in ow.art.objects]
    scene_g = [gi(s[1]) for s in ow.scene]
    centres = [(objT[:, m, :9].reshape(-1, 3, 3) @ cen[m] + objT[:, m, 9:]).astype(np.float32) for m in range(len(cen))]
    keep_sphere, keep_look = {}, {}
    for m in range(len(cen)):
        s = G.slot(m)
        if s < 0:  # too few partners for a grid (cfg4: four statics): the sphere test on both paths
            assert len(G.partners[m]) < 6, (cfg, m)  # every other object of these worlds fits the budget
            continue
        look, _ = G.lookup(s, centres[m])
        kept = G.sphere(s, centres[m])
        assert int(np.count_nonzero(kept & ~look)) == 0, (cfg, m)
        for k, p in enumerate(pair_of[m]):
            keep_sphere[p] = ((kept >> np.uint32(k)) & 1).astype(bool)
            keep_look[p] = ((look >> np.uint32(k)) & 1).astype(bool)

    def side(kind, idx):
        if kind == oracle.KIND_ROBOT:
            return sides[obj_g[idx]], np.ascontiguousarray(objT[:, idx, :])
        T = np.asarray(list(ow.scene[idx][2][0]) + list(ow.scene[idx][2][1]), np.float64)
        return sides[scene_g[idx]], np.ascontiguousarray(np.broadcast_to(T, (n, 12)))

    fp = lambda a: a.ctypes.data_as(_FP) if a is not None else None  # noqa: E731
    tot = dict(sphere_keeps=0, look_keeps=0, final_sphere=0, final_look=0, hits=0, dropped=0)
    for p, pr in enumerate(ow.pairs):
        if frozenset((pr[4], pr[5])) in ow.allowed:
            continue
        (ca, ea, ta), Ta = side(pr[0], pr[1])
        (cb, eb, tb), Tb = side(pr[2], pr[3])
        out = np.zeros(n, np.uint8)
        SH.lib().sh_replay(ca.ctypes.data_as(_DP), fp(ea), fp(ta), Ta.ctypes.data_as(_DP), cb.ctypes.data_as(_DP), fp(eb),
                           fp(tb), Tb.ctypes.data_as(_DP), ctypes.c_long(n), ctypes.c_float(MARGIN),
                           ctypes.c_float(SH.SH_MARGIN), out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)))
        hit = ((masks[:, p >> 5] >> np.uint32(p & 31)) & 1).astype(bool)
        if p in keep_look:
            ks, kl = keep_sphere[p], keep_look[p]
            tot["sphere_keeps"] += int(ks.sum())
            tot["look_keeps"] += int(kl.sum())
        elif pr[2] == oracle.KIND_SCENE:  # an object without a grid: the sphere test on both paths
            rec = G.sobj[pr[3]].astype(np.float64)
            t = (centres[pr[1]].astype(np.float64) - rec[0:3]) @ rec[3:12].reshape(3, 3)
            d = np.linalg.norm(np.maximum(np.abs(t) - rec[12:15], 0.0), axis=1)
            ks = kl = d <= G.r[pr[1]] + float(MARGIN) + 1e-5  # (fp64 with the fp32 test's rounding allowed for)
        else:  # moving-moving: the same sphere-sphere test on both paths
            a, b = pr[1], pr[3]
            d2 = ((centres[a] - centres[b]) ** 2).sum(axis=1)
            rr = np.float32(G.r[a]) + np.float32(G.r[b]) + MARGIN
            ks = kl = d2 <= rr * rr
        tot["final_sphere"] += int(((out == 2) & ks).sum())
        tot["final_look"] += int(((out == 2) & kl).sum())
        tot["hits"] += int(hit.sum())
        tot["dropped"] += int((hit & ~((out == 2) & kl)).sum())
    tot["n"] = n
    tot["h"] = lib().grid_h(G.h)
    tot["cells"] = lib().grid_cells(G.h)
    _REPLAY[cfg] = tot
    return tot


@pytest.mark.parametrize("cfg", [3, 4, "rotated"])
def test_replay_lookup_against_sphere_test(cfg):
    """cfg4's objects have four static partners each, below kGridMinPartners:
    no grid, both paths are the sphere test there; the rotated world is the
    second one with grids."""
    t = replay(cfg)
    assert (t["cells"] > 0) == (cfg != 4)
    extra = (t["final_look"] - t["final_sphere"]) / t["final_sphere"]
    print(f"cfg{cfg}: cell edge {t['h'] * 100:.2f} cm, {t['cells']} cells; moving-static keeps per configuration "
          f"{t['sphere_keeps'] / t['n']:.3f} (sphere test) -> {t['look_keeps'] / t['n']:.3f} (lookup); final candidates "
          f"{t['final_sphere']} -> {t['final_look']} (+{100 * extra:.2f} %), hits {t['hits']}, dropped {t['dropped']}")
    assert t["hits"] > 0 and t["dropped"] == 0
    assert t["final_look"] >= t["final_sphere"]
    assert extra <= 0.01


def _toy(nparts, budget=BUDGET, boxes=None):
    rng = np.random.default_rng(3)
    ns = 40
    rec = np.zeros((ns, 16), np.float32)
    rec[:, 0:3] = rng.uniform(-1, 1, size=(ns, 3))
    rec[:, 3:12] = np.eye(3, dtype=np.float32).reshape(-1)
    rec[:, 12:15] = rng.uniform(0.02, 0.1, size=(ns, 3))
    boxes = boxes or [1.0] * len(nparts)
    lo = [[-b, -b, -b] for b in boxes]
    hi = [[b, b, b] for b in boxes]
    return Grid(lo, hi, [0.1] * len(nparts), [list(range(k)) for k in nparts], rec, budget)


def test_partner_limits_and_determinism():
    G = _toy([32, 33, 0, 6, 5])
    assert [G.slot(c) >= 0 for c in range(5)] == [True, False, False, True, False]
    assert lib().grid_cells(G.h) <= BUDGET
    look, cell = G.lookup(G.slot(0), np.array([[5.0, 0, 0], [np.nan, 0, 0], [0, 0, 0]], np.float32))
    assert look[0] == look[1] == 0xFFFFFFFF and cell[0] == cell[1] == -1 and cell[2] >= 0
    look, _ = G.lookup(G.slot(3), np.array([[0, -7.0, 0]], np.float32))
    assert look[0] == 0x3F
    H = _toy([32, 33, 0, 6, 5])
    assert lib().grid_hash(G.h) == lib().grid_hash(H.h)
    assert lib().grid_h(G.h) >= 0.02


def test_budget_fallback_is_deterministic():
    # a budget too small for the large box at the coarsest edge: it leaves, the others stay
    a = _toy([8, 8, 8], budget=40000, boxes=[0.5, 3.0, 0.4])
    b = _toy([8, 8, 8], budget=40000, boxes=[0.5, 3.0, 0.4])
    assert [a.slot(c) >= 0 for c in range(3)] == [True, False, True]
    assert lib().grid_hash(a.h) == lib().grid_hash(b.h)
    assert lib().grid_cells(a.h) <= 40000 and 0.02 <= lib().grid_h(a.h) <= 0.08 * (1 + 1e-6)
    # nothing fits: no grid at all
    c = _toy([8], budget=8, boxes=[3.0])
    assert c.slot(0) < 0 and lib().grid_cells(c.h) == 0


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_builder_under_sanitizers(tmp_path):
    exe = str(tmp_path / "cull_grid_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-DCULL_GRID_MAIN", "-o", exe, _SRC])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert " bad 0 " in out.stdout
