"""Wide worlds: the Panda plus hundreds of small boxes, for the collide paths
that only worlds with thousands of collision pairs reach (test infrastructure,
shared by tests/test_wide_worlds.py on the host and
tests/test_wide_worlds_gpu.py on the device).

  A  more than 1 024 pairs, 32 < mask words <= 64; a cull block of 256
     threads with more than 64 KiB of dynamic LDS (the 71-80 KiB band)
  B  more than 2 048 pairs, more than 64 mask words
  C  a cull block of 256 threads in the 128-160 KiB band

The boxes are small and spread over a volume larger than the arm's reach, so
that a uniformly sampled state collides about half of the time and the hits
spread over every mask word (many_boxes_world's sizes make nearly every state
collide once there are hundreds of boxes).  The tests assert what each world
must reach; nothing here is tuned to the device's output.

One seeded batch of states per world serves every size: a batch of n rows is
its first n rows, with row 0 replaced by the batch's "marker" row (the first
row of the whole batch whose hits lie in two different mask words, one of
them in the world's last pair columns), so that even the smallest batches
have a hit in a high pair column.  The oracle runs once per world.
"""
import ctypes

import numpy as np

import oracle
import worlds as Wd
from native.host_shim import lib as host_lib

NTHREADS = 8
N_BASE = 3 * 8192 + 77  # the largest batch any test takes (the host pipeline's)

# name: boxes, their side range (smaller where there are more, for similar hit
# rates), seed, rows of the base batch
SPEC = {
    "A": dict(boxes=104, side=(0.03, 0.08), seed=501, rows=N_BASE),
    "B": dict(boxes=200, side=(0.015, 0.04), seed=502, rows=N_BASE),
    "C": dict(boxes=300, side=(0.01, 0.03), seed=503, rows=4160),
}
BOX_LO, BOX_HI = (-0.8, -0.8, -0.3), (0.8, 0.8, 1.15)  # box centres: about the arm's reach

_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def boxes_world(boxes, side_range, seed):
    art = Wd.panda_articulation()
    rng = np.random.default_rng(seed)
    scene = []
    for k in range(boxes):
        side = rng.uniform(side_range[0], side_range[1], size=3)
        c = rng.uniform(BOX_LO, BOX_HI)
        scene.append((f"b{k}",) + Wd._box(side, c))
    return oracle.OracleWorld(art, scene=scene)


def world(name):
    s = SPEC[name]
    return cached(("ow", name), lambda: boxes_world(s["boxes"], s["side"], s["seed"]))


def desc(name):
    return cached(("desc", name), lambda: Wd.desc_arrays(world(name)))


def n_pairs(name):
    return len(desc(name)["pair_a"])


def mask_words(name):
    return max(1, (n_pairs(name) + 31) // 32)


# ------------------------------------------------------------------ cull block / LDS
def cull_saves(d):
    """n_saves of the descriptor's joint tree (bp_build of mpg_broadphase.h)."""
    keep = []

    def I(a):
        a = np.ascontiguousarray(np.asarray(a, dtype=np.int32))
        keep.append(a)
        return a.ctypes.data_as(ctypes.c_void_p)

    def F(a):
        a = np.ascontiguousarray(np.asarray(a, dtype=np.float64))
        keep.append(a)
        return a.ctypes.data_as(ctypes.c_void_p)

    return host_lib().host_cull_saves(len(d["joint_type"]), I(d["joint_type"]), I(d["joint_parent"]),
                                      I(d["joint_q_source"]), F(d["joint_q_const"]), F(d["joint_axis"]),
                                      F(d["joint_placement"]), int(d["dof"]), len(d["link_parent"]),
                                      I(d["link_parent"]), F(d["link_placement"]), len(d["moving_link"]),
                                      I(d["moving_link"]), F(d["moving_offset"]))


def lds_per_thread(n_moving, n_saves, W):
    L = host_lib()
    L.host_cull_lds_per_thread.restype = ctypes.c_long
    return int(L.host_cull_lds_per_thread(int(n_moving), int(n_saves), int(W)))


def choose_block(per_thread):
    """(block, lds bytes) of mpg_broadphase.h's choose_block; (-1, -1) when not even 64 threads fit."""
    lds = ctypes.c_long(0)
    block = host_lib().host_choose_block(ctypes.c_long(int(per_thread)), ctypes.byref(lds))
    return int(block), int(lds.value)


def predicted_cull(name):
    """(block, lds bytes, bytes per thread) mpg_world_create takes for the world."""
    def make():
        d = desc(name)
        per = lds_per_thread(len(d["moving_link"]), cull_saves(d), mask_words(name))
        return choose_block(per) + (per,)
    return cached(("cull", name), make)


# ------------------------------------------------------------------ batches and references
def base(name):
    """(q, flags, masks) of the world's whole batch, read-only; the oracle runs once."""
    def make():
        w = world(name)
        q = Wd.sample_q(w.art, SPEC[name]["rows"], SPEC[name]["seed"] + 1000)
        f, m = w.collide_batch(q, nthreads=NTHREADS)
        for a in (q, f, m):
            a.setflags(write=False)
        return q, f, m
    return cached(("base", name), make)


def columns(m):
    """bool [P32]: pair columns with a hit somewhere in the masks m [n, W]."""
    any_bits = np.bitwise_or.reduce(m, axis=0)
    return ((any_bits[:, None] >> np.arange(32, dtype=np.uint32)) & 1).astype(bool).reshape(-1)


def high_column(name):
    """The pair column a world's hits must reach: 2 048 for more than 64 mask words, else 1 024."""
    return 2048 if mask_words(name) > 64 else 1024


def marker_row(name):
    """Index of the first row with bits in two different mask words, one at or above high_column."""
    _, _, m = base(name)
    hi = high_column(name) // 32
    two = (m != 0).sum(axis=1) >= 2
    high = (m[:, hi:] != 0).any(axis=1)
    idx = np.flatnonzero(two & high)
    assert len(idx), "no row with hits in two mask words and a high pair column"
    return int(idx[0])


def batch(name, n):
    """(q, flags, masks) of the oracle for the world's batch of n rows, read-only."""
    def make():
        q, f, m = base(name)
        assert 1 <= n <= len(q)
        q, f, m = q[:n].copy(), f[:n].copy(), m[:n].copy()
        i = marker_row(name)
        q[0], f[0], m[0] = base(name)[0][i], base(name)[1][i], base(name)[2][i]
        for a in (q, f, m):
            a.setflags(write=False)
        return q, f, m
    return cached(("batch", name, n), make)


def repeated(name, colliding, n):
    """n copies of one row of the base batch: the marker row, or the first free row."""
    def make():
        q, f, m = base(name)
        i = marker_row(name) if colliding else int(np.flatnonzero(f == 0)[0])
        out = (np.ascontiguousarray(np.repeat(q[i:i + 1], n, axis=0)), np.repeat(f[i:i + 1], n),
               np.ascontiguousarray(np.repeat(m[i:i + 1], n, axis=0)))
        for a in out:
            a.setflags(write=False)
        return out
    return cached(("rep", name, bool(colliding), n), make)


def check_oracle_conditions(name, ref, structure=True):
    """What the issue asks of the oracle's own output on a sampled batch: a
    hit rate away from 0 and 1, a hit in a high pair column, and (batches of
    1 000 rows and more: structure) hits in at least 32 mask words and a row
    with bits in two words."""
    _, f, m = ref
    cols = np.flatnonzero(columns(m))
    words = int((np.bitwise_or.reduce(m, axis=0) != 0).sum())
    print(f"world {name}, {len(f)} rows: hit rate {f.mean():.3f}, highest pair column with a hit {cols.max()}, "
          f"{words} of {m.shape[1]} mask words with a hit")
    assert 0.2 < f.mean() < 0.9, (name, len(f), f.mean())
    assert cols.max() >= 1024, (name, len(f), cols.max())
    assert cols.max() >= high_column(name), (name, len(f), cols.max())
    assert ((m != 0).sum(axis=1) >= 2).any(), (name, len(f))
    if structure:
        assert words >= 32, (name, len(f), words)
