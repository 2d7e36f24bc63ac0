"""The cull's support-height axes on the device: every flag and pair bit equals
the oracle's on near-contact batches -- the colliding configurations and the
free ones whose clearance is below 3 cm, the band around the 1.86 cm cull
margin where an unsound cull would flip a bit -- and on a scene with rotated
box statics and a static hull; the narrow phase gets fewer candidates.

The near-contact rows of ``sample_q(art, 16384, 77)`` are kept as indices in
``golden/near_contact_idx.npz`` (the oracle's distance pass over 16384
configurations takes several seconds); ``test_near_contact_rows_are_the_oracles``
recomputes them on the CPU.
"""
import os

import numpy as np
import pytest

import oracle
from oracle import model as M
import worlds as Wd

NTHREADS = min(16, os.cpu_count() or 1)
SEED, N, BAND, CAP = 77, 16384, 0.03, 4096
# (near-contact free, colliding) of the 16384 configurations; cfg4's 1515 free
# rows include two whose distance_batch is -1 (a penetrating pair that float
# MPR reports as free): they stay in the batch
COUNTS = {2: (859, 631), 3: (1372, 2953), 4: (1515, 2402)}
_OW = {}
_REF = {}


def ow(cfg):
    if cfg not in _OW:
        _OW[cfg] = Wd.oracle_world(cfg)
    return _OW[cfg]


def near_contact_rows(cfg):
    """(indices of the free rows with clearance < BAND, of the colliding rows)."""
    q = Wd.sample_q(ow(cfg).art, N, SEED)
    f, _ = ow(cfg).collide_batch(q, nthreads=NTHREADS)
    ds, _, do, _ = ow(cfg).distance_batch(q)
    return np.flatnonzero((f == 0) & (np.minimum(ds, do) < BAND)), np.flatnonzero(f != 0)


def reference(cfg, golden_dir):
    """(q, oracle flags, oracle masks) of the near-contact batch, at most CAP rows."""
    if cfg not in _REF:
        idx = np.load(os.path.join(golden_dir, "near_contact_idx.npz"))["cfg%d" % cfg]
        q = np.ascontiguousarray(Wd.sample_q(ow(cfg).art, N, SEED)[idx[:CAP]])
        _REF[cfg] = (q,) + tuple(ow(cfg).collide_batch(q, nthreads=NTHREADS))
    return _REF[cfg]


@pytest.mark.parametrize("cfg", [2, 3, 4])
def test_near_contact_rows_are_the_oracles(cfg, golden_dir):
    near, coll = near_contact_rows(cfg)
    assert (len(near), len(coll)) == COUNTS[cfg]
    idx = np.load(os.path.join(golden_dir, "near_contact_idx.npz"))["cfg%d" % cfg]
    np.testing.assert_array_equal(idx, np.sort(np.concatenate([near, coll])))


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", [3, 2, 4])
def test_near_contact_batch_matches_oracle(cfg, golden_dir):
    from mplib_amd.batch import DeviceWorld
    q, fo, mo = reference(cfg, golden_dir)
    assert 1000 < len(q) <= CAP and 0 < int((fo == 0).sum()) < len(q)
    d = DeviceWorld(Wd.desc_arrays(ow(cfg)))
    d.set_small_batch_max(0)  # the throughput pipeline (cull_kernel), whatever the batch size
    f, m = d.collide_batch(q)
    np.testing.assert_array_equal(f, fo)
    np.testing.assert_array_equal(m, mo)


def rotated_scene_world():
    """Panda + four non-cubic boxes at random orientations + a cone hull:
    rotated static OBBs and a static support-height table."""
    art = Wd.panda_articulation()
    rng = np.random.default_rng(2024)
    scene = []
    for k in range(4):
        side = rng.uniform(0.03, 0.3, size=3)
        pos = rng.uniform([0.2, -0.5, 0.05], [0.7, 0.5, 0.8])
        w, x, y, z = Wd.random_quat(rng)
        scene.append((f"rbox{k}", M.BoxGeom(tuple(float(s) for s in side)),
                      (M.quat_to_mat(w, x, y, z), [float(v) for v in pos])))
    w, x, y, z = Wd.random_quat(rng)
    scene.append(("cone", Wd.cone_hull(), (M.quat_to_mat(w, x, y, z), [0.45, 0.2, 0.35])))
    return oracle.OracleWorld(art, scene=scene)


@pytest.mark.gpu
def test_rotated_statics_and_static_hull_match_oracle():
    from mplib_amd.batch import DeviceWorld
    o = rotated_scene_world()
    q = Wd.sample_q(o.art, 4096, 78)
    fo, mo = o.collide_batch(q, nthreads=NTHREADS)
    names = o.pair_names()
    for s in ("rbox0", "rbox1", "rbox2", "rbox3", "cone"):  # every static is hit by something
        assert sum(int(((mo[:, p >> 5] >> np.uint32(p & 31)) & 1).sum()) for p, pn in enumerate(names) if pn[1] == s) > 0, s
    d = DeviceWorld(Wd.desc_arrays(o))
    d.set_small_batch_max(0)
    f, m = d.collide_batch(q)
    np.testing.assert_array_equal(f, fo)
    np.testing.assert_array_equal(m, mo)


@pytest.mark.gpu
def test_cfg3_narrow_candidates_below_one_per_configuration():
    """The narrow stage's units (candidates) on the first 4096 configurations
    of the cfg3 batch sample_q(art, 16384, 77): below 1.0 per configuration
    (1.19 without the support-height axes, 0.84 by the host model)."""
    from mplib_amd import scenes
    w, art = scenes.world(3)
    w.set_small_batch_max(0)
    q = np.ascontiguousarray(Wd.sample_q(ow(3).art, N, SEED)[:4096])
    w.collide_batch(q)
    w.profile_enable(True)
    w.profile_read()
    f, m = w.collide_batch(q)
    prof = w.profile_read()
    w.profile_enable(False)
    _, launches, units = prof["narrow"]
    per_cfg = units / len(q)
    print(f"cfg3 narrow candidates: {units:.0f} over {launches:.0f} launches, {per_cfg:.3f} per configuration")
    assert launches >= 1
    assert per_cfg < 1.0
    fo, mo = ow(3).collide_batch(q, nthreads=NTHREADS)
    np.testing.assert_array_equal(f, fo)
    np.testing.assert_array_equal(m, mo)
