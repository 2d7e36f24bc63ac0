"""Survivor bucketing on the GPU (tile-major byte counts -> range_sum ->
range_scan -> scatter), bit-exact against the CPU oracle through the
device-pointer path, which always takes launch_collide.  Sizes sit on the
edges the bucketing has: a partial last tile, a partial last range and group,
a partial last cull block (waves past the last tile), one workspace reused by
a smaller and then a larger call (nothing clears the counts between calls),
and a world with more than 16 mask words (the cull's ballot count path)."""
import numpy as np
import pytest

import oracle
import worlds as Wd
from mplib_amd.batch import DeviceWorld
from test_bucket_index import consts

pytestmark = pytest.mark.gpu

NTHREADS = 8
_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def ow3():
    return cached("ow3", lambda: Wd.oracle_world(3))


def dw3():
    return cached("dw3", lambda: DeviceWorld(Wd.desc_arrays(ow3())))


def many_boxes_world():
    """Panda + 48 boxes: 547 pairs, 18 mask words."""
    def make():
        art = Wd.panda_articulation()
        rng = np.random.default_rng(77)
        scene = []
        for k in range(48):
            side = rng.uniform(0.02, 0.15, size=3)
            c = rng.uniform([-0.6, -0.6, 0.0], [0.8, 0.6, 0.9])
            scene.append((f"b{k}",) + Wd._box(side, c))
        return oracle.OracleWorld(art, scene=scene)
    return cached("ow48", make)


def reference(key, world, q):
    """(q, flags, masks) of the oracle, computed once per key and left unchanged."""
    def make():
        f, m = world.collide_batch(q, nthreads=NTHREADS)
        for a in (q, f, m):
            a.setflags(write=False)
        return q, f, m
    return cached(key, make)


def cfg3_case(n):
    if n == 1:  # a row that collides (the first row of seed 101 does not)
        q, f, _ = reference(("cfg3", 64), ow3(), Wd.sample_q(ow3().art, 64, 101))
        i = int(np.flatnonzero(f)[0])
        return reference(("cfg3", 1), ow3(), np.ascontiguousarray(q[i:i + 1]))
    return reference(("cfg3", n), ow3(), Wd.sample_q(ow3().art, n, 100 + n))


def device_collide(d, q):
    import torch
    qd = torch.from_numpy(np.array(q)).cuda()  # a copy: the shared references are read-only
    fd = torch.full((len(q),), 7, dtype=torch.uint8, device="cuda")
    md = torch.full((len(q), d.mask_words), -1, dtype=torch.int32, device="cuda")
    d.collide_batch(qd, fd, md, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return fd.cpu().numpy(), md.cpu().numpy().view(np.uint32)


def check(d, ref):
    q, fo, mo = ref
    f, m = device_collide(d, q)
    np.testing.assert_array_equal(f, fo)
    np.testing.assert_array_equal(m, mo)


def cfg3_sizes():
    R = 64 * consts()[0]  # configurations per range
    return [1, 63, 64, 65, 255, 256, 257, R - 1, R, R + 1, 3 * R + 17, 20000]


@pytest.mark.parametrize("n", cfg3_sizes())
def test_cfg3_sizes_match_oracle(n):
    pytest.importorskip("torch")
    ref = cfg3_case(n)
    if n == 1:
        assert ref[1][0] == 1
    check(dw3(), ref)


def test_workspace_reuse_large_small_large():
    """One world, one stream: rows and part entries of the larger call lie
    beyond what the smaller call writes and must not leak into it, nor the
    smaller call's into the next larger one."""
    pytest.importorskip("torch")
    d = DeviceWorld(Wd.desc_arrays(ow3()))
    for n in (20000, 65, 20000):
        check(d, cfg3_case(n))


def test_many_mask_words_ballot_count_path():
    pytest.importorskip("torch")
    w = many_boxes_world()
    d = DeviceWorld(Wd.desc_arrays(w))
    assert d.mask_words > 16
    q, f, m = reference(("ow48", 4160), w,Wd.sample_q(w.art, 4160, 9))
    assert 0.5 < f.mean() < 0.8 and int((np.bitwise_or.reduce(m, axis=0) != 0).sum()) > 0
    fs, ms = device_collide(d, q[:65])
    np.testing.assert_array_equal(fs, f[:65])
    np.testing.assert_array_equal(ms, m[:65])
    check(d, (q, f, m))
