"""The narrow phase's tapered task list on the GPU (mpg_bucket.h bk_task_plan;
host rehearsal: tests/test_task_plan.py).  Several task-size levels exist only
for launches with more than 4 * narrow blocks * 128 candidates, about 2^19
rows of cfg3 on a whole chip, so the worlds here are created under
MPG_NARROW_BLOCKS=1: the persistent grid is one block, the target is 4 tasks
and a few thousand candidates run through more than one level, in narrow_kernel,
closed_form_kernel<CLS_MESH> and contact_kernel.  Results are bit-exact
against the CPU oracle (flags, pair masks) and, for contacts, against the
same call on a world with the full grid."""
import ctypes

import numpy as np
import pytest

import worlds as Wd
from mplib_amd import _capi
from mplib_amd.batch import DeviceWorld

pytestmark = pytest.mark.gpu

N3, SEED3 = 4096, 41
N7, SEED7 = 2048, 47
_OW, _REF = {}, {}


def ow(cfg):
    if cfg not in _OW:
        _OW[cfg] = Wd.oracle_world(cfg)
    return _OW[cfg]


def reference(cfg, n, seed):
    """(q, flags, masks) of the oracle, computed once per module."""
    if cfg not in _REF:
        q = Wd.sample_q(ow(cfg).art, n, seed)
        f, m = ow(cfg).collide_batch(q, nthreads=4)
        for a in (q, f, m):
            a.setflags(write=False)
        _REF[cfg] = (q, f, m)
    return _REF[cfg]


def one_block_world(monkeypatch, cfg):
    monkeypatch.setenv("MPG_NARROW_BLOCKS", "1")
    return DeviceWorld(Wd.desc_arrays(ow(cfg)))


def device_collide(d, q):
    """The device-pointer path: always the bulk pipeline, on the null stream's workspace."""
    torch = pytest.importorskip("torch")
    qd = torch.from_numpy(np.array(q)).cuda()  # a copy: the shared reference is read-only
    fd = torch.zeros(len(q), dtype=torch.uint8, device="cuda")
    md = torch.zeros((len(q), d.mask_words), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    d.collide_batch(qd, fd, md)
    info = d.task_plan_info()  # synchronises the stream
    return fd.cpu().numpy(), md.cpu().numpy().view(np.uint32), info


def ceil_div(a, b):
    return -(-a // b)


def test_cfg3_every_level_matches_oracle(monkeypatch):
    q, fo, mo = reference(3, N3, SEED3)
    d = one_block_world(monkeypatch, 3)
    f, m, info = device_collide(d, q)
    print(info)
    np.testing.assert_array_equal(f, fo)
    np.testing.assert_array_equal(m, mo)
    assert info["candidates"] > 4 * 128  # past the clamp of a 4-task target
    assert info["levels"] >= 2
    assert info["tasks"] > ceil_div(info["candidates"], info["task_size"])
    d.close()


def test_cfg3_below_the_clamp_keeps_one_level(monkeypatch):
    q, fo, mo = reference(3, N3, SEED3)
    d = one_block_world(monkeypatch, 3)
    f, m, info = device_collide(d, q[:256])
    print(info)
    np.testing.assert_array_equal(f, fo[:256])
    np.testing.assert_array_equal(m, mo[:256])
    assert 0 < info["candidates"] <= 4 * 128
    assert info["levels"] == 1
    d.close()


def test_cfg7_mesh_pairs_read_the_same_task_list(monkeypatch):
    q, fo, mo = reference(7, N7, SEED7)
    d = one_block_world(monkeypatch, 7)
    f, m, info = device_collide(d, q)
    print(info)
    np.testing.assert_array_equal(f, fo)
    np.testing.assert_array_equal(m, mo)
    assert info["levels"] >= 2
    assert info["tasks"] > ceil_div(info["candidates"], info["task_size"])
    d.close()


def contacts(d, q, n_pairs):
    n = len(q)
    flags = np.zeros(n, np.uint8)
    masks = np.zeros((n, d.mask_words), np.uint32)
    depth, normal, pos = np.zeros((n, n_pairs)), np.zeros((n, n_pairs, 3)), np.zeros((n, n_pairs, 3))
    v = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    _capi.check(_capi.lib().mpg_collide_contacts(d.handle, v(np.ascontiguousarray(q)), n, 0, v(flags), v(masks),
                                                 v(depth), v(normal), v(pos), _capi.MPG_MEM_HOST, None),
                "mpg_collide_contacts")
    return flags, masks, depth, normal, pos, d.task_plan_info()


def test_contacts_equal_the_untapered_call(monkeypatch):
    q, fo, mo = reference(3, N3, SEED3)
    P = len(ow(3).pairs)
    plain = DeviceWorld(Wd.desc_arrays(ow(3)))
    want = contacts(plain, q, P)
    assert want[5]["levels"] == 1
    plain.close()
    d = one_block_world(monkeypatch, 3)
    got = contacts(d, q, P)
    print(got[5])
    assert got[5]["levels"] >= 2
    np.testing.assert_array_equal(got[0], fo)
    np.testing.assert_array_equal(got[1], mo)
    assert want[2].any()
    for a, b in zip(got[:5], want[:5]):
        assert a.tobytes() == b.tobytes()
    d.close()
