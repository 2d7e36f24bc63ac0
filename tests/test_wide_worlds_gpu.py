"""Worlds with thousands of collision pairs on every collide path, bit-exact
against the CPU oracle (tests/wide_worlds.py: worlds A, B and C; the host
half, tests/test_wide_worlds.py, checks what the worlds reach and what the
oracle alone gives on these batches).

Such worlds take code that narrower ones never run: the cull with more than
64 KiB of dynamic LDS (A, C), its ballot count path, range sums that pass
over a count row more than once, a scan that loops over more than 1024 pair
columns and a task prefix of more than one round of 1024 pairs (all three),
both sides of the fold / no-fold decision at sizes where narrow worlds always
fold, the latency path without its resident server, the host pipeline's
unstaged mask pack (B) and the staged one at 37 words (A), and
mpg_collide_count with thousands of LDS counters.  Each test asserts the
property it exists for next to the parity."""
import ctypes

import numpy as np
import pytest

import wide_worlds as WW
from mplib_amd import _capi as C
from mplib_amd import planner
from mplib_amd.batch import DeviceWorld
from test_bucket_index import launch_shape
from test_bucketing import device_collide
from test_wide_worlds import check_world_reaches

pytestmark = pytest.mark.gpu

HOST_CHUNK = 8192
_DW = {}


def dworld(name):
    """One DeviceWorld per wide world for the tests that do not need their own."""
    if name not in _DW:
        _DW[name] = new_dworld(name)
    return _DW[name]


def new_dworld(name):
    P, W, block, _ = check_world_reaches(name)
    d = DeviceWorld(WW.desc(name))
    assert (d.n_pairs, d.mask_words, d.block_size) == (P, W, block)
    return d


def check_device(d, ref):
    q, fo, mo = ref
    f, m = device_collide(d, q)
    np.testing.assert_array_equal(f, fo)
    np.testing.assert_array_equal(m, mo)


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_cull_block_is_the_predicted_one(name):
    """mpg_world_create takes the block (and with it the LDS bytes) the host table predicts."""
    d = dworld(name)
    assert d.block_size == WW.predicted_cull(name)[0] and d.mask_words == WW.mask_words(name)


# bk_fold_sum per (world, rows): 4160 rows fold the range sums into the scan at 37 mask words and not at 70 or 104
FOLD = {"A": {1: True, 65: True, 4160: True, 20000: False}, "B": {1: True, 65: True, 4160: False, 20000: False},
        "C": {65: True, 4160: False}}


@pytest.mark.parametrize("name,n", [(w, n) for w in "ABC" for n in FOLD[w]])
def test_device_path_matches_oracle(name, n):
    pytest.importorskip("torch")
    d = dworld(name)
    shape = launch_shape(n, d.mask_words)
    assert shape["fold"] == FOLD[name][n] and shape["groups"] == (3 if n == 20000 else 1)
    ref = WW.batch(name, n)
    if n == 1:
        assert ref[1][0] == 1
    else:
        WW.check_oracle_conditions(name, ref, structure=n >= 1000)
    check_device(d, ref)


def test_workspace_reuse_large_small_large():
    """One world, one stream: the cull's ballot path writes single count
    bytes into rows that launch_collide clears for this call's tiles only, and
    nothing clears part or grp; the larger call's leftovers must not show."""
    pytest.importorskip("torch")
    d = new_dworld("B")
    for n in (20000, 65, 20000, 1):
        check_device(d, WW.batch("B", n))
    d.close()


@pytest.mark.parametrize("name", ["A", "B"])
@pytest.mark.parametrize("n", [1, 64, 65, 1000])
def test_latency_path_matches_oracle(name, n):
    """Host arrays of at most small_batch_max rows: more mask words than the
    resident server holds, so one small_kernel launch of n_pairs * tiles waves
    per batch and n_pairs * n hit bytes folded on the host; with masks and
    flags only."""
    d = dworld(name)
    assert d.mask_words > 16 and n <= 1024  # kSrvMaxW; the default small_batch_max
    q, fo, mo = WW.batch(name, n)
    if n > 1:
        WW.check_oracle_conditions(name, (q, fo, mo), structure=n >= 1000)
    f, m = d.collide_batch(q)
    np.testing.assert_array_equal(f, fo)
    np.testing.assert_array_equal(m, mo)
    np.testing.assert_array_equal(host_flags_only(d, q), fo)


def host_flags_only(d, q):
    q = np.ascontiguousarray(q)
    fl = np.full(len(q), 0xAB, np.uint8)
    C.check(C.lib().mpg_collide_batch(d.handle, q.ctypes.data_as(ctypes.c_void_p), len(q),
                                      fl.ctypes.data_as(ctypes.c_void_p), None, C.MPG_MEM_HOST, None),
            "mpg_collide_batch")
    return fl


@pytest.mark.parametrize("name", ["A", "B"])
def test_host_pipeline_matches_oracle(monkeypatch, name):
    """Host arrays above small_batch_max in chunks of 8192 rows: four chunks,
    two pack blocks of 4096 rows per chunk (the second one starts at the first
    one's count).  256 rows of 70 mask words exceed the pack's 64 KiB of LDS
    (B: rows written one by one), 37 words do not (A: staged through LDS)."""
    monkeypatch.setenv("MPG_HOST_CHUNK", str(HOST_CHUNK))
    d = new_dworld(name)
    assert (256 * d.mask_words * 4 > 64 * 1024) == (name == "B")
    n = 3 * HOST_CHUNK + 77
    q, fo, mo = WW.batch(name, n)
    WW.check_oracle_conditions(name, (q, fo, mo))
    np.testing.assert_array_equal(host_flags_only(d, q), fo)
    f, m = d.collide_batch(q)
    np.testing.assert_array_equal(f, fo)
    np.testing.assert_array_equal(m, mo)
    d.close()


@pytest.mark.parametrize("colliding", [True, False])
def test_host_pipeline_dense_and_empty_packs(monkeypatch, colliding):
    """Every row colliding (each pack block full) and no row colliding (no packed row at all)."""
    monkeypatch.setenv("MPG_HOST_CHUNK", str(HOST_CHUNK))
    d = new_dworld("B")
    q, fo, mo = WW.repeated("B", colliding, 3 * HOST_CHUNK + 77)
    assert (fo == colliding).all() and ((mo != 0).any(axis=1) == colliding).all()
    f, m = d.collide_batch(q)
    np.testing.assert_array_equal(f, fo)
    np.testing.assert_array_equal(m, mo)
    np.testing.assert_array_equal(host_flags_only(d, q), fo)
    d.close()


def test_pair_counts_are_the_column_popcounts():
    """mpg_collide_count on world B (an LDS counter per pair): the counts are
    the column sums of the masks collide_batch gives for the same samples,
    which are the oracle's."""
    d = dworld("B")
    w = WW.world("B")
    lim = w.art.joint_limits()[:7]
    lo, hi = np.ascontiguousarray(lim[:, 0]), np.ascontiguousarray(lim[:, 1])
    n, seed = 5000, 4242
    counts = np.full(d.n_pairs, -1, np.int64)
    C.check(C.lib().mpg_collide_count(d.handle, lo.ctypes.data_as(ctypes.c_void_p), hi.ctypes.data_as(ctypes.c_void_p),
                                      n, seed, counts.ctypes.data_as(ctypes.c_void_p), None), "mpg_collide_count")
    q = planner.sample_uniform(lo, hi, n, seed)
    f, m = d.collide_batch(q)
    fo, mo = w.collide_batch(q, nthreads=WW.NTHREADS)
    np.testing.assert_array_equal(f, fo)
    np.testing.assert_array_equal(m, mo)
    bits = (m[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1
    want = bits.reshape(n, -1).sum(axis=0)[:d.n_pairs]
    np.testing.assert_array_equal(counts, want)
    assert 0.2 < fo.mean() < 0.9 and (want[2048:] > 0).any() and (want == 0).any()
