"""Survivor bucketing on the host (no GPU): the index arithmetic of
mplib_amd/csrc/mpg_bucket.h, which the cull tail, the three bucketing kernels
and get_workspace share, and a replay of range sum -> scan -> scatter on
random survivor words (tests/native/bucket_replay.cpp).  An out-of-range row
or slot base on the device is a stray write, so it is rehearsed here first."""
import ctypes
import os

import numpy as np
import pytest

from native.host_shim import _build

_HERE = os.path.dirname(os.path.abspath(__file__))
_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = _build(os.path.join(_HERE, "native", "bucket_replay.cpp"), "mplib_amd_bucket_replay")
        _lib.bucket_index_check.argtypes = [ctypes.c_longlong, ctypes.c_longlong, ctypes.c_int, ctypes.c_int]
        _lib.bucket_replay.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_int,
                                       ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    return _lib


def consts():
    out = (ctypes.c_int * 2)()
    lib().bucket_consts(out)
    return out[0], out[1]  # tiles per range, ranges per group


def launch_shape(n, W):
    """tiles, ranges, groups of a launch of n rows with W mask words, and bk_fold_sum's decision for it."""
    out = (ctypes.c_int * 4)()
    lib().bucket_launch_shape(ctypes.c_longlong(n), W, out)
    return dict(tiles=out[0], ranges=out[1], groups=out[2], fold=bool(out[3]))


def tile_counts():
    T, G = consts()
    return sorted({1, 2, max(T - 1, 1), T, T + 1, 3 * T + 5, T * G - 1, T * G, T * G + 1, 16384})


@pytest.mark.parametrize("block", [64, 128, 256])
def test_ranges_partition_tiles_and_sizes_cover_every_write(block):
    """For each tile count and cull block size: ranges partition the tiles and
    groups the ranges, every tile's row is written by exactly one cull wave,
    no wave with tile >= n_tiles passes the guard, and a workspace of any
    capacity >= n holds every count row, part row and group row of the call."""
    for tiles in tile_counts():
        for n in {tiles * 64, tiles * 64 - 63, max(tiles * 64 - 1, 1)}:
            for cap in (n, n + 1, max(n, 20000), 1 << 20):
                if cap < n:
                    continue
                for W in (1, 5, 18, 35, 70):
                    assert lib().bucket_index_check(n, cap, W, block) == 0, (tiles, n, cap, W)


def replay(W, n_pairs, n, cap, block, seed, density=0.06):
    rng = np.random.default_rng(seed)
    bits = rng.random((W * 32, cap)) < density
    bits[n_pairs:] = False
    # a few crowded tiles and pairs: counts up to the 64 a byte must hold
    bits[: min(3, n_pairs), : min(cap, 200)] = True
    surv = np.zeros((W, cap), np.uint32)
    for p in range(W * 32):
        surv[p >> 5] |= bits[p].astype(np.uint32) << np.uint32(p & 31)
    surv = np.ascontiguousarray(surv)
    nc = ctypes.c_longlong(0)
    paths = (ctypes.c_int * 5)()
    rc = lib().bucket_replay(W, n_pairs, n, cap, block, surv.ctypes.data, ctypes.byref(nc), paths)
    assert rc == 0, f"bucket_replay.cpp:{rc} (W={W}, pairs={n_pairs}, n={n}, cap={cap}, block={block})"
    assert nc.value == int(bits[:, :n].sum())
    return dict(fold=bool(paths[0]), sum_passes=paths[1], col_passes=paths[2], rounds=paths[3], groups=paths[4])


# the last three: worlds of a Panda and 100 / 200 boxes (tests/wide_worlds.py),
# and a pair count of a multiple of 1024 plus one
@pytest.mark.parametrize("W,n_pairs", [(1, 7), (5, 129), (18, 547), (35, 1119), (70, 2219), (65, 2049)])
def test_host_replay_matches_direct_lists(W, n_pairs):
    """Stale workspace contents (the replay poisons cnt, part and grp first)
    must not show; candidate lists equal per-pair sorted lists built directly.
    More than 32 mask words: the range sums pass over the count row more than
    once, the scan over the columns more than once, the task prefix runs a
    round per 1024 pairs; 4160 rows fold the range sums into the scan up to 56
    mask words and not above."""
    T, G = consts()
    R = 64 * T
    seen = []
    for i, n in enumerate((1, 63, 64, 65, 255, 256, 257, R - 1, R, R + 1, 3 * R + 17, 4160, G * R + 65)):
        for block in (64, 128, 256):
            seen.append((n, replay(W, n_pairs, n, n + (i % 3) * 777, block, seed=1000 * W + n)))
    for n, p in seen:
        assert p["sum_passes"] == (W * 8 + 255) // 256  # per block
        assert p["col_passes"] == (W * 32 + 1023) // 1024 and p["rounds"] == (n_pairs + 1023) // 1024
        assert p["fold"] == (-(-n // R) * W * 8 <= 4096)
    assert max(p["groups"] for _, p in seen) == 2
    assert dict(seen)[4160]["fold"] == (W <= 56)
    if W > 32:  # narrower worlds fold at every size here
        assert {p["fold"] for _, p in seen} == {True, False}


def test_host_replay_no_pairs():
    replay(1, 0, 300, 300, 256, seed=3)
