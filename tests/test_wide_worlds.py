"""Worlds with thousands of collision pairs, the host half (no GPU).

The cull kernel's block size and dynamic LDS (choose_block and
cull_lds_per_thread of mplib_amd/csrc/mpg_broadphase.h, through
tests/native/host_fk.cpp) over every per-thread size, with the bands in which
a launch asks for more than 64 KiB of dynamic LDS; the three wide worlds of
tests/wide_worlds.py reach the pair counts, mask words and LDS bands they are
named for; and the oracle's own output on every batch the GPU tests
(tests/test_wide_worlds_gpu.py) take is neither all free nor all colliding
and reaches the high pair columns."""
import pytest

import wide_worlds as WW

CU_LDS = 160 * 1024
BLOCKS = (256, 128, 64)


def waves_per_cu(per_thread, block):
    """Resident waves of blocks of `block` threads with per_thread LDS bytes each: at most 32 per CU."""
    lds = per_thread * block
    return 0 if lds > CU_LDS else min(32, CU_LDS // lds * (block // 64))


def lds_bands(lo=64, hi=2560, above=64 * 1024):
    """[(first, last, block)] of the per-thread sizes whose launch takes more than `above` bytes."""
    bands = []
    for p in range(lo, hi + 1):
        block, lds = WW.choose_block(p)
        if lds > above:
            if bands and bands[-1][1] == p - 1 and bands[-1][2] == block:
                bands[-1] = (bands[-1][0], p, block)
            else:
                bands.append((p, p, block))
    return bands


def test_choose_block_keeps_the_most_waves_resident():
    for p in range(64, 2700):
        block, lds = WW.choose_block(p)
        if 64 * p > CU_LDS:  # exactly when not even one wave fits
            assert (block, lds) == (-1, -1), p
            continue
        assert block in BLOCKS and lds == p * block <= CU_LDS, p
        waves = {b: waves_per_cu(p, b) for b in BLOCKS}
        assert waves[block] == max(waves.values()) > 0, (p, block, waves)
        assert all(waves[b] < waves[block] for b in BLOCKS if b > block), (p, block, waves)  # ties: the larger block
    assert WW.choose_block(2560) == (64, CU_LDS) and WW.choose_block(2561) == (-1, -1)


def test_lds_bands_above_64_kib():
    """Where cull_kernel is launched with more than 64 KiB of dynamic LDS: two
    bands of 256-thread blocks (two blocks and one block per CU), then blocks
    of 128 and of 64 threads that fill the CU alone."""
    bands = lds_bands()
    print("per-thread LDS bytes with a launch above 64 KiB (first, last, block):", bands)
    for first, last, block in bands:
        print(f"  {first}..{last} B/thread: block {block}, {first * block / 1024:.1f}..{last * block / 1024:.1f} KiB")
    assert bands == [(285, 320, 256), (513, 640, 256), (854, 1280, 128), (1281, 2560, 64)]


def test_lds_per_thread_formula():
    """records (3 floats per moving object) + FK save slots past the two in
    registers (12 floats) + survivor words + the wave's share of the SAT queue."""
    for nm, ns, W in ((11, 0, 1), (11, 2, 35), (11, 3, 70), (0, 0, 1), (40, 7, 104)):
        assert WW.lds_per_thread(nm, ns, W) == 12 * max(nm, 1) + 48 * max(ns - 2, 0) + 4 * W + 8


WANT = {  # pairs above, mask words (above, at most), cull block, LDS bytes (above, at most)
    "A": dict(pairs=1024, words=(32, 64), block=256, lds=(64 * 1024, 80 * 1024)),
    "B": dict(pairs=2048, words=(64, 10 ** 6), block=None, lds=None),
    "C": dict(pairs=2048, words=(64, 10 ** 6), block=256, lds=(128 * 1024, 160 * 1024)),
}


def check_world_reaches(name):
    want = WANT[name]
    P, W = WW.n_pairs(name), WW.mask_words(name)
    block, lds, per = WW.predicted_cull(name)
    print(f"world {name}: {P} pairs, {W} mask words, {per} B/thread, cull block {block}, {lds} B of LDS")
    assert P == 19 + 11 * WW.SPEC[name]["boxes"]
    assert P > want["pairs"] and want["words"][0] < W <= want["words"][1]
    if want["block"]:
        assert block == want["block"] and want["lds"][0] < lds <= want["lds"][1]
    return P, W, block, lds


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_world_reaches_what_it_is_named_for(name):
    check_world_reaches(name)
    d = WW.desc(name)
    assert WW.predicted_cull(name)[2] == WW.lds_per_thread(len(d["moving_link"]), WW.cull_saves(d), WW.mask_words(name))


# the batches of tests/test_wide_worlds_gpu.py
BATCHES = {"A": (64, 65, 1000, 4160, 20000, WW.N_BASE), "B": (64, 65, 1000, 4160, 20000, WW.N_BASE), "C": (65, 4160)}


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_oracle_alone_meets_the_batch_conditions(name):
    for n in BATCHES[name]:
        WW.check_oracle_conditions(name, WW.batch(name, n), structure=n >= 1000)
    q, f, m = WW.batch(name, 1)
    assert f[0] == 1 and (m[0] != 0).sum() >= 2
    for colliding in (True, False):
        _, fr, mr = WW.repeated(name, colliding, 5)
        assert (fr == colliding).all() and ((mr != 0).any(axis=1) == colliding).all()
