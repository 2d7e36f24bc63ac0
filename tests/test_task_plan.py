"""The narrow phase's task list on the host (no GPU): the task-size levels of
mplib_amd/csrc/mpg_bucket.h (bk_task_plan, bk_pair_tasks, bk_task_range),
which range_scan_kernel, narrow_kernel, closed_form_kernel and contact_kernel
share, replayed by tests/native/task_plan.cpp on random segment lengths.  A
task range past its pair's candidates is a stray read of the candidate list on
the device, so it is rehearsed here first.

task_plan_check (0, or the line of its first failed check) verifies per call:
the tasks of every pair partition [0, len) in order, none empty, none larger
than its level or reaching into the next; the per-pair task counts sum to the
scan loop's prefix and the binary search maps every task back to its pair; a
one-level plan reproduces (k * ts, min(len, k * ts + ts)); a launch with
all <= target_tasks * kTask has one level; 32-bit sums equal 64-bit ones."""
import ctypes
import os

import numpy as np
import pytest

from native.host_shim import _build

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "native", "task_plan.cpp")
_lib = None

TS_MIN, TS_MAX = 8, 128  # MPG_TASK_MIN, MPG_TASK of the product build
TAPER = (0.25, 64)       # MPG_TAPER_C, MPG_TAPER_MIN of the product build
DEEP = dict(c=0.5, s_min=16)  # settings that use every level the plan holds: 128 -> 64 -> 32 -> 16
TARGET = 3072            # 4 * narrow blocks on an MI355X


def lib():
    global _lib
    if _lib is None:
        _lib = _build(_SRC, "mplib_amd_task_plan")
        _lib.task_plan_check.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32,
                                         ctypes.c_uint32, ctypes.c_double, ctypes.c_uint32,
                                         ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_longlong)]
        _lib.task_plan_fill.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                        ctypes.c_double, ctypes.c_uint32, ctypes.c_void_p]
    return _lib


def levels_const():
    out = (ctypes.c_int * 1)()
    lib().task_plan_consts(out)
    return out[0]


def plan(all_, target, ts_min=TS_MIN, ts_max=TS_MAX, c=TAPER[0], s_min=TAPER[1]):
    L = levels_const()
    out = np.zeros(1 + 2 * L, np.uint32)
    lib().task_plan_fill(all_, target, ts_min, ts_max, c, s_min, out.ctypes.data)
    n = int(out[0])
    return n, [int(x) for x in out[1:1 + L]], [int(x) for x in out[1 + L:]]


def check(seg_len, target, ts_min=TS_MIN, ts_max=TS_MAX, c=TAPER[0], s_min=TAPER[1]):
    seg = np.ascontiguousarray(seg_len, dtype=np.uint32)
    lv, nt = ctypes.c_int(0), ctypes.c_longlong(0)
    rc = lib().task_plan_check(seg.ctypes.data, len(seg), target, ts_min, ts_max, c, s_min, ctypes.byref(lv),
                               ctypes.byref(nt))
    assert rc == 0, f"task_plan.cpp:{rc} (pairs={len(seg)}, all={int(seg.sum(dtype=np.uint64))}, target={target}, " \
                    f"ts=[{ts_min}, {ts_max}], c={c}, s_min={s_min})"
    return lv.value, nt.value


def test_plan_levels_follow_the_remaining_candidates():
    """c = 0.5, s_min = 16 at kTask = 128: the last target * 64 candidates are
    tapered 64 -> 32 -> 16; the product's c = 0.25, s_min = 64: the last
    target * 32 candidates in tasks of 64; launches up to target * kTask
    candidates keep one level with the task size from before the plan."""
    all_ = 873368  # cfg3 at 2^20 rows
    n, g, s = plan(all_, TARGET, **DEEP)
    assert n == 4 and s == [128, 64, 32, 16]
    assert g == [0, all_ - 64 * TARGET, all_ - 32 * TARGET, all_ - 16 * TARGET]
    n, g, s = plan(all_, TARGET)
    assert n == 2 and s[:2] == [128, 64] and g[:2] == [0, all_ - 32 * TARGET] and g[2] == g[3] == 0xffffffff
    for a in (0, 1, 7, 27000, TARGET * TS_MAX - 1, TARGET * TS_MAX):
        n, g, s = plan(a, TARGET)
        ts = min(max(-(-a // TARGET), TS_MIN), TS_MAX)
        assert n == 1 and g[0] == 0 and s[0] == (ts + 7) // 8 * 8, a
    assert plan(TARGET * TS_MAX + 1, TARGET)[0] == 2 and plan(TARGET * TS_MAX + 1, TARGET, **DEEP)[0] == 4
    assert plan(10 ** 6, 0)[0] == 1                       # no target: plain kTask tasks
    assert plan(10 ** 6, TARGET, s_min=64)[2][:2] == [128, 64] and plan(10 ** 6, TARGET, s_min=64)[0] == 2
    assert plan(10 ** 6, TARGET, s_min=1)[0] == levels_const()  # never more levels than the plan holds
    assert plan(600, 4, c=4.0, s_min=16)[0] == 4          # c > 1: starts clamp to 0, still ascending


def random_lengths(rng, n_pairs, hi, zeros=0.25):
    seg = rng.integers(0, hi + 1, n_pairs, dtype=np.int64)
    seg[rng.random(n_pairs) < zeros] = 0
    return seg


@pytest.mark.parametrize("target", [0, 1, 4, 64, TARGET])
def test_random_segment_lengths(target):
    rng = np.random.default_rng(17 + target)
    seen = set()
    # 1119 and 2219 pairs: a Panda and 100 / 200 boxes (tests/wide_worlds.py), prefixes of more than 1024 pairs
    for rounds, n_pairs, hi in ((40, 7, 40), (40, 129, 300), (20, 160, 6000), (6, 547, 30000), (3, 160, 1 << 20),
                                (4, 1119, 3000), (3, 2219, 3000), (2, 2219, 20000)):
        for _ in range(rounds):
            seg = random_lengths(rng, n_pairs, hi)
            seen.add(check(seg, target)[0])
            seen.add(check(seg, target, **DEEP)[0])
    assert 1 in seen
    if 1 <= target <= 64:
        assert 2 in seen and levels_const() in seen


def test_pairs_straddling_level_starts():
    """Pairs placed against the level starts g1 < g2 < g3 of a 4-level plan:
    shorter than the smallest level, straddling one, two and three starts,
    and starting exactly on a start."""
    target = 4
    rng = np.random.default_rng(5)
    for total in (600, 777, 4096, 3403):
        n, g, s = plan(total, target, **DEEP)
        assert n == 4
        g1, g2, g3 = g[1:]
        layouts = [
            [g1, g2 - g1, g3 - g2, total - g3],                    # level starts coincide with pair starts
            [g1 - 3, 5, total - g1 - 2],                           # a short pair over g1
            [g1 - 1, g2 - g1 + 2, total - g2 - 1],                 # one pair over g1 and g2
            [g1 - 7, total - g1 + 7],                              # one pair over g1, g2 and g3
            [total],                                               # one pair over every start
            [0, g1, 0, 0, g2 - g1, 0, total - g2],                 # zeros between
            [3] * (total // 3) + [total % 3],                      # all below the smallest level
            [g3 + 1, 1, 1, 1, total - g3 - 4],
        ]
        for seg in layouts:
            assert sum(seg) == total and min(seg) >= 0
            assert check(seg, target, **DEEP)[0] == 4
            assert check(seg, target)[0] == 2
        for _ in range(30):  # random cuts of the same total
            cuts = np.sort(rng.integers(0, total + 1, rng.integers(1, 40)))
            seg = np.diff(np.concatenate([[0], cuts, [total]]))
            assert check(seg, target, **DEEP)[0] == 4


def test_one_level_is_the_plain_list():
    """Below the clamp (cfg2's 2^16 rows, every small test) the tasks are the
    ones before the plan: task_plan_check compares each with (k * ts,
    min(len, k * ts + ts)) and each pair's count with ceil(len / ts)."""
    rng = np.random.default_rng(11)
    for target, hi in ((TARGET, 2400), (TARGET, 170), (4, 3), (64, 60)):
        for _ in range(10):
            seg = random_lengths(rng, 160, hi)
            if seg.sum() > target * TS_MAX:
                seg = seg // 2
            assert check(seg, target)[0] == 1


def test_largest_launch_has_no_32_bit_overflow():
    """2^20 configurations x 160 pairs, every one a candidate."""
    assert check(np.full(160, 1 << 20), TARGET)[0] == 2
    lv, tasks = check(np.full(160, 1 << 20), TARGET, **DEEP)
    assert lv == 4 and tasks > (160 << 20) // TS_MAX
    check(np.full(160, 1 << 20), 1)
    check(np.full(160, 1 << 20), TARGET, ts_max=96, s_min=1)  # sizes that are no power of two


@pytest.mark.parametrize("c,s_min", [(0.25, 16), (1.0, 16), (0.5, 8), (0.5, 32), (1.0, 32), (2.0, 16), (0.5, 64), (1.0, 64)])
def test_other_taper_settings(c, s_min):
    rng = np.random.default_rng(int(c * 100) + s_min)
    for target, n_pairs, hi in ((4, 40, 300), (TARGET, 160, 12000)):
        for _ in range(5):
            check(random_lengths(rng, n_pairs, hi), target, c=c, s_min=s_min)

