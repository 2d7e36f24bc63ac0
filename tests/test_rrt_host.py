"""CPU: the RRTConnect header the device kernels run (mplib_amd/csrc/mpg_rrt.h and
mpg_plan_batch's argument checks in mpg_args_host.h, compiled for the host by
tests/native/rrt_host.cpp) against the numpy restatement of the algorithm in
tests/rrt_cases.py, with the CPU oracle as state validity.  No device.

All comparisons are exact: the arithmetic is a + (b - a) * t, sums of |diff|
in dimension order, one division per motion and ceil, with no library call."""
import numpy as np
import pytest

import rrt_cases as R
from mplib_amd import planner as P

NAMES = ("path", "n_waypoints", "status", "iterations", "tree_sizes")


def assert_same(got, want):
    for name, a, b in zip(NAMES, got, want):
        np.testing.assert_array_equal(a, b, err_msg=name)


def test_recipe_r_header_equals_numpy():
    """The header and the numpy restatement on recipe R and its extra row:
    every output bit-equal.  The numpy reference solves 61 of the 64 rows
    within MAX_ROUNDS = 4000 / MAX_NODES = 1024 (two run out of rounds, one
    fills its start tree), so all three end states are compared; 13 rows grow
    a tree past 256 nodes, more nodes than the device's scan has threads."""
    ref, hdr = R.reference_r(), R.header_r()
    assert_same(hdr, ref)
    _, cnt, st, it, sz = ref
    st, sz = st[:R.N_ROWS], sz[:R.N_ROWS]
    print("recipe R: solved %d, rounds exhausted %d, nodes exhausted %d; rows past 256 nodes %d; longest path %d"
          % ((st == R.SOLVED).sum(), (st == R.ROUNDS_EXHAUSTED).sum(), (st == R.NODES_EXHAUSTED).sum(),
             (sz.max(axis=1) > 256).sum(), cnt.max()))
    assert (st == R.SOLVED).sum() >= 60
    assert (sz.max(axis=1) > 256).any()
    assert (it[:R.N_ROWS][st == R.SOLVED] >= 1).all()


def test_solved_paths_are_valid_solutions():
    """Every solved row of recipe R: the path starts at the start and ends at
    the goal, every state is valid and inside the bounds, every edge is at most
    range long and its DiscreteMotionValidator states are valid; the slots past
    the count repeat the last waypoint, a row without a path holds its start."""
    lo, hi = R.limits()
    start, goal, _ = R.recipe_r()
    path, cnt, st, _, _ = R.header_r()
    sp = R.Space(lo, hi, 0, R.RANGE)
    for r in range(R.N_BATCH):
        if st[r] == R.SOLVED:
            assert 2 <= cnt[r] <= R.MAX_WAYPOINTS
            R.assert_valid_solution(sp, path[r, :cnt[r]], start[r], [goal[r]], R.oracle_valid)
            np.testing.assert_array_equal(path[r, cnt[r]:], np.broadcast_to(path[r, cnt[r] - 1], path[r, cnt[r]:].shape))
        else:
            assert cnt[r] == 0
            np.testing.assert_array_equal(path[r], np.broadcast_to(start[r], path[r].shape))


def test_sampler_is_sample_uniform():
    """Coordinate j of the sample of iteration k is value (k, j) of
    planner.sample_uniform(lo, hi, seed = row seed); without row_seed the row's
    seed is splitmix64(seed + (r + 1) * golden)."""
    import ctypes
    lo, hi = R.limits()
    lib = R.host_lib()
    for row_seed in (0, 12345, 2 ** 64 - 1, R.row_seed_of(7, 3)):
        for k in (0, 1, 17, 3999):
            want = P.sample_uniform(lo, hi, 1, row_seed, offset=k)[0]
            np.testing.assert_array_equal(R.np_sample(lo, hi, row_seed, k), want)
            for j in (0, 3, 6):
                got = lib.rrt_host_sample(R._p(lo), R._p(hi), 7, ctypes.c_ulonglong(row_seed), k, j)
                assert got == want[j], (row_seed, k, j)
    for seed, r in ((0, 0), (7, 3), (2 ** 64 - 1, 64)):
        assert lib.rrt_host_row_seed(ctypes.c_ulonglong(seed), ctypes.c_ulonglong(r)) == R.row_seed_of(seed, r)
    # the first splitmix64 output for seed 0 (test_collision_pair pins the same constant)
    assert R.splitmix64(R._GOLDEN) == 0xE220A8397B1DCDAF


def test_seed_without_row_seed_array():
    """row_seed NULL: the rows' seeds derive from `seed` and the row index."""
    lo, hi = R.limits()
    start, goal, _ = R.recipe_r()
    seeds = np.array([R.row_seed_of(99, r) for r in range(3)], np.uint64)
    got = R.host_plan_batch(lo, hi, start[:3], goal[:3], None, R.oracle_valid, seed=99)
    assert_same(got, R.np_plan_batch(lo, hi, start[:3], goal[:3], seeds, R.oracle_valid))


def test_rounds_follow_from_iterations_and_tree_sizes():
    """A row's rounds (growTree calls) = iterations + nodes added - 1 when it
    solved: every iteration extends once, every connect step either adds a node
    or is the one TRAPPED that ends its chain, and only the solving chain ends
    without one.  The rounds are counted by the numpy model's driver; the
    iterations and tree sizes are the header's.  tools/plan_bench.py reports
    rounds this way."""
    lo, hi = R.limits()
    start, goal, seeds = R.recipe_r()
    ref = R.reference_r()
    solved = lambda rows: [r for r in rows if ref[2][r] == R.SOLVED]  # noqa: E731
    idx = np.array(solved(range(8))[:5] + solved(hard_rows())[:2])
    rounds = []
    R.np_plan_batch(lo, hi, start[idx], goal[idx], seeds[idx], R.oracle_valid, rounds_out=rounds)
    _, _, st, it, sz = R.host_plan_batch(lo, hi, start[idx], goal[idx], seeds[idx], R.oracle_valid)
    assert (st == R.SOLVED).all()
    np.testing.assert_array_equal(rounds, it + sz.sum(axis=1) - 2 - 1)


def hard_rows():
    """Rows of recipe R that need many rounds (a tree past 256 nodes)."""
    return np.flatnonzero(R.reference_r()[4][:R.N_ROWS].max(axis=1) > 256)


@pytest.mark.parametrize("opts,bit", [(dict(max_nodes=8), R.NODES_EXHAUSTED), (dict(max_rounds=5), R.ROUNDS_EXHAUSTED)])
def test_limits_end_the_row(opts, bit):
    lo, hi = R.limits()
    start, goal, seeds = R.recipe_r()
    idx = hard_rows()[:3]
    got = R.host_plan_batch(lo, hi, start[idx], goal[idx], seeds[idx], R.oracle_valid, **opts)
    assert_same(got, R.np_plan_batch(lo, hi, start[idx], goal[idx], seeds[idx], R.oracle_valid, **opts))
    assert (got[2] == bit).all() and (got[1] == 0).all()
    if "max_nodes" in opts:
        assert (got[4].max(axis=1) == 8).all()


def test_truncated_path():
    """max_waypoints = 2 on rows whose path is longer: SOLVED | TRUNCATED, count 0."""
    lo, hi = R.limits()
    start, goal, seeds = R.recipe_r()
    ref = R.reference_r()
    idx = np.flatnonzero((ref[2] == R.SOLVED) & (ref[1] > 2))[:3]
    got = R.host_plan_batch(lo, hi, start[idx], goal[idx], seeds[idx], R.oracle_valid, max_waypoints=2)
    assert_same(got, R.np_plan_batch(lo, hi, start[idx], goal[idx], seeds[idx], R.oracle_valid, max_waypoints=2))
    assert (got[2] == (R.SOLVED | R.TRUNCATED)).all() and (got[1] == 0).all()
    np.testing.assert_array_equal(got[3], ref[3][idx])
    np.testing.assert_array_equal(got[4], ref[4][idx])


def test_invalid_endpoints_and_goal_lists():
    """A colliding start, a colliding only goal, a start outside the bounds,
    and goal lists: [colliding, free] plans to the second goal, [free, free]
    ends at one of the two."""
    import worlds as Wd
    lo, hi = R.limits()
    start, goal, seeds = R.recipe_r()
    bad = np.array(Wd.KAT_COLLIDING)
    assert R.oracle_valid(bad[None])[0] != 0
    out = start[0].copy()
    out[0] = hi[0] + 0.5
    s = np.array([bad, start[0], out, start[0], start[1]])
    g = np.array([[goal[0], goal[0]], [bad, bad], [goal[0], goal[0]], [bad, goal[0]], [goal[1], goal[2]]])
    got = R.host_plan_batch(lo, hi, s, g, seeds[:5], R.oracle_valid)
    assert_same(got, R.np_plan_batch(lo, hi, s, g, seeds[:5], R.oracle_valid))
    path, cnt, st, _, sz = got
    assert list(st[:3]) == [R.START_INVALID, R.GOAL_INVALID, R.START_INVALID]
    assert st[3] == R.SOLVED and sz[3, 1] >= 1
    np.testing.assert_array_equal(path[3, cnt[3] - 1], goal[0])
    assert st[4] == R.SOLVED
    sp = R.Space(lo, hi, 0, R.RANGE)
    R.assert_valid_solution(sp, path[4, :cnt[4]], start[1], [goal[1], goal[2]], R.oracle_valid)


def test_so2_wraps_the_short_way():
    """A 3-slot space whose middle slot is SO2, everything valid: from 3.0 to
    -3.0 the path crosses +-pi (0.28 rad) instead of going 6 rad round, every
    state stays in [-pi, pi], and the header equals the numpy model bit for
    bit; so does a run with an obstacle band across the wrap."""
    lo, hi = np.array([-1.0, -7.0, -2.0]), np.array([1.0, 7.0, 2.0])
    s = np.array([[0.5, 3.0, -1.0], [-0.2, -3.1, 0.3]])
    g = np.array([[-0.5, -3.0, 1.0], [0.4, 2.9, -0.7]])
    seeds = np.array([5, 6], np.uint64)
    free = lambda q: np.zeros(len(q), np.uint8)  # noqa: E731
    kw = dict(range_=0.05, max_rounds=2000, max_nodes=256, max_waypoints=128, so2_mask=2)
    got = R.host_plan_batch(lo, hi, s, g, seeds, free, **kw)
    assert_same(got, R.np_plan_batch(lo, hi, s, g, seeds, free, **kw))
    path, cnt, st, _, _ = got
    assert (st == R.SOLVED).all()
    sp = R.Space(lo, hi, 2, 0.05)
    for r in range(2):
        p = path[r, :cnt[r]]
        R.assert_valid_solution(sp, p, s[r], [g[r]], free)
        assert (np.abs(p[:, 1]) <= np.pi).all()
        assert np.abs(np.diff(p[:, 1])).max() > 6.0  # one edge jumps over the seam
        assert sum(float(sp.distance(a, b)) for a, b in zip(p[:-1], p[1:])) < 4.0
    band = lambda q: ((np.abs(q[:, 1]) > 3.12) & (q[:, 0] > -0.8)).astype(np.uint8)  # noqa: E731
    got = R.host_plan_batch(lo, hi, s, g, seeds, band, **kw)
    assert_same(got, R.np_plan_batch(lo, hi, s, g, seeds, band, **kw))
    assert (got[2] == R.SOLVED).all() and (got[3] > 1).any()


def test_view_figures():
    """extent, longest valid segment, range and the slot block of the Panda and of a space with an SO2 slot."""
    lo, hi = R.limits()
    extent = float((hi - lo).sum())
    rc, msg, rng, lvs, blk = R.host_view(lo, hi, range_=0.1)
    assert (rc, msg) == (0, "") and rng == 0.1 and lvs == pytest.approx(0.01 * extent, rel=1e-15)
    assert blk == int(np.ceil(0.1 / lvs)) + 2 == 3
    rc, _, rng, lvs, blk = R.host_view(lo, hi)  # range 0: OMPL's default
    assert rc == 0 and rng == pytest.approx(0.2 * extent, rel=1e-15) and blk in (22, 23)
    rc, _, rng, lvs, _ = R.host_view([-1.0, -np.inf], [1.0, np.inf], so2_mask=2, range_=1e-7)
    assert rc == 0 and lvs == pytest.approx(0.01 * (2.0 + np.pi), rel=1e-15) and rng == pytest.approx(20 * lvs, rel=1e-15)


REFUSALS = [
    (dict(G=0), "G outside [1, 16]"), (dict(G=17), "G outside [1, 16]"),
    (dict(max_nodes=1), "max_nodes outside [2, 65536]"), (dict(max_nodes=65537), "max_nodes outside [2, 65536]"),
    (dict(max_waypoints=1), "max_waypoints outside [2, 4096]"), (dict(max_waypoints=4097), "max_waypoints outside [2, 4096]"),
    (dict(max_rounds=0), "max_rounds < 1"), (dict(check_every=0), "check_every < 1"),
    (dict(range_=np.inf), "non-finite range"), (dict(range_=np.nan), "non-finite range"),
    (dict(so2_mask=1 << 7), "so2_mask has a bit at or above dof"), (dict(Q=-1), "Q < 0"),
]


@pytest.mark.parametrize("kw,reason", REFUSALS)
def test_argument_refusals(kw, reason):
    lo, hi = R.limits()
    rc, msg, *_ = R.host_view(lo, hi, **kw)
    assert (rc, msg) == (1, reason)


def test_argument_refusals_of_the_space():
    lo, hi = R.limits()
    rc, msg, *_ = R.host_view(np.zeros(33), np.ones(33))
    assert (rc, msg) == (2, "mpg_plan_batch supports dof <= 32")
    assert R.host_view(np.zeros(32), np.ones(32), so2_mask=1 << 31)[0] == 0
    bad_lo = lo.copy()
    bad_lo[2] = -np.inf
    rc, msg, *_ = R.host_view(bad_lo, hi)
    assert rc == 1 and msg.startswith("dof slot 2:")
    assert R.host_view(bad_lo, hi, so2_mask=4)[0] == 0  # an SO2 slot needs no limits
    rc, msg, *_ = R.host_view(hi, lo)
    assert rc == 1 and msg.startswith("dof slot 0:")
    rc, msg, *_ = R.host_view(lo, lo)
    assert (rc, msg) == (1, "the state space has no extent")
    # the trees' doubles: Q * 2 * max_nodes * dof against 2^31, the product named
    per_row = 2 * 65536 * 7
    assert R.host_view(lo, hi, Q=2 ** 31 // per_row, max_nodes=65536)[0] == 0
    rc, msg, *_ = R.host_view(lo, hi, Q=2 ** 31 // per_row + 1, max_nodes=65536)
    assert rc == 1 and msg == "Q * 2 * max_nodes * dof = %d * %d exceeds 2^31 doubles of tree storage" % (
        2 ** 31 // per_row + 1, per_row)
    rc, msg, *_ = R.host_view(lo, hi, Q=2 ** 62, max_nodes=2)
    assert rc == 1 and "exceeds 2^31" in msg
    # the round's states: range 1000 has some 3000 per row
    rc, msg, *_ = R.host_view(lo, hi, Q=2 ** 20, max_nodes=2, range_=1e3)
    assert rc == 1 and msg.endswith("states per round exceeds 2^31")
    rc, msg, *_ = R.host_view(lo, hi, range_=1e9, max_nodes=2)
    assert rc == 1 and msg.startswith("range / (0.01 * extent)")
