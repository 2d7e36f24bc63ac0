"""CPU: the screw-motion header the device kernel runs (mplib_amd/csrc/mpg_screw.h,
compiled for the host by tests/native/screw_host.cpp) against the numpy
restatement of planner.py's plan_screw in tests/screw_cases.py.  No device."""
import numpy as np
import pytest

import screw_cases as S


def _transform(rng, angle, axis=None):
    T = np.eye(4)
    T[:3, :3] = S.axis_angle_mat(S.random_unit(rng, 1)[0] if axis is None else axis, angle)
    T[:3, 3] = rng.normal(scale=0.3, size=3)
    return T


def _angle_of_trace(tr):
    return np.arccos((tr - 1) / 2)


def test_exp_coordinates_match_numpy():
    """pose2exp_coordinate on 1000 random transforms (rotation angle uniform in
    (0.01, 3.1)) and on transforms placed on both sides of the two np.isclose
    thresholds: trace - 3 = -(1e-8 + 3e-5) (1 -+ 1e-3) and trace + 1 = (1e-8 +
    1e-5) (1 -+ 1e-3).  The branch must be equal; the twist within 1e-12 -- the
    two codes differ in operation order and in sin / cos / acos by an ulp; acos
    near the second threshold amplifies an ulp of its argument by 1 / sin(theta)
    ~ 320, and 1 / (2 sin(theta)) scales the skew part by the same factor, so
    ~1e-13 is expected there.  Measured: 5.3e-15."""
    rng = np.random.default_rng(7)
    Ts = [_transform(rng, a) for a in rng.uniform(0.01, 3.1, size=1000)]
    sides = []
    for f in (1 - 1e-3, 1 + 1e-3):
        for _ in range(8):
            sides.append(_transform(rng, _angle_of_trace(3 - (1e-8 + 3e-5) * f)))
            sides.append(_transform(rng, _angle_of_trace(-1 + (1e-8 + 1e-5) * f)))
    Ts += sides
    Ts += [_transform(rng, 0.0), _transform(rng, np.pi), _transform(rng, 1e-3), _transform(rng, np.pi - 1e-3)]
    Ts = np.array(Ts)
    tw, br = S.host_exp(Ts)
    want_br = np.zeros(len(Ts), np.int32)
    worst = 0.0
    for i, T in enumerate(Ts):
        want, want_br[i] = S.pose2exp_coordinate(T)
        if want is not None:
            worst = max(worst, np.abs(tw[i] - want).max())
    np.testing.assert_array_equal(br, want_br)
    print("exp coordinates: branches", np.bincount(want_br, minlength=3), "max|dtwist| %.3g" % worst)
    # all three branches occur, each threshold from both sides
    side_br = want_br[1000:1000 + len(sides)].reshape(2, 8, 2)
    assert (side_br[0, :, 0] == 1).all() and (side_br[1, :, 0] == 0).all()
    assert (side_br[0, :, 1] == 2).all() and (side_br[1, :, 1] == 0).all()
    assert (tw[br == 2] == 0).all()
    assert (tw[br == 1][:, 3:] == 0).all()
    assert worst <= 1e-12


@pytest.fixture(scope="module")
def header_rows():
    q0, goal = S.recipe_s()
    return S.host_header_rows(goal, q0, max_waypoints=512)


def test_recipe_s_matches_plan_screw(header_rows):
    """Recipe S against np_plan_screw.  On the rows whose sigma_min(J) stays >=
    1e-2 along the path status and count are equal and max|dq| <= 1e-9:
    operation order (~1e-16) times kappa(J J^T) <= 1e4 |J|^2, summed over at
    most 24 steps.  Over all 256 rows status or count may differ on at most 8.
    The reference on this recipe: 207 rows reach, 30 end at a limit, 19 stall;
    median 9 waypoints, at most 262; 159 rows are well conditioned (146 reach,
    13 end at a limit, at most 24 waypoints).  Its own two-run figure (second
    run from q_start + 1e-13 N(0, 1)): no status and no count differs on any of
    the 256 rows; the well-conditioned rows move by at most 5.4e-13.  The
    Cholesky form of the reference against pinv: no status or count differs,
    the reaching rows move by at most 6.8e-8 (rows passing near a singularity).
    Measured here: no row differs, max|dq| = 7.8e-14 on the well-conditioned
    rows, 3.7e-8 over all."""
    path, cnt, st = header_rows
    rst, rcnt, _, sig, _ = S.reference_s()
    well = sig >= S.WELL
    assert well.sum() >= 128 and (rst == S.REACHED).sum() >= 150
    differ, dmax = S.compare_paths(st, cnt, path)
    print("recipe S: reach %d limit %d stall %d; well %d; differ %d (well %d); max|dq| well %.3g all %.3g"
          % ((rst == 1).sum(), (rst == 8).sum(), (rst == 4).sum(), well.sum(), differ.sum(), differ[well].sum(),
             dmax[well].max(), dmax.max()))
    assert not differ[well].any()
    assert dmax[well].max() <= 1e-9
    assert differ.sum() <= 8
    assert not differ[rst == S.REACHED].any()


def test_step_length(header_rows):
    """Every step but a REACHED row's last has ||dq| - qpos_step| <= 1e-12
    (the scale qpos_step / |dq| is exact to an ulp of 0.1)."""
    path, cnt, st = header_rows
    worst = 0.0
    for i in range(len(cnt)):
        d = np.linalg.norm(np.diff(path[i, :cnt[i]], axis=0), axis=1)
        if st[i] & S.REACHED:
            assert d[-1] <= 0.1 + 1e-12
            d = d[:-1]
        if len(d):
            worst = max(worst, np.abs(d - 0.1).max())
    print("step length: max||dq| - 0.1| = %.3g" % worst)
    assert worst <= 1e-12


def test_padding_cap_and_end_bits(header_rows):
    """The row loop's bookkeeping: one end bit per row, the slots past count
    repeat the last waypoint, max_waypoints = 4 truncates without changing the
    first four waypoints."""
    path, cnt, st = header_rows
    q0, goal = S.recipe_s()
    assert all(bin(int(s)).count("1") == 1 for s in st)
    for i in range(len(cnt)):
        np.testing.assert_array_equal(path[i, cnt[i]:], np.broadcast_to(path[i, cnt[i] - 1], (512 - cnt[i], 7)))
        np.testing.assert_array_equal(path[i, 0], q0[i])
    p4, c4, s4 = S.host_header_rows(goal, q0, max_waypoints=4)
    more = cnt > 4
    # a row that ends while trying its fifth state (stall, limit) is TRUNCATED at 4 as well
    assert more.any() and (~more).any()
    np.testing.assert_array_equal(p4[:, :4][more], path[:, :4][more])
    assert (s4[more] == S.TRUNCATED).all() and (c4[more] == 4).all()
    short = cnt < 4
    np.testing.assert_array_equal(s4[short], st[short])
    np.testing.assert_array_equal(c4[short], cnt[short])
    np.testing.assert_array_equal(p4[short], path[short][:, :4])
    exact = (cnt == 4) & (st == S.REACHED)
    np.testing.assert_array_equal(s4[exact], st[exact])
