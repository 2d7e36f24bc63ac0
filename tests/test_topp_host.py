"""mpg_topp.h (the code topp_row_kernel / topp_sample_kernel run) compiled for
the host, against the numpy restatement of topp_cases.py: the spline against
scipy's CubicSpline, the controllable sets against HiGHS, the profile's
feasibility and greediness, durations, samples, status paths and
mpg_topp_batch's argument checks.  No GPU.

Measured on the host build (printed by the tests):
spline 6.6e-15 relative (bound 1e-11), K against HiGHS 3.5e-15 relative (bound
1e-6), duration against np_topp 9.9e-16 relative (bound 1e-5: ten times the
worse of the two bounds), samples against np_samples 1.9e-13.
"""
import numpy as np
import pytest

import topp_cases as T

SPLINE_TOL = 1e-11   # operation order and a condition number of a few for the tridiagonal system
K_TOL = 1e-6         # HiGHS works to a feasibility tolerance of 1e-7
DURATION_TOL = 10 * max(SPLINE_TOL, K_TOL)  # Lipschitz in K and the spline; 10 covers the sum over N intervals


def rel(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


# --- 1. spline -----------------------------------------------------------------
@pytest.mark.parametrize("n", [4, 5, 9, 40])
def test_spline_against_cubicspline(n):
    q = np.random.default_rng(100 + n).uniform(T.LIMITS[:, 0], T.LIMITS[:, 1], size=(n, 7))
    s = np.linspace(0.0, 1.0, 57)
    cs = T.np_spline(q)
    got = T.host_spline_eval(q, T.host_spline(q), s)
    worst = max(rel(g, cs(s, d)) for d, g in enumerate(got))
    print(f"spline n={n}: value / first / second derivative within {worst:.2e} relative of CubicSpline")
    assert worst <= SPLINE_TOL


def test_spline_three_points_is_the_parabola():
    q = np.random.default_rng(3).uniform(T.LIMITS[:, 0], T.LIMITS[:, 1], size=(3, 7))
    s = np.linspace(0.0, 1.0, 57)
    M = T.host_spline(q)
    val, d1, d2 = T.host_spline_eval(q, M, s)
    for j in range(7):
        c = np.polyfit([0.0, 0.5, 1.0], q[:, j], 2)
        assert np.abs(val[:, j] - np.polyval(c, s)).max() <= SPLINE_TOL * np.abs(q[:, j]).max()
        assert np.abs(d1[:, j] - np.polyval(np.polyder(c), s)).max() <= SPLINE_TOL * np.abs(d1[:, j]).max()
        assert np.abs(d2[:, j] - 2 * c[0]).max() <= SPLINE_TOL * abs(2 * c[0])
    assert (M == M[0]).all()


def test_spline_two_points_is_exactly_linear():
    q = np.random.default_rng(2).uniform(T.LIMITS[:, 0], T.LIMITS[:, 1], size=(2, 7))
    s = np.linspace(0.0, 1.0, 57)
    M = T.host_spline(q)
    assert (M == 0.0).all()
    val, d1, d2 = T.host_spline_eval(q, M, s)
    assert np.array_equal(val, q[0] * (1.0 - s)[:, None] + q[1] * s[:, None])
    assert np.array_equal(d1, np.broadcast_to(q[1] - q[0], d1.shape)) and (d2 == 0.0).all()


# --- 2. controllable sets --------------------------------------------------------
def test_controllable_sets_against_highs():
    """The header's Fourier-Motzkin K against the LP optimum, interior gridpoints of the unif and three rows."""
    path, cnt, _ = T.recipe_t()
    host, ref = T.host_t(8), T.reference_t(8)
    worst = 0.0
    for r in np.concatenate([T.rows_of("unif"), T.rows_of("three")]):
        N = ref[r]["N"]
        worst = max(worst, (np.abs(host["grid_k"][r, 1:N] - ref[r]["K"][1:N]) / ref[r]["K"][1:N]).max())
    print(f"K: closed form within {worst:.2e} relative of HiGHS")
    assert worst <= K_TOL


# --- 3. feasibility and greediness -----------------------------------------------
@pytest.mark.parametrize("gps", [4, 8])
def test_profile_is_feasible_and_greedy(gps):
    path, cnt, _ = T.recipe_t()
    host = T.host_t(gps)
    assert (host["status"] == T.OK).all()
    for r in range(len(cnt)):
        N = T.grid_size(cnt[r], gps)
        assert N >= 16
        T.check_profile(path[r, :cnt[r]], host["grid_x"][r], host["grid_k"][r], N)
        assert (host["grid_x"][r, N:] == 0.0).all() and (host["grid_t"][r, N:] == host["duration"][r]).all()


# --- 4. duration -----------------------------------------------------------------
@pytest.mark.parametrize("gps", [4, 8])
def test_recipe_condition_holds_on_the_reference(gps):
    """No row of Recipe T stalls on the reference and its profile keeps the rows
    at the gridpoints (to HiGHS's tolerance); if this fails the recipe is wrong."""
    worst = max(T.reference_condition(ref) for ref in T.reference_t(gps).values())
    print(f"reference, grid_per_segment {gps}: largest relative constraint violation {worst:.2e}")
    assert worst <= K_TOL


def test_duration_against_the_reference():
    for ref in T.reference_t(8).values():
        T.reference_condition(ref)
    host, ref = T.host_t(8), T.reference_t(8)
    d_ref = np.array([ref[r]["duration"] for r in range(len(ref))])
    worst = (np.abs(host["duration"] - d_ref) / d_ref).max()
    print(f"duration: within {worst:.2e} relative of np_topp")
    assert worst <= DURATION_TOL


def test_duration_converges_with_the_grid():
    """|d16 - d8| < |d8 - d4| on at least 90 % of the walk rows, on the reference first."""
    walk = T.rows_of("walk")
    refs = [T.reference_t(4), T.reference_t(8), T.reference_t(16, "walk")]
    d4, d8, d16 = (np.array([ref[r]["duration"] for r in walk]) for ref in refs)
    assert (np.abs(d16 - d8) < np.abs(d8 - d4)).mean() >= 0.9, "the recipe, not the header"
    h4, h8, h16 = (T.host_t(g)["duration"][walk] for g in (4, 8, 16))
    print("walk row 0: %.2f / %.2f / %.2f s at grid_per_segment 4 / 8 / 16" % (h4[0], h8[0], h16[0]))
    assert (np.abs(h16 - h8) < np.abs(h8 - h4)).mean() >= 0.9


# --- 5. samples ------------------------------------------------------------------
def test_samples():
    path, cnt, _ = T.recipe_t()
    host = T.host_t(8)
    step = 0.1
    end_vel = diff = grad = 0.0
    for r in range(len(cnt)):
        q, N, m, dur = path[r, :cnt[r]], T.grid_size(cnt[r]), host["n_samples"][r], host["duration"][r]
        assert m == int(dur / step) and m >= 2
        t = host["times"][r, :m]
        assert t[0] == 0.0 and abs(t[-1] - dur) <= np.spacing(dur) * m
        pos, vel, acc = (host[k][r, :m] for k in ("position", "velocity", "acceleration"))
        assert np.abs(pos[0] - q[0]).max() <= 1e-9 and np.abs(pos[-1] - q[-1]).max() <= 1e-9
        end_vel = max(end_vel, np.abs(vel[0]).max(), np.abs(vel[-1]).max())
        ts, p, v, a = T.np_samples(q, host["grid_x"][r, :N + 1], host["grid_t"][r, :N + 1], dur, step)
        assert np.array_equal(ts, t)
        diff = max(diff, np.abs(pos - p).max(), np.abs(vel - v).max(), np.abs(acc - a).max())
        grad = max(grad, np.abs(np.gradient(pos, t, axis=0)[1:-1] - vel[1:-1]).max())
        # the slots past the row's samples repeat the last one
        for k in ("position", "velocity", "acceleration", "times"):
            assert (host[k][r, m:] == host[k][r, m - 1]).all()
    print(f"samples: velocity at the ends {end_vel:.2e}; position / velocity / acceleration within {diff:.2e} of "
          f"np_samples; np.gradient(position) within {grad:.2e} of velocity")
    assert end_vel <= 1e-6
    assert diff <= 1e-9
    assert grad <= 10.0  # a sanity check only: of the order of amax * the sampling step


# --- 6. status paths -------------------------------------------------------------
def one(paths, **kw):
    p, c = T.pack(paths, max_waypoints=kw.pop("max_waypoints", 8))
    return T.host_topp(p, c, **kw), p


def test_rows_without_a_path():
    q = np.random.default_rng(6).uniform(T.LIMITS[:, 0], T.LIMITS[:, 1], size=(3, 7))
    out, p = one([q[:1], q[:0], np.tile(q[0], (3, 1)), q])
    assert out["status"].tolist() == [T.NO_PATH, T.NO_PATH, T.ZERO_LENGTH, T.OK]
    for r in range(3):
        assert out["duration"][r] == 0.0 and out["n_samples"][r] == 0
        assert (out["times"][r] == 0.0).all() and (out["position"][r] == p[r, 0]).all()
        assert (out["velocity"][r] == 0.0).all() and (out["acceleration"][r] == 0.0).all()
        assert (out["grid_x"][r] == 0.0).all() and (out["grid_t"][r] == 0.0).all()
    # a count above max_waypoints is clamped, a negative one is no path
    p2, c2 = T.pack([q, q], max_waypoints=3)
    c2[:] = [7, -1]
    out2 = T.host_topp(p2, c2)
    assert out2["status"].tolist() == [T.OK, T.NO_PATH] and out2["duration"][0] == out["duration"][3]


def test_nan_waypoint_stalls_and_returns():
    q = np.random.default_rng(7).uniform(T.LIMITS[:, 0], T.LIMITS[:, 1], size=(5, 7))
    for where in [(2, 3), (0, 0), (4, 6)]:
        bad = q.copy()
        bad[where] = np.nan
        out, _ = one([bad])
        assert out["status"][0] == T.STALLED and out["duration"][0] == 0.0 and out["n_samples"][0] == 0


def test_truncated_row_keeps_its_duration():
    path, cnt, _ = T.recipe_t()
    full = T.host_t(8)
    out = T.host_topp(path[:1], cnt[:1], max_samples=4)
    assert out["status"][0] == (T.OK | T.TRUNCATED) and out["n_samples"][0] == 0
    assert out["duration"][0] == full["duration"][0] and (out["position"][0] == path[0, 0]).all()
    m = int(full["duration"][1] / 0.1)  # exactly enough room: not truncated
    assert T.host_topp(path[1:2], cnt[1:2], max_samples=m)["status"][0] == T.OK
    assert T.host_topp(path[1:2], cnt[1:2], max_samples=m - 1)["status"][0] == (T.OK | T.TRUNCATED)


def test_velocity_cap_where_no_joint_moves():
    """Two waypoints that differ in joint 2 only: the other joints have q' = 0
    at every gridpoint and no velocity bound, and stay put.  A path that turns
    round in one joint has q' = 0 exactly at a gridpoint: x there is bounded
    by the acceleration row alone, which has no u -- the 1e12 cap is the
    velocity bound; K against the LP."""
    a = np.zeros(7)
    b = a.copy()
    b[2] = 0.5
    out, _ = one([[a, b]])
    assert out["status"][0] == T.OK
    m = out["n_samples"][0]
    keep = [0, 1, 3, 4, 5, 6]
    assert (out["position"][0][:, keep] == 0.0).all() and (out["velocity"][0][:, keep] == 0.0).all()
    assert (out["acceleration"][0][:, keep] == 0.0).all()
    T.check_profile(np.array([a, b]), out["grid_x"][0], out["grid_k"][0], 100)
    x = out["grid_x"][0, :101]
    assert np.abs(0.5 * np.sqrt(x)).max() <= T.VMAX[2] * (1 + 1e-12) and m == int(out["duration"][0] / 0.1)
    turn = np.array([a, b, a])
    out, _ = one([turn])
    ref = T.np_topp(turn)
    assert ref["qp"][50, 2] == 0.0 and ref["xmax"][50] == T.X_CAP
    assert out["status"][0] == T.OK and not ref["stalled"]
    assert (np.abs(out["grid_k"][0, 1:100] - ref["K"][1:100]) / ref["K"][1:100]).max() <= K_TOL
    assert abs(out["duration"][0] - ref["duration"]) <= DURATION_TOL * ref["duration"]


# --- 7. argument checks ----------------------------------------------------------
INVALID, UNSUPPORTED = 1, 2


def test_argument_checks():
    v, a = T.VMAX, T.AMAX
    assert T.host_check(7, 96, 40, v, a) == (0, "")
    assert T.host_check(7, 0, 40, v, a) == (0, "")
    assert T.host_check(33, 1, 40, np.ones(33), np.ones(33)) == (UNSUPPORTED, "mpg_topp_batch supports dof <= 32")
    assert T.host_check(32, 1, 40, np.ones(32), np.ones(32))[0] == 0
    assert T.host_check(7, -1, 40, v, a) == (INVALID, "rows < 0")
    for step in (0.0, -0.1, np.nan, np.inf):
        assert T.host_check(7, 1, 40, v, a, step=step) == (INVALID, "step must be > 0")
    for key, lo, hi, msg in (("grid_per_segment", 1, 64, "grid_per_segment outside [1, 64]"),
                             ("min_grid", 2, 65536, "min_grid outside [2, 65536]"),
                             ("max_samples", 1, 65536, "max_samples outside [1, 65536]")):
        for val in (lo, hi):
            assert T.host_check(7, 1, 40, v, a, **{key: val})[0] == 0, (key, val)
        for val in (lo - 1, hi + 1):
            assert T.host_check(7, 1, 40, v, a, **{key: val}) == (INVALID, msg)
    for mw in (1, 4097):
        assert T.host_check(7, 1, mw, v, a) == (INVALID, "max_waypoints outside [2, 4096]")
    assert T.host_check(7, 1, 2, v, a)[0] == 0 and T.host_check(7, 1, 4096, v, a)[0] == 0
    assert T.host_check(7, 1, 40, None, a) == (INVALID, "vel_limits / acc_limits is NULL")
    assert T.host_check(7, 1, 40, v, None) == (INVALID, "vel_limits / acc_limits is NULL")
    for bad in (0.0, -1.0, np.nan, np.inf):
        lim = v.copy()
        lim[4] = bad
        assert T.host_check(7, 1, 40, lim, a) == (INVALID, "vel_limits[4] must be finite and > 0")
        assert T.host_check(7, 1, 40, v, lim) == (INVALID, "acc_limits[4] must be finite and > 0")


def test_size_checks():
    v, a = T.VMAX, T.AMAX
    cap = 1 << 31
    # rows * max_waypoints * dof
    rows = cap // (4096 * 7)
    assert T.host_check(7, rows, 4096, v, a, grid_per_segment=1, min_grid=2, max_samples=1)[0] == 0
    assert T.host_check(7, rows + 1, 4096, v, a, grid_per_segment=1, min_grid=2, max_samples=1) == (
        INVALID, "rows * max_waypoints * dof exceeds 2^31")
    # rows * max_samples * dof
    rows = cap // (65536 * 7)
    assert T.host_check(7, rows, 2, v, a, min_grid=2, max_samples=65536)[0] == 0
    assert T.host_check(7, rows + 1, 2, v, a, min_grid=2, max_samples=65536) == (
        INVALID, "rows * max_samples * dof exceeds 2^31")
    # rows * (Ncap + 1), Ncap = max(min_grid, grid_per_segment * (max_waypoints - 1))
    rows = cap // 65537
    assert T.host_check(7, rows, 2, v, a, min_grid=65536, max_samples=1)[0] == 0
    assert T.host_check(7, rows + 1, 2, v, a, min_grid=65536, max_samples=1) == (INVALID, "rows * (Ncap + 1) exceeds 2^31")
    ncap = 64 * 999
    rows = cap // (ncap + 1)
    assert T.host_check(1, rows, 1000, [1.0], [1.0], grid_per_segment=64, max_samples=1)[0] == 0
    assert T.host_check(1, rows + 1, 1000, [1.0], [1.0], grid_per_segment=64, max_samples=1)[0] == INVALID


def test_host_memory_row_checks():
    v, a = T.VMAX, T.AMAX
    path, cnt = T.pack([np.ones((3, 7)), np.ones((5, 7))], max_waypoints=5)
    assert T.host_check(7, 2, 5, v, a, path=path, count=cnt) == (0, "")
    high = cnt.copy()
    high[1] = 6
    assert T.host_check(7, 2, 5, v, a, path=path, count=high) == (INVALID, "n_waypoints[1] exceeds max_waypoints")
    for bad in (np.nan, np.inf, -np.inf):
        p = path.copy()
        p[0, 3, 2] = bad  # past row 0's count: not looked at
        assert T.host_check(7, 2, 5, v, a, path=p, count=cnt) == (0, "")
        p[0, 2, 2] = bad
        assert T.host_check(7, 2, 5, v, a, path=p, count=cnt) == (INVALID, "non-finite path value in row 0")
    low = cnt.copy()
    low[0] = -3  # no path; nothing of the row is read
    p = path.copy()
    p[0] = np.nan
    assert T.host_check(7, 2, 5, v, a, path=p, count=low) == (0, "")
