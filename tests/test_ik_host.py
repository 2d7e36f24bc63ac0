"""CPU: the IK header the device kernels run (mplib_amd/csrc/mpg_ik.h, compiled
for the host by tests/native/ik_host.cpp) against the host compute_IK_CLIK
(csrc/host/kinjac.cpp), its limit wrap and distance_6D against a numpy
restatement of planner.py:165-191, and mplib_amd.planner.ik's selection logic
on synthetic rows.  No device."""
import ctypes

import numpy as np
import pytest

import ik_cases as K
from mplib_amd import planner as P


def test_one_step_matches_compute_ik_clik():
    """maxIter = 1 on the recipe A rows with sigma_min(J) >= 1e-2.  The two
    codes differ in operation order only (~1e-16 relative); the Cholesky route
    on J J^T amplifies that by kappa(J J^T) <= (sigma_max / sigma_min)^2 ~ 4e4,
    so ~1e-11 is expected and 1e-9 leaves two orders; an indexing or sign
    mistake is at 1e-3 or more.
    Two-run check of the reference on these rows (second run from q0 + 1e-13 N(0, 1)):
    231 of 256 rows have sigma_min >= 1e-2 (smallest sigma_min 4.2e-4); on
    them the reference moved by at most 4.3e-13 against its perturbed self
    (3.9e-11 over all rows); measured here max|dq| = 1.2e-15 (5.4e-14 over all
    rows).  The reference's q is wrapped by check_joint_limit before the
    comparison, as every row of mpg_ik_batch is."""
    _, pose, q0 = K.recipe("A")
    well = K.sigma_min("A") >= 1e-2
    assert well.sum() >= 200
    ref, _, _ = K.wrapped_reference("A", 1)
    q, st, _, it = K.host_header_rows(pose, q0, max_iter=1)
    d = np.abs(q - ref).max(axis=1)
    print("one step: rows", int(well.sum()), "max|dq|", d[well].max(), "all rows", d.max())
    assert (it <= 1).all()
    assert d[well].max() <= 1e-9


def test_full_run_matches_compute_ik_clik():
    """Recipe A, default options: every row converges in both codes and
    max|dq| <= 1e-6 with at most 2 of the 256 rows over (rows whose iteration
    counts differ by one at the eps crossing, worth ~dt eps / sigma).
    Two-run check of the reference on these rows: 256 / 256 converge in both
    runs, no status differs, final max|dq| median 6.3e-14, max 1.3e-5, 1 row
    above 1e-6.  Measured here: max|dq| = 2.7e-7, 0 rows over, 90 to 111
    iterations per row."""
    _, pose, q0 = K.recipe("A")
    ref, ok, ref_err = K.wrapped_reference("A")
    q, st, err, it = K.host_header_rows(pose, q0)
    assert ok.all()
    assert ((st & P.IK_CONVERGED) != 0).all() and ((st & P.IK_SINGULAR) == 0).all()
    d = np.abs(q - ref).max(axis=1)
    print("full run: max|dq|", d.max(), "rows over 1e-6:", int((d > 1e-6).sum()), "iters", it.min(), it.max())
    assert (d > 1e-6).sum() <= 2
    assert np.abs(err - ref_err).max() <= 1e-9
    # the answer reaches its goal (independent of both solvers): the error is
    # measured in the parent joint's frame, the hand frame sits < 0.25 m from it
    dp, dR = K.fk_residual(q)
    assert dp.max() <= 2 * K.EPS and dR.max() <= 2 * K.EPS


def _wrap_table():
    lo, hi = -2.8973, 2.8973
    rev = [lo, lo + 9e-4, lo - 9e-4, lo - K.TWO_PI + 0.5, hi + 9e-4, hi + 2e-3, hi + K.TWO_PI - 0.5, 0.3, lo + 5 * K.TWO_PI]
    pri = [0.0, 0.04, -9e-4, -2e-3, 0.04 + 9e-4, 0.04 + 2e-3, 0.02, 0.5, -0.5]
    con = [0.0, 3.0, -3.0, 7.0, -7.0, 100.0, 1e-4, np.pi, -np.pi]
    q = np.stack([rev, pri, con], axis=1)
    return q, np.array([lo, 0.0, -np.inf]), np.array([hi, 0.04, np.inf]), np.array([True, False, True])


def test_limit_wrap_matches_numpy():
    """check_joint_limit on a hand-made table: a revolute joint at lo, lo +-
    9e-4, lo - 2 pi + 0.5, hi + 9e-4, hi + 2e-3, hi + 2 pi - 0.5; a prismatic
    joint inside, at and beyond both tolerances; a continuous joint (infinite
    limits: never fails, not wrapped).  Bits exact; values within 4 ulp (IEEE
    +, -, x, / and floor in one order) -- they come out bitwise equal, which
    the last assertion records."""
    q, lo, hi, rev = _wrap_table()
    want, want_fail = K.np_check_joint_limit(q, lo, hi, rev)
    got = np.ascontiguousarray(q.copy())
    fail = np.zeros(q.shape, np.uint8)
    kind = np.where(rev, 1, 2).astype(np.uint8)
    P_ = ctypes.c_void_p
    K.host_lib().ik_host_wrap(3, lo.ctypes.data_as(P_), hi.ctypes.data_as(P_), kind.ctypes.data_as(P_),
                              got.ctypes.data_as(P_), ctypes.c_long(len(q)), fail.ctypes.data_as(P_))
    np.testing.assert_array_equal(fail.astype(bool), want_fail)
    assert want_fail[:8, 0].tolist() == [False, False, False, False, False, True, False, False]
    assert want_fail[:, 1].tolist() == [False, False, False, True, False, True, False, True, True]
    assert not want_fail[:, 2].any() and (got[:, 2] == q[:, 2]).all()
    assert K.ulp_diff(got, want).max() <= 4
    np.testing.assert_array_equal(got, want)  # bitwise equal


def test_distance_6d_matches_numpy():
    rng = np.random.default_rng(5)
    f = K.host_lib().ik_host_distance_6d
    P_ = ctypes.c_void_p
    for _ in range(200):
        a, b = rng.normal(size=7), rng.normal(size=7)
        a[3:] /= np.linalg.norm(a[3:])
        b[3:] /= np.linalg.norm(b[3:])
        if rng.random() < 0.5:
            b[3:] = -a[3:] + 1e-4 * rng.normal(size=4)  # the q1 + q2 branch
        want = K.np_distance_6d(a, b)
        got = f(a.ctypes.data_as(P_), b.ctypes.data_as(P_))
        assert abs(got - want) <= 4 * np.spacing(want)
        assert abs(P.distance_6d(a[:3], a[3:], b[:3], b[3:]) - want) <= 4 * np.spacing(want)


# --- mplib_amd.planner.ik's selection logic, no device ---------------------------
V = P.IK_VALID


def test_select_ik_dedup_in_seed_order():
    start = np.zeros(3)
    q = np.array([[0.0, 0.0, 0.0], [0.05, 0.0, 0.0], [0.2, 0.0, 0.0], [0.25, 0.0, 0.0], [0.0, 0.0, 0.0],
                  [0.0, 1.0, 0.0]])
    status = np.array([V, V, V, V, V & ~P.IK_COLLISION_FREE, V], np.uint8)
    s, goals = P.select_ik(q, status, start)
    assert s == "Success"
    # row 1 is within 0.1 of row 0, row 3 within 0.1 of row 2, row 4 is in collision
    np.testing.assert_array_equal(np.asarray(goals), q[[0, 2, 5]])
    # exactly 0.1 apart is kept (the reference drops on < 0.1)
    q2 = np.array([[0.0, 0.0, 0.0], [0.1, 0.0, 0.0]])
    assert len(P.select_ik(q2, np.array([V, V]), start)[1]) == 2


def test_select_ik_failure_strings():
    q = np.zeros((3, 2))
    none = np.array([0, P.IK_CONVERGED, P.IK_CONVERGED | P.IK_IN_LIMITS], np.uint8)
    assert P.select_ik(q, none, np.zeros(2)) == ("IK Failed! Cannot find valid solution.", None)
    far = np.array([0, V & ~P.IK_WITHIN_THRESHOLD, V & ~P.IK_WITHIN_THRESHOLD], np.uint8)
    s, goals = P.select_ik(q, far, np.zeros(2), threshold=1e-3, distance=lambda r: [9.0, 0.5, 0.25][r])
    assert goals is None
    threshold = 1e-3
    assert s == f"IK Failed! Distance 0.25 is greater than {threshold=}."


def test_select_ik_return_closest_uses_the_2pi_equivalent():
    """planner.py:337-355: joint 0 has a range above 2 pi, so q + 2 pi is the
    same pose; it is taken when it is below the upper limit and nearer to the
    start.  Joint 1's range is below 2 pi: never shifted."""
    upper = np.array([6.5, 2.0])
    equiv = np.array([True, False])
    start = np.array([3.0, 0.0])
    q = np.array([[-3.2, 0.1], [1.0, 1.5]])
    s, best = P.select_ik(q, np.array([V, V]), start, return_closest=True, equiv_mask=equiv, upper=upper)
    assert s == "Success"
    np.testing.assert_allclose(best, [-3.2 + 2 * np.pi, 0.1])  # 3.083: nearer than row 1
    # beyond the upper limit the shift is not allowed: row 1 wins
    s, best = P.select_ik(q, np.array([V, V]), start, return_closest=True, equiv_mask=equiv, upper=np.array([3.0, 2.0]))
    np.testing.assert_array_equal(best, q[1])
