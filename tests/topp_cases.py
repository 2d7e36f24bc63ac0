"""Shared inputs and references of the time-parametrisation tests
(test_topp_host.py, test_topp_batch.py).

np_topp is a numpy restatement of mpg_topp_batch's algorithm (include/mpgpu.h,
DESIGN.md section 14) that shares no step with mplib_amd/csrc/mpg_topp.h: the
spline is scipy.interpolate.CubicSpline, every controllable set K_k is the
optimum of the two-variable linear program (scipy.optimize.linprog, HiGHS) --
no Fourier-Motzkin elimination -- and the forward pass takes each row's bound on
u as it stands, without normalising its sign.

Recipe T: the Panda's seven arm joints, vmax / amax below; for each seed 0..23
np.random.default_rng(seed) draws, in this order, "unif" (17 waypoints uniform
in the joint limits), "walk" (40 waypoints, the cumulative sum of normal(0,
0.05)), "two" and "three" (2 and 3 waypoints uniform in the limits): 96 rows,
max_waypoints 40.  Everything is computed once per process and handed out
read-only.
"""
import ctypes
import functools
import os
import subprocess
import tempfile

import numpy as np
from scipy.interpolate import CubicSpline
from scipy.optimize import linprog

OK, NO_PATH, ZERO_LENGTH, STALLED, TRUNCATED = 1, 2, 4, 8, 16
X_CAP = 1e12
# data/panda/panda.urdf, panda_joint1 .. 7
LIMITS = np.array([[-2.8973, 2.8973], [-1.7628, 1.7628], [-2.8973, 2.8973], [-3.0718, -0.0698], [-2.8973, 2.8973],
                   [-0.0175, 3.7525], [-2.8973, 2.8973]])
VMAX = np.array([2.175, 2.175, 2.175, 2.175, 2.61, 2.61, 2.61])
AMAX = np.array([15.0, 7.5, 10.0, 12.5, 15.0, 20.0, 20.0])
FAMILIES = ("unif", "walk", "two", "three")
SEEDS = 24
MAX_WAYPOINTS = 40

_HERE = os.path.dirname(os.path.abspath(__file__))


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def recipe_t():
    """(path [96, 40, 7] padded with each row's last waypoint, count [96] i32,
    family [96] of FAMILIES' indices); row 4 * seed + family."""
    paths = []
    for seed in range(SEEDS):
        rng = np.random.default_rng(seed)
        paths.append(rng.uniform(LIMITS[:, 0], LIMITS[:, 1], size=(17, 7)))
        paths.append(np.cumsum(rng.normal(0.0, 0.05, size=(40, 7)), axis=0))
        paths.append(rng.uniform(LIMITS[:, 0], LIMITS[:, 1], size=(2, 7)))
        paths.append(rng.uniform(LIMITS[:, 0], LIMITS[:, 1], size=(3, 7)))
    return _ro(*pack(paths), np.tile(np.arange(4), SEEDS))


def pack(paths, max_waypoints=MAX_WAYPOINTS):
    """(path [rows, max_waypoints, dof], count [rows]): the layout mpg_screw_batch / mpg_plan_batch write."""
    dof = np.asarray(paths[0]).shape[1]
    out = np.zeros((len(paths), max_waypoints, dof))
    cnt = np.zeros(len(paths), np.int32)
    for r, p in enumerate(paths):
        p = np.asarray(p, np.float64)
        cnt[r] = len(p)
        out[r, :len(p)] = p
        out[r, len(p):] = p[-1] if len(p) else 0.0
    return out, cnt


def rows_of(family):
    return np.flatnonzero(recipe_t()[2] == FAMILIES.index(family))


def grid_size(n, grid_per_segment=8, min_grid=100):
    return max(min_grid, grid_per_segment * (n - 1))


# --- the numpy restatement ----------------------------------------------------
def np_spline(q):
    """CubicSpline through q [n, dof] at linspace(0, 1, n): not-a-knot, scipy's default."""
    q = np.asarray(q, np.float64)
    return CubicSpline(np.linspace(0.0, 1.0, len(q)), q, axis=0)


def np_rows(qp, qpp, k, delta, K_next, amax):
    """Interval k's rows lo <= cu u + cx x <= hi as (cu, cx, lo, hi) arrays: the
    acceleration at k, at k + 1 of the state x + 2 delta u, the continuation."""
    cu = np.concatenate([qp[k], qp[k + 1] + 2 * delta * qpp[k + 1], [2 * delta]])
    cx = np.concatenate([qpp[k], qpp[k + 1], [1.0]])
    lo = np.concatenate([-amax, -amax, [0.0]])
    hi = np.concatenate([amax, amax, [K_next]])
    return cu, cx, lo, hi


def np_xmax(qp, vmax):
    with np.errstate(divide="ignore", invalid="ignore"):
        b = np.where(qp != 0.0, (vmax / qp) ** 2, np.inf)
    return np.minimum(b.min(axis=1), X_CAP)


def lp_controllable(cu, cx, lo, hi, xmax):
    """max x over 0 <= x <= xmax, u free, lo <= cu u + cx x <= hi (HiGHS)."""
    A = np.column_stack([cx, cu])
    res = linprog([-1.0, 0.0], A_ub=np.vstack([A, -A]), b_ub=np.concatenate([hi, -lo]),
                  bounds=[(0.0, xmax), (None, None)], method="highs")
    assert res.status == 0, res.message
    return max(float(res.x[0]), 0.0)


def np_forward(qp, qpp, K, amax, N):
    delta = 1.0 / N
    x = np.zeros(N + 1)
    for k in range(N):
        cu, cx, lo, hi = np_rows(qp, qpp, k, delta, K[k + 1], amax)
        with np.errstate(divide="ignore", invalid="ignore"):
            ub = np.where(cu > 0, (hi - cx * x[k]) / cu, np.where(cu < 0, (lo - cx * x[k]) / cu, np.inf))
        x[k + 1] = min(max(x[k] + 2 * delta * ub.min(), 0.0), K[k + 1])
    return x


def np_times(x, N):
    r = np.sqrt(x)
    with np.errstate(divide="ignore"):
        return np.concatenate([[0.0], np.cumsum(2.0 / N / (r[:-1] + r[1:]))])


def np_samples(q, x, t, duration, step, max_samples=None):
    """Step 7 on a given profile: (times [m], position, velocity, acceleration [m, dof])."""
    cs = np_spline(q)
    N = len(x) - 1
    m = int(duration / step)
    ts = np.array([i * duration / (m - 1) for i in range(m)]) if m > 1 else np.zeros(m)
    k = np.clip(np.searchsorted(t[:N], ts, side="right") - 1, 0, N - 1)
    tau = ts - t[k]
    udd = (x[k + 1] - x[k]) * N / 2.0
    sd = np.sqrt(x[k]) + udd * tau
    s = np.clip(k / N + np.sqrt(x[k]) * tau + 0.5 * udd * tau ** 2, k / N, (k + 1) / N)
    p1, p2 = cs(s, 1), cs(s, 2)
    return ts, cs(s), p1 * sd[:, None], p1 * udd[:, None] + p2 * (sd ** 2)[:, None]


def np_topp(q, vmax=VMAX, amax=AMAX, step=0.1, grid_per_segment=8, min_grid=100):
    """The whole algorithm on one path q [n, dof], n >= 2: a dictionary of N,
    qp / qpp [N + 1, dof], xmax, K, x, t [N + 1], duration, stalled and the
    samples (times, position, velocity, acceleration)."""
    q = np.asarray(q, np.float64)
    n = len(q)
    N = grid_size(n, grid_per_segment, min_grid)
    cs = np_spline(q)
    sg = np.arange(N + 1) / N
    qp, qpp = cs(sg, 1), cs(sg, 2)
    xmax = np_xmax(qp, vmax)
    K = np.zeros(N + 1)
    for k in range(N - 1, -1, -1):
        K[k] = lp_controllable(*np_rows(qp, qpp, k, 1.0 / N, K[k + 1], amax), xmax[k])
    x = np_forward(qp, qpp, K, amax, N)
    t = np_times(x, N)
    out = dict(N=N, qp=qp, qpp=qpp, xmax=xmax, K=K, x=x, t=t, duration=t[-1],
               stalled=bool(((x[:-1] == 0) & (x[1:] == 0)).any() or not np.isfinite(t[-1])))
    if not out["stalled"]:
        out["times"], out["position"], out["velocity"], out["acceleration"] = np_samples(q, x, t, t[-1], step)
    return out


@functools.lru_cache(maxsize=None)
def reference_t(grid_per_segment=8, family=None):
    """np_topp over Recipe T (one family's rows, or all): {row: its dictionary}."""
    path, cnt, _ = recipe_t()
    rows = range(len(cnt)) if family is None else rows_of(family)
    return {int(r): np_topp(path[r, :cnt[r]], grid_per_segment=grid_per_segment) for r in rows}


def reference_condition(ref):
    """Recipe T's condition on one np_topp result: no stall (interior x >= 1e-9
    max K, a finite duration); returns the largest violation of the rows at
    the gridpoints by the profile's own u."""
    N, x, K = ref["N"], ref["x"], ref["K"]
    assert not ref["stalled"] and np.isfinite(ref["duration"])
    assert (x[1:N] >= 1e-9 * K.max()).all()
    return profile_violation(ref["qp"], ref["qpp"], x, N)


def profile_violation(qp, qpp, x, N, vmax=VMAX, amax=AMAX):
    """max over the gridpoints of (|q'| sqrt x - vmax) / vmax and, with u =
    (x_{k+1} - x_k) / (2 delta), of (|row| - amax) / amax for both acceleration rows."""
    u = (x[1:] - x[:-1]) * N / 2.0
    a0 = qp[:-1] * u[:, None] + qpp[:-1] * x[:-1, None]
    a1 = (qp[1:] + 2.0 / N * qpp[1:]) * u[:, None] + qpp[1:] * x[:-1, None]
    vel = np.abs(qp) * np.sqrt(x)[:, None]
    return max(((np.abs(a0) - amax) / amax).max(), ((np.abs(a1) - amax) / amax).max(), ((vel - vmax) / vmax).max())


def check_profile(q, grid_x, grid_k, N, vmax=VMAX, amax=AMAX):
    """Test 3 on one row's profile x (and controllable sets K, or None): bounds,
    ends, the limits at the gridpoints, greediness.  Derivatives from CubicSpline."""
    cs = np_spline(q)
    sg = np.arange(N + 1) / N
    qp, qpp = cs(sg, 1), cs(sg, 2)
    x = grid_x[:N + 1]
    assert x[0] == 0.0 and x[N] == 0.0 and (x >= 0).all()
    assert (np.abs(qp) * np.sqrt(x)[:, None] <= vmax * (1 + 1e-12)).all()
    u = (x[1:] - x[:-1]) * N / 2.0
    a0 = qp[:-1] * u[:, None] + qpp[:-1] * x[:-1, None]
    a1 = (qp[1:] + 2.0 / N * qpp[1:]) * u[:, None] + qpp[1:] * x[:-1, None]
    assert (np.abs(a0) <= amax * (1 + 1e-9)).all() and (np.abs(a1) <= amax * (1 + 1e-9)).all()
    if grid_k is None:
        return
    K = grid_k[:N + 1]
    assert (x <= K).all()
    at_k = x[1:] == K[1:]
    active = (np.abs(np.abs(a0) - amax) <= 1e-9 * amax).any(axis=1) | (np.abs(np.abs(a1) - amax) <= 1e-9 * amax).any(axis=1)
    clamped = x[1:] == 0.0
    assert (at_k | active | clamped).all(), np.flatnonzero(~(at_k | active | clamped))


# --- mpg_topp.h compiled for the host (tests/native/topp_host.cpp) ------------
_lib = None


def host_lib():
    """Build tests/native/topp_host.cpp into a per-process file and load it."""
    global _lib
    if _lib is None:
        out = os.path.join(tempfile.gettempdir(), "mplib_amd_topp_host_%d_%d.so" % (os.getuid(), os.getpid()))
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", out,
                               os.path.join(_HERE, "native", "topp_host.cpp")])
        _lib = ctypes.CDLL(out)
    return _lib


_P = ctypes.c_void_p


def _ptr(a):
    return _P(a.ctypes.data if a is not None else 0)


def host_spline(q):
    """topp_spline's moments M [n, dof]."""
    q = np.ascontiguousarray(q, dtype=np.float64)
    M = np.zeros_like(q)
    host_lib().topp_host_spline(_ptr(q), q.shape[0], q.shape[1], _ptr(M))
    return M


def host_spline_eval(q, M, s):
    """topp_spline_eval at s [ns]: (value, first, second derivative) [ns, dof]."""
    q = np.ascontiguousarray(q, dtype=np.float64)
    s = np.ascontiguousarray(s, dtype=np.float64)
    out = [np.zeros((len(s), q.shape[1])) for _ in range(3)]
    host_lib().topp_host_spline_eval(_ptr(q), _ptr(np.ascontiguousarray(M)), q.shape[0], q.shape[1], _ptr(s), len(s),
                                     *(_ptr(o) for o in out))
    return out


def result_arrays(rows, dof, max_samples, ncap):
    return dict(times=np.zeros((rows, max_samples)), position=np.zeros((rows, max_samples, dof)),
                velocity=np.zeros((rows, max_samples, dof)), acceleration=np.zeros((rows, max_samples, dof)),
                n_samples=np.zeros(rows, np.int32), duration=np.zeros(rows), status=np.zeros(rows, np.uint8),
                grid_x=np.zeros((rows, ncap + 1)), grid_t=np.zeros((rows, ncap + 1)))


def host_topp(path, count, vmax=VMAX, amax=AMAX, step=0.1, grid_per_segment=8, min_grid=100, max_samples=256):
    """mpg_topp.h's rows on the host: mpg_topp_batch's outputs as a dictionary, and grid_k."""
    path = np.ascontiguousarray(path, dtype=np.float64)
    count = np.ascontiguousarray(count, dtype=np.int32)
    rows, mw, dof = path.shape
    ncap = grid_size(mw, grid_per_segment, min_grid)
    out = result_arrays(rows, dof, max_samples, ncap)
    out["grid_k"] = np.zeros((rows, ncap + 1))
    vmax, amax = (np.ascontiguousarray(a, dtype=np.float64) for a in (vmax, amax))
    rc = host_lib().topp_host_rows(
        _ptr(path), _ptr(count), ctypes.c_long(rows), int(mw), int(dof), _ptr(vmax), _ptr(amax), ctypes.c_double(step),
        int(grid_per_segment), int(min_grid), int(max_samples), _ptr(out["times"]), _ptr(out["position"]),
        _ptr(out["velocity"]), _ptr(out["acceleration"]), _ptr(out["n_samples"]), _ptr(out["duration"]),
        _ptr(out["status"]), _ptr(out["grid_x"]), _ptr(out["grid_t"]), _ptr(out["grid_k"]))
    assert rc == 0
    return out


T_SAMPLES = 512  # room for Recipe T's longest row (31.8 s at step 0.1): no row is truncated


@functools.lru_cache(maxsize=None)
def host_t(grid_per_segment=8, max_samples=T_SAMPLES):
    """host_topp over Recipe T, read-only."""
    path, cnt, _ = recipe_t()
    out = host_topp(path, cnt, grid_per_segment=grid_per_segment, max_samples=max_samples)
    _ro(*out.values())
    return out


def host_check(dof, rows, max_waypoints, vel, acc, step=0.1, grid_per_segment=8, min_grid=100, max_samples=256,
               path=None, count=None):
    """mpg_topp_batch's argument checks: (return code, message)."""
    buf = ctypes.create_string_buffer(256)
    arr = lambda a, t: None if a is None else np.ascontiguousarray(a, dtype=t)  # noqa: E731
    vel, acc, path = arr(vel, np.float64), arr(acc, np.float64), arr(path, np.float64)
    count = arr(count, np.int32)
    rc = host_lib().topp_host_check(int(dof), ctypes.c_long(rows), int(max_waypoints), _ptr(vel), _ptr(acc),
                                    ctypes.c_double(step), int(grid_per_segment), int(min_grid), int(max_samples),
                                    _ptr(path), _ptr(count), buf, len(buf))
    return rc, buf.value.decode()
