"""Shared inputs and references of the IK tests (test_ik_host.py, test_ik_batch.py).

Recipe A, "near" rows: Panda, link panda_hand, q_goal uniform in 0.8 x the
limits, the goal pose the CPU oracle's FK of q_goal, q0 = clip(q_goal +
N(0, 0.2), limits), one goal per row.  Recipe B, "uniform" rows: the same
goals, q0 uniform in the limits.  Everything is computed once per process and
handed out read-only.
"""
import ctypes
import functools
import os
import subprocess
import tempfile

import numpy as np

import worlds as Wd

HAND = 8  # user link index of panda_hand
N_ROWS = 256
EPS = 1e-5
TWO_PI = 2 * np.pi

_HERE = os.path.dirname(os.path.abspath(__file__))


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def oracle_world():
    return Wd.oracle_world(2)


@functools.lru_cache(maxsize=None)
def limits():
    return _ro(np.array(oracle_world().art.joint_limits()[:7], np.float64))[0]


def hand_fk(q7):
    """(pose [n, 7] (p, wxyz), R [n, 3, 3], p [n, 3]) of panda_hand by the CPU oracle."""
    po, objT = oracle_world().fk_batch(np.asarray(q7, np.float64).reshape(-1, 7))
    T = np.asarray(objT)[:, HAND]
    return np.asarray(po)[:, HAND].copy(), T[:, :9].reshape(-1, 3, 3).copy(), T[:, 9:].copy()


@functools.lru_cache(maxsize=None)
def recipe(kind, n=N_ROWS, seed=2024):
    """(q_goal [n, 7], goal_pose [n, 7], q0 [n, 7]); kind 'A' or 'B' (the same goals)."""
    lim = limits()
    rng = np.random.default_rng(seed)
    q_goal = rng.uniform(0.8 * lim[:, 0], 0.8 * lim[:, 1], size=(n, 7))
    near = np.clip(q_goal + rng.normal(scale=0.2, size=(n, 7)), lim[:, 0], lim[:, 1])
    uniform = rng.uniform(lim[:, 0], lim[:, 1], size=(n, 7))
    pose, _, _ = hand_fk(q_goal)
    return _ro(q_goal, pose, near if kind == "A" else uniform)


@functools.lru_cache(maxsize=None)
def pin_model():
    from mplib_amd import scenes
    return scenes.panda().get_pinocchio_model()


def _full(q7):
    return list(np.asarray(q7, np.float64)) + [0.0, 0.0]


def host_clik(pose, q0, max_iter=1000, mask=None, **kw):
    """compute_IK_CLIK (csrc/host/kinjac.cpp) row by row: (q [n, 7], success [n], err [n, 6])."""
    pin = pin_model()
    n = len(q0)
    q, ok, err = np.zeros((n, 7)), np.zeros(n, bool), np.zeros((n, 6))
    m = [] if mask is None else [bool(x) for x in mask] + [False, False]
    for i in range(n):
        qi, s, e = pin.compute_IK_CLIK(HAND, list(pose[i]), _full(q0[i]), m, maxIter=int(max_iter), **kw)
        q[i], ok[i], err[i] = np.asarray(qi)[:7], s, e
    return q, ok, err


@functools.lru_cache(maxsize=None)
def host_reference(kind, max_iter=1000):
    _, pose, q0 = recipe(kind)
    return _ro(*host_clik(pose, q0, max_iter))


@functools.lru_cache(maxsize=None)
def wrapped_reference(kind, max_iter=1000):
    """host_reference with check_joint_limit's wrap applied to q, as step 2 of
    mpg_ik_batch applies it to every row (compute_IK_CLIK itself does not wrap;
    Planner.IK wraps its answer next)."""
    q, ok, err = host_reference(kind, max_iter)
    lim = limits()
    return _ro(np_check_joint_limit(q, lim[:, 0], lim[:, 1], np.ones(7, bool))[0], ok, err)


@functools.lru_cache(maxsize=None)
def sigma_min(kind):
    """Smallest singular value of the hand's LOCAL Jacobian at each start q0."""
    pin = pin_model()
    _, _, q0 = recipe(kind)
    out = np.zeros(len(q0))
    for i, q in enumerate(q0):
        pin.compute_full_jacobian(_full(q))
        out[i] = np.linalg.svd(np.asarray(pin.get_link_jacobian(HAND, True))[:, :7], compute_uv=False).min()
    return _ro(out)[0]


def fk_residual(q, goal_q=None, kind="A", rows=None):
    """(|dp| [n], max|dR| [n]) between the CPU FK of q and the goals of the
    recipe's rows (rows: their indices, default the first len(q))."""
    q_goal = recipe(kind)[0] if goal_q is None else goal_q
    rows = np.arange(len(q)) if rows is None else np.asarray(rows)
    _, Rg, pg = hand_fk(q_goal[rows])
    _, R, p = hand_fk(q)
    return np.linalg.norm(p - pg, axis=1), np.abs(R - Rg).reshape(len(q), -1).max(axis=1)


# --- numpy restatement of planner.py:165-191 --------------------------------
def np_check_joint_limit(q, lo, hi, revolute):
    """check_joint_limit applied fully: (wrapped q, fail per joint).  A joint
    whose limits are not finite never fails and is not wrapped."""
    q = np.array(q, np.float64)
    fail = np.zeros(q.shape, bool)
    for d in range(q.shape[-1]):
        if not (np.isfinite(lo[d]) and np.isfinite(hi[d])):
            continue
        for i in range(len(q)):
            v = q[i, d]
            if revolute[d]:
                if np.abs(v - lo[d]) < 1e-3:
                    continue
                v -= 2 * np.pi * np.floor((v - lo[d]) / (2 * np.pi))
                q[i, d] = v
                fail[i, d] = v > hi[d] + 1e-3
            else:
                fail[i, d] = v < lo[d] - 1e-3 or v > hi[d] + 1e-3
    return q, fail


def np_distance_6d(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.linalg.norm(a[:3] - b[:3]) + min(np.linalg.norm(a[3:] - b[3:]), np.linalg.norm(a[3:] + b[3:]))


def ulp_diff(a, b):
    """|a - b| in units of the spacing at max(|a|, |b|)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b) / np.spacing(np.maximum(np.abs(a), np.abs(b)))


# --- mpg_ik.h compiled for the host (tests/native/ik_host.cpp) ---------------
_lib = None


def host_lib():
    """Build tests/native/ik_host.cpp into a per-process file and load it."""
    global _lib
    if _lib is None:
        out = os.path.join(tempfile.gettempdir(), "mplib_amd_ik_host_%d_%d.so" % (os.getuid(), os.getpid()))
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", out,
                               os.path.join(_HERE, "native", "ik_host.cpp")])
        _lib = ctypes.CDLL(out)
        _lib.ik_host_distance_6d.restype = ctypes.c_double
    return _lib


def host_header_rows(pose, q0, max_iter=1000, mask=None, eps=EPS, dt=0.1, damp=1e-12, threshold=1e-3, desc=None,
                     link=HAND):
    """mpg_ik.h's row on the host: (q [n, dof], status [n], err [n, 6], iters [n])."""
    d = Wd.desc_arrays(oracle_world()) if desc is None else desc
    keep = []

    def arr(a, dt_):
        a = np.ascontiguousarray(np.asarray(a, dtype=dt_))
        keep.append(a)
        return a.ctypes.data_as(ctypes.c_void_p)

    dof = int(d["dof"])
    src = np.asarray(d["joint_q_source"])
    lo, hi, kind = np.full(dof, -np.inf), np.full(dof, np.inf), np.zeros(dof, np.uint8)
    for j, s in enumerate(src):
        if s >= 0:
            lo[s], hi[s] = d["joint_lower"][j], d["joint_upper"][j]
            t = int(d["joint_type"][j])
            kind[s] = 1 if (t <= 3 or t >= 8) else 2
    n = len(q0)
    q = np.zeros((n, dof))
    st = np.zeros(n, np.uint8)
    err = np.zeros((n, 6))
    it = np.zeros(n, np.int32)
    mk = None if mask is None else arr(mask, np.uint8)
    rc = host_lib().ik_host_rows(
        len(d["joint_type"]), arr(d["joint_type"], np.int32), arr(d["joint_parent"], np.int32),
        arr(d["joint_q_source"], np.int32), arr(d["joint_q_const"], np.float64), arr(d["joint_axis"], np.float64),
        arr(d["joint_placement"], np.float64), dof, len(d["link_parent"]), arr(d["link_parent"], np.int32),
        arr(d["link_placement"], np.float64), int(link), arr(lo, np.float64), arr(hi, np.float64), arr(kind, np.uint8),
        mk, arr(pose, np.float64), arr(q0, np.float64), ctypes.c_long(n), ctypes.c_double(eps), int(max_iter),
        ctypes.c_double(dt), ctypes.c_double(damp), ctypes.c_double(threshold), q.ctypes.data_as(ctypes.c_void_p),
        st.ctypes.data_as(ctypes.c_void_p), err.ctypes.data_as(ctypes.c_void_p), it.ctypes.data_as(ctypes.c_void_p))
    assert rc == 0
    return q, st, err, it
