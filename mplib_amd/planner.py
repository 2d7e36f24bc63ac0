"""Batched callers of the validity checker from MPlib's Python facade
(reference mplib/planner.py).

``generate_collision_pair`` is ``Planner.generate_collision_pair``
(planner.py:118-163) with its 10^6-iteration Python loop replaced by one
device call: the random full configurations (fingers included, as
``set_qpos(qpos, True)`` sets them) are drawn on the GPU, evaluated like
``collide_full()`` and counted per link pair on the device
(``PlanningWorld.sample_pair_counts``, C ABI ``mpg_collide_count``).  The
pairs that collide in every sample are written as ``disable_collisions``
entries of an SRDF, in the reference's format.

Sampling: each joint value is uniform in the joint's limits (pinocchio
``randomConfiguration``'s distribution; continuous joints over [-pi, pi]),
drawn by a counter-based generator (splitmix64 of seed and value index,
``sample_uniform`` below restates it) rather than ``std::rand``, so a batch
is reproducible and shardable; the statistic the SRDF rests on (a pair that
collides in every sample) does not depend on the stream.
"""
from __future__ import annotations

import os
import xml.etree.ElementTree as ET
from typing import List, Optional, Sequence, Tuple
from xml.dom import minidom

import numpy as np

_GOLDEN = np.uint64(0x9E3779B97F4A7C15)
_M1 = np.uint64(0xBF58476D1CE4E5B9)
_M2 = np.uint64(0x94D049BB133111EB)


def sample_uniform(lower: Sequence[float], upper: Sequence[float], n: int, seed: int, offset: int = 0) -> np.ndarray:
    """The device sampler (mpg_sample_uniform) on the host: value i of the
    batch (row-major, i = row * dof + k, counted from ``offset`` rows) is
    lower[k] + (upper[k] - lower[k]) * u, u = splitmix64(seed + (i + 1) *
    golden) >> 11 scaled by 2^-53."""
    lo = np.asarray(lower, np.float64)
    hi = np.asarray(upper, np.float64)
    dof = lo.size
    i = np.arange(offset * dof, (offset + n) * dof, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = np.uint64(seed) + (i + np.uint64(1)) * _GOLDEN
        z = (z ^ (z >> np.uint64(30))) * _M1
        z = (z ^ (z >> np.uint64(27))) * _M2
        z = z ^ (z >> np.uint64(31))
    u = (z >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)
    return (lo + (hi - lo) * u.reshape(n, dof)).reshape(n, dof)


def collision_pair_counts(world, sample_time: int = 1000000, seed: int = 0) -> List[Tuple[str, str, int]]:
    """(link_name1, link_name2, count) per pair of the world's collide_full()
    table: in how many of ``sample_time`` random full configurations of the
    planned articulations the pair is reported."""
    counts = world.sample_pair_counts(int(sample_time), int(seed))
    info = world.get_collision_pair_info()
    return [(i[3], i[4], int(c)) for i, c in zip(info, counts)]


def generate_collision_pair(world, link_names: Sequence[str], urdf_path: str, sample_time: int = 1000000,
                            seed: int = 0, srdf_path: Optional[str] = None, verbose: bool = True) -> str:
    """Planner.generate_collision_pair (planner.py:118-163): count, per
    (link1, link2) of ``link_names`` (the planner's user links), the samples in
    which collide_full() reports the pair, and write every pair whose count is
    ``sample_time`` as ``<disable_collisions link1 link2 reason="Default"/>``
    to ``srdf_path`` (default: the URDF path with .srdf).  Returns the path."""
    idx = {n: i for i, n in enumerate(link_names)}
    cnt = np.zeros((len(link_names), len(link_names)), dtype=np.int64)
    for l1, l2, c in collision_pair_counts(world, sample_time, seed):
        if l1 in idx and l2 in idx:
            cnt[idx[l1]][idx[l2]] += c
    root = ET.Element("robot")
    root.set("name", urdf_path.split("/")[-1].split(".")[0])
    srdf = srdf_path or urdf_path.replace(".urdf", ".srdf")
    for i in range(len(link_names)):
        for j in range(len(link_names)):
            if cnt[i][j] == sample_time:
                if verbose:
                    print("Ignore collision pair: (%s, %s), reason:  always collide" % (link_names[i], link_names[j]))
                c = ET.SubElement(root, "disable_collisions")
                c.set("link1", link_names[i])
                c.set("link2", link_names[j])
                c.set("reason", "Default")
    with open(srdf, "w") as f:
        f.write(minidom.parseString(ET.tostring(root)).toprettyxml(indent="    "))
    if verbose:
        print("Saving the SRDF file to %s" % srdf)
    return srdf


# ---------------------------------------------------------------------------
# Planner.IK (planner.py:256-356): the n_init_qpos CLIK runs, their limit /
# collision / distance_6D filter and the selection of the answers, with the
# loop's body done for every (goal, seed) row by one device call
# (PlanningWorld.ik_batch, C ABI mpg_ik_batch).
# ---------------------------------------------------------------------------
IK_CONVERGED, IK_IN_LIMITS, IK_COLLISION_FREE, IK_WITHIN_THRESHOLD, IK_SINGULAR, IK_VALID = 1, 2, 4, 8, 16, 15
_IK_SUCCESS = IK_CONVERGED | IK_IN_LIMITS | IK_COLLISION_FREE  # the loop's `success` before the distance test


def distance_6d(p1, q1, p2, q2) -> float:
    """Planner.distance_6D (planner.py:165-168)."""
    p1, q1, p2, q2 = (np.asarray(a, np.float64) for a in (p1, q1, p2, q2))
    return float(np.linalg.norm(p1 - p2) + min(np.linalg.norm(q1 - q2), np.linalg.norm(q1 + q2)))


def select_ik(q, status, start_qpos, *, threshold: float = 1e-3, return_closest: bool = False, equiv_mask=None,
              upper=None, distance=None):
    """What Planner.IK keeps of one goal's rows (planner.py:289-356).
    ``q`` [S, dof] and ``status`` [S] are the rows in seed order.  The rows
    with every MPG_IK_VALID bit are taken in that order, one within 0.1 (L2
    norm) of an earlier kept one is dropped.  No row kept: the reference's two
    failure strings -- the minimum distance_6D of the rows that converged inside
    the limits without collision (``distance(r)`` gives row r's; it is only
    called for those), or "Cannot find valid solution" when there is none.
    ``return_closest``: the 2 pi-equivalent choice of planner.py:337-355 for
    the joints of ``equiv_mask`` (revolute with a range above 2 pi) against
    their ``upper`` limits, then the answer nearest to ``start_qpos``.
    Returns (status_string, q_goals or None)."""
    q = np.asarray(q, np.float64)
    status = np.asarray(status)
    kept: List[np.ndarray] = []
    min_dis = 1e9
    for r in range(len(q)):
        if (int(status[r]) & _IK_SUCCESS) != _IK_SUCCESS:
            continue
        if int(status[r]) & IK_WITHIN_THRESHOLD:
            min_dis = min(min_dis, 0.0 if distance is None else float(distance(r)))
            if all(np.linalg.norm(k - q[r]) >= 0.1 for k in kept):
                kept.append(q[r].copy())
        else:
            min_dis = min(min_dis, float("inf") if distance is None else float(distance(r)))
    if not kept:
        if min_dis != 1e9:
            return f"IK Failed! Distance {min_dis} is greater than {threshold=}.", None
        return "IK Failed! Cannot find valid solution.", None
    if not return_closest:
        return "Success", kept
    goals = np.asarray(kept)
    start = np.asarray(start_qpos, np.float64)[None]
    if equiv_mask is not None and np.any(equiv_mask):
        em = np.asarray(equiv_mask, bool)
        q1 = goals[:, em]
        q2 = q1 + 2 * np.pi
        s = start[:, em]
        closer = (q2 < np.asarray(upper, np.float64)[None, em]) & (np.abs(q1 - s) > np.abs(q2 - s))
        goals[:, em] = np.where(closer, q2, q1)
    return "Success", goals[np.linalg.norm(goals - start, axis=1).argmin()]


def _state_joint_info(world):
    """(types, limits [dof, 2]) of the world's state: the move-group joints of
    the planned articulations in map order (the layout of set_qpos_all)."""
    types, lims = [], []
    for art in world.get_planned_articulations():
        pin = art.get_pinocchio_model()
        t, l = pin.get_joint_types(), pin.get_joint_limits()
        for i in art.get_move_group_joint_indices():
            types.append(t[i])
            lims.append(l[i][0])
    return types, np.asarray(lims, np.float64).reshape(-1, 2)


def ik(world, link, goal_pose, start_qpos, mask=None, *, n_init_qpos: int = 20, threshold: float = 1e-3,
       return_closest: bool = False, seed: int = 0):
    """Planner.IK over the world's state (the planned articulations' move-group
    joints): ``goal_pose`` (7,) returns (status_string, q_goals or None) as the
    reference does -- q_goals a list of states, or one state with
    ``return_closest``; an (M, 7) array returns a list of such pairs, all from
    one device call.  ``link``: a planned articulation's user link name (or a
    world link index); ``mask``: True freezes a state value; seed 0 of each
    goal is ``start_qpos``, the others are drawn on the device."""
    goals = np.asarray(goal_pose, np.float64)
    single = goals.ndim == 1
    goals = goals.reshape(-1, 7)
    start = np.asarray(start_qpos, np.float64).reshape(-1)
    q, status, _, _ = world.ik_batch(link, goals, start_qpos=start, n_init_qpos=int(n_init_qpos),
                                     mask=None if mask is None or len(mask) == 0 else np.asarray(mask, bool),
                                     seed=int(seed), threshold=float(threshold))
    types, lims = _state_joint_info(world)
    equiv = np.array([t.startswith("JointModelR") for t in types], bool) & (lims[:, 1] - lims[:, 0] > 2 * np.pi)
    li = world.ik_link_index(link) if isinstance(link, str) else int(link)
    out = []
    for g in range(len(goals)):
        def distance(r, g=g):  # only for the failure string's minimum
            pose = world.fk_link_pose(q[g, r], li)
            return distance_6d(goals[g, :3], goals[g, 3:], pose[:3], pose[3:])
        out.append(select_ik(q[g], status[g], start, threshold=threshold, return_closest=return_closest,
                             equiv_mask=equiv, upper=lims[:, 1], distance=distance))
    return out[0] if single else out


# ---------------------------------------------------------------------------
# Planner.TOPP (planner.py:358-375): the time-optimal parametrisation of
# joint-space paths under velocity and acceleration limits, many paths in one
# device call (PlanningWorld.topp_batch, C ABI mpg_topp_batch).
# ---------------------------------------------------------------------------
TOPP_OK, TOPP_NO_PATH, TOPP_ZERO_LENGTH, TOPP_STALLED, TOPP_TRUNCATED = 1, 2, 4, 8, 16
_TOPP_NAMES = ((TOPP_OK, "OK"), (TOPP_NO_PATH, "NO_PATH"), (TOPP_ZERO_LENGTH, "ZERO_LENGTH"), (TOPP_STALLED, "STALLED"),
               (TOPP_TRUNCATED, "TRUNCATED"))
_TOPP_KEYS = ("time", "position", "velocity", "acceleration")  # the reference's keys (planner.py:512-519)
_TOPP_MAX_SAMPLES = 65536


def topp_reason(status: int) -> str:
    """The names of a topp_batch row's status bits."""
    return ", ".join(n for b, n in _TOPP_NAMES if int(status) & b)


def _topp_rows(world, path, count, joint_vel_limits, joint_acc_limits, step):
    """One topp_batch call over path [rows, max_waypoints, dof] / count [rows],
    and a second one with room for the longest row when the default 256
    samples truncate some.  Returns per row (status, duration, (times,
    position, velocity, acceleration) cut to the row's samples)."""
    vel = np.asarray(joint_vel_limits, np.float64)
    acc = np.asarray(joint_acc_limits, np.float64)
    res = world.topp_batch(path, count, vel, acc, step=float(step))
    status, dur = res[6], res[5]
    cut = (status & TOPP_TRUNCATED) != 0
    if cut.any():
        need = int((dur[cut] / float(step)).max())
        if need <= _TOPP_MAX_SAMPLES:
            res = world.topp_batch(path, count, vel, acc, step=float(step), max_samples=need)
            status, dur = res[6], res[5]
    return [(int(status[r]), float(dur[r]), tuple(a[r, :res[4][r]].copy() for a in res[:4])) for r in range(len(count))]


def _pack_paths(paths):
    """(path [rows, max_waypoints, dof] padded with each row's last waypoint, count [rows])."""
    paths = [np.asarray(p, np.float64) for p in paths]
    if any(p.ndim != 2 for p in paths):
        raise ValueError("a path must be [n, dof]")
    mw = max([2] + [len(p) for p in paths])
    out = np.zeros((len(paths), mw, paths[0].shape[1] if paths else 0))
    for r, p in enumerate(paths):
        if len(p):
            out[r, :len(p)] = p
            out[r, len(p):] = p[-1]
    return out, np.array([len(p) for p in paths], np.int32)


def topp(world, path, joint_vel_limits, joint_acc_limits, step: float = 0.1):
    """Planner.TOPP: one path [n, dof] returns the reference's tuple (times,
    position, velocity, acceleration, duration); a list of paths returns a list
    of such tuples, all from one device call.  A path that cannot be
    parametrised (fewer than two waypoints, all waypoints equal, a stalled
    profile, more than 65536 samples) raises ValueError with the names of its
    status bits -- in a list it is None instead."""
    single = not isinstance(path, (list, tuple))
    packed, count = _pack_paths([path] if single else path)
    out = []
    for st, dur, arrays in _topp_rows(world, packed, count, joint_vel_limits, joint_acc_limits, step):
        out.append(arrays + (dur,) if st == TOPP_OK else None)
        if single and st != TOPP_OK:
            raise ValueError("topp: " + topp_reason(st))
    return out[0] if single else out


def _add_topp(world, results, ok, path, count, joint_vel_limits, joint_acc_limits, time_step):
    """The time parametrisation of the Success rows (ok [rows] bool) of a
    batch into their dictionaries: the reference's keys, or "topp": the
    status bits' names where a row is not parametrised."""
    if joint_vel_limits is None or joint_acc_limits is None or not np.any(ok):
        return
    rows = _topp_rows(world, path, np.where(ok, count, 0).astype(np.int32), joint_vel_limits, joint_acc_limits,
                      time_step)
    for i in np.flatnonzero(ok):
        st, dur, arrays = rows[i]
        if st == TOPP_OK:
            results[i].update(zip(_TOPP_KEYS, arrays), duration=dur)
        else:
            results[i]["topp"] = topp_reason(st)


# ---------------------------------------------------------------------------
# Planner.plan_screw (planner.py:526-671): the straight-line screw motion to a
# goal pose, its waypoints integrated and collision-checked by one device call
# (PlanningWorld.plan_screw_batch, C ABI mpg_screw_batch).  The result is the
# joint-space path the reference hands to TOPP-RA, and with the joint limits
# given its time parametrisation (topp above).
# ---------------------------------------------------------------------------
SCREW_REACHED, SCREW_COLLISION_FREE, SCREW_VALID = 1, 2, 3
SCREW_STALLED, SCREW_LIMIT, SCREW_TRUNCATED, SCREW_SINGULAR, SCREW_ROT_PI = 4, 8, 16, 32, 64
_SCREW_REASONS = ((SCREW_STALLED, "STALLED"), (SCREW_LIMIT, "LIMIT"), (SCREW_TRUNCATED, "TRUNCATED"),
                  (SCREW_SINGULAR, "SINGULAR"), (SCREW_ROT_PI, "ROT_PI"))


def screw_reason(status: int, first_hit: int = -1) -> str:
    """Why a row of plan_screw_batch is not a Success: the names of its end
    bit and, when a waypoint collides, COLLISION with the waypoint's index."""
    names = [n for b, n in _SCREW_REASONS if int(status) & b]
    if not int(status) & SCREW_COLLISION_FREE:
        names.append("COLLISION" if first_hit < 0 else f"COLLISION at waypoint {int(first_hit)}")
    return ", ".join(names)


def plan_screw(world, link, goal_pose, current_qpos, qpos_step: float = 0.1, *, max_waypoints: int = 64,
               joint_vel_limits=None, joint_acc_limits=None, time_step: float = 0.1):
    """Planner.plan_screw over the world's state: ``goal_pose`` (7,) returns
    {"status": "Success", "path": [count, dof]} or {"status": "screw plan
    failed", "reason": names of the status bits}; an (n, 7) array returns a
    list of such dictionaries, all from one device call, every row starting at
    ``current_qpos`` ((dof,) or [n, dof]).  ``link``: a planned articulation's
    user link name (or a world link index).  With ``joint_vel_limits`` and
    ``joint_acc_limits`` [dof] every Success also carries the reference's
    "time", "position", "velocity", "acceleration" and "duration" (one
    topp_batch call over the rows, samples every ``time_step``), or "topp":
    the names of the status bits of a path that could not be parametrised.
    The articulations' qpos is not touched."""
    goals = np.asarray(goal_pose, np.float64)
    single = goals.ndim == 1
    goals = goals.reshape(-1, 7)
    path, count, status, hit = world.plan_screw_batch(link, goals, np.asarray(current_qpos, np.float64),
                                                      qpos_step=float(qpos_step), max_waypoints=int(max_waypoints))
    out = []
    ok = (np.asarray(status) & SCREW_VALID) == SCREW_VALID
    for i in range(len(goals)):
        if ok[i]:
            out.append({"status": "Success", "path": path[i, :count[i]].copy()})
        else:
            out.append({"status": "screw plan failed", "reason": screw_reason(status[i], hit[i])})
    _add_topp(world, out, ok, path, count, joint_vel_limits, joint_acc_limits, time_step)
    return out[0] if single else out


# ---------------------------------------------------------------------------
# Planner.plan (planner.py:358-524): the RRTConnect searches of many (start,
# goals) rows in one device call (PlanningWorld.plan_batch, C ABI
# mpg_plan_batch), the IK in front of them for goals given as poses, and with
# the joint limits given the paths' time parametrisation (topp above).
# ---------------------------------------------------------------------------
PLAN_SOLVED, PLAN_START_INVALID, PLAN_GOAL_INVALID = 1, 2, 4
PLAN_ROUNDS_EXHAUSTED, PLAN_NODES_EXHAUSTED, PLAN_TRUNCATED = 8, 16, 32
_PLAN_REASONS = ((PLAN_START_INVALID, "START_INVALID"), (PLAN_GOAL_INVALID, "GOAL_INVALID"),
                 (PLAN_ROUNDS_EXHAUSTED, "ROUNDS_EXHAUSTED"), (PLAN_NODES_EXHAUSTED, "NODES_EXHAUSTED"),
                 (PLAN_TRUNCATED, "TRUNCATED"))


def plan_reason(status: int) -> str:
    """Why a row of plan_batch is not a Success: the names of its status bits."""
    return ", ".join(n for b, n in _PLAN_REASONS if int(status) & b)


def plan_batch(world, start_qpos, goal_qpos, *, range: float = 0.0, max_rounds: int = 20000, max_nodes: int = 2048,
               max_waypoints: int = 256, seed: int = 0, row_seed=None, check_every: int = 8,
               joint_vel_limits=None, joint_acc_limits=None, time_step: float = 0.1):
    """Planner.plan's RRTConnect for many queries in one device call:
    ``goal_qpos`` [Q, dof] (one goal state per row) or [Q, G, dof], every row
    starting at ``start_qpos`` ((dof,) or [Q, dof]).  Returns per row {"status":
    "Success", "path": [count, dof]} or {"status": "plan failed", "reason":
    names of the status bits}.  The paths are RRTConnect's, not simplified
    (the reference does not simplify them either).  With ``joint_vel_limits``
    and ``joint_acc_limits`` [dof] every Success also carries the reference's
    "time", "position", "velocity", "acceleration" and "duration" (one
    topp_batch call over the rows, samples every ``time_step``), or "topp": the
    names of the status bits of a path that could not be parametrised.  The
    articulations' qpos is not touched."""
    path, count, status, _, _ = world.plan_batch(np.asarray(start_qpos, np.float64), np.asarray(goal_qpos, np.float64),
                                                 range=float(range), max_rounds=int(max_rounds),
                                                 max_nodes=int(max_nodes), max_waypoints=int(max_waypoints),
                                                 seed=int(seed), row_seed=row_seed, check_every=int(check_every))
    out = []
    for i in np.arange(len(status)):
        if int(status[i]) == PLAN_SOLVED:
            out.append({"status": "Success", "path": path[i, :count[i]].copy()})
        else:
            out.append({"status": "plan failed", "reason": plan_reason(status[i])})
    _add_topp(world, out, np.asarray(status) == PLAN_SOLVED, path, count, joint_vel_limits, joint_acc_limits, time_step)
    return out


def plan_to_pose_batch(world, link, goal_poses, start_qpos, *, max_goals: int = 4, n_init_qpos: int = 20,
                       threshold: float = 1e-3, ik_seed: int = 0, joint_vel_limits=None, joint_acc_limits=None,
                       time_step: float = 0.1, **plan_options):
    """What Planner.plan does, for M goal poses [M, 7] of
    ``link`` at once: one ik_batch call (``n_init_qpos`` seeds per pose, seed 0
    = ``start_qpos`` (dof,)), up to ``max_goals`` of each pose's valid answers
    (Planner.IK's selection: seed order, none within 0.1 of an earlier one) as
    the row's goal states, then one plan_batch call over the poses that have
    an answer.  Returns per pose plan_batch's dictionary, or {"status": "IK
    failed", "reason": Planner.IK's message}.  ``joint_vel_limits`` /
    ``joint_acc_limits`` / ``time_step``: the paths' time parametrisation, as
    in plan_batch.  ``plan_options``: plan_batch's."""
    goals = np.asarray(goal_poses, np.float64).reshape(-1, 7)
    start = np.asarray(start_qpos, np.float64).reshape(-1)
    q, status, _, _ = world.ik_batch(link, goals, start_qpos=start, n_init_qpos=int(n_init_qpos), seed=int(ik_seed),
                                     threshold=float(threshold))
    out = [None] * len(goals)
    rows, states = [], []
    G = max(1, min(int(max_goals), 16))
    for g in np.arange(len(goals)):
        msg, kept = select_ik(q[g], status[g], start, threshold=threshold)
        if kept is None:
            out[g] = {"status": "IK failed", "reason": msg}
            continue
        kept = kept[:G]
        rows.append(int(g))
        states.append(np.array(kept + [kept[0]] * (G - len(kept))))  # a repeated goal is a second root on the same state
    if rows:
        for g, res in zip(rows, plan_batch(world, start, np.array(states), joint_vel_limits=joint_vel_limits,
                                           joint_acc_limits=joint_acc_limits, time_step=time_step, **plan_options)):
            out[g] = res
    return out
