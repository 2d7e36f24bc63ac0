"""Shared inputs and references of the batched-RRTConnect tests
(test_rrt_host.py, test_plan_batch.py).

np_plan_batch is a numpy restatement of mpg_plan_batch's algorithm written
from the OMPL 1.6 semantics test_planner.py's docstring lists, not from
mplib_amd/csrc/mpg_rrt.h: each row is RRTConnect::solve as a Python generator
-- the loop `sample, growTree(tree), growTree(other) while ADVANCED, swap` --
that yields the states a growTree call validates (DiscreteMotionValidator:
checkMotion(a, b) looks at b, then interpolate(a, b, j / nd), nd = ceil(d /
(0.01 extent)); the goal tree asks isValid(new) && checkMotion(new, near)) and
is sent their flags.  One yield is one round; the driver answers every row's
yield of a round with one call of the validity callback.  The three stated
deviations: the sample of iteration k is lo + (hi - lo) * u, u = (splitmix64(
row_seed + (k * dof + j + 1) * golden) >> 11) * 2^-53; every valid goal is a
goal-tree root from the start; an invalid start is reported.

Recipe R: the cfg3 scene (Panda + 10 boxes); 512 states drawn with
Wd.sample_q(art, 512, seed=2026), the first 128 the CPU oracle finds
collision-free kept: 64 starts, then 64 goals; range = 0.1; row_seed[r] =
12345 + 7919 r.  A 65th row (start of row 0, goal of row 1, its own seed)
follows them for the tests that want a batch one row past the wave.
MAX_ROUNDS / MAX_NODES / MAX_WAYPOINTS below were fixed with np_plan_batch
alone, on the CPU, with the oracle as validity: it solves 61 of the 64 rows
(two run out of rounds, one fills its start tree), 41 of them in their first
iteration; the longest path has 370 waypoints, 13 rows grow a tree past 256
nodes.  With 20000 rounds and 4096 nodes all 64 solve, the largest tree has
1858 nodes.  Everything is computed once per process and handed out read-only.
"""
import ctypes
import functools
import os

import numpy as np

import worlds as Wd
from native import host_shim

SOLVED, START_INVALID, GOAL_INVALID, ROUNDS_EXHAUSTED, NODES_EXHAUSTED, TRUNCATED = 1, 2, 4, 8, 16, 32
N_ROWS = 64   # recipe R
N_BATCH = 65  # with the extra row
RANGE = 0.1
MAX_ROUNDS = 4000
MAX_NODES = 1024
MAX_WAYPOINTS = 512

_M64 = (1 << 64) - 1
_GOLDEN = 0x9E3779B97F4A7C15
_PI = float(np.pi)
_EPS = float(np.finfo(np.float64).eps)


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


# --- the sampler ----------------------------------------------------------------
def splitmix64(z):
    z &= _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def row_seed_of(seed, r):
    return splitmix64(seed + (r + 1) * _GOLDEN)


def np_sample(lo, hi, row_seed, k):
    dof = len(lo)
    u = np.array([(splitmix64(int(row_seed) + (k * dof + j + 1) * _GOLDEN) >> 11) * 2.0 ** -53 for j in range(dof)])
    return lo + (hi - lo) * u


# --- OMPL's compound space of RealVector(1) / SO2 subspaces, weights 1 --------------
class Space:
    def __init__(self, lo, hi, so2_mask=0, range_=0.0):
        self.dof = len(lo)
        self.so2 = np.array([(so2_mask >> i) & 1 for i in range(self.dof)], bool)
        self.lo = np.where(self.so2, -_PI, np.asarray(lo, np.float64))
        self.hi = np.where(self.so2, _PI, np.asarray(hi, np.float64))
        extent = 0.0
        for i in range(self.dof):
            extent += _PI if self.so2[i] else self.hi[i] - self.lo[i]
        self.extent = extent
        self.lvs = extent * 0.01
        self.range = range_ if range_ > 1e-6 else 0.2 * extent

    def distance(self, a, b):
        """a [dof] or [n, dof] against b [dof]: the subspaces' distances added in order."""
        a = np.asarray(a)
        d = np.zeros(a.shape[:-1])
        for i in range(self.dof):
            x = np.abs(a[..., i] - b[i])
            if self.so2[i]:
                x = np.where(x > _PI, 2.0 * _PI - x, x)
            d = d + x
        return d

    def interpolate(self, a, b, t):
        out = a + (b - a) * t
        for i in np.flatnonzero(self.so2):
            diff = b[i] - a[i]
            if abs(diff) <= _PI:
                out[i] = a[i] + diff * t
            else:
                diff = 2.0 * _PI - diff if diff > 0.0 else -2.0 * _PI - diff
                v = a[i] - diff * t
                if v > _PI:
                    v -= 2.0 * _PI
                elif v < -_PI:
                    v += 2.0 * _PI
                out[i] = v
        return out

    def equal(self, a, b):
        return bool((np.abs(a - b) <= 2.0 * _EPS)[~self.so2].all() and (np.abs(a - b) < 2.0 * _EPS)[self.so2].all())

    def in_bounds(self, s):
        real = ~self.so2
        if (s[self.so2] < -_PI).any() or (s[self.so2] > _PI).any():
            return False
        return not ((s[real] - _EPS > self.hi[real]).any() or (s[real] + _EPS < self.lo[real]).any())

    def motion_states(self, a, b):
        nd = int(np.ceil(float(self.distance(a, b)) / self.lvs))
        return [b] + [self.interpolate(a, b, j / nd) for j in range(1, nd)]


TRAPPED, ADVANCED, REACHED = 0, 1, 2


class _Tree:
    def __init__(self, dof, cap):
        self.st = np.zeros((cap, dof))
        self.parent = np.full(cap, -1, np.int64)
        self.n = 0
        self.cap = cap

    def add(self, s, parent):
        self.st[self.n] = s
        self.parent[self.n] = parent
        self.n += 1
        return self.n - 1


class _Full(Exception):
    pass


class _Row:
    """One row's outputs and its generator."""

    def __init__(self, sp, start, goals, seed, max_nodes, max_waypoints):
        self.sp, self.start, self.goals, self.seed = sp, start, goals, seed
        self.max_nodes, self.max_waypoints = max_nodes, max_waypoints
        self.status, self.iterations, self.path = 0, 0, None
        self.rounds = -1  # the start / goal check is not a round
        self.trees = [_Tree(sp.dof, max_nodes), _Tree(sp.dof, max_nodes)]
        self.gen = self._solve()

    def _grow(self, t, target, k):
        sp, tree = self.sp, self.trees[t]
        near = int(np.argmin(sp.distance(tree.st[:tree.n], target)))  # the first of equal minima
        a = tree.st[near].copy()
        d = float(sp.distance(a, target))
        new, reach = target, True
        if d > sp.range:
            new = sp.interpolate(a, target, sp.range / d)
            if sp.equal(a, new):
                yield k, []
                return TRAPPED, -1
            reach = False
        states = sp.motion_states(a, new) if t == 0 else [new] + sp.motion_states(new, a)
        flags = yield k, states
        if np.any(flags):
            return TRAPPED, -1
        if tree.n >= tree.cap:
            raise _Full()
        return (REACHED if reach else ADVANCED), tree.add(new, near)

    def _solve(self):
        sp = self.sp
        flags = yield 0, [self.start] + list(self.goals)
        if flags[0] or not sp.in_bounds(self.start):
            self.status |= START_INVALID
        else:
            self.trees[0].add(self.start, -1)
        for g, f in zip(self.goals, flags[1:]):
            if f or not sp.in_bounds(g):
                continue
            if self.trees[1].n >= self.max_nodes:
                self.status |= NODES_EXHAUSTED
                break
            self.trees[1].add(g, -1)
        if self.trees[1].n == 0:
            self.status |= GOAL_INVALID
        if self.status:
            return
        k = 0
        try:
            while True:
                t = k & 1  # the trees swap every iteration
                k += 1
                r, added = yield from self._grow(t, np_sample(sp.lo, sp.hi, self.seed, k - 1), k)
                if r == TRAPPED:
                    continue
                target = self.trees[t].st[added].copy()
                r, other = yield from self._grow(1 - t, target, k)
                while r == ADVANCED:
                    r, other = yield from self._grow(1 - t, target, k)
                if r == REACHED:
                    sm, gm = (added, other) if t == 0 else (other, added)
                    self._finish(sm, gm)
                    return
        except _Full:
            self.status |= NODES_EXHAUSTED

    def _finish(self, sm, gm):
        ts, tg = self.trees
        if ts.parent[sm] >= 0:  # the connection state is in both trees
            sm = ts.parent[sm]
        else:
            gm = tg.parent[gm]
        p = []
        while sm >= 0:
            p.append(ts.st[sm])
            sm = ts.parent[sm]
        p.reverse()
        while gm >= 0:
            p.append(tg.st[gm])
            gm = tg.parent[gm]
        self.status |= SOLVED
        if len(p) > self.max_waypoints:
            self.status |= TRUNCATED
        else:
            self.path = np.array(p)


def np_plan_batch(lo, hi, start, goal, row_seed, valid, *, range_=RANGE, max_rounds=MAX_ROUNDS, max_nodes=MAX_NODES,
                  max_waypoints=MAX_WAYPOINTS, so2_mask=0, rounds_out=None):
    """(path [Q, max_waypoints, dof], n_waypoints, status, iterations, tree_sizes [Q, 2]).
    valid(states [n, dof]) -> flags [n], 0 = valid.  rounds_out: a list that receives the rounds each row took."""
    start = np.asarray(start, np.float64)
    Q, dof = start.shape
    goal = np.asarray(goal, np.float64).reshape(Q, -1, dof)
    sp = Space(lo, hi, so2_mask, range_)
    rows = [_Row(sp, start[r], goal[r], int(row_seed[r]), max_nodes, max_waypoints) for r in range(Q)]

    def serve(asks):
        """One validity call for every pending ask; the rows' next asks."""
        states = [s for _, (_, st) in asks for s in st]
        flags = valid(np.array(states).reshape(-1, dof)) if states else np.zeros(0, np.uint8)
        nxt, pos = [], 0
        for row, (k, st) in asks:
            row.iterations = k
            row.rounds += 1
            try:
                nxt.append((row, row.gen.send(flags[pos:pos + len(st)])))
            except StopIteration:
                pass
            pos += len(st)
        return nxt

    asks = serve([(row, next(row.gen)) for row in rows])  # start and goals: not a round
    for _ in range(max_rounds):
        if not asks:
            break
        asks = serve(asks)
    for row, _ in asks:
        row.status |= ROUNDS_EXHAUSTED
    if rounds_out is not None:
        rounds_out.extend(row.rounds for row in rows)
    path = np.repeat(start[:, None, :], max_waypoints, axis=1)
    count = np.zeros(Q, np.int32)
    for r, row in enumerate(rows):
        if row.path is not None:
            count[r] = len(row.path)
            path[r, :count[r]] = row.path
            path[r, count[r]:] = row.path[-1]
    return (path, count, np.array([row.status for row in rows], np.uint8),
            np.array([row.iterations for row in rows], np.int32),
            np.array([[row.trees[0].n, row.trees[1].n] for row in rows], np.int32))


# --- validity: the CPU oracle, with a memo so the second model pays nothing -----------
@functools.lru_cache(maxsize=None)
def oracle3():
    return Wd.oracle_world(3)


_memo = {}


def oracle_valid(states):
    """flags of the cfg3 oracle (0 = valid); states seen before come from a memo."""
    states = np.ascontiguousarray(states, np.float64).reshape(-1, 7)
    keys = [s.tobytes() for s in states]
    miss = [i for i, k in enumerate(keys) if k not in _memo]
    if miss:
        f, _ = oracle3().collide_batch(states[miss], nthreads=min(16, os.cpu_count() or 1))
        for i, v in zip(miss, f):
            _memo[keys[i]] = int(v != 0)
    return np.array([_memo[k] for k in keys], np.uint8)


@functools.lru_cache(maxsize=None)
def limits():
    lim = np.array(oracle3().art.joint_limits()[:7], np.float64)
    return _ro(lim[:, 0].copy(), lim[:, 1].copy())


@functools.lru_cache(maxsize=None)
def recipe_r():
    """(start [65, 7], goal [65, 7], row_seed [65] uint64): recipe R's 64 rows, then the extra one."""
    q = Wd.sample_q(oracle3().art, 512, 2026)
    free = q[oracle_valid(q) == 0][:2 * N_ROWS]
    assert len(free) == 2 * N_ROWS
    seeds = (12345 + 7919 * np.arange(N_BATCH)).astype(np.uint64)
    start = np.vstack([free[:N_ROWS], free[:1]])
    goal = np.vstack([free[N_ROWS:], free[N_ROWS + 1:N_ROWS + 2]])
    return _ro(start, goal, seeds)


@functools.lru_cache(maxsize=None)
def reference_r():
    lo, hi = limits()
    s, g, seeds = recipe_r()
    return _ro(*np_plan_batch(lo, hi, s, g, seeds, oracle_valid))


# --- mpg_rrt.h compiled for the host (tests/native/rrt_host.cpp) ------------------------
_VALID_FN = ctypes.CFUNCTYPE(None, ctypes.POINTER(ctypes.c_double), ctypes.c_long, ctypes.POINTER(ctypes.c_ubyte))
_lib = None


def host_lib():
    global _lib
    if _lib is None:
        _lib = host_shim._build(os.path.join(os.path.dirname(host_shim.__file__), "rrt_host.cpp"), "mplib_amd_rrt_host")
        _lib.rrt_host_sample.restype = ctypes.c_double
        _lib.rrt_host_row_seed.restype = ctypes.c_ulonglong
    return _lib


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def host_plan_batch(lo, hi, start, goal, row_seed, valid, *, range_=RANGE, max_rounds=MAX_ROUNDS, max_nodes=MAX_NODES,
                    max_waypoints=MAX_WAYPOINTS, so2_mask=0, seed=0):
    """mpg_rrt.h's rows on the host, in lockstep: the outputs of np_plan_batch.
    row_seed None: the rows' seeds come from ``seed``."""
    lo, hi = np.ascontiguousarray(lo, np.float64), np.ascontiguousarray(hi, np.float64)
    start = np.ascontiguousarray(start, np.float64)
    Q, dof = start.shape
    goal = np.ascontiguousarray(np.asarray(goal, np.float64).reshape(Q, -1, dof))
    G = goal.shape[1]
    rs = None if row_seed is None else np.ascontiguousarray(row_seed, np.uint64)

    def cb(states, n, flags):
        f = valid(np.ctypeslib.as_array(states, shape=(n * dof,)).reshape(n, dof).copy()) if n else ()
        for i, v in enumerate(f):
            flags[i] = int(v)

    path = np.zeros((Q, max_waypoints, dof))
    count = np.zeros(Q, np.int32)
    status = np.zeros(Q, np.uint8)
    iters = np.zeros(Q, np.int32)
    sizes = np.zeros((Q, 2), np.int32)
    rc = host_lib().rrt_host_plan(_p(lo), _p(hi), dof, _p(start), _p(goal), ctypes.c_long(Q), G,
                                  None if rs is None else _p(rs), ctypes.c_double(range_), int(max_rounds),
                                  int(max_nodes), int(max_waypoints), ctypes.c_ulonglong(seed), ctypes.c_uint(so2_mask),
                                  _VALID_FN(cb), _p(path), _p(count), _p(status), _p(iters), _p(sizes))
    assert rc == 0, rc
    return path, count, status, iters, sizes


@functools.lru_cache(maxsize=None)
def header_r():
    lo, hi = limits()
    s, g, seeds = recipe_r()
    return _ro(*host_plan_batch(lo, hi, s, g, seeds, oracle_valid))


def host_view(lo, hi, Q=1, G=1, *, range_=0.0, max_rounds=100, max_nodes=64, max_waypoints=16, check_every=8,
              so2_mask=0):
    """fill_rrt_view: (code, message, range, lvs, block); code 0 ok, 1 MPG_E_INVALID, 2 MPG_E_UNSUPPORTED."""
    lo, hi = np.ascontiguousarray(lo, np.float64), np.ascontiguousarray(hi, np.float64)
    rng, lvs, blk = ctypes.c_double(), ctypes.c_double(), ctypes.c_int()
    msg = ctypes.create_string_buffer(256)
    rc = host_lib().rrt_host_view(_p(lo), _p(hi), len(lo), ctypes.c_long(Q), int(G), ctypes.c_double(range_),
                                  int(max_rounds), int(max_nodes), int(max_waypoints), int(check_every),
                                  ctypes.c_uint(so2_mask), ctypes.byref(rng), ctypes.byref(lvs), ctypes.byref(blk), msg,
                                  len(msg))
    return rc, msg.value.decode(), rng.value, lvs.value, blk.value


def assert_valid_solution(sp, path, start, goals, valid):
    """A solved row's path as OMPL defines a valid solution (the logic of
    test_planner.assert_valid_solution): endpoints, every state valid and
    inside the bounds, every edge at most range, every edge's validator
    states valid."""
    assert np.array_equal(path[0], start)
    assert any(np.array_equal(path[-1], g) for g in goals)
    assert not valid(path).any()
    assert (path >= sp.lo - 1e-12).all() and (path <= sp.hi + 1e-12).all()
    for a, b in zip(path[:-1], path[1:]):
        assert float(sp.distance(a, b)) <= sp.range * (1 + 1e-12)
        assert not valid(np.array(sp.motion_states(a, b))).any()
