"""GPU: mpg_topp_batch (DeviceWorld.topp_batch / topp_batch_device,
PlanningWorld.topp_batch / topp_batch_device, mplib_amd.planner.topp and the
time parametrisation of plan_screw / plan_batch) against the host build of the
header the kernels run.  Inputs and references: tests/topp_cases.py.

The device's results equal the host build's bit for bit: the arithmetic is + -
* / sqrt in fp64 with contraction off on both sides and the only reduction over
lanes is a minimum."""
import ctypes
import functools

import numpy as np
import pytest

import screw_cases as S
import topp_cases as T
import worlds as Wd
from mplib_amd import _capi as C
from mplib_amd import planner as P
from mplib_amd import scenes

pytestmark = pytest.mark.gpu

NAMES = ("times", "position", "velocity", "acceleration", "n_samples", "duration", "status", "grid_x", "grid_t")
LINK = "panda_hand"


@functools.lru_cache(maxsize=None)
def dev_world():
    from mplib_amd.batch import DeviceWorld
    return DeviceWorld(Wd.desc_arrays(Wd.oracle_world(3)))


@functools.lru_cache(maxsize=None)
def world_art(cfg=3):
    return scenes.world(cfg)


def world():
    return world_art()[0]


def assert_same(got, want, rows=slice(None)):
    for name, a in zip(NAMES, got):
        a = a.cpu().numpy() if hasattr(a, "cpu") else a
        np.testing.assert_array_equal(a, want[name][rows], err_msg=name)


# --- 8. device equals host build ---------------------------------------------------
@pytest.mark.parametrize("gps,max_samples,rows", [(4, T.T_SAMPLES, 96), (8, 256, 96), (8, 256, 1), (8, 256, 63),
                                                  (8, 256, 64), (8, 256, 65)])
def test_device_equals_host_build(gps, max_samples, rows):
    """Recipe T at grid_per_segment 4 (no row truncated) and at the defaults
    (the rows longer than 25.6 s are OK | TRUNCATED), and its leading rows at
    the wave-count edges: every output bit for bit."""
    path, cnt, _ = T.recipe_t()
    want = T.host_t(gps, max_samples)
    got = dev_world().topp_batch(path[:rows], cnt[:rows], T.VMAX, T.AMAX, grid_per_segment=gps,
                                 max_samples=max_samples, return_grid=True)
    assert_same(got, want, slice(0, rows))
    if rows == 96:
        assert ((want["status"] & T.TRUNCATED) != 0).any() == (max_samples == 256)


# --- 9. tests 3 and 6 on device results ----------------------------------------------
@pytest.mark.parametrize("gps", [4, 8])
def test_device_profile_is_feasible_and_greedy(gps):
    path, cnt, _ = T.recipe_t()
    got = dict(zip(NAMES, dev_world().topp_batch(path, cnt, T.VMAX, T.AMAX, grid_per_segment=gps,
                                                 max_samples=T.T_SAMPLES, return_grid=True)))
    assert (got["status"] == T.OK).all()
    K = T.host_t(gps)["grid_k"]  # the controllable sets are no output of the call
    for r in range(len(cnt)):
        T.check_profile(path[r, :cnt[r]], got["grid_x"][r], K[r], T.grid_size(cnt[r], gps))


def test_device_status_paths():
    dw = dev_world()
    q = np.random.default_rng(6).uniform(T.LIMITS[:, 0], T.LIMITS[:, 1], size=(3, 7))
    a = np.zeros(7)
    b = a.copy()
    b[2] = 0.5
    p, c = T.pack([q[:1], q[:0], np.tile(q[0], (3, 1)), q, [a, b], [a, b, a]], max_waypoints=8)
    want = T.host_topp(p, c)
    got = dw.topp_batch(p, c, T.VMAX, T.AMAX, return_grid=True)
    assert_same(got, want)
    assert got[6].tolist() == [T.NO_PATH, T.NO_PATH, T.ZERO_LENGTH, T.OK, T.OK, T.OK]
    for r in range(3):
        assert got[5][r] == 0.0 and got[4][r] == 0 and (got[1][r] == p[r, 0]).all() and (got[2][r] == 0.0).all()
    m = got[4][3]
    assert m == int(got[5][3] / 0.1) and (got[1][3, m:] == got[1][3, m - 1]).all() and (got[0][3, m:] == got[0][3, m - 1]).all()
    # truncation keeps the duration
    cut = dw.topp_batch(p[3:4], c[3:4], T.VMAX, T.AMAX, max_samples=4)
    assert cut[6][0] == (T.OK | T.TRUNCATED) and cut[4][0] == 0 and cut[5][0] == got[5][3]
    assert (cut[1][0] == p[3, 0]).all()
    # host memory: a non-finite value inside a row's count and a count above max_waypoints are refused
    bad = p.copy()
    bad[3, 1, 4] = np.nan
    with pytest.raises(ValueError, match="non-finite path value in row 3"):
        dw.topp_batch(bad, c, T.VMAX, T.AMAX)
    high = c.copy()
    high[4] = 9
    with pytest.raises(ValueError, match=r"n_waypoints\[4\] exceeds max_waypoints"):
        dw.topp_batch(p, high, T.VMAX, T.AMAX)


def test_device_memory_nan_and_clamped_count():
    """Device buffers are not checked: a NaN waypoint ends STALLED, a count above max_waypoints is clamped."""
    import torch
    dw = dev_world()
    q = np.random.default_rng(7).uniform(T.LIMITS[:, 0], T.LIMITS[:, 1], size=(5, 7))
    bad = q.copy()
    bad[2, 3] = np.nan
    p, c = T.pack([bad, q], max_waypoints=5)
    c[1] = 9
    out = dw.topp_batch_device(torch.from_numpy(p).cuda(), torch.from_numpy(c).cuda(), T.VMAX, T.AMAX)
    torch.cuda.synchronize()
    c[1] = 5
    want = T.host_topp(p, c)
    assert out[6].cpu().tolist() == [T.STALLED, T.OK] and out[4][0].item() == 0 and out[5][0].item() == 0.0
    for name, a in zip(NAMES[:7], out):
        np.testing.assert_array_equal(a.cpu().numpy()[1], want[name][1], err_msg=name)


# --- 10. device path ---------------------------------------------------------------
def test_screw_then_topp_on_one_stream():
    """plan_screw_batch_device, then topp_batch_device on its path / count
    tensors, both enqueued on one stream with no host copy between them."""
    import torch
    w = world()
    li = w.ik_link_index(LINK)
    q0, goal = S.recipe_s()
    hp, hc, hs, _ = w.plan_screw_batch(LINK, goal, q0)
    short = np.flatnonzero(hc < 2)[:2]
    idx = np.concatenate([np.setdiff1d(np.arange(16 - len(short)), short), short]).astype(int)
    n, mw, ms, g = len(idx), 64, 256, T.grid_size(64) + 1
    print("rows with fewer than 2 waypoints in the slice:", len(short))
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        gd = torch.from_numpy(goal[idx].copy()).cuda()
        sd = torch.from_numpy(q0[idx].copy()).cuda()
        f64 = dict(dtype=torch.float64, device="cuda")
        path, cnt = torch.zeros(n, mw, 7, **f64), torch.zeros(n, dtype=torch.int32, device="cuda")
        st = torch.zeros(n, dtype=torch.uint8, device="cuda")
        out = (torch.zeros(n, ms, **f64), torch.zeros(n, ms, 7, **f64), torch.zeros(n, ms, 7, **f64),
               torch.zeros(n, ms, 7, **f64), torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(n, **f64),
               torch.zeros(n, dtype=torch.uint8, device="cuda"), torch.zeros(n, g, **f64), torch.zeros(n, g, **f64))
    stream.synchronize()  # the inputs are in place; the calls below only enqueue
    w.plan_screw_batch_device(li, gd.data_ptr(), sd.data_ptr(), n, path.data_ptr(), cnt.data_ptr(), st.data_ptr(), 0,
                              stream.cuda_stream)
    w.topp_batch_device(path.data_ptr(), cnt.data_ptr(), n, mw, T.VMAX, T.AMAX, *(t.data_ptr() for t in out),
                        stream.cuda_stream)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(path.cpu().numpy(), hp[idx])
    np.testing.assert_array_equal(cnt.cpu().numpy(), hc[idx])
    want = dict(zip(NAMES, w.topp_batch(hp[idx], hc[idx], T.VMAX, T.AMAX, return_grid=True)))
    assert_same(out, want)
    status = out[6].cpu().numpy()
    assert (status[hc[idx] < 2] == T.NO_PATH).all() and ((status & T.OK) != 0).sum() >= 8
    assert_same(want.values(), T.host_topp(hp[idx], hc[idx]))


# --- 11. two streams ---------------------------------------------------------------
def test_two_streams_do_not_share_a_workspace():
    import torch
    dw = dev_world()
    path, cnt, _ = T.recipe_t()
    want = T.host_t(8, 256)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    parts = ((0, 40), (40, 96))
    ins = []
    for s, (a, b) in zip(streams, parts):
        with torch.cuda.stream(s):
            ins.append((torch.from_numpy(path[a:b].copy()).cuda(), torch.from_numpy(cnt[a:b].copy()).cuda()))
        s.synchronize()
    outs = []
    for rep in range(2):  # the second pass reuses both workspaces
        outs = []
        for s, (p, c) in zip(streams, ins):
            with torch.cuda.stream(s):
                outs.append(dw.topp_batch_device(p, c, T.VMAX, T.AMAX, return_grid=True, stream=s.cuda_stream))
    torch.cuda.synchronize()
    for (a, b), out in zip(parts, outs):
        assert_same(out, want, slice(a, b))
    for s in streams:
        C.check(C.lib().mpg_release_stream(dw.handle, ctypes.c_void_p(s.cuda_stream)), "mpg_release_stream")


# --- 12. facade --------------------------------------------------------------------
KEYS = ("time", "position", "velocity", "acceleration", "duration")


def check_result(r, step=0.1):
    assert r["status"] == "Success" and all(k in r for k in KEYS), r.keys()
    m = int(r["duration"] / step)
    assert r["time"].shape == (m,) and r["position"].shape == r["velocity"].shape == r["acceleration"].shape == (m, 7)
    assert r["time"][0] == 0.0 and abs(r["time"][-1] - r["duration"]) <= np.spacing(r["duration"]) * m
    np.testing.assert_allclose(r["position"][0], r["path"][0], rtol=0, atol=1e-9)
    np.testing.assert_allclose(r["position"][-1], r["path"][-1], rtol=0, atol=1e-9)
    assert np.abs(r["velocity"][[0, -1]]).max() <= 1e-6  # at rest at both ends


def test_facade():
    import rrt_cases as R
    w = world()
    art = world_art()[1]
    keep = np.array(art.get_qpos())
    q0, goal = S.recipe_s()
    plain = P.plan_screw(w, LINK, goal[:8], q0[:8])
    timed = P.plan_screw(w, LINK, goal[:8], q0[:8], joint_vel_limits=T.VMAX, joint_acc_limits=T.AMAX)
    assert sum(r["status"] == "Success" for r in plain) >= 4
    for a, b in zip(plain, timed):
        assert set(a) == {"status", "path"} or set(a) == {"status", "reason"}
        if a["status"] != "Success":
            assert a == b
            continue
        np.testing.assert_array_equal(a["path"], b["path"])
        check_result(b)
        times, pos, vel, acc, dur = P.topp(w, a["path"], T.VMAX, T.AMAX)
        assert dur == b["duration"]
        for x, k in zip((times, pos, vel, acc), KEYS):
            np.testing.assert_array_equal(x, b[k])
    # without the keywords: what the call returned before, key for key
    again = P.plan_screw(w, LINK, goal[:8], q0[:8])
    for a, b in zip(plain, again):
        assert a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)
    one = P.plan_screw(w, LINK, goal[0], q0[0], joint_vel_limits=T.VMAX, joint_acc_limits=T.AMAX, time_step=0.05)
    if one["status"] == "Success":
        check_result(one, 0.05)
    # plan_batch: 8 queries that solve in few iterations
    kw = dict(range=R.RANGE, max_rounds=R.MAX_ROUNDS, max_nodes=R.MAX_NODES, max_waypoints=R.MAX_WAYPOINTS)
    start, goal_q, seeds = R.recipe_r()
    _, _, st, iters, _ = w.plan_batch(start[:24], goal_q[:24], row_seed=seeds[:24], **kw)
    easy = np.argsort(np.where(st == P.PLAN_SOLVED, iters, 1 << 30), kind="stable")[:8]
    plain = P.plan_batch(w, start[easy], goal_q[easy], row_seed=seeds[easy], **kw)
    timed = P.plan_batch(w, start[easy], goal_q[easy], row_seed=seeds[easy], joint_vel_limits=T.VMAX,
                         joint_acc_limits=T.AMAX, **kw)
    assert all(r["status"] == "Success" and set(r) == {"status", "path"} for r in plain)
    for a, b in zip(plain, timed):
        np.testing.assert_array_equal(a["path"], b["path"])
        check_result(b)
    # the reference's tuple, a list of paths, and a path that cannot be parametrised
    both = P.topp(w, [plain[0]["path"], plain[1]["path"][:1], plain[1]["path"]], T.VMAX, T.AMAX)
    assert both[1] is None and len(both[0]) == 5 and both[0][4] == timed[0]["duration"]
    np.testing.assert_array_equal(both[2][1], timed[1]["position"])
    with pytest.raises(ValueError, match="NO_PATH"):
        P.topp(w, plain[0]["path"][:1], T.VMAX, T.AMAX)
    assert P.topp_reason(T.OK | T.TRUNCATED) == "OK, TRUNCATED" and P.topp_reason(T.STALLED) == "STALLED"
    # a path longer than 256 samples is parametrised again with room for it
    slow = P.topp(w, plain[0]["path"], T.VMAX / 50, T.AMAX)
    assert slow[4] > 25.6 and len(slow[0]) == int(slow[4] / 0.1)
    np.testing.assert_array_equal(np.array(art.get_qpos()), keep)
    assert (C.MPG_TOPP_OK, C.MPG_TOPP_NO_PATH, C.MPG_TOPP_ZERO_LENGTH, C.MPG_TOPP_STALLED, C.MPG_TOPP_TRUNCATED) == (
        P.TOPP_OK, P.TOPP_NO_PATH, P.TOPP_ZERO_LENGTH, P.TOPP_STALLED, P.TOPP_TRUNCATED) == (1, 2, 4, 8, 16)


# --- 13. rows = 0 and the ABI's error returns ----------------------------------------
def test_no_rows_and_argument_errors():
    dw = dev_world()
    out = dw.topp_batch(np.zeros((0, 40, 7)), np.zeros(0, np.int32), T.VMAX, T.AMAX, return_grid=True)
    assert out[0].shape == (0, 256) and out[1].shape == (0, 256, 7) and out[7].shape == (0, 313)
    out = world().topp_batch(np.zeros((0, 40, 7)), np.zeros(0, np.int32), T.VMAX, T.AMAX)
    assert len(out) == 7 and out[1].shape == (0, 256, 7)
    L, h = C.lib(), dw.handle
    P_ = ctypes.c_void_p
    vel, acc = T.VMAX.copy(), T.AMAX.copy()
    vp, ap = P_(vel.ctypes.data), P_(acc.ctypes.data)

    def call(rows=0, mw=40, o=None, v=vp, a=ap, bufs=None, mem=C.MPG_MEM_HOST, world=h):
        o = C.ToppOptions(0.1, 8, 100, 256) if o is None else o
        bufs = [None] * 9 if bufs is None else bufs
        rc = L.mpg_topp_batch(world, bufs[0], bufs[1], rows, mw, v, a, ctypes.byref(o), *bufs[2:9], None, None, mem, None)
        return rc, L.mpg_last_error().decode()

    assert call()[0] == C.MPG_OK
    assert L.mpg_topp_batch(h, None, None, 0, 40, vp, ap, None, *([None] * 9), C.MPG_MEM_DEVICE, None) == C.MPG_OK
    assert call(world=None) == (C.MPG_E_INVALID, "world is NULL")
    assert call(rows=-1) == (C.MPG_E_INVALID, "rows < 0")
    assert call(mem=7)[0] == C.MPG_E_INVALID
    for o, msg in ((C.ToppOptions(0.0, 8, 100, 256), "step must be > 0"),
                   (C.ToppOptions(0.1, 0, 100, 256), "grid_per_segment outside [1, 64]"),
                   (C.ToppOptions(0.1, 65, 100, 256), "grid_per_segment outside [1, 64]"),
                   (C.ToppOptions(0.1, 8, 1, 256), "min_grid outside [2, 65536]"),
                   (C.ToppOptions(0.1, 8, 65537, 256), "min_grid outside [2, 65536]"),
                   (C.ToppOptions(0.1, 8, 100, 0), "max_samples outside [1, 65536]"),
                   (C.ToppOptions(0.1, 8, 100, 65537), "max_samples outside [1, 65536]")):
        assert call(o=o) == (C.MPG_E_INVALID, msg)
    for mw in (1, 4097):
        assert call(mw=mw) == (C.MPG_E_INVALID, "max_waypoints outside [2, 4096]")
    assert call(v=None) == (C.MPG_E_INVALID, "vel_limits / acc_limits is NULL")
    vel[3] = np.inf
    assert call() == (C.MPG_E_INVALID, "vel_limits[3] must be finite and > 0")
    vel[3] = T.VMAX[3]
    acc[0] = 0.0
    assert call() == (C.MPG_E_INVALID, "acc_limits[0] must be finite and > 0")
    acc[0] = T.AMAX[0]
    assert call(rows=(1 << 31) // (4096 * 7) + 1, mw=4096) == (C.MPG_E_INVALID, "rows * max_waypoints * dof exceeds 2^31")
    assert call(rows=4682, mw=2, o=C.ToppOptions(0.1, 8, 2, 65536)) == (
        C.MPG_E_INVALID, "rows * max_samples * dof exceeds 2^31")
    assert call(rows=32768, mw=2, o=C.ToppOptions(0.1, 8, 65536, 1)) == (C.MPG_E_INVALID, "rows * (Ncap + 1) exceeds 2^31")
    rc, msg = call(rows=1)
    assert rc == C.MPG_E_INVALID and msg.endswith("is NULL")
    with pytest.raises(ValueError):
        dw.topp_batch(np.zeros((1, 40, 6)), np.zeros(1, np.int32), T.VMAX, T.AMAX)
    with pytest.raises(ValueError, match="max_waypoints"):
        dw.topp_batch(np.zeros((1, 1, 7)), np.zeros(1, np.int32), T.VMAX, T.AMAX)
    with pytest.raises(ValueError):
        world().topp_batch(np.zeros((1, 40, 7)), np.zeros(1, np.int32), T.VMAX[:6], T.AMAX)
