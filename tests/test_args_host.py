"""The argument checks and launch set-up the batch entry points share
(mplib_amd/csrc/mpg_args_host.h, compiled for the host by
tests/native/args_host.cpp): pose checks, free_pose / free_rows, sampling
ranges, the common part of an IkView and the LDS formula.  No GPU.
"""
import ctypes

import numpy as np
import pytest

from native.host_shim import args_lib

TOL = 1e-6
OK, NONFINITE, NORM = 0, 1, 2
DP = ctypes.POINTER(ctypes.c_double)


def dp(a):
    return None if a is None else a.ctypes.data_as(DP)


def check_pose7(p, count=None):
    p = np.ascontiguousarray(p, dtype=np.float64)
    count = p.size // 7 if count is None else count
    return args_lib().args_check_pose7(dp(p), ctypes.c_long(count), ctypes.c_double(TOL))


def pose(norm=1.0, slot=3):
    """A pose whose quaternion has one component, `norm`, at `slot` (3..6)."""
    p = np.array([0.1, -0.2, 0.3, 0.0, 0.0, 0.0, 0.0])
    p[slot] = norm
    return p


def message(fault, what):
    buf = ctypes.create_string_buffer(128)
    n = args_lib().args_pose_message(fault, what.encode(), buf, len(buf))
    assert n < len(buf)
    return buf.value.decode()


def test_quaternion_norm_tolerance():
    """Norms 1 +- 1e-6 pass and 1 +- 2e-6 do not, in every quaternion slot.
    The check is |norm - 1| <= 1e-6 with an exact subtraction (the norm is
    within a factor 2 of 1), so it is exact for the double it is given: the
    double 0.999999 itself lies 2.9e-17 outside (1 - 0.999999 =
    1.0000000000287557e-06 > the double 1e-6) and the lower accepted norm is
    its neighbour towards 1, one ulp (1.1e-16) from the decimal; the double
    1.000001 lies inside (1.000001 - 1 = 9.999999999177334e-07)."""
    lower = np.nextafter(1.0 - 1e-6, 1.0)
    assert abs(lower - (1.0 - 1e-6)) <= np.spacing(1.0 - 1e-6)
    for slot in range(3, 7):
        for norm in (lower, 1.0, 1.0 + 1e-6, -1.0):
            assert check_pose7(pose(norm, slot)) == OK, (slot, norm)
        for norm in (1.0 - 2e-6, 1.0 + 2e-6, 0.0):
            assert check_pose7(pose(norm, slot)) == NORM, (slot, norm)
    assert check_pose7([0, 0, 0, 0.5, 0.5, 0.5, 0.5]) == OK


@pytest.mark.parametrize("slot", range(7))
@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_non_finite_value_in_each_slot(slot, bad):
    """The fault is in the second of three poses; the count decides whether it is seen."""
    p = np.stack([pose(), pose(), pose()])
    p[1, slot] = bad
    assert check_pose7(p, 1) == OK
    assert check_pose7(p, 2) == NONFINITE
    assert check_pose7(p) == NONFINITE


def test_no_poses_and_the_reported_reason():
    assert check_pose7(np.zeros(0), 0) == OK
    assert args_lib().args_check_pose7(None, ctypes.c_long(0), ctypes.c_double(TOL)) == OK
    p = np.stack([pose(), pose(0.5), pose()])
    p[2, 0] = np.nan  # the first fault decides
    assert check_pose7(p) == NORM
    assert check_pose7(p[::-1]) == NONFINITE
    assert message(NONFINITE, "free pose") == "non-finite free pose"
    assert message(NONFINITE, "goal pose") == "non-finite goal pose"
    assert message(NORM, "goal pose") == "goal pose quaternion is not of unit norm (within 1e-6)"
    assert "unit norm" in message(NORM, "free pose") and "free pose" in message(NORM, "free pose")


def test_free_columns_of_link_pose_rows():
    """Only the last n_free links of every row are looked at."""
    L, n_links, n_free, n = args_lib(), 4, 2, 3
    rows = np.full((n, n_links, 7), np.nan)
    rows[:, n_links - n_free:] = pose()

    def cols(r, count, free=n_free):
        return L.args_check_free_columns(dp(r), ctypes.c_long(count), n_links, free, ctypes.c_double(TOL))

    assert cols(rows, n) == OK
    assert cols(rows, n, 0) == OK and cols(rows, 0) == OK
    bad = rows.copy()
    bad[2, 3, 5] = np.inf
    assert cols(bad, 2) == OK and cols(bad, 3) == NONFINITE
    bad = rows.copy()
    bad[1, 2, 3] = 1.0 + 2e-6
    assert cols(bad, 1) == OK and cols(bad, 3) == NORM
    assert cols(np.full((n, n_links, 7), np.nan), n, n_links) == NONFINITE


def test_free_rows():
    L, P, n = args_lib(), np.tile(pose(), (10, 1)), 5

    def free_args(p, rows, n_free):
        return L.args_check_free_args(dp(p), ctypes.c_long(rows), ctypes.c_long(n), n_free)

    for rows in (1, n):
        assert free_args(P, rows, 2) is None
    for rows in (0, 2, n + 1):
        assert b"free_rows" in free_args(P, rows, 2), rows
    for rows in (0, 1, 2, n, n + 1):  # no array: free_rows is not looked at
        assert free_args(None, rows, 2) is None and free_args(None, rows, 0) is None
    assert b"no free frames" in free_args(P, 1, 0)
    assert b"free_rows" in free_args(P, 3, 0)  # the row count is refused first


def fill_range(lower, upper, dof):
    lo, hi = np.full(64, 7.0), np.full(64, 7.0)
    lower, upper = (None if a is None else np.ascontiguousarray(a, dtype=np.float64) for a in (lower, upper))
    why = args_lib().args_fill_sample_range(dp(lower), dp(upper), dof, dp(lo), dp(hi))
    return why, lo, hi


def test_sampling_ranges():
    why, lo, hi = fill_range(None, None, 0)
    assert why is None and not lo.any() and not hi.any()
    lower, upper = -np.arange(1.0, 65.0), np.arange(1.0, 65.0)
    why, lo, hi = fill_range(lower, upper, 64)
    assert why is None and np.array_equal(lo, lower) and np.array_equal(hi, upper)
    why, lo, hi = fill_range(lower, upper, 3)
    assert why is None and np.array_equal(lo[:3], lower[:3]) and not lo[3:].any() and not hi[3:].any()
    assert fill_range(lower, upper, 65)[0] is not None and fill_range(lower, upper, -1)[0] is not None
    why, lo, hi = fill_range([0.5, 2.0], [0.5, 3.0], 2)  # lo == hi
    assert why is None and lo[0] == hi[0] == 0.5
    assert b"lower <= upper" in fill_range([0.0, 2.0], [1.0, 1.0], 2)[0]
    assert fill_range([0.0, 2.0], [1.0, 1.0], 1)[0] is None  # the fault is past dof
    for bad in (np.inf, -np.inf, np.nan):
        assert b"finite" in fill_range([0.0, 0.0], [1.0, bad], 2)[0]
        assert b"finite" in fill_range([bad, 0.0], [1.0, 1.0], 2)[0]


def test_common_ik_view_fill():
    """Two links; link 1 hangs under joints 1, 2, 3, of which joint 2 is a
    mimic (no dof slot: source -1), and slot 1 (joint 3) has no lower limit.
    The expected view is written out by hand."""
    L = args_lib()
    ia = lambda v: np.array(v, np.int32)  # noqa: E731
    cs, cl, cj, src = ia([0, 1]), ia([1, 3]), ia([1, 1, 2, 3]), ia([0, -1, 1])
    lo, hi, kind = np.array([-1.0, -np.inf]), np.array([1.0, 2.0]), np.array([1, 2], np.uint8)
    ip = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731

    def view(link, mask):
        head = np.zeros(3, np.int32)
        move = np.full(16, 9, np.uint8)
        k, b, f = (np.full(32, 9, np.uint8) for _ in range(3))
        vlo, vhi = np.full(32, 9.0), np.full(32, 9.0)
        L.args_fill_ik_view(ip(cs), ip(cl), ip(cj), ip(src), dp(lo), dp(hi), ip(kind), link, 2, ip(mask), ip(head),
                            ip(move), ip(k), ip(b), ip(f), dp(vlo), dp(vhi))
        return [a.tolist() for a in (head, move[:3], k[:2], b[:2], f[:2], vlo[:2], vhi[:2])]

    limits = [[-1.0, -np.inf], [1.0, 2.0]]
    assert view(1, None) == [[1, 1, 3], [1, 0, 1], [1, 2], [1, 0], [0, 0]] + limits
    assert view(1, np.array([0, 1], np.uint8)) == [[1, 1, 3], [1, 0, 0], [1, 2], [1, 0], [0, 1]] + limits
    assert view(1, np.array([1, 0], np.uint8))[1] == [0, 0, 1]
    head, move = view(0, None)[:2]
    assert head == [0, 0, 1] and move[0] == 1


def test_lds_bytes_and_mem_kind():
    """Per chain joint 8 slots of 64 lanes and 16 table doubles, 3 table ints:
    8 * 528 + 12 bytes; an empty chain counts as one joint."""
    L = args_lib()
    assert [L.args_ik_lds_bytes(cl) for cl in (0, 1, 7, 15)] == [4236, 4236, 7 * 4236, 15 * 4236]
    assert [L.args_mem_ok(m) for m in (0, 1, -1, 2)] == [1, 1, 0, 0]
