"""CPU: the trajectory entry points (gf_traj_group, gf_tstats_run, gf_traj_select) exist, refuse bad
arguments with GF_ERR_ARG before any device call (no GPU in this container), and the plain-Python
restatement the GPU tests compare against (tests/traj_ref.py) reproduces a hand-computed vector."""
import ctypes as C
import math

import numpy as np
import pytest

import spatialflink_amd as sf
from spatialflink_amd import _lib

import traj_ref as R


def _pts(n, objid=1, ts=1):
    return _lib.GfPoints(None, None, objid, ts, n)


def test_entry_points_reject_bad_arguments_without_a_device():
    L = _lib.lib()
    h = C.c_void_p()
    fake_ctx = None  # a null context is refused first
    assert L.gf_traj_group(fake_ctx, C.byref(_pts(0)), C.byref(h)) == _lib.GF_ERR_ARG
    assert h.value is None
    assert L.gf_traj_group(fake_ctx, None, C.byref(h)) == _lib.GF_ERR_ARG
    assert L.gf_traj_group(fake_ctx, C.byref(_pts(-1)), C.byref(h)) == _lib.GF_ERR_ARG
    assert L.gf_traj_group(fake_ctx, C.byref(_pts(1 << 32)), C.byref(h)) == _lib.GF_ERR_ARG
    assert L.gf_traj_group(fake_ctx, C.byref(_pts(5, objid=None)), C.byref(h)) == _lib.GF_ERR_ARG
    cnt, cnt2 = C.c_int64(), C.c_int64()
    assert L.gf_traj_groups_info(None, C.byref(cnt), C.byref(cnt2)) == _lib.GF_ERR_ARG
    assert L.gf_traj_groups_read(None, None, None, None) == _lib.GF_ERR_ARG
    assert L.gf_traj_groups_set_long_threshold(None, 300) == _lib.GF_ERR_ARG
    assert L.gf_tstats_run(None, C.byref(_pts(0)), None, 0, None, None, None, None, 0, C.byref(cnt)) == _lib.GF_ERR_ARG
    assert L.gf_traj_select(None, C.byref(_pts(0)), None, None, None, 0, None, None, None, None, 0, C.byref(cnt),
                            C.byref(cnt2)) == _lib.GF_ERR_ARG
    L.gf_traj_groups_destroy(None)  # a no-op


def test_kernel_ids_and_mirror_are_exported():
    assert (_lib.K_TRAJ_GROUP, _lib.K_TSTATS, _lib.K_TRAJ_SELECT) == (12, 13, 14)
    for name in ("PointTStatsQuery", "group_by_objid", "sub_trajectories", "TStatsResult", "SubTrajectories"):
        assert hasattr(sf, name) and name in sf.__all__


@pytest.mark.parametrize("qt", [sf.QueryType.RealTime, sf.QueryType.CountBased, sf.QueryType.RealTimeNaive])
def test_tstats_is_window_based_only(qt):
    with pytest.raises(ValueError, match="Not yet support"):
        sf.PointTStatsQuery(sf.QueryConfiguration(qt)).run(None)


def test_restatement_reproduces_the_hand_vector():
    A = [(100, 100, 0), (0, 0, 10), (3, 4, 20), (9, 9, 15), (6, 8, 20), (6, 8, 30)]
    B = [(7, 7, 12)]
    assert R.tstats_one(A) == (10.0, 20, 0.5)  # counted: ts 10, 20, 30 -> 5 + 5; the ts-0 and the late points drop out
    S, T, V = R.tstats_one(B)
    assert (S, T) == (0.0, 0) and math.isnan(V)
    # interleaved, B first in the window: rows B, then A
    rows = [("B", B[0]), ("A", A[0]), ("A", A[1]), ("A", A[2]), ("A", A[3]), ("A", A[4]), ("A", A[5])]
    obj = np.array([{"A": 5, "B": -(1 << 63) + 3}[o] for o, _ in rows], np.int64)
    x = np.array([p[0] for _, p in rows], np.float64)
    y = np.array([p[1] for _, p in rows], np.float64)
    ts = np.array([p[2] for _, p in rows], np.int64)
    keys, off, perm = R.group_ref(obj)
    np.testing.assert_array_equal(keys, [-(1 << 63) + 3, 5])
    np.testing.assert_array_equal(off, [0, 1, 7])
    np.testing.assert_array_equal(perm, [0, 1, 2, 3, 4, 5, 6])
    k, S, T, V = R.tstats_ref(x, y, ts, keys, off, perm)
    assert S.tolist() == [0.0, 10.0] and T.tolist() == [0, 20]
    assert math.isnan(V[0]) and V[1] == 0.5
    # sub-trajectories: a hit on A's fourth point gives A whole, in arrival order
    hit = np.zeros(7, bool)
    hit[4] = True
    sk, so, sx, sy, st, si = R.subtraj_ref(x, y, ts, keys, off, perm, hit)
    assert sk.tolist() == [5] and so.tolist() == [0, 6] and si.tolist() == [1, 2, 3, 4, 5, 6]
    assert st.tolist() == [0, 10, 20, 15, 20, 30]
