"""GPU: the window-based tKnn -- gf_tknn_run / gf_tknn_read through TrajectoryGroups.tknn and
PointPointTKNNQuery -- against the restatement of tests/tknn_ref.py.  Everything is compared exactly:
keys, the distances' bit patterns, cells_t, the CSR, the order, and gf_tknn_info's counters.  The windows
(tests/tknn_cases.py) are the smallest that reach every path: a wave boundary, the truncation that tells
the contract from a global minimum, bit-equal distances across rank k, one cell over ~5k objIDs (both
sides of the big-cell threshold, k larger than a block), one (cell, objID) pair holding 95 % of the
window, and 200k points of every kind of key with out-of-grid and non-finite coordinates."""
import ctypes as C
import math

import numpy as np
import pytest

import spatialflink_amd as sf
from spatialflink_amd import _lib

import tknn_cases as W

pytestmark = pytest.mark.gpu

COLS = ("keys", "dist", "cells", "off", "x", "y", "ts", "idx")
# mix200k's queries: (qx, qy, r, naive).  The population lives in cells 30 .. 60 of both axes.
MIX = {
    "inside_L1": (116.45, 40.27, W.R1, False),
    "inside_L2": (116.45, 40.27, W.R2, False),
    "corner_clipped": (115.5005, 39.6005, 0.021 * 34.5, False),  # cell (0, 0), L = 35: N is clipped to 0 .. 35
    "outside_empty": (115.0, 39.0, W.R2, False),                 # cell (-24, -29), L = 2: N is empty
    "outside_clipped": (115.0, 39.0, 0.021 * 59.5, False),       # L = 60: N = 0 .. 36 x 0 .. 31
    "r0_all_cells": (116.45, 40.27, 0.0, False),
    "naive": (116.45, 40.27, W.R2, True),
}


def device_window(name):
    x, y, obj, ts = (a.copy() for a in W.window(name)[:4])  # (the shared arrays are read-only)
    return sf.PointWindow.from_numpy(x, y, obj, ts, start=1_000, end=11_000)


def as_bytes(res):
    return b"".join(np.ascontiguousarray(getattr(res, "objID" if c == "keys" else c)).tobytes() for c in COLS)


def check(res, exp):
    """a TKNNResult against tknn_ref's dict, exactly; -> the result's bytes"""
    info = res.info
    assert (info["in_cells"], info["pairs"], info["records"]) == (exp["in_cells"], exp["pairs"], exp["records"])
    assert (info["rows"], info["npts"]) == (len(exp["keys"]), len(exp["idx"]))
    for c in COLS:
        got = getattr(res, "objID" if c == "keys" else c)
        assert got.dtype == exp[c].dtype, c
        a, b = (got.view(np.int64), exp[c].view(np.int64)) if got.dtype == np.float64 else (got, exp[c])
        np.testing.assert_array_equal(a, b, err_msg=c)
    return as_bytes(res)


def run_and_check(g, name, q, k, **kw):
    qx, qy, r, naive = q
    exp = W.expected(name, qx, qy, r, k, naive)
    return check(g.tknn(W.grid(), sf.Point("q", qx, qy, 0), r, k, naive=naive, **kw), exp), exp


QG = (W.Q[0], W.Q[1], W.R2, False)


@pytest.mark.parametrize("k", [2, 3])
def test_hand_vector(gpu, k):
    g = sf.TrajectoryGroups(device_window("hand12"))
    _, exp = run_and_check(g, "hand12", QG, k)
    assert exp["keys"].tolist() == [r[0] for r in W.HAND12_ROWS[k]]
    assert exp["cells"].tolist() == [r[2] for r in W.HAND12_ROWS[k]]
    assert exp["idx"].tolist() == [i for r in W.HAND12_ROWS[k] for i in r[3]]
    g.close()


@pytest.mark.parametrize("k", [3, 64])
def test_one_cell_of_65_trajectories_crosses_a_wave(gpu, k):
    g = sf.TrajectoryGroups(device_window("wave65"))
    _, exp = run_and_check(g, "wave65", QG, k)
    assert (exp["pairs"], exp["records"], len(exp["keys"])) == (65, k, k)
    g.close()


def test_truncation_happens_before_the_size_rule(gpu):
    g = sf.TrajectoryGroups(device_window("truncate"))
    _, exp = run_and_check(g, "truncate", QG, 4)
    assert exp["keys"].tolist() == [3, 1] and exp["cells"].tolist() == [1, 1]  # (test_tknn_ref.py: not the shortcut's rows)
    g.close()


@pytest.mark.parametrize("k", [3, 9])
def test_bit_equal_distances_are_ordered_by_trajectory_rank(gpu, k):
    x, y, obj = W.window("ties")[:3]
    d = W.R.distances(W.Q[0], W.Q[1], x, y).view(np.int64)
    near = d[(np.abs(x - W.Q[0]) < 0.01) & (np.abs(y - W.Q[1]) < 0.01)]
    side = d[(np.abs(np.abs(x - W.Q[0]) - 2.0 ** -6) < 1e-9)]
    assert len(set(near.tolist())) == 1 and len(near) == 10 and len(set(side.tolist())) == 1 and len(side) == 8
    g = sf.TrajectoryGroups(device_window("ties"))
    _, exp = run_and_check(g, "ties", QG, k)
    keys = W.window("ties")[6][0].tolist()  # first-occurrence order
    rank = [keys.index(o) for o in exp["keys"].tolist()]
    if k == 3:  # the query cell's 7 tied pairs straddle rank k
        assert len(set(exp["dist"].view(np.int64).tolist())) == 1 and rank == sorted(rank)
    else:  # all 7, then 2 of the 4 tied trajectories of the side cells: the final cut straddles the tie
        assert len(exp["keys"]) == 9 and exp["dist"].view(np.int64)[7] == exp["dist"].view(np.int64)[8] == side[0]
        assert rank[:7] == sorted(rank[:7]) and rank[7:] == sorted(rank[7:])
    g.close()


def test_one_hot_cell_on_both_sides_of_the_big_cell_threshold(gpu):
    g = sf.TrajectoryGroups(device_window("hotcell20k"))
    for k in (50, 3000):
        seen = set()
        b, exp = run_and_check(g, "hotcell20k", QG, k)  # the default: the cell is big (sorted)
        assert exp["pairs"] > 4000 and len(set(zip(exp["pair_cx"].tolist(), exp["pair_cy"].tolist()))) == 1
        assert exp["records"] == k and len(exp["keys"]) > 0.9 * k
        seen.add(b)
        for big_cell in (1 << 31, 2, 0):  # counted inside the cell by every pair; sorted; the default again
            seen.add(run_and_check(g, "hotcell20k", QG, k, big_cell=big_cell)[0])
        assert len(seen) == 1
    g.close()


def test_one_pair_holding_most_of_the_window(gpu):
    x, y, obj = W.window("hotpair20k")[:3]
    hot = obj == 7
    d = W.R.distances(W.Q[0], W.Q[1], x, y)
    assert hot.sum() > 18_000 and (d[hot] == d[hot].min()).sum() > 10  # its minimum is held by many points
    g = sf.TrajectoryGroups(device_window("hotpair20k"))
    for k in (1, 5, 100):
        run_and_check(g, "hotpair20k", QG, k)
    run_and_check(g, "hotpair20k", (W.Q[0], W.Q[1], 0.0, False), 100)
    run_and_check(g, "hotpair20k", (W.Q[0], W.Q[1], 0.0, True), 100)
    g.close()


@pytest.mark.parametrize("case", list(MIX))
def test_mixed_window(gpu, case):
    q = MIX[case]
    g = sf.TrajectoryGroups(device_window("mix200k"))
    for k in (1, 50, 5000):
        _, exp = run_and_check(g, "mix200k", q, k)
    if case == "outside_empty":
        assert exp["in_cells"] == 0 and len(exp["keys"]) == 0
    else:
        assert exp["in_cells"] > 1000 and 0 < len(exp["keys"]) and exp["cells"].max() > 1
    if case in ("inside_L1", "inside_L2"):
        assert len(exp["keys"]) < 5000  # k = 5000 exceeds the survivors
    if case in ("r0_all_cells", "naive", "outside_clipped", "corner_clipped"):
        col0 = (exp["pair_cx"] == 0) | (exp["pair_cy"] == 0)  # NaN coordinates have cell 0
        assert (exp["pair_first_nan"] & col0).sum() >= 6 and (exp["pair_later_nan"] & col0).sum() >= 6
    if case == "naive":
        n = 100
        out = (exp["pair_cx"] < 0) | (exp["pair_cx"] >= n) | (exp["pair_cy"] < 0) | (exp["pair_cy"] >= n)
        assert out.sum() > 1000  # out-of-grid cells are cells of N
        keys = set(W.window("mix200k")[2].tolist())
        assert {_lib.OBJID_NULL, W.EMPTY_MARK, W.I64_MIN} <= keys
    g.close()


def test_big_cell_threshold_at_forcing_values(gpu):
    g = sf.TrajectoryGroups(device_window("mix200k"))
    q = MIX["r0_all_cells"]
    a, exp = run_and_check(g, "mix200k", q, 50)
    cells, sizes = np.unique(np.stack([exp["pair_cx"], exp["pair_cy"]], 1), axis=0, return_counts=True)
    assert sizes.min() < 2 and 150 <= sizes.max() < 512  # both sides of 2 and of 150 are populated; the default: none big
    assert run_and_check(g, "mix200k", q, 50, big_cell=2)[0] == a        # cells of one pair counted, the others sorted
    assert run_and_check(g, "mix200k", q, 50, big_cell=150)[0] == a
    assert run_and_check(g, "mix200k", q, 50, big_cell=1)[0] == a        # every cell sorted
    assert run_and_check(g, "mix200k", q, 50, big_cell=1 << 31)[0] == a  # every cell counted
    with pytest.raises(ValueError):
        g.tknn(W.grid(), sf.Point("q", q[0], q[1], 0), q[2], 50, big_cell=-1)
    g.close()


def test_runs_are_byte_identical(gpu):
    q = MIX["r0_all_cells"]
    g = sf.TrajectoryGroups(device_window("mix200k"))
    a = run_and_check(g, "mix200k", q, 50)[0]
    assert run_and_check(g, "mix200k", q, 50)[0] == a
    g.close()
    fresh = sf.TrajectoryGroups(device_window("mix200k"))
    assert run_and_check(fresh, "mix200k", q, 50)[0] == a
    fresh.close()


def test_a_second_window_through_the_same_objects(gpu):
    g = sf.TrajectoryGroups(device_window("mix200k"))
    run_and_check(g, "mix200k", MIX["naive"], 50)
    g.regroup(device_window("hotcell20k"))
    run_and_check(g, "hotcell20k", QG, 50)
    g.regroup(device_window("hand12"))
    run_and_check(g, "hand12", QG, 3)
    g.regroup(device_window("mix200k"))
    run_and_check(g, "mix200k", MIX["inside_L2"], 50)
    g.close()


def test_small_capacities_return_the_full_counts_and_a_prefix(gpu):
    g = sf.TrajectoryGroups(device_window("wave65"))
    exp = W.expected("wave65", *QG[:3], 10, False)
    res = g.tknn(W.grid(), sf.Point("q", *W.Q, 0), W.R2, 10, cap_rows=4, cap_pts=5)
    assert (res.info["rows"], res.info["npts"]) == (10, 20)
    np.testing.assert_array_equal(res.objID, exp["keys"][:4])
    np.testing.assert_array_equal(res.off, exp["off"][:5])
    np.testing.assert_array_equal(res.idx, exp["idx"][:5])
    # the arrays past the capacities stay untouched
    L = _lib.lib()
    keys, idx = np.full(10, -7, np.int64), np.full(20, 77, np.uint32)
    assert L.gf_tknn_read(g._tknn, keys.ctypes.data, None, None, None, 4, None, None, None, idx.ctypes.data, 5) == _lib.GF_OK
    assert keys[4:].tolist() == [-7] * 6 and idx[5:].tolist() == [77] * 15 and keys[:4].tolist() == exp["keys"][:4].tolist()
    g.close()


def test_candidate_layers_of_zero_are_refused(gpu):
    # ceil(r / cellLength) is 0 only where the quotient underflows: not on the Beijing grid (cell length < 1)
    coarse = sf.UniformGrid(10, 0.0, 100.0, 0.0, 100.0)
    assert coarse.getCandidateNeighboringLayers(5e-324) == 0
    g = sf.TrajectoryGroups(device_window("hand12"))
    with pytest.raises(_lib.CandidateLayersError):
        g.tknn(coarse, sf.Point("q", 50.0, 50.0, 0), 5e-324, 3)
    x, y, obj, ts = W.window("hand12")[:4]  # NAIVE never asks for layers
    check(g.tknn(coarse, sf.Point("q", 50.0, 50.0, 0), 5e-324, 3, naive=True),
          W.R.tknn_ref(coarse, x, y, obj, ts, 50.0, 50.0, 5e-324, 3, naive=True))
    g.close()


def test_empty_window_and_empty_cell_set(gpu):
    e = np.empty(0)
    g = sf.TrajectoryGroups(sf.PointWindow.from_numpy(e, e, e.astype(np.int64), e.astype(np.int64)))
    for naive in (False, True):
        res = g.tknn(W.grid(), sf.Point("q", *W.Q, 0), W.R2, 5, naive=naive)
        assert len(res) == 0 and res.off.tolist() == [0] and res.info["in_cells"] == 0 and res.tuples() == []
    g.regroup(device_window("hand12"))
    res = g.tknn(W.grid(), sf.Point("q", 115.0, 39.0, 0), W.R2, 5)  # the query far outside: no cell of N is valid
    assert len(res) == 0 and res.info == dict(rows=0, npts=0, in_cells=0, pairs=0, records=0)
    res = g.tknn(W.grid(), sf.Point("q", 0.0, 0.0, 0), W.R2, 5)  # every point outside N
    assert len(res) == 0 and res.info["in_cells"] == 0
    g.close()


def test_query_mirror_end_to_end(gpu):
    grid = W.grid()
    pts = [sf.Point("bus-7", 116.5, 40.002, 10), sf.Point("12", 116.5, 40.001, 50), sf.Point("bus-7", 116.51, 40.0, 40),
           sf.Point("tram", 116.5, 40.0005, 5), sf.Point("12", 117.0, 40.5, 60), sf.Point("bus-7", 115.0, 39.0, 70)]
    w = sf.PointWindow.from_points(pts, start=0, end=10_000)
    qp = sf.Point("q", *W.Q, 0)
    q = sf.PointPointTKNNQuery(sf.QueryConfiguration(sf.QueryType.WindowBased), grid)
    res = q.run(w, qp, W.R2, 2)
    # the query cell's list is (tram, 12): bus-7 is cut there and keeps its cell (48, 19) distance
    assert res.objid_strings() == ["12", "bus-7"] and res.cells.tolist() == [1, 1]
    assert res.tuples() == [("12", math.sqrt((40.0 - 40.001) * (40.0 - 40.001))),
                            ("bus-7", math.sqrt((116.5 - 116.51) * (116.5 - 116.51)))]
    assert res.linestrings() == [[(116.5, 40.001), (117.0, 40.5)], [(116.5, 40.002), (116.51, 40.0), (115.0, 39.0)]]
    assert res.ts.tolist() == [50, 60, 10, 40, 70] and res.idx.tolist() == [1, 4, 0, 2, 5]
    res = q.run(w, qp, W.R2, 3)
    assert res.objid_strings() == ["12", "bus-7"] and res.cells.tolist() == [1, 2]
    assert [len(l) for l in res.linestrings(repeat=True)] == (res.cells * np.diff(res.off)).tolist() == [2, 6]
    nv = q.runNaive(w, qp, W.R2, 3)
    assert nv.objid_strings() == ["12", "bus-7"] and nv.cells.tolist() == [2, 3]  # the far cells are cells of N too
    g = sf.TrajectoryGroups(w)
    assert as_bytes(q.run(w, qp, W.R2, 3, groups=g)) == as_bytes(res)
    g.close()
    with pytest.raises(ValueError, match="Not yet support"):
        sf.PointPointTKNNQuery(sf.QueryConfiguration(sf.QueryType.RealTime), grid).run(w, qp, W.R2, 3)


def test_argument_errors_with_a_device(gpu):
    L = _lib.lib()
    w = device_window("hand12")
    g = sf.TrajectoryGroups(w)
    grid = W.grid().c_grid
    ctx = g.ctx.handle
    h = C.c_void_p()

    def run(pts, qx=W.Q[0], qy=W.Q[1], r=W.R2, k=3, mode=_lib.TKNN_GRID, grid=grid, out=h):
        return L.gf_tknn_run(g.handle, C.byref(grid) if grid is not None else None,
                             C.byref(pts) if pts is not None else None, qx, qy, r, k, mode, C.byref(out))

    for col in ("x", "y", "objID", "ts"):
        bad = w.c_struct()
        setattr(bad, col, None)
        assert run(bad) == _lib.GF_ERR_ARG and b"null x / y / objID / ts" in L.gf_ctx_last_error(ctx)
    pts = w.c_struct()
    assert run(None) == _lib.GF_ERR_ARG and run(pts, grid=None) == _lib.GF_ERR_ARG
    assert run(pts, k=0) == _lib.GF_ERR_ARG and run(pts, k=-5) == _lib.GF_ERR_ARG
    assert run(pts, qx=math.nan) == _lib.GF_ERR_ARG and run(pts, qy=math.nan) == _lib.GF_ERR_ARG
    assert run(pts, r=math.nan) == _lib.GF_ERR_ARG and run(pts, r=-0.5) == _lib.GF_ERR_ARG
    assert run(pts, mode=2) == _lib.GF_ERR_ARG
    flat = _lib.GfGrid(100, 0, 1.0, 1.0, 0.0, 1.0, 0.0)  # cellLength 0
    assert run(pts, grid=flat) == _lib.GF_ERR_ARG
    short = sf.PointWindow.from_numpy(*(a[:5].copy() for a in W.window("hand12")[:4]))
    assert run(short.c_struct()) == _lib.GF_ERR_ARG and b"not the grouped window" in L.gf_ctx_last_error(ctx)
    assert h.value is None
    assert run(pts) == _lib.GF_OK and h.value is not None
    octx, other = _lib.Context(0), C.c_void_p()
    assert L.gf_traj_group(octx.handle, C.byref(pts), C.byref(other)) == _lib.GF_OK
    assert L.gf_tknn_run(other, C.byref(grid), C.byref(pts), W.Q[0], W.Q[1], W.R2, 3, 0, C.byref(h)) == _lib.GF_ERR_ARG
    assert b"another context" in L.gf_ctx_last_error(octx.handle)
    L.gf_traj_groups_destroy(other)
    assert L.gf_tknn_set_thresholds(h, -1) == _lib.GF_ERR_ARG
    assert L.gf_tknn_read(h, None, None, None, None, -1, None, None, None, None, 0) == _lib.GF_ERR_ARG
    rows = C.c_int64()
    assert L.gf_tknn_info(h, C.byref(rows), None, None, None, None) == _lib.GF_OK and rows.value == 3
    L.gf_tknn_destroy(h)
    run_and_check(g, "hand12", QG, 3)  # the groups are still good
    g.close()
