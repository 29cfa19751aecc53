"""CPU: the tKnn contract's closed forms (include/geoflink_hip.h, what the kernels compute) against the
literal transcription of the reference's window-based pipeline (tests/tknn_ref.py), the vectorised
whole-window reference against both, a hand-computed vector, the window that tells the contract from
the "global minimum per objID" shortcut, and what needs no device: the argument checks, the kernel id,
the mirror's names."""
import ctypes as C
import math
import random

import numpy as np
import pytest

import spatialflink_amd as sf
from spatialflink_amd import _lib

import tknn_cases as W
import tknn_ref as R


def _random_window(rng, nan):
    """a few objIDs over a few cells around Q, distances on a coarse lattice: ties are the rule"""
    n = rng.randint(1, 40)
    nobj = rng.randint(1, 8)
    obj = np.array([rng.randint(0, nobj - 1) * 5 - 7 for _ in range(n)], np.int64)
    x = np.array([W.Q[0] + rng.randint(-3, 3) * W.CL / 2 for _ in range(n)])
    y = np.array([W.Q[1] + rng.randint(-3, 3) * W.CL / 2 for _ in range(n)])
    if nan:
        for i in range(n):
            if rng.random() < 0.15:
                (x if rng.random() < 0.5 else y)[i] = math.nan
    ts = np.arange(n, dtype=np.int64)
    return x, y, obj, ts


def _tables(x, y, obj, r, naive):
    g = W.grid()
    cx, cy = R.cells_of(g, x, y)
    d = R.distances(W.Q[0], W.Q[1], x, y)
    mask = R.cell_mask(g, cx, cy, W.Q[0], W.Q[1], r, naive)
    return R.window_tables(cx, cy, obj, d, mask)


def _same(a, b):
    return len(a) == len(b) and all(p[0] == q[0] and R.cmp_key(p[1]) == R.cmp_key(q[1]) for p, q in zip(a, b))


def test_closed_forms_match_the_naive_loop_under_shuffled_record_orders():
    rng = random.Random(20241020)
    for _ in range(1500):
        x, y, obj, ts = _random_window(rng, nan=False)
        k = rng.choice([1, 2, 3, 50])
        cell_points, traj_len, rank = _tables(x, y, obj, 0.0, True)
        clo = R.tknn_closed(cell_points, traj_len, rank, k)
        cells = list(cell_points)
        for _ in range(3):
            rng.shuffle(cells)
            lit = R.tknn_loop(cell_points, cells, traj_len, rank, k, naive=True)
            assert _same(lit, clo), (x, y, obj, k)
            assert [e[2] for e in lit] == [c * traj_len[o] for o, _, c in clo]  # the LineString: cells_t x len_t


def test_grid_distance_is_the_loop_value_when_the_nearest_cell_arrives_first():
    rng = random.Random(20241021)
    for _ in range(800):
        x, y, obj, ts = _random_window(rng, nan=True)
        k = rng.choice([1, 2, 50])
        cell_points, traj_len, rank = _tables(x, y, obj, rng.choice([0.0, W.R1, W.R2]), False)
        lists = {c: R.cell_apply(p, k, rank) for c, p in cell_points.items()}
        for o, D, ncells in R.tknn_closed(cell_points, traj_len, rank, k):
            holding = [c for c, l in lists.items() if any(e[0] == o for e in l)]
            assert len(holding) == ncells
            near = min(holding, key=lambda c: R.cmp_key(dict(lists[c])[o]))
            order = [near] + [c for c in cell_points if c != near]
            # "the first record to arrive" is D_t under this order (the final cut lifted to see every objID)
            lit = {e[0]: e for e in R.tknn_loop(cell_points, order, traj_len, rank, k, naive=False, k_final=1 << 30)}
            assert R.cmp_key(lit[o][1]) == R.cmp_key(D) and lit[o][2] == ncells * traj_len[o]


def test_vectorised_reference_matches_the_closed_forms():
    rng = random.Random(20241022)
    g = W.grid()
    for _ in range(600):
        x, y, obj, ts = _random_window(rng, nan=True)
        k = rng.choice([1, 2, 3, 50])
        r = rng.choice([0.0, W.R1, W.R2])
        naive = rng.random() < 0.4
        cell_points, traj_len, rank = _tables(x, y, obj, r, naive)
        clo = R.tknn_closed(cell_points, traj_len, rank, k)
        ref = R.tknn_ref(g, x, y, obj, ts, W.Q[0], W.Q[1], r, k, naive)
        assert ref["keys"].tolist() == [e[0] for e in clo]
        assert ref["dist"].view(np.int64).tolist() == np.array([e[1] for e in clo], np.float64).view(np.int64).tolist()
        assert ref["cells"].tolist() == [e[2] for e in clo]
        assert ref["in_cells"] == sum(len(p) for p in cell_points.values())
        assert ref["pairs"] == sum(len({o for o, _ in p}) for p in cell_points.values())
        for j, o in enumerate(ref["keys"].tolist()):
            assert ref["idx"][ref["off"][j]:ref["off"][j + 1]].tolist() == np.flatnonzero(obj == o).tolist()


@pytest.mark.parametrize("k", [2, 3])
def test_hand_vector(k):
    x, y, obj, ts = W.window("hand12")[:4]
    ref = W.expected("hand12", W.Q[0], W.Q[1], W.R2, k, False)
    rows = W.HAND12_ROWS[k]
    assert ref["keys"].tolist() == [r[0] for r in rows]
    assert ref["cells"].tolist() == [r[2] for r in rows]
    assert ref["dist"].tolist() == [math.sqrt((W.Q[1] - y[r[1]]) * (W.Q[1] - y[r[1]]) + (W.Q[0] - x[r[1]]) * (W.Q[0] - x[r[1]]))
                                    for r in rows]
    assert ref["idx"].tolist() == [i for r in rows for i in r[3]]
    assert ref["off"].tolist() == np.r_[0, np.cumsum([len(r[3]) for r in rows])].tolist()
    assert (ref["in_cells"], ref["pairs"]) == (9, 7)
    assert ref["records"] == {2: 5, 3: 7}[k]


def _shortcut(x, y, obj, mask, d, k):
    """NOT the contract: the global minimum per objID over N, then the top k of the multi-point objIDs"""
    best = {}
    for i in np.flatnonzero(mask).tolist():
        best[int(obj[i])] = min(best.get(int(obj[i]), math.inf), float(d[i]))
    multi = [(v, o) for o, v in best.items() if (obj == o).sum() >= 2]
    return [(o, v) for v, o in sorted(multi)[:k]]


def test_truncation_window_differs_from_the_global_minimum_shortcut():
    x, y, obj, ts, cx, cy, _ = W.window("truncate")
    k = 4
    ref = W.expected("truncate", W.Q[0], W.Q[1], W.R2, k, False)
    d = R.distances(W.Q[0], W.Q[1], x, y)
    far = float(d[(obj == 1) & (cx == 48)][0])
    # C, then A by its FAR cell's distance with one cell; B (only in the near cell) is absent
    assert ref["keys"].tolist() == [3, 1] and ref["cells"].tolist() == [1, 1]
    assert ref["dist"][1] == far and far > float(d[(obj == 1) & (cx == 47)][0])
    short = _shortcut(x, y, obj, R.cell_mask(W.grid(), cx, cy, W.Q[0], W.Q[1], W.R2, False), d, k)
    assert [o for o, _ in short] == [1, 2, 3]
    assert short != list(zip(ref["keys"].tolist(), ref["dist"].tolist()))


def _pts(n, x=1, y=1, objid=1, ts=1):
    return _lib.GfPoints(x, y, objid, ts, n)


def test_entry_points_reject_bad_arguments_without_a_device():
    L = _lib.lib()
    h = C.c_void_p()
    g = W.grid().c_grid
    # a null groups object (and with it a null context) is refused first
    assert L.gf_tknn_run(None, C.byref(g), C.byref(_pts(0)), 1.0, 1.0, 1.0, 5, _lib.TKNN_GRID, C.byref(h)) == _lib.GF_ERR_ARG
    assert L.gf_tknn_run(None, C.byref(g), None, 1.0, 1.0, 1.0, 5, _lib.TKNN_NAIVE, C.byref(h)) == _lib.GF_ERR_ARG
    assert L.gf_tknn_run(None, C.byref(g), C.byref(_pts(0)), 1.0, 1.0, 1.0, 0, _lib.TKNN_GRID, C.byref(h)) == _lib.GF_ERR_ARG
    assert L.gf_tknn_run(None, C.byref(g), C.byref(_pts(0)), math.nan, 1.0, 1.0, 5, _lib.TKNN_GRID, C.byref(h)) == _lib.GF_ERR_ARG
    assert L.gf_tknn_run(None, C.byref(g), C.byref(_pts(0)), 1.0, 1.0, -1.0, 5, _lib.TKNN_GRID, C.byref(h)) == _lib.GF_ERR_ARG
    assert h.value is None
    c = [C.c_int64() for _ in range(5)]
    assert L.gf_tknn_info(None, *(C.byref(v) for v in c)) == _lib.GF_ERR_ARG
    assert L.gf_tknn_read(None, None, None, None, None, 0, None, None, None, None, 0) == _lib.GF_ERR_ARG
    assert L.gf_tknn_set_thresholds(None, 2) == _lib.GF_ERR_ARG
    L.gf_tknn_destroy(None)  # a no-op


def test_kernel_id_and_mirror_are_exported():
    assert _lib.K_TKNN == 16
    assert (_lib.TKNN_GRID, _lib.TKNN_NAIVE) == (0, 1)
    for name in ("PointPointTKNNQuery", "TKNNResult"):
        assert hasattr(sf, name) and name in sf.__all__
    assert hasattr(sf.TrajectoryGroups, "tknn")
    for m in ("objid_strings", "tuples", "linestrings"):
        assert hasattr(sf.TKNNResult, m)


@pytest.mark.parametrize("qt", [sf.QueryType.RealTime, sf.QueryType.CountBased, sf.QueryType.RealTimeNaive])
def test_tknn_is_window_based_only(qt):
    q = sf.PointPointTKNNQuery(sf.QueryConfiguration(qt), W.grid())
    with pytest.raises(ValueError, match="Not yet support"):
        q.run(None, None, 0.1, 3)
    with pytest.raises(ValueError, match="Not yet support"):
        q.runNaive(None, None, 0.1, 3)
