"""CPU: the tJoin contract's closed form (include/geoflink_hip.h, what the kernels compute) against the
literal walk of the reference's window-based pipeline (tests/tjoin_ref.py) on random small windows, the
closed form fed the C oracle's point-point join pairs against the same walk, the hand vector, and what
needs no device: the argument checks, the kernel id, the mirror's names."""
import ctypes as C
import math
import random

import numpy as np
import pytest

import spatialflink_amd as sf
from spatialflink_amd import _lib

import tjoin_cases as W
import tjoin_ref as R

RADII = (0.0, 0.5, 0.75, 1.0, 1.5)  # r == 0; L = 1 (0.75 and 1.0 are lattice distances: exact ties with r); L = 2


def _random_window(rng, nobj):
    """<= 60 points on a quarter-cell lattice reaching outside the 8 x 8 grid: ts ties, single-point
    trajectories, out-of-grid and NaN coordinates"""
    n = rng.randint(0, 60)
    obj = np.array([rng.randint(0, nobj - 1) * 5 - 7 for _ in range(n)], np.int64)
    for i in range(n):
        if rng.random() < 0.05:
            obj[i] = 1000 + i  # an objID of its own: a single-point trajectory
    x = np.array([rng.randint(-6, 38) * 0.25 for _ in range(n)], np.float64)
    y = np.array([rng.randint(-6, 38) * 0.25 for _ in range(n)], np.float64)
    for i in range(n):
        if rng.random() < 0.05:
            (x if rng.random() < 0.5 else y)[i] = math.nan
    ts = np.array([rng.randint(0, 6) for _ in range(n)], np.int64)
    return x, y, obj, ts


def _brute_pairs(grid, O, Q, r):
    """the matching point pairs of section 1, pair by pair"""
    n = grid.getNumGridPartitions()
    L = None if r == 0 else grid.getCandidateNeighboringLayers(r)
    oc = [grid.cellOf(a, b) for a, b in zip(O[0].tolist(), O[1].tolist())]
    qc = [grid.cellOf(a, b) for a, b in zip(Q[0].tolist(), Q[1].tolist())]
    out = []
    for i, (cx, cy) in enumerate(oc):
        if not (0 <= cx < n and 0 <= cy < n):
            continue
        for j, (ax, ay) in enumerate(qc):
            if L is not None and (abs(ax - cx) > L or abs(ay - cy) > L):
                continue
            if R.distance(O[0][i], O[1][i], Q[0][j], Q[1][j]) <= r:
                out.append((i, j))
    return np.array(out, np.int64).reshape(-1, 2)


def _agree(grid, O, Q, r, single, pairs):
    clo = R.tjoin_closed(pairs, O, Q, single)
    rows = list(zip(clo["okey"].tolist(), clo["qkey"].tolist()))
    # tuples in the query window's order: the row set with each row's kept query point
    point_rows, traj_rows, _ = R.tjoin_loop(grid, O, Q, r, single, order="query")
    assert sorted((a, b, j) for a, b, _, j in point_rows) == sorted((a, b, j) for (a, b), j in zip(rows, clo["q_latest"].tolist()))
    # tuples in the ordinary window's order: firstPoint per ordinary objID; the same rows, the kept point's ts too
    point_rows2, traj_rows2, first = R.tjoin_loop(grid, O, Q, r, single, order="ordinary")
    assert first == R.first_point(clo)
    assert all(f == first[a] for a, _, f, _ in point_rows2)
    qts = np.asarray(Q[3]).tolist()
    assert sorted((a, b, qts[j]) for a, b, _, j in point_rows2) == sorted((a, b, qts[j]) for a, b, _, j in point_rows)
    assert sorted(traj_rows2) == sorted(traj_rows)
    # the emitted pairs
    assert sorted(traj_rows) == sorted(rw for rw, e in zip(rows, clo["emit"].tolist()) if e)
    assert len(rows) == len(set(rows)) == clo["rows"]
    for side, slot, window in (("ordinary", "oslot", O), ("query", "qslot", Q)):
        csr = clo[side]
        for u, k in enumerate(csr["keys"].tolist()):  # whole, once, in arrival order
            assert csr["idx"][csr["off"][u]:csr["off"][u + 1]].tolist() == np.flatnonzero(window[2] == k).tolist()
        keys_of_rows = clo["okey" if side == "ordinary" else "qkey"]
        assert all(csr["keys"][s] == k for s, k, e in zip(clo[slot].tolist(), keys_of_rows.tolist(), clo["emit"].tolist()) if e)
        assert all(s == -1 for s, e in zip(clo[slot].tolist(), clo["emit"].tolist()) if not e)
    return clo


def test_closed_form_matches_the_literal_walk_on_random_windows():
    rng = random.Random(20261020)
    g = W.small_grid()
    seen_rows = seen_unemitted = 0
    for _ in range(300):
        O, Q = _random_window(rng, rng.randint(1, 7)), _random_window(rng, rng.randint(1, 7))
        r = rng.choice(RADII)
        clo = _agree(g, O, Q, r, False, _brute_pairs(g, O, Q, r))
        seen_rows += clo["rows"]
        seen_unemitted += clo["rows"] - clo["emitted"]
    assert seen_rows > 1000 and seen_unemitted > 50


def test_closed_form_matches_the_literal_walk_single():
    rng = random.Random(20261021)
    g = W.small_grid()
    for it in range(150):
        O = _random_window(rng, rng.randint(1, 7))
        if it % 2:  # every point inside the grid: the join is symmetric
            O = (np.clip(np.nan_to_num(O[0], nan=3.0), 0.0, 7.75), np.clip(np.nan_to_num(O[1], nan=3.0), 0.0, 7.75), O[2], O[3])
        r = rng.choice(RADII)
        clo = _agree(g, O, O, r, True, _brute_pairs(g, O, O, r))
        rows = set(zip(clo["okey"].tolist(), clo["qkey"].tolist()))
        assert all(a != b for a, b in rows)
        # (a point outside the grid matches as a query point and never as an ordinary one)
        assert not it % 2 or all((b, a) in rows for a, b in rows)


def test_closed_form_over_the_oracle_pairs_matches_the_literal_walk(oracle_mod):
    rng = random.Random(20261022)
    g = W.small_grid()
    og = oracle_mod.grid(8, 0.0, 8.0, 0.0, 8.0)
    for _ in range(200):
        O, Q = _random_window(rng, rng.randint(1, 7)), _random_window(rng, rng.randint(1, 7))
        r = rng.choice(RADII)
        st, pairs = oracle_mod.join_pp(og, og, O[0], O[1], Q[0], Q[1], r)
        assert st == 0
        assert sorted(map(tuple, pairs.tolist())) == sorted(map(tuple, _brute_pairs(g, O, Q, r).tolist()))
        _agree(g, O, Q, r, False, pairs)


def test_hand_vector():
    g = W.small_grid()
    clo = _agree(g, W.HAND_O, W.HAND_Q, W.HAND_R, False, _brute_pairs(g, W.HAND_O, W.HAND_Q, W.HAND_R))
    got = list(zip(*(clo[c].tolist() for c in ("okey", "qkey", "p_first", "q_latest", "emit", "oslot", "qslot"))))
    assert got == [tuple(r) for r in W.HAND_ROWS]
    for side, exp in (("ordinary", W.HAND_ORDINARY), ("query", W.HAND_QUERY)):
        assert {k: clo[side][k].tolist() for k in exp} == exp
    assert R.first_point(clo) == W.HAND_FIRST_POINT
    # what the vector is there for
    cell = lambda w, i: g.cellOf(float(w[0][i]), float(w[1][i]))  # noqa: E731
    assert cell(W.HAND_Q, 0) != cell(W.HAND_Q, 1) and W.HAND_Q[3][3] == W.HAND_Q[3][4]
    assert [cell(W.HAND_Q, i) for i in (7, 8, 9)] == [(1, 7)] * 3 and W.HAND_Q[3][9] < W.HAND_Q[3][8] < W.HAND_Q[3][7]


def test_negative_radius_is_the_layers_error():
    with pytest.raises(ValueError, match="candidateNeighboringLayers"):
        R.tjoin_loop(W.small_grid(), W.HAND_O, W.HAND_Q, -1.0)


def _pts(n, x=1, y=1, objid=1, ts=1):
    return _lib.GfPoints(x, y, objid, ts, n)


def test_entry_points_reject_bad_arguments_without_a_device():
    L = _lib.lib()
    h = C.c_void_p()
    g = W.small_grid().c_grid
    # a null groups object (and with it a null context) is refused first
    for mode in (_lib.TJOIN_PAIR, _lib.TJOIN_SINGLE, 7):
        assert L.gf_tjoin_run(None, C.byref(_pts(0)), None, C.byref(_pts(0)), C.byref(g), 1.0, mode, C.byref(h)) == _lib.GF_ERR_ARG
    assert L.gf_tjoin_run(None, None, None, None, None, math.nan, 0, None) == _lib.GF_ERR_ARG
    assert h.value is None
    c = [C.c_int64() for _ in range(7)]
    assert L.gf_tjoin_info(None, *(C.byref(v) for v in c)) == _lib.GF_ERR_ARG
    assert L.gf_tjoin_read_rows(None, None, None, None, None, None, None, None, 0) == _lib.GF_ERR_ARG
    assert L.gf_tjoin_read_trajs(None, 0, None, None, 0, None, None, None, None, 0) == _lib.GF_ERR_ARG
    assert L.gf_tjoin_set_table_slots(None, 16) == _lib.GF_ERR_ARG
    L.gf_tjoin_destroy(None)  # a no-op


def test_kernel_id_and_mirror_are_exported():
    assert _lib.K_TJOIN == 17
    assert (_lib.TJOIN_PAIR, _lib.TJOIN_SINGLE) == (0, 1)
    for name in ("PointPointTJoinQuery", "TJoinResult"):
        assert hasattr(sf, name) and name in sf.__all__
    assert hasattr(sf.TrajectoryGroups, "tjoin")
    for m in ("first_point", "point_pairs", "trajectory_pairs"):
        assert hasattr(sf.TJoinResult, m)
    for name in ("gf_tjoin_run", "gf_tjoin_destroy", "gf_tjoin_info", "gf_tjoin_read_rows", "gf_tjoin_read_trajs",
                 "gf_tjoin_set_table_slots"):
        assert name in _lib.EXPORTS and hasattr(_lib.lib(), name)


@pytest.mark.parametrize("qt", [sf.QueryType.RealTime, sf.QueryType.CountBased, sf.QueryType.RealTimeNaive])
def test_tjoin_is_window_based_only(qt):
    q = sf.PointPointTJoinQuery(sf.QueryConfiguration(qt), W.small_grid())
    with pytest.raises(ValueError, match="Not yet support"):
        q.run(None, None, 0.1)
    with pytest.raises(ValueError, match="Not yet support"):
        q.runSingle(None, 0.1)
