"""Plain-Python restatement of the window-based tKnn (the reference of tests/test_tknn_ref.py and
tests/test_gpu_tknn.py).

* cell_apply / tknn_loop: a literal transcription of TKNNQuery.kNNEvaluationWindowed.apply
  (TKNNQuery.java:66-100) per cell, then the join with the unfiltered window, the per-objID LineString
  construction and the windowAll of PointPointTKNNQuery.java (windowBased :203-310, windowBasedNaive
  :536-623).  Java's HashMaps are dicts in arrival order; where the reference sorts a HashMap's entries by
  value (ties in HashMap iteration order, unspecified) the ties are broken by the trajectory's
  first-occurrence rank, the order the contract fixes.  The loop is parameterised by the order in which
  the cells' records arrive.
* tknn_closed: the closed forms of include/geoflink_hip.h, in plain Python.
* tknn_ref: a whole window, vectorised -- cells through the host gf_cell_of, trajectories through
  traj_ref.group_ref -- as the arrays gf_tknn_read returns, plus the counters of gf_tknn_info and the
  pair table.
Distances are numpy float64 element-wise operations (no fused multiply-add), in the reference's order
sqrt((qy - y) * (qy - y) + (qx - x) * (qx - x)); every NaN is Double.doubleToLongBits' one pattern.
"""
import math

import numpy as np

from tagg_ref import cells_of
from traj_ref import group_ref

NAN = np.array([0x7FF8000000000000], np.uint64).view(np.float64)[0]


def distances(qx, qy, x, y):
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    with np.errstate(all="ignore"):
        d = np.sqrt((qy - y) * (qy - y) + (qx - x) * (qx - x))
    return np.where(np.isnan(d), NAN, d)


def cmp_key(d):
    """Double.compareTo of distances (never negative, never -0.0): NaN after everything"""
    return (1, 0.0) if math.isnan(d) else (0, d)


def cell_apply(points, k, rank):
    """kNNEvaluationWindowed.apply for ONE cell: points = (objID, distance) in arrival order -> the
    emitted (objID, distance) records"""
    obj_map = {}
    for obj, new in points:
        existing = obj_map.get(obj)
        if existing is None:
            obj_map[obj] = new
        elif new < existing:
            obj_map[obj] = new
    lst = sorted(obj_map.items(), key=lambda e: (cmp_key(e[1]), rank[e[0]]))
    out = []
    for key, value in lst:
        if len(out) == k:
            break
        out.append((key, value))
    return out


def tknn_loop(cell_points, cell_order, traj_len, rank, k, naive, k_final=None):
    """cell_points: {cell: [(objID, distance), ...]} of the cells of N, arrival order; cell_order: the
    cells in the order their records arrive; traj_len: {objID: points in the whole window}.
    k_final: the windowAll's k where a test wants to see past the final cut (the reference has one k).
    -> [(objID, distance, coordinates in the LineString)] in emission order"""
    k_final = k if k_final is None else k_final
    records = [rec for c in cell_order for rec in cell_apply(cell_points[c], k, rank)]
    # the join: every record meets every point of its objID in the unfiltered window
    joined = [(obj, d) for obj, d in records for _ in range(traj_len[obj])]
    if not naive:
        per = {}
        for obj, d in joined:  # keyBy(objID): coordinateList, and the first record's distance
            e = per.setdefault(obj, [0, d])
            e[0] += 1
        traj_dist, size = {}, {}
        for obj, (cnt, d) in per.items():
            if cnt > 1:
                traj_dist[obj] = d
                size[obj] = cnt
        out = []
        for obj, d in sorted(traj_dist.items(), key=lambda e: (cmp_key(e[1]), rank[e[0]])):
            if len(out) == k_final:
                break
            out.append((obj, d, size[obj]))
        return out
    trajectories, dist = {}, {}
    for obj, d in joined:
        if obj in trajectories:
            trajectories[obj] += 1
            if dist[obj] > d:
                dist[obj] = d
        else:
            trajectories[obj] = 1
            dist[obj] = d
    out = []
    for obj, d in sorted(dist.items(), key=lambda e: (cmp_key(e[1]), rank[e[0]])):
        if len(out) == k_final:
            break
        if trajectories[obj] > 1:
            out.append((obj, d, trajectories[obj]))
    return out


def tknn_closed(cell_points, traj_len, rank, k):
    """the contract's steps 3 .. 7 -> [(objID, D_t, cells_t)] in result order"""
    per_t = {}
    for c, points in cell_points.items():
        pair = {}
        for obj, d in points:
            pair.setdefault(obj, []).append(d)
        dd = {}
        for obj, ds in pair.items():
            good = [v for v in ds if not math.isnan(v)]
            dd[obj] = NAN if math.isnan(ds[0]) or not good else min(good)
        for obj, d in sorted(dd.items(), key=lambda e: (cmp_key(e[1]), rank[e[0]]))[:k]:
            per_t.setdefault(obj, []).append(d)
    rows = [(obj, min(ds, key=cmp_key), len(ds)) for obj, ds in per_t.items() if traj_len[obj] >= 2]
    rows.sort(key=lambda e: (cmp_key(e[1]), rank[e[0]]))
    return rows[:k]


def cell_mask(grid, cx, cy, qx, qy, r, naive):
    """the points in N; raises ValueError where the reference exits (candidate layers <= 0)"""
    cx, cy = np.asarray(cx, np.int64), np.asarray(cy, np.int64)
    if naive:
        return np.ones(len(cx), bool)
    n = grid.c_grid.n
    valid = (cx >= 0) & (cx < n) & (cy >= 0) & (cy < n)
    if r == 0:
        return valid
    L = grid.getCandidateNeighboringLayers(r)
    if L <= 0:
        raise ValueError("candidate layers <= 0")
    qcx, qcy = grid.cellOf(qx, qy)
    return valid & (np.abs(cx - qcx) <= L) & (np.abs(cy - qcy) <= L)


def window_tables(cx, cy, obj, d, mask):
    """(cell_points, traj_len, rank) of a window for tknn_loop / tknn_closed"""
    keys, off, _ = group_ref(obj)
    rank = {k: t for t, k in enumerate(keys.tolist())}
    traj_len = {k: int(off[t + 1] - off[t]) for t, k in enumerate(keys.tolist())}
    cell_points = {}
    for i in np.flatnonzero(mask).tolist():
        cell_points.setdefault((int(cx[i]), int(cy[i])), []).append((int(obj[i]), float(d[i])))
    return cell_points, traj_len, rank


def tknn_ref(grid, x, y, obj, ts, qx, qy, r, k, naive=False, cells=None, groups=None):
    """A whole window -> dict(keys, dist, cells, off, x, y, ts, idx, in_cells, pairs, records, pair_first_nan,
    pair_later_nan, pair_cx, pair_cy); cells = (cx, cy) and groups = group_ref(obj) may be passed in (shared)."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    obj, ts = np.asarray(obj, np.int64), np.asarray(ts, np.int64)
    cx, cy = cells if cells is not None else cells_of(grid, x, y)
    keys, off, perm = groups if groups is not None else group_ref(obj)
    nt = len(keys)
    t_of = np.empty(len(obj), np.int64)
    t_of[perm.astype(np.int64)] = np.repeat(np.arange(nt), np.diff(off))
    d = distances(qx, qy, x, y)
    e = np.flatnonzero(cell_mask(grid, cx, cy, qx, qy, r, naive))
    res = dict(in_cells=len(e), pairs=0, records=0)
    empty = dict(keys=np.empty(0, np.int64), dist=np.empty(0), cells=np.empty(0, np.int32), off=np.zeros(1, np.int64),
                 x=np.empty(0), y=np.empty(0), ts=np.empty(0, np.int64), idx=np.empty(0, np.uint32))
    if len(e) == 0:
        return {**res, **empty}
    ck = (cx[e].astype(np.int64) << 32) | (cy[e].astype(np.int64) & 0xFFFFFFFF)
    o = np.lexsort((e, t_of[e], ck))  # by (cell, trajectory, window index)
    e, ck, te, de = e[o], ck[o], t_of[e][o], d[e][o]
    start = np.flatnonzero(np.r_[True, (ck[1:] != ck[:-1]) | (te[1:] != te[:-1])])
    p_ck, p_t = ck[start], te[start]
    first_nan = np.isnan(de[start])
    with np.errstate(all="ignore"):
        p_d = np.fmin.reduceat(de, start)  # the minimum of the non-NaN distances (NaN: none)
    nan_count = np.add.reduceat(np.isnan(de).astype(np.int64), start)
    p_d = np.where(first_nan | np.isnan(p_d), NAN, p_d)
    # the cells' lists
    po = np.lexsort((p_t, p_d, np.isnan(p_d), p_ck))
    cstart = np.flatnonzero(np.r_[True, p_ck[po][1:] != p_ck[po][:-1]])
    rank_in_cell = np.arange(len(po)) - np.repeat(cstart, np.diff(np.r_[cstart, len(po)]))
    rec = po[rank_in_cell < k]
    res.update(pairs=len(start), records=len(rec), pair_first_nan=first_nan, pair_later_nan=(nan_count > 0) & ~first_nan,
               pair_cx=(p_ck >> 32).astype(np.int32), pair_cy=p_ck.astype(np.int32))
    # per trajectory
    r_t, r_d = p_t[rec], p_d[rec]
    ro = np.lexsort((r_d, np.isnan(r_d), r_t))
    tstart = np.flatnonzero(np.r_[True, r_t[ro][1:] != r_t[ro][:-1]])
    tt, D = r_t[ro][tstart], r_d[ro][tstart]
    ncell = np.diff(np.r_[tstart, len(ro)])
    keep = np.diff(off)[tt] >= 2
    tt, D, ncell = tt[keep], D[keep], ncell[keep]
    fo = np.lexsort((tt, D, np.isnan(D)))[:k]
    tt, D, ncell = tt[fo], D[fo], ncell[fo]
    lens = np.diff(off)[tt]
    ooff = np.zeros(len(tt) + 1, np.int64)
    ooff[1:] = np.cumsum(lens)
    idx = np.concatenate([perm[off[t]:off[t + 1]] for t in tt.tolist()]).astype(np.uint32) if len(tt) else empty["idx"]
    ii = idx.astype(np.int64)
    return {**res, **dict(keys=keys[tt], dist=D.astype(np.float64), cells=ncell.astype(np.int32), off=ooff, x=x[ii], y=y[ii],
                          ts=ts[ii], idx=idx)}
