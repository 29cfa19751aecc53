"""Plain-Python restatement of the window-based tJoin (the reference of tests/test_tjoin_ref.py and
tests/test_gpu_tjoin.py).

* tjoin_loop: a literal walk of PointPointTJoinQuery.windowBased / commonSingle over two windows in
  arrival order: the query points replicated to getNeighboringCells (UniformGrid.java:261-293), the join
  on the cell with the distance filter (and, for commonSingle, the objID test as the contract keeps it),
  the per-objID HashMap loop (PointPointTJoinQuery.java:263-286: firstPoint, secondIDPointMap replaced iff
  new.ts > old.ts) and the two joins against GenerateWindowedTrajectory's streams (TJoinQuery.java:165-192:
  at least two points).  Java's HashMaps are dicts in arrival order.  The order in which the join's
  tuples reach the HashMap loop is unspecified in Flink, and the loop reads it twice: firstPoint is the
  first tuple's ordinary point, and a query point replaces an equal-ts one never, so the first to arrive
  stays.  The contract fixes each by its own window's order -- the ordinary window's for firstPoint, the
  query window's for the tie -- and the walk takes the tuples' order as a parameter: "ordinary" = sorted by
  (p, q), "query" = by (q, p).  Cells are int pairs; they equal the reference's "%05d%05d" Strings wherever
  an index fits five characters.
* tjoin_closed: the closed form of include/geoflink_hip.h, section by section, as a NumPy reduction of a
  list of matching point pairs -> the arrays gf_tjoin_read_rows / gf_tjoin_read_trajs return.
Distances are Python floats (IEEE binary64, no fused multiply-add) in DistanceFunctions.java:60-63's
order; the sum of the two squares commutes, so the value is the point-point join's."""
import math

import numpy as np


def distance(x1, y1, x2, y2):
    return math.sqrt((y2 - y1) * (y2 - y1) + (x2 - x1) * (x2 - x1))


def neighboring_cells(grid, r, cx, cy):
    """getNeighboringCells as (cx, cy) pairs; raises where the reference calls System.exit(1)"""
    n = grid.getNumGridPartitions()
    if r == 0:
        return [(i, j) for i in range(n) for j in range(n)]
    L = grid.getCandidateNeighboringLayers(r)
    if L <= 0:
        raise ValueError("candidateNeighboringLayers cannot be 0 or less")
    return [(i, j) for i in range(max(cx - L, 0), min(cx + L, n - 1) + 1)
            for j in range(max(cy - L, 0), min(cy + L, n - 1) + 1)]


def tjoin_loop(grid, O, Q, r, single=False, order="ordinary"):
    """O, Q: (x, y, objID, ts) sequences in arrival order -> (point_rows, traj_rows, first_point):
    point_rows = [(ordinary objID, query objID, firstPoint's index, the kept query point's index)] (the
    joinedFilteredOutput / commonSingle's result), traj_rows = [(ordinary objID, query objID)] (the final
    Tuple2<LineString, LineString>), first_point = {ordinary objID: index}."""
    ox, oy, oobj, ots = (np.asarray(a).tolist() for a in O)
    qx, qy, qobj, qts = (np.asarray(a).tolist() for a in Q)
    replicated = {}
    for j in range(len(qx)):
        for c in neighboring_cells(grid, r, *grid.cellOf(qx[j], qy[j])):
            replicated.setdefault(c, []).append(j)
    join_output = []
    for i in range(len(ox)):
        for j in replicated.get(grid.cellOf(ox[i], oy[i]), ()):
            if single and oobj[i] == qobj[j]:
                continue  # no need to join a trajectory with itself
            if distance(ox[i], oy[i], qx[j], qy[j]) <= r:
                join_output.append((i, j))
    if order == "query":
        join_output.sort(key=lambda e: (e[1], e[0]))
    by_obj = {}
    for e in join_output:  # keyBy(e.f0.objID)
        by_obj.setdefault(oobj[e[0]], []).append(e)
    point_rows, first_point = [], {}
    for key, inputs in by_obj.items():
        second, first, first_set = {}, None, False
        for i, j in inputs:
            if not first_set:
                first, first_set = i, True
            existing = second.get(qobj[j])
            if existing is not None:
                if qts[j] > qts[existing]:
                    second[qobj[j]] = j
            else:
                second[qobj[j]] = j
        first_point[key] = first
        for k2, j in second.items():
            point_rows.append((key, k2, first, j))

    def trajectories(obj):  # GenerateWindowedTrajectory: coordinateList.size() > 1
        cnt = {}
        for k in obj:
            cnt[k] = cnt.get(k, 0) + 1
        return {k for k, c in cnt.items() if c > 1}

    to, tq = trajectories(oobj), trajectories(qobj)
    traj_rows = [(k, k2) for k, k2, _, _ in point_rows if k in to and k2 in tq]
    return point_rows, traj_rows, first_point


def _ranks(obj):
    """-> (first-occurrence rank per point, keys in rank order)"""
    obj = np.asarray(obj, np.int64)
    u, first, inv = np.unique(obj, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")
    rank = np.empty(len(u), np.int64)
    rank[order] = np.arange(len(u))
    return rank[inv.reshape(-1)], u[order]


def _csr(window, t, nt, sel):
    """the trajectories sel (ascending ranks) of a window, whole, in arrival order"""
    x, y, obj, ts = window
    perm = np.argsort(t, kind="stable")
    off = np.concatenate([[0], np.cumsum(np.bincount(t, minlength=nt))]).astype(np.int64)
    segs = [perm[off[s]:off[s + 1]] for s in sel.tolist()]
    idx = np.concatenate(segs).astype(np.uint32) if segs else np.empty(0, np.uint32)
    lens = np.array([len(s) for s in segs], np.int64)
    return {"off": np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), "idx": idx,
            "x": np.asarray(x, np.float64)[idx], "y": np.asarray(y, np.float64)[idx], "ts": np.asarray(ts, np.int64)[idx]}


def tjoin_closed(pairs, O, Q, single=False):
    """pairs: int [m, 2] matching (ordinary index, query index) pairs, in any order, duplicates allowed ->
    dict: okey, qkey, p_first, q_latest, emit, oslot, qslot (the row table, ascending by (t_o, t_q)),
    ordinary / query (dicts keys, off, x, y, ts, idx), rows, emitted."""
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    oobj, qobj = np.asarray(O[2], np.int64), np.asarray(Q[2], np.int64)
    qts = np.asarray(Q[3], np.int64)
    to, okeys = _ranks(oobj)
    tq, qkeys = _ranks(qobj)
    p, q = pairs[:, 0], pairs[:, 1]
    if single:
        keep = oobj[p] != qobj[q]
        p, q = p[keep], q[keep]
    ntq = max(len(qkeys), 1)
    key = to[p] * ntq + tq[q] if len(p) else np.empty(0, np.int64)
    # section 3: per row the least p, and the q of the largest ts, among equal ts the least index
    o1 = np.lexsort((p, key))
    o2 = np.lexsort((q, -qts[q], key))
    ks = key[o1]
    head = np.ones(len(ks), bool)
    head[1:] = ks[1:] != ks[:-1]
    rows = ks[head]
    r_to, r_tq = rows // ntq, rows % ntq
    out = {"okey": okeys[r_to], "qkey": qkeys[r_tq], "p_first": p[o1][head].astype(np.uint32),
           "q_latest": q[o2][head].astype(np.uint32)}
    # section 4: the size rule over the WHOLE windows
    olen, qlen = np.bincount(to, minlength=len(okeys)), np.bincount(tq, minlength=len(qkeys))
    emit = (olen[r_to] >= 2) & (qlen[r_tq] >= 2) if len(rows) else np.zeros(0, bool)
    out["emit"] = emit
    # section 5: per side the distinct trajectories of the emitted rows, ascending rank
    for name, r_t, t, keys, window, slot in (("ordinary", r_to, to, okeys, O, "oslot"), ("query", r_tq, tq, qkeys, Q, "qslot")):
        sel = np.unique(r_t[emit])
        csr = _csr(window, t, len(keys), sel)
        csr["keys"] = keys[sel]
        out[name] = csr
        s = np.full(len(rows), -1, np.int32)
        s[emit] = np.searchsorted(sel, r_t[emit]).astype(np.int32)
        out[slot] = s
    out["rows"], out["emitted"] = len(rows), int(emit.sum())
    return out


def first_point(res):
    """{ordinary objID key: the minimum of p_first over its rows} of a tjoin_closed dict"""
    fp = {}
    for k, v in zip(res["okey"].tolist(), res["p_first"].tolist()):
        fp[k] = min(fp.get(k, v), v)
    return fp
