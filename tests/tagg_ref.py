"""Plain-Python restatement of tAggregate (the reference of tests/test_tagg_ref.py and
tests/test_gpu_tagg.py).

* cell_loop: a literal transcription of TimeWindowProcessFunction.process (TAggregateQuery.java:
  498-613) for the points of ONE cell in arrival order -- the reference.  Java's HashMaps are dicts;
  the ALL map is returned in insertion order (objIDs by their first point in the cell), the order the
  contract fixes where Flink leaves it open.
* cell_closed: the closed forms of include/geoflink_hip.h (L_o, e_o, s_o, f_o and the lexicographic
  winners), which the kernels compute.
* rows_of: the emission rules per aggregate name, literally (equalsIgnoreCase, Math.round).
* tagg_ref: a whole window -- cells through the host gf_cell_of, in first-occurrence order, each cell
  through cell_loop -- as the per-cell table and the ALL CSR.
"""
import math
from fractions import Fraction

import numpy as np

LONG_MAX, LONG_MIN = (1 << 63) - 1, -(1 << 63)


def cell_loop(points):
    """points: (objID, ts) in arrival order -> dict(count, sum, minLen, minKey, maxLen, maxKey, lengths);
    minKey / maxKey are None where the reference still holds its initial ""."""
    min_ts, max_ts, length = {}, {}, {}
    min_len, min_key = LONG_MAX, None
    max_len, max_key = LONG_MIN, None
    total = 0
    for obj, ts in points:
        cur_min = min_ts.get(obj)
        cur_max = max_ts.get(obj)
        mn, mx = cur_min, cur_max
        if cur_min is not None:
            if ts < cur_min:
                min_ts[obj] = ts
                mn = ts
            if ts > cur_max:
                max_ts[obj] = ts
                mx = ts
            cur_len = length[obj]
            new_len = mx - mn
            if cur_len != new_len:
                length[obj] = new_len
                total -= cur_len
                total += new_len
            if new_len > max_len:
                max_len, max_key = new_len, obj
            if new_len < min_len:
                min_len, min_key = new_len, obj
        else:
            min_ts[obj] = ts
            max_ts[obj] = ts
            length[obj] = 0
    return dict(count=len(length), sum=total, minLen=min_len, minKey=min_key, maxLen=max_len, maxKey=max_key,
                lengths=length)


def cell_closed(points):
    """points: (window index, objID, ts) of one cell, ascending index -> the same dict plus multi"""
    per = {}
    for i, obj, ts in points:
        per.setdefault(obj, []).append((i, ts))
    total, multi = 0, 0
    best_min, best_max = None, None  # (e, s, key), (L, f, key)
    lengths = {}
    for obj, pl in per.items():
        tmin, tmax = min(t for _, t in pl), max(t for _, t in pl)
        L = tmax - tmin
        lengths[obj] = L
        total += L
        if len(pl) >= 2:
            multi += 1
            e, s = abs(pl[1][1] - pl[0][1]), pl[1][0]
            f = max(next(i for i, t in pl if t == tmax), next(i for i, t in pl if t == tmin), s)
            if best_min is None or (e, s) < best_min[:2]:
                best_min = (e, s, obj)
            if best_max is None or L > best_max[0] or (L == best_max[0] and f < best_max[1]):
                best_max = (L, f, obj)
    return dict(count=len(per), sum=total, multi=multi,
                minLen=best_min[0] if best_min else LONG_MAX, minKey=best_min[2] if best_min else None,
                maxLen=best_max[0] if best_max else LONG_MIN, maxKey=best_max[2] if best_max else None,
                lengths=lengths)


def java_round(q):
    """Math.round(double) -> long: floor(q + 1/2) of the exact q"""
    return math.floor(Fraction(q) + Fraction(1, 2))


def rows_of(function, cell):
    """One cell's emitted row for an aggregate name: None (nothing emitted) or (kind, key, value);
    ALL's value is the lengths map.  `cell` is a cell_loop dict."""
    f = function.upper()  # equalsIgnoreCase on ASCII names
    if f == "SUM":
        return ("SUM", None, cell["sum"]) if cell["sum"] > 0 else None
    if f == "AVG":
        if cell["sum"] > 0:
            return ("AVG", None, java_round(float(cell["sum"]) * 1.0 / (float(cell["count"]) * 1.0)))
        return None
    if f == "MIN":
        return ("MIN", cell["minKey"], cell["minLen"]) if cell["minLen"] != LONG_MAX else None
    if f == "MAX":
        return ("MAX", cell["maxKey"], cell["maxLen"]) if cell["maxLen"] != LONG_MIN else None
    return ("ALL", None, cell["lengths"])


def cells_of(grid, x, y):
    """(cx, cy) int32 per point through the host gf_cell_of"""
    pairs = [grid.cellOf(a, b) for a, b in zip(np.asarray(x, np.float64).tolist(), np.asarray(y, np.float64).tolist())]
    c = np.array(pairs, np.int32).reshape(-1, 2)
    return c[:, 0].copy(), c[:, 1].copy()


def tagg_ref(cx, cy, obj, ts):
    """A window -> (table, (off, keys, lens), cells): table = dict of arrays as gf_tagg_read_cells (keys the
    reference leaves at "" are 0), the ALL CSR, and the cell_loop dicts, cells in first-occurrence order."""
    first, members = {}, []
    for i, c in enumerate(zip(np.asarray(cx).tolist(), np.asarray(cy).tolist())):
        j = first.get(c)
        if j is None:
            first[c] = len(members)
            members.append([i])
        else:
            members[j].append(i)
    ol, tl = np.asarray(obj, np.int64).tolist(), np.asarray(ts, np.int64).tolist()
    cells = [cell_loop([(ol[i], tl[i]) for i in m]) for m in members]
    multi = []
    for m in members:
        seen = {}
        for i in m:
            seen[ol[i]] = seen.get(ol[i], 0) + 1
        multi.append(sum(1 for v in seen.values() if v >= 2))
    table = dict(
        cx=np.array([c[0] for c in first], np.int32), cy=np.array([c[1] for c in first], np.int32),
        count=np.array([c["count"] for c in cells], np.int64), multi=np.array(multi, np.int64),
        sum=np.array([c["sum"] for c in cells], np.int64),
        minLen=np.array([c["minLen"] for c in cells], np.int64),
        minKey=np.array([c["minKey"] or 0 for c in cells], np.int64),
        maxLen=np.array([c["maxLen"] for c in cells], np.int64),
        maxKey=np.array([c["maxKey"] or 0 for c in cells], np.int64))
    off = np.zeros(len(cells) + 1, np.int64)
    if cells:
        off[1:] = np.cumsum([c["count"] for c in cells])
    keys = np.array([k for c in cells for k in c["lengths"]], np.int64)
    lens = np.array([v for c in cells for v in c["lengths"].values()], np.int64)
    return table, (off, keys, lens), cells


def rows_ref(function, table, cells):
    """The emitted rows of a window for an aggregate name -> dict(kind, cx, cy, count, key, value) arrays
    (key 0 where the reference's key is ""; ALL: the payload is the map, value = the cell's sum as
    gf_tagg_rows reports it)."""
    keep, key, value = [], [], []
    kind = function.upper() if function.upper() in ("SUM", "AVG", "MIN", "MAX") else "ALL"
    for j, c in enumerate(cells):
        r = rows_of(function, c)
        if r is None:
            continue
        assert r[0] == kind
        keep.append(j)
        key.append(r[1] or 0)
        value.append(c["sum"] if kind == "ALL" else r[2])
    keep = np.array(keep, np.int64)
    return dict(kind=kind, keep=keep, cx=table["cx"][keep], cy=table["cy"][keep], count=table["count"][keep],
                key=np.array(key, np.int64), value=np.array(value, np.int64))
