"""The restatement of the geometry-window operators (include/geoflink_hip.h, "polygon and linestring
windows"): PolygonPointRangeQuery / LineStringPointRangeQuery (range/PolygonPointRangeQuery.java:116-196,
range/LineStringPointRangeQuery.java:118-191) and PolygonPointKNNQuery / LineStringPointKNNQuery
(knn/*.java with KNNQuery.kNNWinAllEvaluationPolygonStream) as literal Python loops over the window:
the cell rectangle of every object as a set, the HashSet walk with its break, the heap and the dedupe.
Composed from what oracle/oracle.py exports (gc_sets_point, layers, assign_cells,
point_polygon_distance, point_bbox_distance) and the chain distance of tests/linestring_cases.py.
A second, closed-form statement (emitted iff all-G, or filtered and min d <= r) stands beside it for
tests/test_geomwin_ref.py.  No GPU, no torch."""
from __future__ import annotations

import functools

import numpy as np

import linestring_cases as LC
import oracle as O

POLYGON, LINESTRING = 1, 2


class LayersError(Exception):
    """getNeighboringCells: 'candidateNeighboringLayers cannot be 0 or less' (System.exit(1))"""


@functools.lru_cache(maxsize=None)
def _hyp():
    f = np.frompyfunc(O.lib().orc_hypot, 2, 1)

    def hypot(a, b):
        with np.errstate(all="ignore"):
            return f(a, b).astype(np.float64)
    return hypot


def grid_of(n, box):
    return O.grid(n, *box)


# ---- window objects ----------------------------------------------------------------------------------
def valid(kind, obj):
    """a polygon: at least a shell, every ring closed with >= 4 vertices; a linestring: >= 2 vertices"""
    if kind == LINESTRING:
        return len(obj) >= 2
    return len(obj) >= 1 and all(len(r) >= 4 and tuple(r[0]) == tuple(r[-1]) for r in obj)


def bbox(kind, obj):
    """(x1, y1, x2, y2): the vertex envelope -- a polygon's is its shell's"""
    ring = obj if kind == LINESTRING else obj[0]
    xs, ys = [float(v[0]) for v in ring], [float(v[1]) for v in ring]
    return min(xs), min(ys), max(xs), max(ys)


def cell_rect(g, bb):
    """HelperClass.assignGridCellID(bbox): (cx1, cy1, cx2, cy2), not clamped"""
    cx, cy = O.assign_cells(g, [bb[0], bb[2]], [bb[1], bb[3]])
    return int(cx[0]), int(cy[0]), int(cx[1]), int(cy[1])


def cell_set(rect):
    cx1, cy1, cx2, cy2 = rect
    return [(i, j) for i in range(cx1, cx2 + 1) for j in range(cy1, cy2 + 1)]


_DIST = {}  # (id(obj), point, metric, approximate) -> (obj, d): computed once, shared by every radius and test


def distance(kind, obj, px, py, metric=0, approximate=False):
    """the distance of a VALID object to one point, as the reference computes it"""
    key = (id(obj), float(px), float(py), metric, bool(approximate))
    hit = _DIST.get(key)
    if hit is not None and hit[0] is obj:
        return hit[1]
    if approximate:
        d = float(O.point_bbox_distance(px, py, *bbox(kind, obj)))
    elif kind == POLYGON:
        d = float(O.point_polygon_distance(px, py, O.Polygons([obj]), 0, metric))
    else:
        d = float(LC.chain_distance(np.array([px]), np.array([py]), obj, metric, _hyp())[0])
    _DIST[key] = (obj, d)
    return d


# ---- query side --------------------------------------------------------------------------------------
def query_sets(g, qx, qy, r):
    """(N, G) as sets of (cx, cy): N = the union of getNeighboringCells(r, point) -- valid cells only;
    r == 0: the whole grid; candidate layers <= 0: LayersError --, G = the union of
    getGuaranteedNeighboringCells(r, point.gridID)."""
    n = g.n
    gl, cl = O.layers(g, r)
    if r != 0 and cl <= 0:
        raise LayersError()
    N, G = set(), set()
    qcx, qcy = O.assign_cells(g, qx, qy)
    for cx, cy in zip(qcx, qcy):
        Gq, Cq = O.gc_sets_point(g, r, int(cx), int(cy))
        G |= Gq
        N |= {c for c in (Gq | Cq) if 0 <= c[0] < n and 0 <= c[1] < n}
    if r == 0:
        N = {(i, j) for i in range(n) for j in range(n)}
    return N, G


# ---- range -------------------------------------------------------------------------------------------
def range_literal(g, kind, objs, qx, qy, r, approximate=False, metric=0, order=None, info=None):
    """Emitted object indices, ascending.  order(cells): reorders an object's cell list in place (the
    HashSet's iteration order is unspecified).  info (a dict) receives filtered / all_guaranteed / tested."""
    N, G = query_sets(g, qx, qy, r)
    out, filtered, allg, tested = [], 0, 0, 0
    for i, obj in enumerate(objs):
        if not valid(kind, obj):
            continue
        cells = cell_set(cell_rect(g, bbox(kind, obj)))
        if order is not None:
            order(cells)
        if not any(c in N for c in cells):  # HelperClass.cellBasedPolygonFlatMap
            continue
        filtered += 1
        counter = 0
        for c in cells:
            if c in G:
                counter += 1
                if counter == len(cells):
                    out.append(i)
                    allg += 1
            else:
                tested += 1
                for px, py in zip(qx, qy):
                    if distance(kind, obj, px, py, metric, approximate) <= r:
                        out.append(i)
                        break
                break
    if info is not None:
        info.update(filtered=filtered, all_guaranteed=allg, tested=tested)
    return np.array(out, np.int64)


def _masks(g, qx, qy, r):
    N, G = query_sets(g, qx, qy, r)
    inN, inG = np.zeros((g.n, g.n), bool), np.zeros((g.n, g.n), bool)
    for c in N:
        inN[c] = True
    for c in G:
        if 0 <= c[0] < g.n and 0 <= c[1] < g.n:
            inG[c] = True
    return inN, inG


def rect_counts(mask, rect):
    """(members of mask in rect n grid, cells of rect): what the summed-area tables answer"""
    n = mask.shape[0]
    cx1, cy1, cx2, cy2 = rect
    a, b, c, d = max(cx1, 0), max(cy1, 0), min(cx2, n - 1), min(cy2, n - 1)
    inside = int(mask[a:c + 1, b:d + 1].sum()) if a <= c and b <= d else 0
    return inside, (cx2 - cx1 + 1) * (cy2 - cy1 + 1)


def range_closed_form(g, kind, objs, qx, qy, r, approximate=False, metric=0):
    """emitted iff valid and (every cell in G, or some cell in N and min over the points of d <= r)"""
    inN, inG = _masks(g, qx, qy, r)
    out = []
    for i, obj in enumerate(objs):
        if not valid(kind, obj):
            continue
        rect = cell_rect(g, bbox(kind, obj))
        if rect_counts(inN, rect)[0] == 0:
            continue
        cg, area = rect_counts(inG, rect)
        if cg == area or min(distance(kind, obj, px, py, metric, approximate) for px, py in zip(qx, qy)) <= r:
            out.append(i)
    return np.array(out, np.int64)


# ---- kNN ---------------------------------------------------------------------------------------------
def knn_literal(g, kind, objs, keys, qx, qy, r, k, approximate=False, metric=0):
    """(objID keys, d, idx): the candidates (a cell in N, d <= r) through a bounded heap by (d, key, idx),
    then one entry per key -- the library's record contract."""
    N, _ = query_sets(g, [qx], [qy], r)
    cand = []
    for i, obj in enumerate(objs):
        if not valid(kind, obj):
            continue
        if not any(c in N for c in cell_set(cell_rect(g, bbox(kind, obj)))):
            continue
        d = distance(kind, obj, qx, qy, metric, approximate)
        if d <= r:
            cand.append((d, int(keys[i]), i))
    cand.sort()
    seen, rows = set(), []
    for d, key, i in cand:  # the dedupe keeps each key's first = smallest (d, idx)
        if key in seen:
            continue
        seen.add(key)
        rows.append((d, key, i))
        if len(rows) == k:
            break
    return (np.array([v[1] for v in rows], np.int64), np.array([v[0] for v in rows], np.float64),
            np.array([v[2] for v in rows], np.int64))


def realized_distances(kind, objs, qx, qy, metric=0, approximate=False):
    """every finite distance the case realizes, for the radii at and one ulp around them"""
    out = set()
    for obj in objs:
        if valid(kind, obj):
            for px, py in zip(qx, qy):
                d = distance(kind, obj, px, py, metric, approximate)
                if 0 < d < 1e300:
                    out.add(d)
    return sorted(out)


def case_radii(case, qx, qy, metric, approximate, limit=3):
    """the layer regimes of the case's grid (guaranteed layers 1, 0 and -1), r = 0, and a few realized distances
    with their ulp neighbours"""
    cl = (case["grid"][1][1] - case["grid"][1][0]) / case["grid"][0]
    rs = [3.0 * cl, 1.6 * cl, 0.75 * cl, 0.0]
    near = [d for d in realized_distances(case["kind"], case["objs"], qx, qy, metric, approximate) if d <= 3.0 * cl]
    for d in near[:: max(1, len(near) // limit)][:limit]:
        rs += [float(np.nextafter(d, 0.0)), d, float(np.nextafter(d, np.inf))]
    return rs
