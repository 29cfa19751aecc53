"""The restatement of the eight geometry-pair operators (include/geoflink_hip.h, "geometry windows against
polygon and linestring queries"): {Polygon,LineString}{Polygon,LineString}{Range,KNN}Query (WindowBased) as
literal Python loops -- the query-side HashSets built cell by cell, the HashSet walk over an object's cells
with its break, the loop over the query set with its break, the heap and the dedupe.  Composed from what
oracle/oracle.py exports (layers, assign_cells, distance, hypot), tests/geomwin_ref.py (validity, bbox,
cell rectangles) and tests/poly_cases.py (the ring locator); new here are a literal
Distance.segmentToSegment / DistanceOp and getBBoxBBoxMinEuclideanDistance.  A numpy form of the facet
distance stands beside the scalar one for the long geometries, and a closed-form statement of the operators
(rectangles instead of cell sets, any cell order) beside the literal one.  No GPU, no torch."""
from __future__ import annotations

import math

import numpy as np

import geomwin_ref as GR
import oracle as O
import poly_cases as PC

POLYGON, LINESTRING = GR.POLYGON, GR.LINESTRING
DBL_MAX = 1.7976931348623157e308
JAVA_MIN_VALUE = 4.9e-324


# ---- Distance.pointToSegment / segmentToSegment, literally ----------------------------------------------
def point_to_segment(p, a, b, metric=0):
    (px, py), (ax, ay), (bx, by) = p, a, b
    if ax == bx and ay == by:
        return O.distance(px, py, ax, ay, metric)
    len2 = (bx - ax) * (bx - ax) + (by - ay) * (by - ay)
    r = ((px - ax) * (bx - ax) + (py - ay) * (by - ay)) / len2
    if r <= 0.0:
        return O.distance(px, py, ax, ay, metric)
    if r >= 1.0:
        return O.distance(px, py, bx, by, metric)
    s = ((ay - py) * (bx - ax) - (ax - px) * (by - ay)) / len2
    return abs(s) * math.sqrt(len2)


def envelopes_intersect(a, b, c, d):
    """Envelope.intersects(p1, p2, q1, q2) with p = AB, q = CD"""
    minq, maxq, minp, maxp = min(c[0], d[0]), max(c[0], d[0]), min(a[0], b[0]), max(a[0], b[0])
    if minp > maxq or maxp < minq:
        return False
    minq, maxq, minp, maxp = min(c[1], d[1]), max(c[1], d[1]), min(a[1], b[1]), max(a[1], b[1])
    return not (minp > maxq or maxp < minq)


def segment_to_segment(a, b, c, d, metric=0):
    a, b, c, d = (tuple(map(float, v)) for v in (a, b, c, d))
    if a == b:
        return point_to_segment(a, c, d, metric)
    if c == d:
        return point_to_segment(d, a, b, metric)
    no_intersection = False
    if not envelopes_intersect(a, b, c, d):
        no_intersection = True
    else:
        denom = (b[0] - a[0]) * (d[1] - c[1]) - (b[1] - a[1]) * (d[0] - c[0])
        if denom == 0:
            no_intersection = True
        else:
            r_num = (a[1] - c[1]) * (d[0] - c[0]) - (a[0] - c[0]) * (d[1] - c[1])
            s_num = (a[1] - c[1]) * (b[0] - a[0]) - (a[0] - c[0]) * (b[1] - a[1])
            s = s_num / denom
            r = r_num / denom
            if r < 0 or r > 1 or s < 0 or s > 1:
                no_intersection = True
    if no_intersection:
        m = point_to_segment(a, c, d, metric)
        for v in (point_to_segment(b, c, d, metric), point_to_segment(c, a, b, metric), point_to_segment(d, a, b, metric)):
            if v < m:
                m = v
        return m
    return 0.0


# ---- DistanceOp -------------------------------------------------------------------------------------------
def lines_of(kind, geom):
    """LinearComponentExtracter: a polygon's rings (shell first), a linestring's one chain"""
    return [geom] if kind == LINESTRING else list(geom)


def first_coordinate(kind, geom):
    v = geom[0] if kind == LINESTRING else geom[0][0]
    return float(v[0]), float(v[1])


def holds(p, rings):
    """PointLocator.locate(p, polygon) != EXTERIOR"""
    px, py = np.array([p[0]]), np.array([p[1]])
    loc = int(PC.ring_locate(px, py, [tuple(map(float, v)) for v in rings[0]])[0])
    if loc == PC.LOC_E:
        return False
    if loc == PC.LOC_B:
        return True
    for hole in rings[1:]:
        hl = int(PC.ring_locate(px, py, [tuple(map(float, v)) for v in hole])[0])
        if hl == PC.LOC_I:
            return False
        if hl == PC.LOC_B:
            return True
    return True


def facet_distance(qkind, q, okind, o, metric=0):
    """the scalar loop of DistanceOp.computeMinDistanceLines without its envelope skip (contract 5b)"""
    md = DBL_MAX
    for la in lines_of(qkind, q):
        for lb in lines_of(okind, o):
            for i in range(len(la) - 1):
                for j in range(len(lb) - 1):
                    d = segment_to_segment(la[i], la[i + 1], lb[j], lb[j + 1], metric)
                    if d < md:
                        md = d
                    if md <= 0.0:
                        return md
    return md


def _p2s_np(px, py, ax, ay, bx, by):
    """pointToSegment's case analysis over arrays -> (end, dx, dy, interior d), as poly_cases._segment"""
    with np.errstate(all="ignore"):
        deg = (ax == bx) & (ay == by)
        len2 = (bx - ax) * (bx - ax) + (by - ay) * (by - ay)
        r = ((px - ax) * (bx - ax) + (py - ay) * (by - ay)) / len2
        enda = deg | (r <= 0.0)
        endb = ~enda & (r >= 1.0)
        s = ((ay - py) * (bx - ax) - (ax - px) * (by - ay)) / len2
        return enda | endb, np.where(enda, px - ax, px - bx), np.where(enda, py - ay, py - by), np.abs(s) * np.sqrt(len2)


def _pair_matrix(la, lb, metric, bound):
    """[segments of la, segments of lb] of segmentToSegment.  metric 1: the endpoint cases take fdlibm's hypot
    only where the sqrt form is <= bound (the others are +inf: they cannot be the minimum, see
    poly_cases.ring_min_distance)."""
    A = np.array(la, np.float64)
    Cc = np.array(lb, np.float64)
    ax, ay, bx, by = (v[:, None] for v in (A[:-1, 0], A[:-1, 1], A[1:, 0], A[1:, 1]))
    cx, cy, dx, dy = (v[None, :] for v in (Cc[:-1, 0], Cc[:-1, 1], Cc[1:, 0], Cc[1:, 1]))
    shape = np.broadcast(ax, cx).shape
    ax, ay, bx, by, cx, cy, dx, dy = (np.broadcast_to(v, shape) for v in (ax, ay, bx, by, cx, cy, dx, dy))
    hyp = GR._hyp()

    def value(t):
        end, ex, ey, di = t
        with np.errstate(all="ignore"):
            d = np.sqrt(ex * ex + ey * ey)
        if metric == 1:
            need = end & (d <= bound)
            d = np.where(end, np.inf, d)
            if need.any():
                d[need] = hyp(ex[need], ey[need])
        return np.where(end, d, di)

    with np.errstate(all="ignore"):
        t1 = value(_p2s_np(ax, ay, cx, cy, dx, dy))
        t2 = value(_p2s_np(bx, by, cx, cy, dx, dy))
        t3 = value(_p2s_np(cx, cy, ax, ay, bx, by))
        t4 = value(_p2s_np(dx, dy, ax, ay, bx, by))
        m = t1
        for t in (t2, t3, t4):
            m = np.where(t < m, t, m)
        apart = (np.minimum(ax, bx) > np.maximum(cx, dx)) | (np.maximum(ax, bx) < np.minimum(cx, dx)) | \
                (np.minimum(ay, by) > np.maximum(cy, dy)) | (np.maximum(ay, by) < np.minimum(cy, dy))
        denom = (bx - ax) * (dy - cy) - (by - ay) * (dx - cx)
        r = ((ay - cy) * (dx - cx) - (ax - cx) * (dy - cy)) / denom
        s = ((ay - cy) * (bx - ax) - (ax - cx) * (by - ay)) / denom
        apart = apart | (denom == 0) | (r < 0) | (r > 1) | (s < 0) | (s > 1)
        out = np.where(apart, m, 0.0)
        deg_c = (cx == dx) & (cy == dy)
        out = np.where(deg_c, t4, out)
        out = np.where((ax == bx) & (ay == by), t1, out)
    return out


def facet_distance_np(qkind, q, okind, o, metric=0):
    """facet_distance by matrices (the minimum of non-NaN values does not depend on the order)"""
    def sweep(bound):
        md = DBL_MAX
        for la in lines_of(qkind, q):
            for lb in lines_of(okind, o):
                m = _pair_matrix(la, lb, metric if bound is not None else 0, bound)
                m = m[m == m]
                if m.size and float(m.min()) < md:
                    md = float(m.min())
        return md
    m0 = sweep(None)
    return m0 if metric == 0 else sweep(m0 * (1 + 1e-9))


_DIST = {}


def distance(qkind, q, okind, o, metric=0, approximate=False, numpy_form=None):
    """DistanceFunctions.getDistance(query, object) / getBBoxBBoxMinEuclideanDistance(query.bbox, object.bbox)
    of two VALID geometries; cached by identity for every radius and test"""
    key = (id(q), id(o), qkind, okind, metric, bool(approximate))
    hit = _DIST.get(key)
    if hit is not None and hit[0] is q and hit[1] is o:
        return hit[2]
    if approximate:
        d = bbox_bbox_distance(GR.bbox(qkind, q), GR.bbox(okind, o))
    elif qkind == POLYGON and holds(first_coordinate(okind, o), q):
        d = 0.0
    elif okind == POLYGON and holds(first_coordinate(qkind, q), o):
        d = 0.0
    else:
        nseg = sum(len(l) - 1 for l in lines_of(qkind, q)) * sum(len(l) - 1 for l in lines_of(okind, o))
        use_np = nseg > 64 if numpy_form is None else numpy_form
        d = (facet_distance_np if use_np else facet_distance)(qkind, q, okind, o, metric)
    _DIST[key] = (q, o, d)
    return d


# ---- DistanceFunctions.getBBoxBBoxMinEuclideanDistance, literally ---------------------------------------
def _pp(c1, c2):
    """getPointPointEuclideanDistance(Coordinate, Coordinate)"""
    lon, lat, lon1, lat1 = c1[0], c1[1], c2[0], c2[1]
    return math.sqrt((lat1 - lat) * (lat1 - lat) + (lon1 - lon) * (lon1 - lon))


def _border(p, c1, c2):
    """getPointLineStringNearestBBoxBorderMinEuclideanDistance(p, c1, c2)"""
    x, y, x1, y1, x2, y2 = p[0], p[1], c1[0], c1[1], c2[0], c2[1]
    if x1 == x2:
        return _pp((x, y), (x1, y))
    if y1 == y2:
        return _pp((x, y), (x, y1))
    return JAVA_MIN_VALUE


def bbox_bbox_distance(box1, box2):
    """box = (x1, y1, x2, y2); box1 is the query's in every operator"""
    x1, y1, x2, y2 = map(float, box1)
    a1, a2, a3, a4 = (x1, y1), (x2, y1), (x2, y2), (x1, y2)
    p1, q1, p2, q2 = map(float, box2)
    b1, b2, b3, b4 = (p1, q1), (p2, q1), (p2, q2), (p1, q2)
    if p2 <= x1:
        if q2 <= y1:
            return _pp(a1, b3)
        elif q1 >= y2:
            return _pp(a4, b2)
        return _border(b2, a1, a4)
    elif p1 >= x2:
        if q2 <= y1:
            return _pp(a2, b4)
        elif q1 >= y2:
            return _pp(a3, b1)
        return _border(b1, a2, a3)
    if q2 <= y1:
        return _border(b4, a1, a2)
    elif q1 >= y2:
        return _border(b1, a3, a4)
    return 0.0


# ---- query side -------------------------------------------------------------------------------------------
def _valid_key(n, i, j):
    return 0 <= i < n and 0 <= j < n


def guaranteed_cells(g, r, cell):
    """UniformGrid.getGuaranteedNeighboringCells(r, cellID) -- :165-190: layers 0 adds the cell with no validKey"""
    gl, _ = O.layers(g, r)
    out = set()
    if gl == 0:
        out.add(cell)
    elif gl > 0:
        for i in range(cell[0] - gl, cell[0] + gl + 1):
            for j in range(cell[1] - gl, cell[1] + gl + 1):
                if _valid_key(g.n, i, j):
                    out.add((i, j))
    return out


def candidate_cells(g, r, cell, guaranteed):
    """UniformGrid.getCandidateNeighboringCells(r, cellID, guaranteed) -- :368-395"""
    _, cl = O.layers(g, r)
    out = set()
    if cl > 0:
        for i in range(cell[0] - cl, cell[0] + cl + 1):
            for j in range(cell[1] - cl, cell[1] + cl + 1):
                if _valid_key(g.n, i, j) and (i, j) not in guaranteed:
                    out.add((i, j))
    return out


def query_cells(g, qkind, q):
    return GR.cell_set(GR.cell_rect(g, GR.bbox(qkind, q)))


def query_sets(g, qkind, queries, r):
    """(N, G) as sets of (cx, cy) in or out of the grid: the operators' loop over the query set"""
    G, Cn = set(), set()
    for q in queries:
        Gq = set()
        for cell in query_cells(g, qkind, q):
            Gq |= guaranteed_cells(g, r, cell)
        G |= Gq
        for cell in query_cells(g, qkind, q):
            Cn |= candidate_cells(g, r, cell, G)
    return G | Cn, G


def refused(g, qkind, queries, r):
    """the documented deviation: guaranteed layers 0, several queries, a query rectangle leaving the grid"""
    gl, _ = O.layers(g, r)
    return gl == 0 and len(queries) > 1 and any(not _valid_key(g.n, *c) for q in queries for c in query_cells(g, qkind, q))


# ---- range ------------------------------------------------------------------------------------------------
def range_literal(g, okind, objs, qkind, queries, r, approximate=False, metric=0, order=None, info=None):
    N, G = query_sets(g, qkind, queries, r)
    out, filtered, allg, tested = [], 0, 0, 0
    for i, obj in enumerate(objs):
        if not GR.valid(okind, obj):
            continue
        cells = GR.cell_set(GR.cell_rect(g, GR.bbox(okind, obj)))
        if order is not None:
            order(cells)
        if not any(c in N for c in cells):  # HelperClass.cellBasedPolygonFlatMap / cellBasedLineStringFlatMap
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
                for q in queries:
                    if distance(qkind, q, okind, obj, metric, approximate) <= r:
                        out.append(i)
                        break
                break
    if info is not None:
        info.update(filtered=filtered, all_guaranteed=allg, tested=tested)
    return np.array(out, np.int64)


def _grown(rect, layers, n):
    """the valid cells within `layers` of a cell of rect, as a clipped rectangle (None: empty)"""
    a, b = max(rect[0] - layers, 0), max(rect[1] - layers, 0)
    c, d = min(rect[2] + layers, n - 1), min(rect[3] + layers, n - 1)
    return (a, b, c, d) if a <= c and b <= d else None


def _in_any(cell, rects):
    return any(rc is not None and rc[0] <= cell[0] <= rc[2] and rc[1] <= cell[1] <= rc[3] for rc in rects)


def range_closed_form(g, okind, objs, qkind, queries, r, approximate=False, metric=0):
    """emitted iff valid and (every cell in G, or some cell in N and min over the queries of d <= r), with
    G and N as unions of rectangles: R_q itself at layers 0, R_q grown and clipped otherwise"""
    gl, cl = O.layers(g, r)
    rq = [GR.cell_rect(g, GR.bbox(qkind, q)) for q in queries]
    Gr = [] if gl < 0 else (rq if gl == 0 else [_grown(rc, gl, g.n) for rc in rq])
    Nr = Gr + ([_grown(rc, cl, g.n) for rc in rq] if cl > 0 else [])
    out = []
    for i, obj in enumerate(objs):
        if not GR.valid(okind, obj):
            continue
        cells = GR.cell_set(GR.cell_rect(g, GR.bbox(okind, obj)))
        if not any(_in_any(c, Nr) for c in reversed(cells)):
            continue
        if all(_in_any(c, Gr) for c in cells) or min(distance(qkind, q, okind, obj, metric, approximate) for q in queries) <= r:
            out.append(i)
    return np.array(out, np.int64)


# ---- kNN --------------------------------------------------------------------------------------------------
def knn_literal(g, okind, objs, keys, qkind, query, r, k, approximate=False, metric=0):
    """(objID keys, d, idx): the candidates (a cell in N, d <= r) through a bounded heap by (d, key, idx), then
    one entry per key -- the library's record contract"""
    N, _ = query_sets(g, qkind, [query], r)
    cand = []
    for i, obj in enumerate(objs):
        if not GR.valid(okind, obj):
            continue
        if not any(c in N for c in GR.cell_set(GR.cell_rect(g, GR.bbox(okind, obj)))):
            continue
        d = distance(qkind, query, okind, obj, metric, approximate)
        if d <= r:
            cand.append((d, int(keys[i]), i))
    cand.sort()
    seen, rows = set(), []
    for d, key, i in cand:
        if key in seen:
            continue
        seen.add(key)
        rows.append((d, key, i))
        if len(rows) == k:
            break
    return (np.array([v[1] for v in rows], np.int64), np.array([v[0] for v in rows], np.float64),
            np.array([v[2] for v in rows], np.int64))


def realized_distances(okind, objs, qkind, queries, metric=0, approximate=False):
    out = set()
    for obj in objs:
        if GR.valid(okind, obj):
            for q in queries:
                d = distance(qkind, q, okind, obj, metric, approximate)
                if 0 < d < 1e300:
                    out.add(d)
    return sorted(out)


def case_radii(case, qkind, queries, metric, approximate, limit=3):
    """the layer regimes of the case's grid (guaranteed layers 1, 0 and -1), r = 0, and a few realized
    distances with their ulp neighbours"""
    cl = (case["grid"][1][1] - case["grid"][1][0]) / case["grid"][0]
    rs = [3.0 * cl, 1.6 * cl, 0.75 * cl, 0.0]
    near = [d for d in realized_distances(case["kind"], case["objs"], qkind, queries, metric, approximate) if d <= 3.0 * cl]
    for d in near[:: max(1, len(near) // limit)][:limit]:
        rs += [float(np.nextafter(d, 0.0)), d, float(np.nextafter(d, np.inf))]
    return rs
