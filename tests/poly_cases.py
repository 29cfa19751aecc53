"""Shared case generator of the polygon-geometry tests (tests/test_poly_geometry.py on the CPU,
tests/test_gpu_poly_geometry.py on the GPU): a catalogue of degenerate and many-vertex polygons
placed in the Beijing grid (n = 100), probes on and around every vertex, edge, vertex ordinate and
envelope side, a window per shape -- and an INDEPENDENT reference of the JTS 1.16.1 point-polygon
geometry (RayCrossingCounter behind PointLocator's envelope test, RobustDeterminant's sign,
Distance.pointToSegment, DistanceOp's shell / holes containment and facet distance) and of the
three polygon operators built on it, in numpy float64 (element-wise IEEE arithmetic, unfused: what
Java computes), vectorized over the points.  The orientation sign is exact: the plain-double
determinant decides where its rounding error bound certifies the sign, fractions.Fraction
(tests/golden/pyref.py) everywhere else.  The reference never calls the C oracle, except for the
hypot metric's distance values (the hypot the CPU tests tie to rational arithmetic, as in
tests/edge_cases.py).  No GPU, no torch."""
from __future__ import annotations

import functools
import math
import random

import numpy as np

import edge_cases as E
import pyref

BEIJING = E.BEIJING
GRID_N = 100
CL = (BEIJING[1] - BEIJING[0]) / GRID_N
U = 2.0 ** -46                 # the lattice unit: spacing of doubles in [64, 128)
DBL_MAX = 1.7976931348623157e308
LOC_I, LOC_B, LOC_E = 0, 1, 2
# The operators have no cells at r == 0 (guaranteed layers -1, candidate layers 0): they return
# nothing.  TINY stands for "d <= 0" with one candidate layer: every nonzero distance the
# catalogue realizes is far above it (asserted by the CPU tests), so a point is within TINY of a
# polygon exactly when its computed distance is 0.
TINY = 2.0 ** -70
BIG_R = 2.5 * CL               # guaranteed layers 0 (the bbox cells), candidate layers 3
KNN_R = 2.0 * CL
JOIN_KEEP = 4                  # kJoinKeep of the join kernels
JOIN_WORK = 1024               # worklist entries per block round (kJoinWork)
JOIN_ROUND = 256               # queued points per block round (kBlock)


# Switch of one "teeth" check: False drops pointToSegment's A == B branch, as a restatement without
# it would compute (len2 == 0: r and s are 0 / 0 = NaN, and a NaN distance is never the minimum).
DEGENERATE_BRANCH = True
# Switch of another: False lets RayCrossingCounter's horizontal-edge branch `continue` without its
# boundary test (a point on a horizontal edge is then located by the crossing parity alone).
HORIZONTAL_BRANCH = True


def ulps(v, k):
    for _ in range(abs(k)):
        v = np.nextafter(v, np.inf if k > 0 else -np.inf)
    return float(v)


# ---------------------------------------------------------------------------------------------
# the independent reference: geometry
# ---------------------------------------------------------------------------------------------
def sign_det(x1, y1, x2, y2, exact=True):
    """Sign of x1*y2 - y1*x2 per element.  exact: the plain-double sign where |det| exceeds its
    rounding error bound (two rounded products and one rounded difference: below
    2^-52 (|x1 y2| + |y1 x2|); 2^-50 is used), Fraction arithmetic elsewhere.  not exact: the
    plain-double sign (the switch of the "teeth" checks)."""
    a, b = x1 * y2, y1 * x2
    det = a - b
    s = np.sign(det).astype(np.int64)
    if exact:
        unsure = ~(np.abs(det) > 2.0 ** -50 * (np.abs(a) + np.abs(b)))
        for k in np.flatnonzero(unsure):
            s[k] = pyref._sgn_det(float(x1[k]), float(y1[k]), float(x2[k]), float(y2[k]))
    return s


def _closed(ring):
    ring = [(float(a), float(b)) for a, b in ring]
    return ring if ring[0] == ring[-1] else ring + [ring[0]]


def ring_area(ring):
    a = 0.0
    for (x1, y1), (x2, y2) in zip(ring[:-1], ring[1:]):
        a += x1 * y2 - x2 * y1
    return abs(a) / 2.0


def ordered(poly):
    """Closed rings, the largest-area ring first (Polygon.createPolygonArray: the shell), the others
    by descending area.  The catalogue's rings have distinct areas."""
    rings = [_closed(r) for r in poly]
    return sorted(rings, key=ring_area, reverse=True) if len(rings) > 1 else rings


def envelope(ring):
    xs, ys = [v[0] for v in ring], [v[1] for v in ring]
    return min(xs), max(xs), min(ys), max(ys)


def ring_locate(px, py, ring, exact=True):
    """PointLocator.locateInPolygonRing per point: LOC_E outside the ring's envelope, else
    RayCrossingCounter.locatePointInRing.  A return of BOUNDARY is absorbing, so the edges may be
    taken one at a time over all points."""
    minx, maxx, miny, maxy = envelope(ring)
    out = np.full(len(px), LOC_E, np.int8)
    # a NaN x never reaches the locator (polygon_distance): it stays LOC_E here
    idx = np.flatnonzero(~((px > maxx) | (px < minx) | (py > maxy) | (py < miny)) & (px == px))
    x, y = px[idx], py[idx]
    bnd = np.zeros(len(idx), bool)
    cross = np.zeros(len(idx), np.int64)
    for i in range(1, len(ring)):
        (p1x, p1y), (p2x, p2y) = ring[i], ring[i - 1]
        act = ~((p1x < x) & (p2x < x))
        bnd |= act & (x == p2x) & (y == p2y)
        if p1y == p2y:   # the horizontal-edge branch (for the other points the crossing test is false)
            if HORIZONTAL_BRANCH:
                bnd |= act & (y == p1y) & (x >= min(p1x, p2x)) & (x <= max(p1x, p2x))
            continue
        j = np.flatnonzero(act & (((p1y > y) & (p2y <= y)) | ((p2y > y) & (p1y <= y))))
        if len(j):
            x1, y1, x2, y2 = p1x - x[j], p1y - y[j], p2x - x[j], p2y - y[j]
            s = sign_det(x1, y1, x2, y2, exact)
            bnd[j] |= s == 0
            s = np.where(y2 < y1, -s, s)
            cross[j] += s > 0
    out[idx] = np.where(bnd, LOC_B, np.where(cross % 2 == 1, LOC_I, LOC_E))
    return out


def env_distance(ring, px, py):
    """Envelope.distance of the ring's envelope to the point's."""
    minx, maxx, miny, maxy = envelope(ring)
    with np.errstate(all="ignore"):
        out = (px > maxx) | (px < minx) | (py > maxy) | (py < miny)
        dx = np.where(maxx < px, px - maxx, np.where(minx > px, minx - px, 0.0))
        dy = np.where(maxy < py, py - maxy, np.where(miny > py, miny - py, 0.0))
        d = np.where(dx == 0.0, dy, np.where(dy == 0.0, dx, np.sqrt(dx * dx + dy * dy)))
    return np.where(out, d, 0.0)


def _segment(px, py, a, b):
    """Distance.pointToSegment's case analysis -> (end, dx, dy, interior distance): where `end`, the
    distance is distance(p, an endpoint) with the differences (dx, dy); elsewhere fabs(s) * sqrt(len2)."""
    (ax, ay), (bx, by) = a, b
    if ax == bx and ay == by:
        if DEGENERATE_BRANCH:
            return np.ones(len(px), bool), px - ax, py - ay, None
        return np.zeros(len(px), bool), px - ax, py - ay, np.full(len(px), np.nan)   # 0 / 0 throughout
    len2 = (bx - ax) * (bx - ax) + (by - ay) * (by - ay)
    r = ((px - ax) * (bx - ax) + (py - ay) * (by - ay)) / len2
    enda = r <= 0.0
    endb = ~enda & (r >= 1.0)
    s = ((ay - py) * (bx - ax) - (ax - px) * (by - ay)) / len2
    return enda | endb, np.where(enda, px - ax, px - bx), np.where(enda, py - ay, py - by), np.abs(s) * math.sqrt(len2)


def ring_min_distance(px, py, ring, metric=0, hyp=None):
    """min over the ring's segments of pointToSegment, NaN never taken (d < md).  metric 1 calls
    hyp(dx, dy) only for the endpoint cases that can be the minimum: the sqrt form is within 3 ulps
    and hyp within 1 ulp of the true value, so an endpoint whose sqrt form exceeds the ring's sqrt-form
    minimum by more than 1e-9 relative has a hyp above the minimum."""
    def sweep(bound):
        m = np.full(len(px), np.inf)
        for a, b in zip(ring[:-1], ring[1:]):
            end, dx, dy, di = _segment(px, py, a, b)
            d = np.sqrt(dx * dx + dy * dy)
            if bound is not None:
                need = end & (d <= bound)
                d = np.where(end, np.inf, d)
                if need.any():
                    d[need] = hyp(dx[need], dy[need])
            if di is not None:
                d = np.where(end, d, di)
            m = np.where(d < m, d, m)
        return m
    with np.errstate(all="ignore"):
        m0 = sweep(None)
        return m0 if metric == 0 else sweep(m0 * (1 + 1e-9))


def polygon_distance(px, py, rings, metric=0, hyp=None, exact=True):
    """DistanceOp(point, polygon).distance() per point -> (d, [location per ring]).  rings: closed,
    the shell first.  A NaN x skips the containment test (the restatement's documented deviation)."""
    px, py = np.asarray(px, np.float64), np.asarray(py, np.float64)
    locs = [ring_locate(px, py, rg, exact) for rg in rings]
    shell = np.where(px == px, locs[0], LOC_E)
    zero = shell == LOC_B
    und = shell == LOC_I                    # inside the shell, no hole has decided yet
    for hl in locs[1:]:
        zero |= und & (hl == LOC_B)
        und &= hl == LOC_E                  # INTERIOR of a hole: not inside, the loop ends
    zero |= und
    md = np.full(len(px), DBL_MAX)
    for rg in rings:
        skip = env_distance(rg, px, py) > md
        rm = ring_min_distance(px, py, rg, metric, hyp)
        md = np.where(~skip & (rm < md), rm, md)
    return np.where(zero, 0.0, md), locs


def bbox_distance(x, y, bb):
    """DistanceFunctions.getPointPolygonBBoxMinEuclideanDistance per point; bb = (x1, y1, x2, y2)."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    x1, y1, x2, y2 = bb

    def ppe(lon1, lat1):
        a, b = lat1 - y, lon1 - x
        return np.sqrt(a * a + b * b)

    def border(ax, ay, bx, by):
        if ax == bx:
            return ppe(ax, y)
        if ay == by:
            return ppe(x, ay)
        return np.full(len(x), 5e-324)
    with np.errstate(all="ignore"):
        left, right, lo, hi = x <= x1, x >= x2, y <= y1, y >= y2
        return np.select([left & lo, left & hi, left, right & lo, right & hi, right, lo, hi],
                         [ppe(x1, y1), ppe(x1, y2), border(x1, y1, x1, y2), ppe(x2, y1), ppe(x2, y2),
                          border(x2, y1, x2, y2), border(x1, y1, x2, y1), border(x1, y2, x2, y2)], 0.0)


def shell_bbox(rings):
    minx, maxx, miny, maxy = envelope(rings[0])
    return minx, miny, maxx, maxy


# ---------------------------------------------------------------------------------------------
# the independent reference: operators
# ---------------------------------------------------------------------------------------------
class Grid:
    def __init__(self, n=GRID_N, box=BEIJING):
        self.n = n
        self.minX, self.maxX, self.minY, self.maxY = box
        self.cl = (self.maxX - self.minX) / n

    def cells(self, x, y):
        return (E.ref_cells(x, self.minX, self.cl).astype(np.int64), E.ref_cells(y, self.minY, self.cl).astype(np.int64))

    def valid(self, cx, cy):
        return (cx >= 0) & (cy >= 0) & (cx < self.n) & (cy < self.n)

    def layers(self, r):
        return E.ref_layers(self.cl, r)

    def poly_cells(self, cx, cy, bb, r):
        """(inG, inC) of one polygon: its bbox cells B (no validity test), G = B for 0 guaranteed
        layers / the valid cells within g > 0 layers of B, C = the valid cells within the candidate
        layers of B."""
        gl, cL = self.layers(r)
        (x1, x2), (y1, y2) = self.cells(np.array([bb[0], bb[2]]), np.array([bb[1], bb[3]]))
        valid = self.valid(cx, cy)

        def within(k):
            return (cx >= x1 - k) & (cx <= x2 + k) & (cy >= y1 - k) & (cy <= y2 + k)
        inG = within(0) if gl == 0 else (valid & within(gl) if gl > 0 else np.zeros(len(cx), bool))
        inC = valid & within(cL) if cL > 0 else np.zeros(len(cx), bool)
        return inG, inC


def near_mask(G, x, y, bb, layers=4):
    """Points whose cell lies within `layers` cells of the bbox cells: the only ones an operator at
    r <= (layers - 1) cell lengths can ask the polygon's distance for with an answer <= r."""
    cx, cy = G.cells(x, y)
    (x1, x2), (y1, y2) = G.cells(np.array([bb[0], bb[2]]), np.array([bb[1], bb[3]]))
    return (cx >= x1 - layers) & (cx <= x2 + layers) & (cy >= y1 - layers) & (cy <= y2 + layers)


def distance_matrix(G, x, y, polys, metric=0, hyp=None, exact=True, approximate=False):
    """[npoly, n]: the (approximate: bbox) distance of every point to every polygon (ordered rings);
    +inf where the point is more than 4 cells from the polygon's bbox cells (see near_mask)."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    D = np.full((len(polys), len(x)), np.inf)
    for q, rings in enumerate(polys):
        bb = shell_bbox(rings)
        m = np.flatnonzero(near_mask(G, x, y, bb))
        if approximate:
            D[q, m] = bbox_distance(x[m], y[m], bb)
        else:
            D[q, m] = polygon_distance(x[m], y[m], rings, metric, hyp, exact)[0]
    return D


def ref_range_ppoly(G, x, y, polys, r, D):
    """The window-based point-polygon range query -> ascending indices: a point of a guaranteed
    cell, or of a candidate cell with some polygon within r.  D = distance_matrix(...)."""
    cx, cy = G.cells(x, y)
    inG = np.zeros(len(cx), bool)
    inC = np.zeros(len(cx), bool)
    for rings in polys:
        g, c = G.poly_cells(cx, cy, shell_bbox(rings), r)
        inG |= g
        inC |= c
    return np.flatnonzero(inG | (inC & (D <= r).any(axis=0)))


def ref_join_ppoly(G, x, y, polys, r, D, approximate=False):
    """The point-polygon window join -> sorted pairs [m, 2] (point, polygon): polygon q is replicated
    to its own guaranteed and candidate cells, a co-located pair is kept if approximate or d <= r."""
    cx, cy = G.cells(x, y)
    out = []
    for q, rings in enumerate(polys):
        g, c = G.poly_cells(cx, cy, shell_bbox(rings), r)
        key = g | c
        p = np.flatnonzero(key if approximate else key & (D[q] <= r))
        out.append(np.stack([p, np.full(len(p), q, np.int64)], axis=1))
    out = np.concatenate(out) if out else np.zeros((0, 2), np.int64)
    return out[np.lexsort((out[:, 1], out[:, 0]))].astype(np.int64)


def ref_knn_ppoly(G, x, y, obj, rings, r, k, d):
    """The polygon-query kNN contract: points of the polygon's candidate / guaranteed cells with
    d <= r, one entry per objID (its smallest (d, idx)), ordered by (d, objID), the first k ->
    (objID, d, idx).  d = distance_matrix(...)[0]."""
    cx, cy = G.cells(x, y)
    g, c = G.poly_cells(cx, cy, shell_bbox(rings), r)
    idx = np.flatnonzero((g | c) & (d <= r))
    o, dd = np.asarray(obj, np.int64)[idx], d[idx]
    order = np.lexsort((idx, dd, o))
    o, dd, idx = o[order], dd[order], idx[order]
    first = np.ones(len(o), bool)
    first[1:] = o[1:] != o[:-1]
    o, dd, idx = o[first], dd[first], idx[first]
    order = np.lexsort((o, dd))[:k]
    return o[order], dd[order], idx[order]


# ---------------------------------------------------------------------------------------------
# the catalogue
# ---------------------------------------------------------------------------------------------
def _rect(x1, y1, x2, y2):
    return [(x1, y1), (x2, y1), (x2, y2), (x1, y2), (x1, y1)]


def _comb():
    """Four axis-aligned teeth, a pointed tooth whose peak sits at the tops' ordinate (up-down), a V
    valley at the valleys' ordinate, and a collinear vertex at the valleys' ordinate on each vertical
    side (up-up on the left, down-down on the right)."""
    X, Y, W = 116.0, 40.0, 2.0 ** -7
    yb, yv, yt = Y, Y + W, Y + 3 * W
    v = [(X, yb), (X, yv), (X, yt)]
    for t in range(4):
        a = X + 2 * t * W
        v += [(a + W, yt), (a + W, yv), (a + 2 * W, yv), (a + 2 * W, yt)]
    v.pop()                                      # the fifth tooth is the pointed one
    v += [(X + 8.5 * W, yt), (X + 9 * W, yv), (X + 10 * W, yt), (X + 10 * W, yv), (X + 10 * W, yb), (X, yb)]
    return [[v]]


def _star():
    """14 vertices, 7 reflex, symmetric about a vertical axis: mirrored vertices share an ordinate
    exactly (offsets are multiples of 2^-20 from a dyadic centre, so edge midpoints are exact too)."""
    cx, cy, q = 116.3125, 40.3125, 2.0 ** 20
    off = []
    for i in range(8):   # from the top vertex down the right side
        rad = 0.1 if i % 2 == 0 else 0.04
        ang = math.pi / 2 - 2 * math.pi * i / 14
        off.append((round(rad * math.cos(ang) * q) / q, round(rad * math.sin(ang) * q) / q))
    off[0] = (0.0, off[0][1])
    off[7] = (0.0, off[7][1])
    right = [(cx + dx, cy + dy) for dx, dy in off]
    left = [(cx - dx, cy + dy) for dx, dy in off[6:0:-1]]
    return [[right + left + [right[0]]]]


def _staircase():
    x, y, s = 116.5, 40.0, 2.0 ** -4
    return [[[(x, y), (x + 3 * s, y), (x + 3 * s, y + s), (x + 2 * s, y + s), (x + 2 * s, y + 2 * s), (x + s, y + 2 * s),
              (x + s, y + 3 * s), (x, y + 3 * s), (x, y)]]]


RECT_BOX = (115.625, 40.5, 115.625 + 5 * 2.0 ** -6, 40.5625)   # the box of the true rectangles
NEAR_RECTS = ("plain", "mid_vertex", "dup_corner", "cw0", "cw1", "cw2", "cw3", "bowtie", "three_corners", "zero_width")
TRUE_RECTS = NEAR_RECTS[1:7]
NON_RECTS = NEAR_RECTS[7:]


def _near_rects():
    x1, y1, x2, y2 = RECT_BOX
    xm = x1 + 2 * 2.0 ** -6
    cw = [(x1, y1), (x1, y2), (x2, y2), (x2, y1)]
    out = [[_rect(x1, y1, x2, y2)],
           [[(x1, y1), (xm, y1), (x2, y1), (x2, y2), (x1, y2), (x1, y1)]],
           [[(x1, y1), (x2, y1), (x2, y1), (x2, y2), (x1, y2), (x1, y1)]]]
    out += [[cw[s:] + cw[:s] + [cw[s]]] for s in range(4)]
    bx, cx_, zx = x1 + 0.15625, x1 + 0.3125, x1 + 0.46875
    w, h = x2 - x1, y2 - y1
    out.append([[(bx, y1), (bx + w, y1), (bx, y1 + h), (bx + w, y1 + h), (bx, y1)]])          # all four corners
    out.append([[(cx_, y1), (cx_ + w, y1), (cx_ + w, y1 + h), (cx_ + w, y1), (cx_, y1)]])     # three corners, back along a side
    out.append([[(zx, y1), (zx, y1 + h), (zx, y1 + h), (zx, y1), (zx, y1)]])                 # zero width
    return out


def _holed(hole_first=False):
    """A shell with three holes: a triangle touching the shell at a shell vertex, a triangle sharing
    an ordinate with a shell vertex, a small square far from the other rings."""
    X, Y = 115.625, 39.6875
    s = 0.3125
    shell = [(X, Y), (X + s, Y), (X + s, Y + 0.125), (X + s + 0.03125, Y + 0.1875), (X + s, Y + s), (X, Y + s),
             (X, Y + 0.15625), (X, Y)]
    touch = [(X, Y + 0.15625), (X + 0.0625, Y + 0.125), (X + 0.0625, Y + 0.1875), (X, Y + 0.15625)]
    share = [(X + 0.125, Y + 0.125), (X + 0.1875, Y + 0.125), (X + 0.15625, Y + 0.21875), (X + 0.125, Y + 0.125)]
    far = _rect(X + 0.265625, Y + 0.015625, X + 0.28125, Y + 0.03125)
    return [[far, share, touch, shell] if hole_first else [shell, touch, share, far]]


def _spike_dup():
    X, Y = 116.1875, 39.6875
    return [[[(X, Y), (X + 0.1875, Y), (X + 0.1875, Y), (X + 0.1875, Y + 0.1875), (X + 0.09375, Y + 0.1875),
              (X + 0.09375, Y + 0.28125), (X + 0.09375, Y + 0.1875), (X, Y + 0.1875), (X, Y)]]]


def _sliver():
    a, b = (116.8, 40.2), (117.2, 40.47)
    return [[[a, b, (b[0], ulps(b[1], 40)), a]]]


def _circle(cx, cy, rad, nv):
    ring = [(cx + rad * math.cos(2 * math.pi * i / nv), cy + rad * math.sin(2 * math.pi * i / nv)) for i in range(nv)]
    return ring + [ring[0]]


def _ngon():
    return [[_circle(116.7, 39.75, 0.1, 1000)],
            [_circle(117.0, 39.75, 0.1, 1000), _circle(117.01, 39.76, 0.03, 300)]]


def _egcd(a, b):
    if b == 0:
        return a, 1, 0
    g, s, t = _egcd(b, a % b)
    return g, t, s - (a // b) * t


def collinear_case(rnd, jbits, lo=1):
    """(A, B, C, D, j): lattice offsets with A D - B C == j exactly, |j| in [2^(jbits-1), 2^jbits),
    every offset in [lo, 2^44)."""
    while True:
        c0, d0 = rnd.randrange(2 ** 9, 2 ** 11), rnd.randrange(2 ** 9, 2 ** 11)
        g, s, t = _egcd(c0, d0)
        if g != 1:
            continue
        a0, b0 = t, -s                          # a0 d0 - b0 c0 == 1
        M = rnd.randrange(2 ** 31, 2 ** 32)
        A, B = c0 * M + a0, d0 * M + b0
        j = rnd.choice((-1, 1)) * rnd.randrange(2 ** (jbits - 1), 2 ** jbits)
        C, D = A + j * c0, B + j * d0
        if min(A, B, C, D) < lo or max(A, B, C, D) >= 2 ** 44:
            continue
        assert A * D - B * C == j
        return A, B, C, D, j


def collinear_triangle(P, case):
    """The triangle p1 = P + (A, B) U, p2 = P - (C, D) U, far: its edge p1 p2 straddles P's ray at
    j U^2 / |p1 p2| from P."""
    A, B, C, D, _ = case
    p1, p2 = (P[0] + A * U, P[1] + B * U), (P[0] - C * U, P[1] - D * U)
    return [p1, p2, (P[0] + 0.3, P[1] - 0.2), p1]


TILED_N = 1536
STACK_N = 64
STACK_P = (117.0, 40.75)


@functools.lru_cache(maxsize=None)
def collinear_tiled():
    """(probes [(x, y)], polygons): TILED_N triangles with |j| in [2^30, 2^34), each translated with
    its probe by multiples of 2^-5 (the lattice stays exact)."""
    rnd = random.Random(46)
    pos = [(115.75 + i / 32, 39.875 + k / 32) for i in range(50) for k in range(36)]
    rnd.shuffle(pos)
    probes = pos[:TILED_N]
    polys = [[collinear_triangle(P, collinear_case(rnd, 31 + q % 4))] for q, P in enumerate(probes)]
    return probes, polys


@functools.lru_cache(maxsize=None)
def collinear_stacked():
    rnd = random.Random(64)
    return [[collinear_triangle(STACK_P, collinear_case(rnd, 31 + q % 4, lo=2 ** 40))] for q in range(STACK_N)]


def stack_core():
    """(x1, y1, x2, y2): a box inside every stacked triangle's envelope."""
    return STACK_P[0] - 2.0 ** -6, STACK_P[1] - 0.19, STACK_P[0] + 0.29, STACK_P[1] + 2.0 ** -6


SHAPES = ("comb", "star", "staircase", "near_rects", "holed", "holed_rev", "spike_dup", "sliver", "ngon")
NAMES = SHAPES + ("collinear_tiled", "collinear_stacked")


@functools.lru_cache(maxsize=None)
def raw_polygons(name):
    """The entry's polygons as a caller gives them (rings unordered, maybe open)."""
    if name == "collinear_tiled":
        return collinear_tiled()[1]
    if name == "collinear_stacked":
        return collinear_stacked()
    return {"comb": _comb, "star": _star, "staircase": _staircase, "near_rects": _near_rects, "holed": _holed,
            "holed_rev": lambda: _holed(True), "spike_dup": _spike_dup, "sliver": _sliver, "ngon": _ngon}[name]()


@functools.lru_cache(maxsize=None)
def polygons(name):
    """The entry's polygons as the geometry sees them: closed rings, the shell first."""
    return [ordered(p) for p in raw_polygons(name)]


# ---------------------------------------------------------------------------------------------
# probes and windows
# ---------------------------------------------------------------------------------------------
def _sub(seq, limit):
    seq = list(seq)
    return seq[::max(1, -(-len(seq) // limit))]


def shape_probes(rings):
    """The probes of one polygon (see the module docstring of tests/test_poly_geometry.py)."""
    px, py = [], []

    def add(a, b):
        px.append(float(a))
        py.append(float(b))
    for ring in rings:
        edges = list(zip(ring[:-1], ring[1:]))
        for (vx, vy) in _sub(ring[:-1], 40):                      # vertices and their 8 ulp neighbours
            for i in (-1, 0, 1):
                for k in (-1, 0, 1):
                    add(ulps(vx, i), ulps(vy, k))
        for (ax, ay), (bx, by) in _sub(edges, 40):                # on the edge and on its extension
            for t in (0.25, 0.5, 0.75, -0.5, 1.5):
                mx, my = ax + t * (bx - ax), ay + t * (by - ay)
                add(mx, my)
                for k in (-2, -1, 1, 2):
                    add(ulps(mx, k), my)
                    add(mx, ulps(my, k))
        minx, maxx, miny, maxy = envelope(ring)
        w, h = max(maxx - minx, CL / 4), max(maxy - miny, CL / 4)
        for yv in _sub(sorted({v[1] for v in ring}), 30):         # rays through the vertex ordinates
            for k in (-1, 0, 1):
                for xx in np.linspace(minx - 0.13 * w, maxx + 0.11 * w, 11):
                    add(xx, ulps(yv, k))
        for xx in (ulps(minx, -1), minx, (minx + maxx) / 2, maxx, ulps(maxx, 1)):   # envelope sides and corners
            for yy in (ulps(miny, -1), miny, (miny + maxy) / 2, maxy, ulps(maxy, 1)):
                add(xx, yy)
        rng = np.random.default_rng(len(ring))
        for xx, yy in zip(rng.uniform(minx, maxx, 60), rng.uniform(miny, maxy, 60)):  # interiors (holes' too)
            add(xx, yy)
        cx, cy = sum(v[0] for v in ring[:-1]) / (len(ring) - 1), sum(v[1] for v in ring[:-1]) / (len(ring) - 1)
        add(cx, cy)
    return px, py


def _sliver_extra(rings):
    """Interior points of the sliver (between its two long edges, near the wide end) and every double
    on its 40-ulp short edge."""
    (ax, ay), (bx, by), (cx, cy) = rings[0][:3]
    px, py = [], []
    for t in np.linspace(0.55, 0.99, 40):
        x = ax + t * (bx - ax)
        lo, hi = ay + (x - ax) / (bx - ax) * (by - ay), ay + (x - ax) / (cx - ax) * (cy - ay)
        px.append(x)
        py.append((lo + hi) / 2)
    for k in range(1, 40):
        px.append(bx)
        py.append(ulps(by, k))
    return px, py


@functools.lru_cache(maxsize=None)
def probes(name):
    """(x, y) of the entry's probes, read-only; the last four are NaN x, NaN y, both, and a point
    outside the grid."""
    polys = polygons(name)
    if name == "collinear_tiled":
        P = collinear_tiled()[0]
        px, py = [p[0] for p in P], [p[1] for p in P]
        for (x, y) in P[:64]:
            for i, k in ((-1, 0), (1, 0), (0, -1), (0, 1)):
                px.append(ulps(x, i))
                py.append(ulps(y, k))
    elif name == "collinear_stacked":
        px, py = [STACK_P[0]], [STACK_P[1]]
        for i in (-1, 0, 1):
            for k in (-1, 0, 1):
                px.append(ulps(STACK_P[0], i))
                py.append(ulps(STACK_P[1], k))
    else:
        px, py = [], []
        for rings in polys:
            a, b = shape_probes(rings)
            px += a
            py += b
        if name == "sliver":
            a, b = _sliver_extra(polys[0])
            px += a
            py += b
    minx, maxx, miny, maxy = extent(name)
    px += [np.nan, (minx + maxx) / 2, np.nan, BEIJING[0] - 0.01]
    py += [(miny + maxy) / 2, np.nan, np.nan, (miny + maxy) / 2]
    x, y = np.array(px), np.array(py)
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y


def extent(name):
    env = [envelope(rings[0]) for rings in polygons(name)]
    return min(e[0] for e in env), max(e[1] for e in env), min(e[2] for e in env), max(e[3] for e in env)


@functools.lru_cache(maxsize=None)
def window(name):
    """(x, y, objID, probe_idx): the entry's probes shuffled with a fixed seed into random points
    around the shape; n is odd and no multiple of 64; objIDs repeat.  probe_idx[i] is the window
    index of probe i."""
    px, py = probes(name)
    rng = np.random.default_rng(sum(map(ord, name)))
    minx, maxx, miny, maxy = extent(name)
    if name == "collinear_stacked":   # most points inside every triangle's envelope (see stack_core)
        x1, y1, x2, y2 = stack_core()
        nr = 1400
        rx = np.concatenate([rng.uniform(x1, x2, nr - 120), rng.uniform(minx - 4 * CL, maxx + 4 * CL, 120)])
        ry = np.concatenate([rng.uniform(y1, y2, nr - 120), rng.uniform(miny - 4 * CL, maxy + 4 * CL, 120)])
    else:
        nr = 600 if name == "collinear_tiled" else 5000
        rx = rng.uniform(minx - 4 * CL, maxx + 4 * CL, nr)
        ry = rng.uniform(miny - 4 * CL, maxy + 4 * CL, nr)
    n = len(px) + nr
    while n % 2 == 0 or n % 64 == 0:
        n += 1
    extra = n - len(px) - nr
    x = np.concatenate([px, rx, rng.uniform(minx, maxx, extra)])
    y = np.concatenate([py, ry, rng.uniform(miny, maxy, extra)])
    perm = rng.permutation(n)
    pidx = np.empty(n, np.int64)
    pidx[perm] = np.arange(n)
    x, y = x[perm], y[perm]
    obj = (np.arange(n) % max(1, n // 3)).astype(np.int64)
    probe_idx = pidx[:len(px)]
    for a in (x, y, obj, probe_idx):
        a.setflags(write=False)
    assert n <= 40_000
    return x, y, obj, probe_idx


_DIST = {}


def window_distances(name, metric, hyp, exact=True, approximate=False):
    """distance_matrix of the entry's window on the n = 100 grid, computed once."""
    key = (name, metric, exact, approximate)
    if key not in _DIST:
        x, y, _, _ = window(name)
        D = distance_matrix(Grid(), x, y, polygons(name), metric, hyp, exact, approximate)
        D.setflags(write=False)
        _DIST[key] = D
    return _DIST[key]


def realized_radii(name, metric, hyp):
    """[d]: realized distances of probes outside the shape (the smallest, about 0.3 and about 1.2
    cell lengths: below cl * sqrt(2), so that no cell is guaranteed and the probe at d flips between
    r = d and r = nextafter(d, 0)); for the holed shapes also the distance of a probe inside a hole."""
    x, y, _, pi = window(name)
    if name.startswith("collinear"):   # the probes lie inside other triangles: every window point serves
        pi = np.arange(len(x))
    D = window_distances(name, metric, hyp)
    d = D.min(axis=0)[pi]
    cx, cy = Grid().cells(x[pi], y[pi])
    ok = np.isfinite(d) & (d > 0) & (d < 1.3 * CL) & Grid().valid(cx, cy)
    if name.startswith("collinear"):
        ok &= d > 1e-6   # the probes' own 2^-56 distances are the TINY cases
    cand = np.sort(d[ok])
    out = [float(cand[0])] + [float(cand[np.argmin(np.abs(cand - t * CL))]) for t in (0.3, 1.2)]
    if name.startswith("holed"):
        rings = polygons(name)[0]
        inhole = ring_locate(x[pi], y[pi], rings[2]) == LOC_I
        out.append(float(np.sort(d[ok & inhole])[0]))
    return list(dict.fromkeys(out))


def radii(name, metric, hyp):
    """Every radius of the entry: 0 (no cells: empty results), TINY (d <= 0), the realized radii and
    their lower neighbours, and one of 2.5 cell lengths (guaranteed cells exist)."""
    out = [0.0, TINY]
    if name == "collinear_tiled":   # 1536 overlapping polygons: the smallest realized radius only, no BIG_R
        d = realized_radii(name, metric, hyp)[0]
        return out + [d, E.toward0(d)]
    for d in realized_radii(name, metric, hyp):
        out += [d, E.toward0(d)]
    return out + [BIG_R]


def gpu_radii(name, metric, hyp):
    """The radii the GPU file runs at every kernel variant: TINY, the first and the last realized
    radius with their lower neighbours, BIG_R (0 and the other realized radii run once, at the
    default variant)."""
    rr = realized_radii(name, metric, hyp)
    out = [TINY]
    for d in dict.fromkeys((rr[0], rr[-1]) if name != "collinear_tiled" else rr[:1]):
        out += [d, E.toward0(d)]
    return out + ([BIG_R] if name != "collinear_tiled" else [])
