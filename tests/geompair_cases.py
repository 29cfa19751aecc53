"""Case builders of the geometry-pair tests (tests/test_geompair_ref.py on the CPU, tests/test_gpu_geompair.py
on the GPU): hand-built segment pairs, hand-built geometry pairs and query sets on the 10 x 10 unit grid of
tests/geomwin_cases.py (cell length exactly 1).  A window case is geomwin_cases' dict (kind, grid, objs, keys);
its `queries` maps a name to (query kind, [query geometries]).  No GPU, no torch."""
from __future__ import annotations

import functools
import math

import numpy as np

import geomwin_cases as GC

POLYGON, LINESTRING = GC.POLYGON, GC.LINESTRING
UNIT = GC.UNIT
square, triangle, ngon, zigzag = GC.square, GC.triangle, GC.ngon, GC.zigzag
PAIRS = ((POLYGON, POLYGON), (POLYGON, LINESTRING), (LINESTRING, POLYGON), (LINESTRING, LINESTRING))  # (window, query)

# ---- segment pairs: (name, A, B, C, D, what the exact answer is or None) ---------------------------------
EPS = 2.0 ** -52
SEGMENT_PAIRS = [
    ("proper_crossing", (0.0, 0.0), (2.0, 2.0), (0.0, 2.0), (2.0, 0.0), 0.0),
    ("touch_endpoint_r0", (1.0, 1.0), (3.0, 1.0), (1.0, 0.0), (1.0, 2.0), 0.0),      # A on CD: r == 0
    ("touch_endpoint_r1", (0.0, 1.0), (1.0, 1.0), (1.0, 0.0), (1.0, 2.0), 0.0),      # B on CD: r == 1
    ("touch_endpoint_s0", (0.0, 0.0), (2.0, 0.0), (1.0, 0.0), (1.0, 3.0), 0.0),      # C on AB: s == 0
    ("touch_endpoint_s1", (0.0, 0.0), (2.0, 0.0), (1.0, 3.0), (1.0, 0.0), 0.0),      # D on AB: s == 1
    ("shared_endpoint", (0.0, 0.0), (1.0, 1.0), (1.0, 1.0), (2.0, 0.0), 0.0),
    ("collinear_overlapping", (0.0, 0.0), (2.0, 0.0), (1.0, 0.0), (3.0, 0.0), 0.0),  # denom == 0: the point-segment minimum
    ("collinear_disjoint", (0.0, 0.0), (1.0, 0.0), (3.0, 0.0), (4.0, 0.0), 2.0),
    ("collinear_diagonal", (0.0, 0.0), (1.0, 1.0), (3.0, 3.0), (4.0, 4.0), None),
    ("parallel", (0.0, 0.0), (2.0, 0.0), (0.5, 1.0), (1.5, 1.0), 1.0),
    ("parallel_offset", (0.0, 0.0), (2.0, 0.0), (3.0, 1.0), (5.0, 1.0), None),
    ("a_equals_b", (1.0, 1.0), (1.0, 1.0), (0.0, 0.0), (2.0, 0.0), 1.0),
    ("c_equals_d", (0.0, 0.0), (2.0, 0.0), (1.0, 1.0), (1.0, 1.0), 1.0),
    ("both_degenerate", (1.0, 1.0), (1.0, 1.0), (4.0, 5.0), (4.0, 5.0), 5.0),
    ("both_degenerate_same", (1.0, 1.0), (1.0, 1.0), (1.0, 1.0), (1.0, 1.0), 0.0),
    ("envelope_disjoint", (0.0, 0.0), (1.0, 1.0), (2.0, 0.0), (3.0, 1.0), None),
    ("envelopes_meet_no_crossing", (0.0, 0.0), (2.0, 2.0), (1.5, 0.0), (2.0, 0.4), None),
    ("near_parallel_tiny_denom", (0.0, 0.0), (1.0, 1.0), (0.0, 1e-9), (1.0, 1.0 + 1e-9 + 4 * EPS), None),
    ("near_parallel_crossing", (0.0, 0.0), (1.0, 1.0), (0.0, 2 * EPS), (1.0, 1.0 - 2 * EPS), 0.0),
    ("t_junction_interior", (0.0, 0.0), (4.0, 0.0), (2.0, 0.0), (2.0, 5.0), 0.0),
    ("perpendicular_gap", (0.0, 0.0), (4.0, 0.0), (2.0, 0.3), (2.0, 5.0), 0.3),
]


def random_segment_pairs(n=400, seed=11):
    """on a coarse lattice, so that touching, collinear and degenerate pairs occur often"""
    rnd = np.random.default_rng(seed)
    v = rnd.integers(0, 5, (n, 8)).astype(np.float64) * 0.25
    return [((r[0], r[1]), (r[2], r[3]), (r[4], r[5]), (r[6], r[7])) for r in v]


# ---- geometry pairs ---------------------------------------------------------------------------------------
Q_HOLED = [square(2.0, 2.0, 6.0), square(4.0, 4.0, 2.0)]   # the hole (4, 4) - (6, 6)
Q_RING_CHAIN = square(2.0, 2.0, 6.0)                       # the same shell as a closed linestring: contains nothing

# shapes (closed rings) placed against Q_HOLED; as a linestring window each is its shell taken as a chain
SHAPES = [
    ("inside_no_contact", [square(2.5, 2.5, 0.5)]),            # 0 by the first-vertex rule; 0.5 from the chain
    ("inside_hole", [square(4.5, 4.5, 0.5)]),                  # inside the hole: the distance to the hole ring, 0.5
    ("first_vertex_on_edge", [[(2.0, 3.0), (1.5, 3.0), (1.5, 3.5), (2.0, 3.0)]]),
    ("first_vertex_on_vertex", [[(8.0, 8.0), (8.5, 8.5), (8.5, 8.0), (8.0, 8.0)]]),
    ("first_outside_crossing", [[(1.0, 5.0), (3.0, 5.0), (3.0, 5.5), (1.0, 5.0)]]),   # 0 by intersection
    ("contains_query", [square(1.0, 1.0, 8.0)]),               # the query wholly inside a window polygon
    ("query_in_its_hole", [square(0.5, 0.5, 9.0), square(1.5, 1.5, 7.0)]),  # polygon: 0.5 (hole ring to the shell)
    ("apart_right", [square(8.5, 2.0, 0.5)]),                  # 0.5
    ("apart_diagonal", [square(8.3, 8.4, 0.5)]),               # a corner-to-corner distance
    ("touching_edge", [square(8.0, 5.0, 0.5)]),                # shares part of the edge x = 8
    ("collinear_apart", [[(8.0, 8.5), (8.0, 9.5), (8.7, 9.5), (8.0, 8.5)]]),          # collinear with x = 8, 0.5 above
    ("straddles_hole_edge", [square(3.5, 4.5, 1.0)]),          # first vertex in the solid part, crosses the hole ring
    ("on_hole_edge", [[(4.0, 5.0), (4.5, 5.2), (4.5, 4.8), (4.0, 5.0)]]),             # first vertex on the hole's ring
    ("far", [square(0.1, 0.1, 0.3)]),
]
INVALID = {POLYGON: [[[(5.1, 5.1), (5.3, 5.1), (5.1, 5.1)]], [[(5.1, 5.1), (5.3, 5.1), (5.3, 5.3), (5.1, 5.3)]], []],
           LINESTRING: [[(5.5, 5.5)], []]}


def as_kind(kind, rings):
    return rings if kind == POLYGON else list(rings[0])


def _case(kind, objs, queries, keys=None):
    keys = np.arange(len(objs), dtype=np.int64) if keys is None else np.asarray(keys, np.int64)
    return dict(kind=kind, grid=UNIT, objs=objs, keys=keys, queries=queries)


QUERY_SETS = {
    # name: {query kind: [geometries]}
    "holed": {POLYGON: [Q_HOLED], LINESTRING: [Q_RING_CHAIN]},
    "small": {POLYGON: [[square(5.2, 5.2, 0.5)]], LINESTRING: [[(5.2, 5.2), (5.7, 5.6)]]},
    "overlapping": {POLYGON: [[square(1.2, 1.2, 1.0)], [square(1.8, 1.5, 1.5)], [triangle(7.2, 7.2, 0.9)]],
                    LINESTRING: [[(1.2, 1.2), (2.2, 2.1)], [(1.8, 1.5), (3.3, 1.6), (3.2, 3.0)], [(7.2, 7.2), (8.1, 7.4)]]},
    "leaving": {POLYGON: [[square(-0.6, 4.2, 1.0)]], LINESTRING: [[(-0.6, 4.2), (0.4, 5.2)]]},   # R_q = [-1..0] x [4..5]
    "outside": {POLYGON: [[square(-1.6, 4.2, 0.3)]], LINESTRING: [[(-1.6, 4.2), (-1.3, 4.5)]]},  # R_q wholly outside
}
REFUSED_SETS = {
    "leaving_set": {POLYGON: [[square(-0.6, 4.2, 1.0)], [square(5.2, 5.2, 0.5)]],
                    LINESTRING: [[(-0.6, 4.2), (0.4, 5.2)], [(5.2, 5.2), (5.7, 5.6)]]},
}
# objects for the out-of-grid corner: in cell (-1, 4) outside the grid (matches G at layers 0), partly out and
# within R_q, beyond R_q in cell (-2, 4) (dropped by the filter though within r), out above the rectangle
CORNER_SHAPES = [
    ("out_cell_in_rq", [square(-0.9, 4.3, 0.2)]),
    ("partly_out_in_rq", [square(-0.5, 4.5, 0.8)]),
    ("out_cell_beyond_rq", [square(-1.9, 4.3, 0.2)]),
    ("out_and_wider_than_rq", [square(-0.5, 4.5, 1.8)]),
    ("in_grid_near", [square(1.2, 4.4, 0.3)]),
]


@functools.lru_cache(maxsize=None)
def pairs(kind):
    """the hand-built geometry pairs, the corner objects, the invalid objects and a background of one small
    object per cell, as a window of `kind`"""
    objs = [as_kind(kind, s) for _, s in SHAPES + CORNER_SHAPES] + INVALID[kind]
    for i in range(10):
        for j in range(10):
            objs.append(as_kind(kind, [triangle(i + 0.3, j + 0.35, 0.25)]))
    keys = [(7 * i) % 23 for i in range(len(objs))]   # duplicate objID keys
    return _case(kind, objs, QUERY_SETS, keys)


@functools.lru_cache(maxsize=None)
def sized(kind, n):
    c = GC.sized(kind, n)
    return dict(c, queries=QUERY_SETS)


def long_chain(nseg, x0=1.0, y0=5.0, x1=9.0, amp=0.4):
    """a zigzag of nseg segments across the grid"""
    return [(x0 + (x1 - x0) * i / nseg, y0 + (amp if i & 1 else 0.0) + 0.3 * math.sin(i / 97.0)) for i in range(nseg + 1)]


@functools.lru_cache(maxsize=None)
def long_queries(nseg=2000):
    """a long query linestring and a long query ring (a polygon with a hole) of about nseg segments"""
    return {POLYGON: [[ngon(5.0, 5.0, 2.6, nseg + 1), ngon(5.0, 5.0, 1.0, 65)]], LINESTRING: [long_chain(nseg)]}


@functools.lru_cache(maxsize=None)
def with_long_object(kind, nv=1000):
    """the sized window of 257 with one object of about nv vertices (taken by a wave at the default threshold)"""
    c = GC.sized(kind, 257)
    big = [ngon(4.6, 5.3, 1.7, nv), ngon(4.6, 5.3, 0.6, 40)] if kind == POLYGON else long_chain(nv - 1, 0.5, 3.0, 9.5, 0.7)
    objs = list(c["objs"]) + [big]
    keys = np.concatenate([c["keys"], [5]])
    return dict(kind=kind, grid=UNIT, objs=objs, keys=keys, queries=QUERY_SETS)


@functools.lru_cache(maxsize=None)
def segment_window(n_lattice=400):
    """every hand-built and lattice segment pair's CD as a 2-vertex linestring object (a degenerate CD is a
    legal chain of two equal vertices); the ABs are the queries, one at a time"""
    pairs = [(a, b, c, d) for _, a, b, c, d, _ in SEGMENT_PAIRS] + random_segment_pairs(n_lattice)
    objs = [[c, d] for _, _, c, d in pairs]
    return _case(LINESTRING, objs, {}), [[a, b] for a, b, _, _ in pairs]


# zero-length edges inside rings and chains (a repeated vertex at the start, in the middle, before the
# closing vertex), and boxes of zero width or height for the approximate distance
DEGENERATE_RINGS = [
    [(2.0, 2.0), (2.0, 2.0), (3.0, 2.0), (3.0, 3.0), (2.0, 3.0), (2.0, 2.0)],
    [(5.0, 2.0), (6.0, 2.0), (6.0, 2.0), (6.0, 3.0), (5.0, 3.0), (5.0, 3.0), (5.0, 2.0)],
    [(2.5, 5.0), (3.5, 5.0), (3.5, 6.0), (3.5, 6.0), (3.5, 6.0), (2.5, 5.0)],
    [(6.2, 6.2), (6.2, 6.2), (6.2, 6.2), (6.2, 6.2)],                       # a ring of one point, four times
    [(4.0, 4.0), (4.6, 4.0), (4.0, 4.0), (4.0, 4.0)],                       # a ring collapsed to a segment
]
AXIS_CHAINS = [
    [(4.0, 1.5), (5.5, 1.5)],     # zero height, below the vertical query and across its x
    [(5.0, 7.0), (5.0, 8.5)],     # zero width, collinear with the vertical query
    [(7.0, 4.5), (7.0, 5.5)],     # zero width, beside it
    [(1.0, 5.0), (4.0, 5.0)],     # zero height, beside it
    [(5.0, 5.0), (5.0, 5.0)],     # a point on it
    [(4.5, 3.0), (5.5, 3.2)],     # an ordinary box below it
]
DEGENERATE_QUERIES = {
    "repeated": {POLYGON: [[[(3.2, 2.4), (3.2, 2.4), (4.4, 2.4), (4.4, 3.4), (4.4, 3.4), (3.2, 3.4), (3.2, 2.4)]]],
                 LINESTRING: [[(3.2, 2.4), (3.2, 2.4), (4.4, 2.4), (4.4, 2.4), (4.4, 3.4)]]},
    "vertical": {POLYGON: [[[(5.0, 4.0), (5.0, 6.0), (5.0, 4.0), (5.0, 4.0)]]],   # a ring with a zero-width box
                 LINESTRING: [[(5.0, 4.0), (5.0, 6.0)]]},
    "horizontal": {POLYGON: [[[(4.0, 5.0), (6.0, 5.0), (4.0, 5.0), (4.0, 5.0)]]],
                   LINESTRING: [[(4.0, 5.0), (6.0, 5.0)]]},
}


@functools.lru_cache(maxsize=None)
def degenerate(kind):
    if kind == POLYGON:
        objs = [[r] for r in DEGENERATE_RINGS] + [[square(1.5, 1.5, 2.0), DEGENERATE_RINGS[0]]]
        objs += [[[c[0], c[1], c[0], c[0]]] for c in AXIS_CHAINS]   # the chain there and back: a ring with the same box
    else:
        objs = [list(r) for r in DEGENERATE_RINGS] + [list(c) for c in AXIS_CHAINS]
        objs += [[(3.0, 3.0), (3.0, 3.0), (3.0, 3.0)], [(8.0, 8.0), (8.5, 8.5), (8.5, 8.5), (9.0, 8.0)]]
    return _case(kind, objs, DEGENERATE_QUERIES)


def csr(case):
    return GC.csr(case)


def query_csr(qkind, queries):
    """(ring_off or None, vert_off, vx, vy): the query set as the C ABI takes it"""
    return GC.csr(dict(kind=qkind, objs=queries))
