"""The restatement of the six geometry-stream joins (include/geoflink_hip.h, "geometry-stream joins"):
{Polygon,LineString}{Point,Polygon,LineString}JoinQuery as a literal hash join -- the ordinary side replicated
to the cells of its rectangle, each query to its literally built cell set, joined on (cx, cy), tested with
d <= r in the operator's own argument order -- and, beside it, the closed form the library computes: E_q, the
multiplicity m, the tiles and the reference-tile rule, function for function as
spatialflink_amd/csrc/gf_geomjoin_plan.hpp states them (Python integers do not overflow, so m here is the
plain arithmetic).  Cell sets and distances come from tests/geompair_ref.py and tests/geomwin_ref.py.
No GPU, no torch."""
from __future__ import annotations

import geompair_ref as PR
import geomwin_ref as GR
import oracle as O

POLYGON, LINESTRING, POINT = GR.POLYGON, GR.LINESTRING, 0
LayersError = GR.LayersError
MAX_M = 2 ** 32 - 1
LONG_TILES = 16
MAX_TILE_SIDE = 1024

# name: (ordinary kind, query kind, the ordinary geometry is the distance's first argument)
OPERATORS = {
    "PolygonPointJoinQuery": (POLYGON, POINT, False),
    "LineStringPointJoinQuery": (LINESTRING, POINT, False),
    "PolygonPolygonJoinQuery": (POLYGON, POLYGON, False),
    "PolygonLineStringJoinQuery": (POLYGON, LINESTRING, True),   # getDistance(poly, q)
    "LineStringPolygonJoinQuery": (LINESTRING, POLYGON, False),
    "LineStringLineStringJoinQuery": (LINESTRING, LINESTRING, False),
}


def query_valid(qkind, q):
    return qkind == POINT or GR.valid(qkind, q)


def pair_distance(okind, obj, qkind, q, metric=0, approximate=False, first_is_ordinary=False):
    """the operator's d of two valid sides"""
    if qkind == POINT:
        return GR.distance(okind, obj, q[0], q[1], metric, approximate)
    if first_is_ordinary:
        return PR.distance(okind, obj, qkind, q, metric, approximate)
    return PR.distance(qkind, q, okind, obj, metric, approximate)


# ---- the literal join ---------------------------------------------------------------------------------------
def query_cell_set(qg, qkind, q, r):
    """K(q) as a set of (cx, cy), built cell by cell: getNeighboringCells for a point (LayersError when the
    candidate layers are not positive), G u C of getReplicated*QueryStream for a geometry"""
    if qkind == POINT:
        return GR.query_sets(qg, [q[0]], [q[1]], r)[0]
    return PR.query_sets(qg, qkind, [q], r)[0]


def join_literal(ug, qg, okind, objs, qkind, queries, r, approximate=False, metric=0, first_is_ordinary=False):
    """the multiset of emitted (ordinary idx, query idx), sorted: one entry per shared cell key"""
    table = {}
    for o, obj in enumerate(objs):
        if GR.valid(okind, obj):
            for cell in GR.cell_set(GR.cell_rect(ug, GR.bbox(okind, obj))):
                table.setdefault(cell, []).append(o)
    out = []
    for qi, q in enumerate(queries):
        if not query_valid(qkind, q):
            continue
        for cell in query_cell_set(qg, qkind, q, r):
            for o in table.get(cell, ()):
                if pair_distance(okind, objs[o], qkind, q, metric, approximate, first_is_ordinary) <= r:
                    out.append((o, qi))
    return sorted(out)


def key_matches(ug, qg, okind, objs, qkind, queries, r):
    """{(o, q): shared cell keys} of the same hash join before any distance test: the candidates and their m"""
    table = {}
    for o, obj in enumerate(objs):
        if GR.valid(okind, obj):
            for cell in GR.cell_set(GR.cell_rect(ug, GR.bbox(okind, obj))):
                table.setdefault(cell, []).append(o)
    out = {}
    for qi, q in enumerate(queries):
        if query_valid(qkind, q):
            for cell in query_cell_set(qg, qkind, q, r):
                for o in table.get(cell, ()):
                    out[(o, qi)] = out.get((o, qi), 0) + 1
    return out


def join_hashed(ug, qg, okind, objs, qkind, queries, r, approximate=False, metric=0, first_is_ordinary=False, info=None):
    """join_literal's distinct triples with each pair's distance taken once; info receives candidates and nrep"""
    cand = key_matches(ug, qg, okind, objs, qkind, queries, r)
    out = sorted((o, qi, min(m, MAX_M)) for (o, qi), m in cand.items()
                 if pair_distance(okind, objs[o], qkind, queries[qi], metric, approximate, first_is_ordinary) <= r)
    if info is not None:
        info.update(candidates=len(cand), nrep=sum(t[2] for t in out))
    return out


def triples_of(multiset):
    """sorted distinct (o, q, min(m, 2^32 - 1)) of a sorted multiset of pairs"""
    counts = {}
    for p in multiset:
        counts[p] = counts.get(p, 0) + 1
    return sorted((o, q, min(m, MAX_M)) for (o, q), m in counts.items())


# ---- the closed form: gf_geomjoin_plan.hpp, function for function ---------------------------------------------
EMPTY = (0, 0, -1, -1)


def empty(a):
    return a[0] > a[2] or a[1] > a[3]


def meet(a, b):
    return max(a[0], b[0]), max(a[1], b[1]), min(a[2], b[2]), min(a[3], b[3])


def grid_rect(n):
    return 0, 0, n - 1, n - 1


def leaves(a, n):
    return not empty(a) and (a[0] < 0 or a[1] < 0 or a[2] >= n or a[3] >= n)


def expand(rq, c, n, whole):
    if whole:
        return grid_rect(n)
    if c <= 0 or empty(rq):
        return EMPTY
    return meet((rq[0] - c, rq[1] - c, rq[2] + c, rq[3] + c), grid_rect(n))


def area(a):
    return 0 if empty(a) else (a[2] - a[0] + 1) * (a[3] - a[1] + 1)


def multiplicity(ro, eq, rq, out_members, n):
    m = area(meet(ro, eq))
    if out_members:
        both = meet(ro, rq)
        m += area(both) - area(meet(both, grid_rect(n)))
    return min(m, MAX_M)


def tile_shift(n, c, requested=0):
    want = requested
    if want <= 0:
        want = min(2 * c + 1 if c > 0 else 1, n)
    shift = 0
    while shift < 31 and (1 << shift) < want:
        shift += 1
    while shift < 31 and ((n - 1) >> shift) + 1 > MAX_TILE_SIDE:
        shift += 1
    return shift


def tiles_side(n, shift):
    return ((n - 1) >> shift) + 1


def tile_of(cx, cy, shift, nt):
    return (cy >> shift) * nt + (cx >> shift)


def tiles_covered(a, shift):
    return 0 if empty(a) else ((a[2] >> shift) - (a[0] >> shift) + 1) * ((a[3] >> shift) - (a[1] >> shift) + 1)


def tiles_of(a, shift, nt):
    return [ty * nt + tx for ty in range(a[1] >> shift, (a[3] >> shift) + 1) for tx in range(a[0] >> shift, (a[2] >> shift) + 1)]


def ref_tile(ro, eq, shift, nt):
    b = meet(ro, eq)
    return -1 if empty(b) else tile_of(b[0], b[1], shift, nt)


def class_query(rq, eq, out_members, n, shift, long_tiles, brute):
    outside = out_members and leaves(rq, n)
    if empty(eq) and not outside:
        return 0
    if brute or outside:
        return 2
    return 1 if tiles_covered(eq, shift) <= long_tiles else 2


def class_object(ro, n, shift, long_tiles, brute):
    if empty(ro):
        return 0
    if brute:
        return 2
    return 1 if tiles_covered(meet(ro, grid_rect(n)), shift) <= long_tiles else 2


class Sides:
    """the rectangles of one join: R_o of the valid objects, R_q and E_q of the valid queries, and the layer
    facts of r on qgrid (LayersError for a point query whose candidate layers are not positive)"""

    def __init__(self, ug, qg, okind, objs, qkind, queries, r):
        gl, cl = O.layers(qg, r)
        self.n, self.c = qg.n, cl
        self.whole = qkind == POINT and r == 0
        if qkind == POINT and not self.whole and cl <= 0:
            raise LayersError()
        self.out_members = qkind != POINT and cl > 0 and gl == 0
        self.ro = {o: GR.cell_rect(ug, GR.bbox(okind, obj)) for o, obj in enumerate(objs) if GR.valid(okind, obj)}
        self.rq = {}
        for qi, q in enumerate(queries):
            if qkind == POINT:
                cx, cy = O.assign_cells(qg, [q[0]], [q[1]])
                self.rq[qi] = (int(cx[0]), int(cy[0]), int(cx[0]), int(cy[0]))
            elif GR.valid(qkind, q):
                self.rq[qi] = GR.cell_rect(qg, GR.bbox(qkind, q))
        self.eq = {qi: expand(rq, self.c, self.n, self.whole) for qi, rq in self.rq.items()}

    def m(self, o, qi):
        return multiplicity(self.ro[o], self.eq[qi], self.rq[qi], self.out_members, self.n)


def candidates_closed_form(S):
    """sorted (o, q, m) of every pair with m > 0"""
    return sorted((o, qi, S.m(o, qi)) for o in S.ro for qi in S.rq if S.m(o, qi) > 0)


def candidates_by_tiles(S, tile_side=0, long_tiles=0, brute=False, info=None):
    """The library's candidate generation, as a list (NOT a set: a pair found twice appears twice): the CSR of
    the short queries by tile, one walk per short object over the tiles of R_o n grid taking a pair at its
    reference tile only, and the rectangle pass over (long object, any query) and (short object, long query)."""
    long_tiles = long_tiles or LONG_TILES
    shift = tile_shift(S.n, S.c, tile_side)
    nt = tiles_side(S.n, shift)
    ocls = {o: class_object(ro, S.n, shift, long_tiles, brute) for o, ro in S.ro.items()}
    qcls = {qi: class_query(S.rq[qi], S.eq[qi], S.out_members, S.n, shift, long_tiles, brute) for qi in S.rq}
    csr = {}
    for qi, cls in qcls.items():
        if cls == 1:
            for t in tiles_of(S.eq[qi], shift, nt):
                csr.setdefault(t, []).append(qi)
    out = []
    for o, cls in ocls.items():
        if cls == 1:
            rg = meet(S.ro[o], grid_rect(S.n))
            if not empty(rg):
                for t in tiles_of(rg, shift, nt):
                    for qi in csr.get(t, ()):
                        if ref_tile(S.ro[o], S.eq[qi], shift, nt) == t:
                            out.append((o, qi, S.m(o, qi)))
        for qi, qc in qcls.items():
            if (cls == 2 and qc != 0) or (cls == 1 and qc == 2):
                if S.m(o, qi) > 0:
                    out.append((o, qi, S.m(o, qi)))
    if info is not None:
        info.update(long_objects=sum(c == 2 for c in ocls.values()), long_queries=sum(c == 2 for c in qcls.values()),
                    shift=shift)
    return sorted(out)


def join_closed_form(ug, qg, okind, objs, qkind, queries, r, approximate=False, metric=0, first_is_ordinary=False, info=None):
    """sorted distinct (o, q, m): the candidates with d <= r; info receives candidates and nrep"""
    S = Sides(ug, qg, okind, objs, qkind, queries, r)
    cand = candidates_closed_form(S)
    out = [(o, qi, m) for o, qi, m in cand
           if pair_distance(okind, objs[o], qkind, queries[qi], metric, approximate, first_is_ordinary) <= r]
    if info is not None:
        info.update(candidates=len(cand), nrep=sum(t[2] for t in out))
    return out


def point_distances(okind, objs, points, metric=0, approximate=False):
    out = set()
    for obj in objs:
        if GR.valid(okind, obj):
            for p in points:
                d = GR.distance(okind, obj, p[0], p[1], metric, approximate)
                if 0 < d < 1e300:
                    out.add(d)
    return sorted(out)
