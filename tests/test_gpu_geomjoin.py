"""GPU: the six geometry-stream joins (gf_geom_join_run / gf_geom_join_run_points; the
{Polygon,LineString}{Point,Polygon,LineString}JoinQuery operators) against the restatement of
tests/geomjoin_ref.py, exactly: the sorted (ordinary idx, query idx, m) triples equal, the replication count
and the info counters consistent -- exact and approximate, both metrics, every wide_vertices threshold (every
candidate by waves, the middle, the default, lanes only) and every tuning (default, tile side 1 and 16,
long_tiles 1, brute), at the layer regimes, r = 0 and realized distances with their ulp neighbours.  Small
shapes only: the 10 x 10 unit grid."""
import ctypes as C
import functools
import math
import random

import numpy as np
import pytest

import spatialflink_amd as sf
from spatialflink_amd import _lib

import geomjoin_ref as J
import geompair_cases as PCS
import geompair_ref as PR
import geomwin_cases as GC
import geomwin_ref as GR

pytestmark = pytest.mark.gpu

POLYGON, LINESTRING, POINT = J.POLYGON, J.LINESTRING, J.POINT
DEFAULT = 0
THRESHOLDS = (1, 64, DEFAULT, GC.INT32_MAX)
TUNINGS = {"default": (0, 0, 0), "tile1": (1, 0, 0), "tile16": (16, 0, 0), "long1": (0, 1, 0), "brute": (0, 0, 1)}
MODES = ((False, 0), (False, 1), (True, 0), (True, 1))
REGIMES = (3.0, 1.6, 0.75)   # the unit grid: guaranteed layers 1, 0, -1


def _grid():
    return sf.UniformGrid(PCS.UNIT[0], *PCS.UNIT[1])


def _conf(approximate=False, metric=0):
    conf = sf.QueryConfiguration(sf.QueryType.WindowBased)
    conf.setApproximateQuery(approximate)
    conf.distanceMetric = metric
    return conf


def _window(kind, geoms, gpu):
    if kind == POINT:
        return sf.PointWindow.from_numpy(np.array([p[0] for p in geoms], np.float64), np.array([p[1] for p in geoms], np.float64),
                                         device=gpu.index)
    ro, vo, vx, vy = GC.csr(dict(kind=kind, objs=geoms))
    return sf.GeometryWindow.from_csr(kind, ro, vo, vx, vy, device=gpu.index)


def _op(name, approximate=False, metric=0, tuning="default"):
    op = getattr(sf, name)(_conf(approximate, metric), _grid(), _grid())
    op.tile_side, op.long_tiles, op.brute = TUNINGS[tuning]
    return op


def _triples(res):
    return [(int(p[0]), int(p[1]), int(m)) for p, m in zip(res.pairs, res.multiplicity)]


@functools.lru_cache(maxsize=None)
def _unit():
    return GR.grid_of(*PCS.UNIT)


@functools.lru_cache(maxsize=None)
def _objects(kind):
    big = [PCS.square(-0.5, -0.5, 11.0)] if kind == POLYGON else [(-0.5, -0.5), (10.5, 10.5)]   # covers every tile
    return PCS.pairs(kind)["objs"] + [big]


@functools.lru_cache(maxsize=None)
def _queries(qkind):
    if qkind == POINT:
        return [(float(x), float(y)) for qx, qy in GC.QUERIES_UNIT.values() for x, y in zip(qx, qy)]
    return [q for by_kind in PCS.QUERY_SETS.values() for q in by_kind[qkind]] + PCS.INVALID[qkind]


@functools.lru_cache(maxsize=None)
def _classes(okind, qkind, r, tuning):
    """(long objects, long queries) of the restatement's bin stage: they depend on the rectangles, r and the tuning only"""
    S = J.Sides(_unit(), _unit(), okind, _objects(okind), qkind, _queries(qkind), r)
    info = {}
    J.candidates_by_tiles(S, TUNINGS[tuning][0], TUNINGS[tuning][1], bool(TUNINGS[tuning][2]), info)
    return info["long_objects"], info["long_queries"]


def _radii(okind, objs, qkind, qs, metric, approximate, first):
    """the layer regimes, r = 0, and two realized distances with their ulp neighbours"""
    ds = sorted({d for o in objs if GR.valid(okind, o) for q in qs if J.query_valid(qkind, q)
                 for d in [J.pair_distance(okind, o, qkind, q, metric, approximate, first)] if 0 < d <= 3.0})
    near = []
    for d in ds[:: max(1, len(ds) // 2)][:2]:
        near += [float(np.nextafter(d, 0.0)), d, float(np.nextafter(d, np.inf))]
    return list(REGIMES) + [0.0], near


def _check(op, w, qw, ix, qix, okind, objs, qkind, qs, r, approximate, metric, first, expected, what):
    key = (r, approximate, metric)
    if key not in expected:
        info = {}
        expected[key] = (J.join_hashed(_unit(), _unit(), okind, objs, qkind, qs, r, approximate, metric, first, info), info)
    exp, info = expected[key]
    res = op.run(w, qw, r, index=ix, query_index=qix)
    assert _triples(res) == exp, what
    assert res.nrep == info["nrep"] == int(res.multiplicity.sum()) == len(res.replicated()), what
    gi = op.info()
    assert gi["candidates"] == info["candidates"], (what, gi)
    if approximate:
        assert gi["box_dropped"] == gi["tested"] == gi["wave_path"] == 0, (what, gi)
    else:   # every candidate is dropped by the box test or has its distance evaluated; a hit was evaluated
        assert gi["box_dropped"] + gi["tested"] == gi["candidates"] and len(exp) <= gi["tested"], (what, gi)
        assert 0 <= gi["wave_path"] <= gi["tested"], (what, gi)
    return res, gi


@pytest.mark.parametrize("approximate,metric", MODES)
@pytest.mark.parametrize("name", list(J.OPERATORS))
def test_the_join_equals_the_restatement_for_every_threshold_and_tuning(name, approximate, metric, gpu, oracle_mod):
    """hand-built pairs, objects and query rectangles leaving the grid (the keys outside it at guaranteed layers
    0), an object covering every tile, invalid geometries on both sides, a background object per cell (pairs
    with m > 1)"""
    okind, qkind, first = J.OPERATORS[name]
    objs, qs = _objects(okind), _queries(qkind)
    w, qw = _window(okind, objs, gpu), _window(qkind, qs, gpu)
    ix = sf.GeometryIndex(w, _grid())
    qix = sf.GeometryIndex(qw, _grid()) if qkind != POINT else None
    regimes, near = _radii(okind, objs, qkind, qs, metric, approximate, first)
    expected, seen = {}, dict(pairs=0, repeated=0, waved=0, long_o=0, long_q=0)
    for thr in THRESHOLDS:
        ix.set_thresholds(thr)
        if qix is not None:
            qix.set_thresholds(thr)
        for tuning in TUNINGS:
            op = _op(name, approximate, metric, tuning)
            reduced = (thr, tuning) in ((DEFAULT, "default"), (1, "brute"), (GC.INT32_MAX, "tile1"))
            for r in regimes + (near if reduced else []):
                res, gi = _check(op, w, qw, ix, qix, okind, objs, qkind, qs, r, approximate, metric, first, expected,
                                 (name, thr, tuning, r))
                if not approximate:
                    assert thr != 1 or gi["wave_path"] == gi["tested"]
                    assert thr != GC.INT32_MAX or gi["wave_path"] == 0
                if r in regimes:   # the classes of the run are the restatement's
                    assert (gi["long_objects"], gi["long_queries"]) == _classes(okind, qkind, r, tuning), (tuning, r, gi)
                seen["pairs"] += len(res.pairs)
                seen["repeated"] += int((res.multiplicity > 1).sum())
                seen["waved"] += gi["wave_path"]
                seen["long_o"] += gi["long_objects"]
                seen["long_q"] += gi["long_queries"]
            op.close()
    assert seen["pairs"] > 0 and seen["repeated"] > 0 and seen["long_o"] > 0 and seen["long_q"] > 0, seen
    assert approximate or seen["waved"] > 0
    if qkind == POINT:   # r == 0: every valid cell is a key
        assert expected[(0.0, approximate, metric)][1]["candidates"] > 100 * len(qs)
    else:
        assert expected[(0.0, approximate, metric)] == ([], dict(candidates=0, nrep=0))
    ix.close()
    if qix is not None:
        qix.close()


@pytest.mark.parametrize("name", ["PolygonLineStringJoinQuery", "LineStringPolygonJoinQuery", "PolygonPolygonJoinQuery",
                                  "LineStringLineStringJoinQuery"])
def test_degenerate_edges_and_boxes(name, gpu, oracle_mod):
    """zero-length edges, rings collapsed to a segment or a point, zero-width and zero-height boxes: the bbox-bbox
    function's argument order is the operator's own"""
    okind, qkind, first = J.OPERATORS[name]
    case = PCS.degenerate(okind)
    objs = case["objs"]
    qs = [q for by_kind in case["queries"].values() for q in by_kind[qkind]]
    w, qw = _window(okind, objs, gpu), _window(qkind, qs, gpu)
    ix, qix = sf.GeometryIndex(w, _grid()), sf.GeometryIndex(qw, _grid())
    swapped = 0
    for approximate, metric in MODES:
        regimes, near = _radii(okind, objs, qkind, qs, metric, approximate, first)
        expected = {}
        for tuning in ("default", "brute"):
            op = _op(name, approximate, metric, tuning)
            for r in regimes + near:
                _check(op, w, qw, ix, qix, okind, objs, qkind, qs, r, approximate, metric, first, expected, (name, tuning, r))
                if approximate:
                    other = J.join_hashed(_unit(), _unit(), okind, objs, qkind, qs, r, True, metric, not first)
                    swapped += other != expected[(r, approximate, metric)][0]
            op.close()
    assert name != "PolygonLineStringJoinQuery" or swapped > 0
    ix.close()
    qix.close()


@pytest.mark.parametrize("name", ["PolygonPolygonJoinQuery", "PolygonLineStringJoinQuery", "LineStringPolygonJoinQuery",
                                  "LineStringPointJoinQuery", "PolygonPointJoinQuery"])
def test_long_geometries_on_either_side(name, gpu, oracle_mod):
    """a 1,000-vertex object among 257 small ones against a 2,000-segment query and small ones: the wave path at
    the default threshold, by the second geometry of the operator's order"""
    okind, qkind, first = J.OPERATORS[name]
    objs = PCS.with_long_object(okind, nv=1000)["objs"]
    if qkind == POINT:
        qs = [(5.1, 5.2), (4.6, 5.3), (0.2, 9.7), (11.0, 5.0)]
    else:
        qs = PCS.long_queries(2000)[qkind] + PCS.QUERY_SETS["overlapping"][qkind]
    w, qw = _window(okind, objs, gpu), _window(qkind, qs, gpu)
    ix = sf.GeometryIndex(w, _grid())
    qix = sf.GeometryIndex(qw, _grid()) if qkind != POINT else None
    expected, waved = {}, {}
    for thr in (DEFAULT, 1, GC.INT32_MAX):
        ix.set_thresholds(thr)
        if qix is not None:
            qix.set_thresholds(thr)
        for tuning in ("default", "long1"):
            op = _op(name, False, 0, tuning)
            for r in (0.75, 3.0):
                _, gi = _check(op, w, qw, ix, qix, okind, objs, qkind, qs, r, False, 0, first, expected, (name, thr, tuning, r))
                waved[thr] = waved.get(thr, 0) + gi["wave_path"]
            op.close()
    # default threshold 384: only the long second geometry goes to waves -- the 1,000-vertex object, or, when the
    # ordinary polygon is first, the 2,000-segment query linestring against every object it is tested with
    assert 0 < waved[DEFAULT] < waved[1] and waved[GC.INT32_MAX] == 0, waved
    ix.close()
    if qix is not None:
        qix.close()


def _scatter_points(n, seed=5):
    rnd = random.Random(seed)
    return [(rnd.uniform(-0.5, 10.5), rnd.uniform(-0.5, 10.5)) for _ in range(n)]


@pytest.mark.parametrize("name", ["PolygonPointJoinQuery", "LineStringPointJoinQuery", "PolygonPolygonJoinQuery",
                                  "LineStringLineStringJoinQuery"])
def test_window_sizes_on_both_sides_with_one_joiner(name, gpu, oracle_mod):
    """ordinary windows of 0, 1, 63, 64, 65 and 3,001 objects against query sides of 0, 1, 65 and 257, every run
    through ONE joiner (a larger window, then smaller ones, then larger again: the scratch only grows); the
    3,001 x 257 geometry join is approximate (its exact reference would take minutes in Python)"""
    okind, qkind, first = J.OPERATORS[name]
    op = _op(name)
    aop = _op(name, approximate=True)
    sizes = [(3001, 257), (0, 65), (65, 0), (1, 1), (63, 65), (64, 257), (65, 65), (3001, 1), (64, 65), (3001, 257)]
    total = 0
    for no, nq in sizes:
        objs = GC.sized(okind, no)["objs"]
        qs = _scatter_points(nq) if qkind == POINT else GC.sized(qkind, nq, seed=9)["objs"]
        w, qw = _window(okind, objs, gpu), _window(qkind, qs, gpu)
        run = aop if (qkind != POINT and no * nq > 100000) else op
        for r in ((0.75,) if no * nq > 100000 else (0.75, 1.6)):
            info = {}
            exp = J.join_hashed(_unit(), _unit(), okind, objs, qkind, qs, r, run is aop, 0, first, info)
            for tuning in ("default", "tile1", "brute"):
                run.tile_side, run.long_tiles, run.brute = TUNINGS[tuning]
                res = run.run(w, qw, r)
                assert _triples(res) == exp and res.nrep == info["nrep"], (name, no, nq, tuning, r)
                assert run.info()["candidates"] == info["candidates"]
                total += len(exp)
    assert total > 1000
    op.close()
    aop.close()


def test_capacity_layers_refusals_and_a_shared_index(gpu, oracle_mod):
    L = _lib.lib()
    objs, pts = _objects(POLYGON), _queries(POINT)
    lines = _queries(LINESTRING)
    w, pw, lw = _window(POLYGON, objs, gpu), _window(POINT, pts, gpu), _window(LINESTRING, lines, gpu)
    g = _grid()
    ix, lix = sf.GeometryIndex(w, g), sf.GeometryIndex(lw, g)
    ctx = ix.ctx
    j = C.c_void_p()
    assert L.gf_geom_join_create(ctx.handle, C.byref(j)) == 0
    exp = J.join_hashed(_unit(), _unit(), POLYGON, objs, POINT, pts, 1.6)
    n, m = C.c_int64(), C.c_int64()
    ps = pw.c_struct()

    def run_points(r, pairs, cap):
        return L.gf_geom_join_run_points(j, ix.handle, C.byref(g.c_grid), C.byref(ps), r, 0, 0, pairs, cap, C.byref(n), C.byref(m))

    import torch
    # cap = 0 counts only (no pairs at all: GF_OK only when there is nothing to write)
    assert run_points(1.6, None, 0) == _lib.GF_ERR_CAPACITY and n.value == len(exp) and m.value == sum(t[2] for t in exp)
    assert len(exp) > 1
    buf = torch.full((3 * len(exp) + 3,), -1, dtype=torch.int32, device=gpu)
    assert run_points(1.6, buf.data_ptr(), len(exp) - 1) == _lib.GF_ERR_CAPACITY and n.value == len(exp)
    assert int(buf[3 * (len(exp) - 1)]) == -1        # nothing written beyond cap
    assert run_points(1.6, buf.data_ptr(), len(exp)) == 0 and n.value == len(exp)
    got = buf[: 3 * len(exp)].cpu().numpy().view(np.uint32).astype(np.int64).reshape(-1, 3)
    assert sorted(map(tuple, got.tolist())) == exp and int(buf[3 * len(exp)]) == -1
    # the layers: a point query refuses a negative and a NaN radius, a geometry query selects nothing
    for r in (-0.5, math.nan):
        assert run_points(r, None, 0) == _lib.GF_ERR_LAYERS
        assert L.gf_geom_join_run(j, ix.handle, lix.handle, r, 0, 0, 1, None, 0, C.byref(n), C.byref(m)) == 0 and n.value == 0
    with pytest.raises(_lib.CandidateLayersError):
        _op("PolygonPointJoinQuery").run(w, pw, -1.0, index=ix)
    # refusals
    E = _lib.GF_ERR_ARG
    assert run_points(1.6, None, -1) == E and run_points(1.6, None, 5) == E              # negative cap; null pairs with cap > 0
    assert L.gf_geom_join_run_points(j, ix.handle, C.byref(g.c_grid), C.byref(ps), 1.6, 0, 2, None, 0, C.byref(n), C.byref(m)) == E
    assert L.gf_geom_join_run_points(j, ix.handle, None, C.byref(ps), 1.6, 0, 0, None, 0, C.byref(n), C.byref(m)) == E
    assert L.gf_geom_join_run_points(j, ix.handle, C.byref(g.c_grid), C.byref(ps), 1.6, 0, 0, None, 0, None, C.byref(m)) == E
    assert L.gf_geom_join_run(j, ix.handle, None, 1.6, 0, 0, 0, None, 0, C.byref(n), C.byref(m)) == E
    assert L.gf_geom_join_run(j, ix.handle, lix.handle, 1.6, 0, 7, 0, None, 0, C.byref(n), C.byref(m)) == E
    assert L.gf_geom_join_run(j, lix.handle, ix.handle, 1.6, 0, 0, 1, None, 0, C.byref(n), C.byref(m)) == E   # first_is_ordinary:
    assert L.gf_geom_join_run(j, ix.handle, ix.handle, 1.6, 0, 0, 1, None, 0, C.byref(n), C.byref(m)) == E    # polygon x linestring only
    assert L.gf_geom_join_set_tuning(j, -1, 0, 0) == E and L.gf_geom_join_set_tuning(j, 0, -1, 0) == E
    assert L.gf_geom_join_set_tuning(j, 0, 0, 2) == E
    other = _lib.Context(gpu.index)
    j2 = C.c_void_p()
    assert L.gf_geom_join_create(other.handle, C.byref(j2)) == 0
    assert L.gf_geom_join_run(j2, ix.handle, lix.handle, 1.6, 0, 0, 0, None, 0, C.byref(n), C.byref(m)) == E   # another context
    assert L.gf_geom_join_run_points(j2, ix.handle, C.byref(g.c_grid), C.byref(ps), 1.6, 0, 0, None, 0, C.byref(n), C.byref(m)) == E
    L.gf_geom_join_destroy(j2)
    # one index shared by a join, a range query and the join again
    jop = _op("PolygonLineStringJoinQuery")
    want = J.join_hashed(_unit(), _unit(), POLYGON, objs, LINESTRING, lines, 1.6, False, 0, True)
    first = jop.run(w, lw, 1.6, index=ix, query_index=lix)
    rop = sf.PolygonLineStringRangeQuery(_conf(), g)
    q = PCS.QUERY_SETS["small"][LINESTRING]
    ref = PR.range_literal(_unit(), POLYGON, objs, LINESTRING, q, 1.6)
    assert np.array_equal(rop.run(w, [sf.LineString(q[0])], 1.6, index=ix).indices().astype(np.int64), ref)
    again = jop.run(w, lw, 1.6, index=ix, query_index=lix)
    assert _triples(first) == _triples(again) == want and len(want) > 0
    jop.close()
    L.gf_geom_join_destroy(j)
    ix.close()
    lix.close()
