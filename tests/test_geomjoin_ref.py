"""CPU: the restatement of the geometry-stream joins (tests/geomjoin_ref.py) holds the rules of
include/geoflink_hip.h, "geometry-stream joins": the literal hash join on cell keys equals the closed form (E_q,
the multiplicity m) for the six operators, on one grid and on two different ones, at every layer regime, at
r = 0, negative and NaN; the tile rule yields every candidate exactly once for any tile side and long_tiles;
the PolygonLineString argument order is observable; and the header's cell arithmetic, built as a stand-alone
program under the host sanitizers, agrees with the restatement up to the saturated indices.  The new C ABI is
present and refuses null handles before any device call.  No GPU."""
import ctypes as C
import math
import os
import random
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import geomjoin_ref as J
import geompair_cases as PCS
import geomwin_cases as GC
import geomwin_ref as GR

POLYGON, LINESTRING, POINT = J.POLYGON, J.LINESTRING, J.POINT
SEVEN = (7, (0.0, 10.0, 0.0, 10.0))      # cell length 10 / 7 over the same box
GRIDS = {"unit": (PCS.UNIT, PCS.UNIT), "seven": (SEVEN, SEVEN), "two_grids": (PCS.UNIT, SEVEN)}
MODES = ((False, 0), (False, 1), (True, 0))
REGIMES = (3.0, 1.6, 0.75)               # x the query grid's cell length: guaranteed layers 1, 0, -1


def objects(kind):
    """hand-built shapes, objects leaving the grid on the left, invalid objects, one small object per cell"""
    return PCS.pairs(kind)["objs"]


def queries(qkind):
    if qkind == POINT:
        pts = []
        for qx, qy in GC.QUERIES_UNIT.values():       # "outside": a query point outside the grid
            pts += [(float(x), float(y)) for x, y in zip(qx, qy)]
        return pts
    out = [q for by_kind in PCS.QUERY_SETS.values() for q in by_kind[qkind]]   # "leaving", "outside": rectangles off the grid
    return out + PCS.INVALID[qkind]


def _cl(grid):
    return (grid[1][1] - grid[1][0]) / grid[0]


@pytest.fixture(scope="module")
def grids(oracle_mod):
    return {k: (GR.grid_of(*u), GR.grid_of(*q), _cl(q)) for k, (u, q) in GRIDS.items()}


@pytest.mark.parametrize("gname", list(GRIDS))
@pytest.mark.parametrize("op", list(J.OPERATORS))
def test_the_literal_join_equals_the_closed_form(op, gname, grids):
    okind, qkind, first = J.OPERATORS[op]
    ug, qg, cl = grids[gname]
    objs, qs = objects(okind), queries(qkind)
    seen = dict(pairs=0, repeated=0, outside=0, invalid_o=0, invalid_q=0)
    seen["invalid_o"] = sum(not GR.valid(okind, o) for o in objs)
    seen["invalid_q"] = 1 if qkind == POINT else sum(not GR.valid(qkind, q) for q in qs)
    for k in REGIMES:
        r = k * cl
        gl, c = J.O.layers(qg, r)
        assert gl == {3.0: 1, 1.6: 0, 0.75: -1}[k] and c > gl
        for approximate, metric in MODES:
            lit = J.join_literal(ug, qg, okind, objs, qkind, qs, r, approximate, metric, first)
            info = {}
            got = J.join_closed_form(ug, qg, okind, objs, qkind, qs, r, approximate, metric, first, info)
            assert J.triples_of(lit) == got, (op, gname, k, approximate, metric)
            assert info["nrep"] == len(lit) and info["candidates"] >= len(got)
            seen["pairs"] += len(got)
            seen["repeated"] += sum(m > 1 for _, _, m in got)
            if qkind != POINT and gl == 0:   # a key outside the grid: only R_q's own cells at guaranteed layers 0
                S = J.Sides(ug, qg, okind, objs, qkind, qs, r)
                seen["outside"] += sum(J.area(J.meet(S.ro[o], S.rq[q])) > J.area(J.meet(J.meet(S.ro[o], S.rq[q]), J.grid_rect(S.n)))
                                       for o, q, _ in got)
    assert seen["pairs"] > 0 and seen["repeated"] > 0 and seen["invalid_o"] > 0 and seen["invalid_q"] > 0, seen
    # (on two grids the objects' out-of-grid cells are ugrid's and share no key with R_q's, taken on qgrid)
    assert qkind == POINT or gname == "two_grids" or seen["outside"] > 0, seen


@pytest.mark.parametrize("op", list(J.OPERATORS))
def test_r_zero_negative_and_nan(op, grids):
    okind, qkind, first = J.OPERATORS[op]
    ug, qg, _ = grids["unit"]
    objs, qs = objects(okind), queries(qkind)
    if qkind == POINT:
        # r == 0: every valid cell is a key, so every in-grid cell of R_o matches; d <= 0 keeps the touching pairs
        lit = J.join_literal(ug, qg, okind, objs, qkind, qs, 0.0, False, 0, first)
        got = J.join_closed_form(ug, qg, okind, objs, qkind, qs, 0.0, False, 0, first)
        assert J.triples_of(lit) == got
        S = J.Sides(ug, qg, okind, objs, qkind, qs, 0.0)
        assert S.whole and all(eq == (0, 0, 9, 9) for eq in S.eq.values())
        assert len(J.candidates_closed_form(S)) > len(S.rq) * 100   # the whole grid: (nearly) every object
        if okind == POLYGON:
            assert len(got) > 0                                      # a query point inside a polygon: d = 0
        for r in (-0.5, math.nan):
            with pytest.raises(J.LayersError):
                J.join_literal(ug, qg, okind, objs, qkind, qs, r, False, 0, first)
            with pytest.raises(J.LayersError):
                J.join_closed_form(ug, qg, okind, objs, qkind, qs, r, False, 0, first)
    else:
        for r in (0.0, -0.5, math.nan):                              # K = {}: no pairs, no error
            assert J.join_literal(ug, qg, okind, objs, qkind, qs, r, False, 0, first) == []
            info = {}
            assert J.join_closed_form(ug, qg, okind, objs, qkind, qs, r, False, 0, first, info) == []
            assert info["candidates"] == 0


@pytest.mark.parametrize("gname", list(GRIDS))
@pytest.mark.parametrize("op", ["PolygonPointJoinQuery", "LineStringPolygonJoinQuery", "PolygonLineStringJoinQuery"])
def test_the_tile_rule_yields_every_candidate_exactly_once(op, gname, grids):
    okind, qkind, _ = J.OPERATORS[op]
    ug, qg, cl = grids[gname]
    big = [PCS.square(-0.5, -0.5, 11.0)] if okind == POLYGON else [(-0.5, -0.5), (10.5, 10.5)]   # covers every tile
    objs, qs = objects(okind) + [big], queries(qkind)
    classes = set()
    for r in [k * cl for k in REGIMES] + ([0.0] if qkind == POINT else []):
        S = J.Sides(ug, qg, okind, objs, qkind, qs, r)
        want = J.candidates_closed_form(S)
        assert len(want) > 0 and len(set((o, q) for o, q, _ in want)) == len(want)
        for tile_side in (0, 1, 2, 4, 16):
            for long_tiles in (1, 0, 10 ** 9):
                info = {}
                got = J.candidates_by_tiles(S, tile_side, long_tiles, False, info)
                assert got == want, (op, gname, r, tile_side, long_tiles)
                classes.add((info["long_objects"] > 0, info["long_queries"] > 0))
        assert J.candidates_by_tiles(S, 0, 0, True) == want
    assert (False, False) in classes or (False, True) in classes   # a run with no long object ...
    assert (True, True) in classes                                   # ... and one with both kinds of long side


def test_the_default_tile_side_and_its_cap():
    assert J.tile_shift(500, 1) == 2 and J.tile_shift(500, 2) == 3 and J.tile_shift(500, 0) == 0   # 2c + 1 = 3 -> 4; 5 -> 8
    assert J.tile_shift(10, 7) == 4 and J.tile_shift(10, 2 ** 31 - 1) == 4                          # min(2c + 1, n) = 10 -> 16
    assert J.tile_shift(10, 3, 3) == 2 and J.tile_shift(10, 3, 16) == 4                            # a requested side, rounded up
    assert J.tile_shift(46340, 0) == 6 and J.tiles_side(46340, 6) == 725                           # at most 1024 tiles a side
    assert J.tile_shift(2 ** 31 - 1, 0, 1) == 21 and J.tiles_side(2 ** 31 - 1, 21) == 1024


def test_the_polygon_linestring_argument_order_is_observable(grids):
    """getDistance(poly, q): on the zero-width and zero-height boxes the bbox-bbox function is not symmetric, so
    the approximate join with the arguments swapped gives another result"""
    ug, qg, _ = grids["unit"]
    case = PCS.degenerate(POLYGON)
    qs = [q for by_kind in case["queries"].values() for q in by_kind[LINESTRING]]
    radii = set()
    for o in case["objs"]:
        for q in qs:
            radii.add(J.pair_distance(POLYGON, o, LINESTRING, q, 0, True, True))
            radii.add(J.pair_distance(POLYGON, o, LINESTRING, q, 0, True, False))
    differ = 0
    for r in sorted(d for d in radii if 0 < d <= 3.0):
        own = J.join_closed_form(ug, qg, POLYGON, case["objs"], LINESTRING, qs, r, True, 0, True)
        swapped = J.join_closed_form(ug, qg, POLYGON, case["objs"], LINESTRING, qs, r, True, 0, False)
        assert J.triples_of(J.join_literal(ug, qg, POLYGON, case["objs"], LINESTRING, qs, r, True, 0, True)) == own
        differ += own != swapped
    assert differ > 0
    assert J.OPERATORS["PolygonLineStringJoinQuery"][2] and sum(v[2] for v in J.OPERATORS.values()) == 1


# ---- the header's arithmetic under the host sanitizers --------------------------------------------------------
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1


def _plan_checks():
    rnd = random.Random(3)
    sat = [(I32_MIN, I32_MIN, I32_MAX, I32_MAX), (I32_MIN, 0, I32_MAX, 0), (I32_MAX - 1, 3, I32_MAX, 5), (I32_MIN, -4, I32_MIN + 2, 9),
           (I32_MIN, I32_MIN, 5, I32_MAX), (-3, -3, 12, 12), (0, 0, 0, 0), (5, 5, 4, 4)]
    rects = list(sat)
    for _ in range(40):
        x, y = rnd.randint(-4, 12), rnd.randint(-4, 12)
        rects.append((x, y, x + rnd.randint(0, 6), y + rnd.randint(0, 6)))
    lines = []
    for n in (1, 7, 10, 500, 46340, I32_MAX):
        for c in (-1, 0, 1, 3, I32_MAX):
            for req in (0, 1, 2, 3, 16, 4096):
                s = J.tile_shift(n, c, req)
                lines.append(f"T {n} {c} {req} {s} {J.tiles_side(n, s)}")
            for ro in rects:
                for rq in rnd.sample(rects, 6) + sat[:2]:
                    for whole, out in ((0, 0), (0, 1), (1, 0)):
                        eq = J.expand(rq, c, n, bool(whole))
                        m = J.multiplicity(ro, eq, rq, bool(out), n)
                        lines.append("M %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d" % (*ro, *rq, c, n, whole, out, *eq, m))
                        shift = J.tile_shift(n, c, rnd.choice((0, 1, 4)))
                        nt = J.tiles_side(n, shift)
                        lines.append("R %d %d %d %d %d %d %d %d %d %d %d %d" % (*ro, *eq, shift, nt, J.ref_tile(ro, eq, shift, nt),
                                                                                 J.tiles_covered(eq, shift)))
                        lt, brute = rnd.choice((1, 16, 10 ** 9)), rnd.choice((0, 0, 1))
                        lines.append("C %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d" % (
                            *ro, *rq, c, n, whole, out, shift, lt, brute, J.class_object(ro, n, shift, lt, bool(brute)),
                            J.class_query(rq, eq, bool(out), n, shift, lt, bool(brute))))
    return lines


def test_the_cell_arithmetic_under_the_host_sanitizers(tmp_path):
    # the saturated rectangles realize what must not overflow: an area of 2^64 and a multiplicity above 2^32 - 1
    full = (I32_MIN, I32_MIN, I32_MAX, I32_MAX)
    assert J.area(full) == 2 ** 64
    assert J.multiplicity(full, J.expand(full, 1, 10, False), full, True, 10) == J.MAX_M
    assert J.multiplicity(full, J.expand((2, 2, 3, 3), 1, 10, False), (2, 2, 3, 3), True, 10) == 16
    exe = str(tmp_path / "geomjoin_plan_main")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-I/opt/rocm/include",
                    "-D__HIP_PLATFORM_AMD__", os.path.join(ROOT, "tests", "native", "geomjoin_plan_main.cpp"), "-o", exe],
                   check=True)
    lines = _plan_checks()
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1")
    run = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, env=env)
    assert run.returncode == 0, run.stderr[-2000:]
    assert run.stdout.split() == ["ok", str(len(lines))] and len(lines) > 20000


# ---- the C ABI and the mirror, without a device -----------------------------------------------------------------
NEW_SYMBOLS = ("gf_geom_join_create", "gf_geom_join_destroy", "gf_geom_join_run", "gf_geom_join_run_points",
               "gf_geom_join_info", "gf_geom_join_set_tuning")


def test_the_new_symbols_are_declared_exported_and_bound():
    from spatialflink_amd import _lib

    header = open(os.path.join(ROOT, "include", "geoflink_hip.h")).read()
    L = _lib.lib()
    for s in NEW_SYMBOLS:
        assert s + "(" in header and s in _lib.EXPORTS and hasattr(L, s), s
        assert getattr(L, s).argtypes is not None
    assert L.gf_abi_version() == 2 and "#define GF_K_COUNT       20" in header


def test_null_handles_are_refused_before_any_device_call():
    """(the refusals that need a joiner -- contexts, metric, cap, first_is_ordinary, the layers -- are held on
    the device in tests/test_gpu_geomjoin.py: a joiner needs a context)"""
    import spatialflink_amd as sf
    from spatialflink_amd import _lib

    L = _lib.lib()
    E = _lib.GF_ERR_ARG
    g = sf.UniformGrid(PCS.UNIT[0], *PCS.UNIT[1])
    h, n, m = C.c_void_p(), C.c_int64(), C.c_int64()
    pts = _lib.GfPoints()
    assert L.gf_geom_join_create(None, C.byref(h)) == E and not h.value
    assert L.gf_geom_join_run(None, None, None, 1.0, 0, 0, 0, None, 0, C.byref(n), C.byref(m)) == E
    assert L.gf_geom_join_run_points(None, None, C.byref(g.c_grid), C.byref(pts), 1.0, 0, 0, None, 0, C.byref(n), C.byref(m)) == E
    assert L.gf_geom_join_info(None, None, None, None, None, None, None) == E
    assert L.gf_geom_join_set_tuning(None, 0, 0, 0) == E
    L.gf_geom_join_destroy(None)


def test_the_mirror_classes():
    import spatialflink_amd as sf

    u, q = sf.UniformGrid(PCS.UNIT[0], *PCS.UNIT[1]), sf.UniformGrid(SEVEN[0], *SEVEN[1])
    for name, (okind, qkind, first) in J.OPERATORS.items():
        cls = getattr(sf, name)
        assert name in sf.__all__ and issubclass(cls, sf.spatialOperators.SpatialOperator)
        assert (cls._kind, cls._query_kind, bool(cls._first_is_ordinary)) == (okind, qkind, first)
        op = cls(sf.QueryConfiguration(sf.QueryType.WindowBased), u, q)
        assert op.getSpatialIndex() is u and op.index2 is q and cls(op.conf, u).index2 is u
        for qt in (sf.QueryType.CountBased, sf.QueryType.RealTimeNaive, None):
            with pytest.raises(ValueError, match="Not yet support"):
                cls(sf.QueryConfiguration(qt), u, q).run(None, None, 1.0)
        for qt in (sf.QueryType.RealTime, sf.QueryType.WindowBased):   # both run the window evaluation: the windows are checked next
            with pytest.raises(ValueError, match="window"):
                cls(sf.QueryConfiguration(qt), u, q).run(None, None, 1.0)
    res = sf.GeomJoinResult(np.array([[0, 1], [2, 3]]), np.array([2, 1]), 3)
    assert "GeomJoinResult" in sf.__all__ and res.replicated().tolist() == [[0, 1], [0, 1], [2, 3]]
