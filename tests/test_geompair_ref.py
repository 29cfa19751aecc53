"""CPU: the restatement of the geometry-pair operators (tests/geompair_ref.py) holds the rules of
include/geoflink_hip.h, "geometry windows against polygon and linestring queries": the literal
segmentToSegment on hand-built segment pairs, DistanceOp on hand-built geometry pairs, the query-side cell
sets, the bbox-bbox function in its nine positions, the literal operators against their closed form in any
cell order -- and the pure host part of the query (the rectangle-marked tables) under the host sanitizers.
The new C ABI is present and refuses bad arguments before any device call.  No GPU."""
import ctypes as C
import math
import os
import random
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import geompair_cases as PCS
import geompair_ref as R
import geomwin_ref as GR

POLYGON, LINESTRING = R.POLYGON, R.LINESTRING


@pytest.fixture(scope="module")
def grid(oracle_mod):
    return GR.grid_of(*PCS.UNIT)


# ---- segment pairs ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", PCS.SEGMENT_PAIRS, ids=[p[0] for p in PCS.SEGMENT_PAIRS])
def test_segment_to_segment_on_hand_built_pairs(pair, oracle_mod):
    name, a, b, c, d, want = pair
    for metric in (0, 1):
        got = R.segment_to_segment(a, b, c, d, metric)
        if want is not None:
            assert got == want, (name, metric, got)
        # swapping the two segments negates denom and exchanges r and s, and takes the same four point-segment
        # distances: the same bits (reversing a segment's direction is NOT bit-symmetric, so the order of the
        # vertices as stored is part of the rule)
        assert got == R.segment_to_segment(c, d, a, b, metric), name
        m = R._pair_matrix([a, b], [c, d], metric, math.inf)
        assert m.shape == (1, 1) and float(m[0, 0]) == got, (name, metric)


def test_segment_to_segment_named_values(oracle_mod):
    p = {n: (a, b, c, d) for n, a, b, c, d, _ in PCS.SEGMENT_PAIRS}
    assert R.segment_to_segment(*p["collinear_diagonal"]) == math.sqrt(8.0)
    assert R.segment_to_segment(*p["parallel_offset"]) == math.sqrt(2.0)
    assert R.segment_to_segment(*p["envelope_disjoint"]) == R.point_to_segment((2.0, 0.0), (0.0, 0.0), (1.0, 1.0))
    assert not R.envelopes_intersect(*p["envelope_disjoint"]) and R.envelopes_intersect(*p["envelopes_meet_no_crossing"])
    assert R.segment_to_segment(*p["envelopes_meet_no_crossing"]) > 0.0
    a, b, c, d = p["near_parallel_tiny_denom"]
    denom = (b[0] - a[0]) * (d[1] - c[1]) - (b[1] - a[1]) * (d[0] - c[0])
    assert denom != 0.0 and abs(denom) < 1e-14   # parallel to rounding: r and s are huge, no intersection
    got = R.segment_to_segment(a, b, c, d)
    assert 0.0 < got and abs(got - 1e-9 / math.sqrt(2.0)) < 1e-15
    a, b, c, d = p["near_parallel_crossing"]
    assert 0.0 < abs((b[0] - a[0]) * (d[1] - c[1]) - (b[1] - a[1]) * (d[0] - c[0])) < 1e-14


def test_scalar_and_numpy_forms_agree_on_random_lattice_pairs(oracle_mod):
    pairs = PCS.random_segment_pairs()
    kinds = dict(zero=0, degenerate=0, positive=0)
    for a, b, c, d in pairs:
        for metric in (0, 1):
            got = R.segment_to_segment(a, b, c, d, metric)
            m = R._pair_matrix([a, b], [c, d], metric, math.inf)
            assert float(m[0, 0]) == got, (a, b, c, d, metric)
        kinds["zero"] += got == 0.0
        kinds["degenerate"] += a == b or c == d
        kinds["positive"] += got > 0.0
    assert min(kinds.values()) > 10, kinds


# ---- geometry pairs ---------------------------------------------------------------------------------------
def _shape(name, kind):
    return PCS.as_kind(kind, dict(PCS.SHAPES)[name])


def test_polygon_query_against_the_hand_built_shapes(oracle_mod):
    q = PCS.Q_HOLED
    d = lambda name, kind: R.distance(POLYGON, q, kind, _shape(name, kind))  # noqa: E731
    for kind in (POLYGON, LINESTRING):
        assert d("inside_no_contact", kind) == 0.0           # the first-vertex rule, no boundary contact
        assert R.facet_distance(POLYGON, q, kind, _shape("inside_no_contact", kind)) == 0.5
        assert d("inside_hole", kind) == 0.5                 # inside the hole: exterior; the hole ring is 0.5 away
        assert d("first_vertex_on_edge", kind) == 0.0
        assert d("first_vertex_on_vertex", kind) == 0.0
        assert d("first_outside_crossing", kind) == 0.0      # by intersection
        assert not R.holds(R.first_coordinate(kind, _shape("first_outside_crossing", kind)), q)
        assert d("apart_right", kind) == 0.5
        # corner (8, 8) to vertex (8.3, 8.4): the differences as the doubles give them
        assert d("apart_diagonal", kind) == math.sqrt((8.3 - 8.0) * (8.3 - 8.0) + (8.4 - 8.0) * (8.4 - 8.0))
        assert d("touching_edge", kind) == 0.0
        assert d("collinear_apart", kind) == 0.5
        assert d("straddles_hole_edge", kind) == 0.0
        assert d("on_hole_edge", kind) == 0.0
        assert d("far", kind) > 1.5
    # the query wholly inside a window polygon: 0 by the query's first vertex; inside a closed chain: 1.0
    assert d("contains_query", POLYGON) == 0.0 and d("contains_query", LINESTRING) == 1.0
    # the query inside the object's hole: the hole ring is 0.5 from the query's shell
    assert d("query_in_its_hole", POLYGON) == 0.5 and d("query_in_its_hole", LINESTRING) == 1.5


def test_a_closed_linestring_contains_nothing(oracle_mod):
    q = PCS.Q_RING_CHAIN
    for kind in (POLYGON, LINESTRING):
        assert R.distance(LINESTRING, q, kind, _shape("inside_no_contact", kind)) == 0.5
        assert R.distance(LINESTRING, q, kind, _shape("inside_hole", kind)) == 2.5
        assert R.distance(LINESTRING, q, kind, _shape("first_vertex_on_edge", kind)) == 0.0
    # ... but a window polygon contains the chain's first vertex
    assert R.distance(LINESTRING, q, POLYGON, _shape("contains_query", POLYGON)) == 0.0
    assert R.distance(LINESTRING, q, LINESTRING, _shape("contains_query", LINESTRING)) == 1.0


def test_numpy_facets_equal_the_scalar_loop(oracle_mod):
    case = PCS.pairs(POLYGON)
    for qkind in (POLYGON, LINESTRING):
        for q in PCS.QUERY_SETS["holed"][qkind] + PCS.QUERY_SETS["overlapping"][qkind]:
            for okind in (POLYGON, LINESTRING):
                for name, s in PCS.SHAPES:
                    o = PCS.as_kind(okind, s)
                    for metric in (0, 1):
                        assert R.facet_distance_np(qkind, q, okind, o, metric) == R.facet_distance(qkind, q, okind, o, metric), \
                            (qkind, okind, name, metric)
    assert len(case["objs"]) > 100


# ---- the bbox-bbox function -------------------------------------------------------------------------------
def test_bbox_bbox_in_nine_positions_and_on_equal_edges(oracle_mod):
    q = (4.0, 4.0, 6.0, 7.0)
    box = lambda x, y: (x, y, x + 1.0, y + 1.0)  # noqa: E731
    h = math.hypot
    want = {
        (1.0, 1.0): h(2.0, 2.0), (4.5, 1.0): 2.0, (8.0, 1.0): h(2.0, 2.0),
        (1.0, 5.0): 2.0, (4.5, 5.0): 0.0, (8.0, 5.0): 2.0,
        (1.0, 9.0): h(2.0, 2.0), (4.5, 9.0): 2.0, (8.0, 9.0): h(2.0, 2.0),
    }
    for (x, y), d in want.items():
        assert R.bbox_bbox_distance(q, box(x, y)) == d, (x, y)
    # equal edges: p2 == x1 takes the first branch (a border distance of 0, not the overlap's 0.0 -- the same value)
    assert R.bbox_bbox_distance(q, (3.0, 5.0, 4.0, 6.0)) == 0.0
    assert R.bbox_bbox_distance(q, (3.0, 3.0, 4.0, 4.0)) == 0.0          # corner to corner
    assert R.bbox_bbox_distance(q, (6.0, 7.0, 7.0, 8.0)) == 0.0
    assert R.bbox_bbox_distance(q, (3.0, 2.0, 4.0, 3.0)) == 1.0          # p2 == x1 and below: a1 - b3 = (0, 1)
    # overlapping in x by a sliver, touching in y: the third branch's border distance
    assert R.bbox_bbox_distance(q, (3.0, 3.0, 4.5, 4.0)) == 0.0
    assert R.bbox_bbox_distance(q, (3.0, 2.0, 4.5, 3.5)) == 0.5
    # a zero-width query box (a vertical line): the third branch's border test takes x1 == x2 first and
    # measures x, not y -- the reference's own behaviour, restated
    assert R.bbox_bbox_distance((5.0, 4.0, 5.0, 6.0), (4.0, 1.0, 5.5, 2.0)) == 1.0
    assert R.bbox_bbox_distance((4.0, 4.0, 6.0, 6.0), (4.5, 1.0, 5.5, 2.0)) == 2.0
    # not symmetric in its arguments on degenerate boxes, so the order (query first) matters
    assert R.bbox_bbox_distance((4.0, 1.0, 5.5, 2.0), (5.0, 4.0, 5.0, 6.0)) == 2.0


# ---- the query side ---------------------------------------------------------------------------------------
def test_query_sets_at_every_layer_regime(grid, oracle_mod):
    q = PCS.QUERY_SETS["small"][POLYGON]          # R_q = the cell (5, 5)
    N, G = R.query_sets(grid, POLYGON, q, 3.0)    # g = 1, c = 3
    assert G == {(i, j) for i in (4, 5, 6) for j in (4, 5, 6)} and N == {(i, j) for i in range(2, 9) for j in range(2, 9)}
    N, G = R.query_sets(grid, POLYGON, q, 1.6)    # g = 0, c = 2
    assert G == {(5, 5)} and N == {(i, j) for i in range(3, 8) for j in range(3, 8)}
    N, G = R.query_sets(grid, POLYGON, q, 0.75)   # g = -1, c = 1
    assert G == set() and N == {(i, j) for i in (4, 5, 6) for j in (4, 5, 6)}
    for r in (0.0, -1.0):                         # r == 0: c = 0, g = -1 -> nothing, NOT the whole grid
        assert R.query_sets(grid, POLYGON, q, r) == (set(), set())
    big = PCS.QUERY_SETS["holed"][POLYGON]        # R_q = [2..8] x [2..8]
    N, G = R.query_sets(grid, POLYGON, big, 1.6)
    assert G == {(i, j) for i in range(2, 9) for j in range(2, 9)} and N == {(i, j) for i in range(10) for j in range(10)}


def test_a_query_rectangle_leaving_the_grid_at_layers_0(grid, oracle_mod):
    for qkind in (POLYGON, LINESTRING):
        q = PCS.QUERY_SETS["leaving"][qkind]
        assert GR.cell_rect(grid, GR.bbox(qkind, q[0])) == (-1, 4, 0, 5)
        N, G = R.query_sets(grid, qkind, q, 1.6)
        assert G == {(-1, 4), (-1, 5), (0, 4), (0, 5)}          # no validKey at layers 0
        assert {c for c in N if c[0] < 0} == {(-1, 4), (-1, 5)}  # N's only members outside the grid
        N3, G3 = R.query_sets(grid, qkind, q, 3.0)              # layers 1: validKey drops them
        assert all(0 <= c[0] < 10 and 0 <= c[1] < 10 for c in N3 | G3)
        assert not R.refused(grid, qkind, q, 1.6)
        assert R.refused(grid, qkind, PCS.REFUSED_SETS["leaving_set"][qkind], 1.6)
        assert not R.refused(grid, qkind, PCS.REFUSED_SETS["leaving_set"][qkind], 3.0)
    for okind in (POLYGON, LINESTRING):
        case = PCS.pairs(okind)
        names = [n for n, _ in PCS.SHAPES + PCS.CORNER_SHAPES]
        for qkind in (POLYGON, LINESTRING):
            info = {}
            got = R.range_literal(grid, okind, case["objs"], qkind, PCS.QUERY_SETS["leaving"][qkind], 1.6, info=info)
            hit = {names[i] for i in got if i < len(names)}
            # an object cell outside the grid matches G: emitted with no distance test
            assert {"out_cell_in_rq", "partly_out_in_rq"} <= hit and info["all_guaranteed"] >= 2
            # one cell further out: within r, but no cell in N
            o = case["objs"][names.index("out_cell_beyond_rq")]
            assert R.distance(qkind, PCS.QUERY_SETS["leaving"][qkind][0], okind, o) <= 1.6 and "out_cell_beyond_rq" not in hit
            assert "out_and_wider_than_rq" in hit    # not all-G (wider than R_q), but at distance 0
            # the reference's answer for the refused set is still stated
            ref = R.range_literal(grid, okind, case["objs"], qkind, PCS.REFUSED_SETS["leaving_set"][qkind], 1.6)
            assert set(got.tolist()) < set(ref.tolist())


def test_r_zero_and_negative_select_nothing(grid, oracle_mod):
    for okind, qkind in PCS.PAIRS:
        case = PCS.pairs(okind)
        for name, sets in PCS.QUERY_SETS.items():
            for r in (0.0, -0.5):
                assert len(R.range_literal(grid, okind, case["objs"], qkind, sets[qkind], r)) == 0
            assert len(R.knn_literal(grid, okind, case["objs"], case["keys"], qkind, sets[qkind][0], 0.0, 5)[0]) == 0


@pytest.mark.parametrize("okind,qkind", PCS.PAIRS)
def test_the_literal_operators_equal_the_closed_form_in_any_cell_order(okind, qkind, grid, oracle_mod):
    case = PCS.pairs(okind)
    rnd = random.Random(5)
    orders = (None, lambda c: c.reverse(), lambda c: rnd.shuffle(c))
    seen = dict(allg=0, tested=0, emitted=0)
    sets = dict(PCS.QUERY_SETS, **PCS.REFUSED_SETS)
    for name, by_kind in sets.items():
        queries = by_kind[qkind]
        for approximate, metric in ((False, 0), (False, 1), (True, 0)):
            for r in R.case_radii(case, qkind, queries, metric, approximate):
                want = R.range_closed_form(grid, okind, case["objs"], qkind, queries, r, approximate, metric)
                for order in orders:
                    info = {}
                    got = R.range_literal(grid, okind, case["objs"], qkind, queries, r, approximate, metric, order, info)
                    assert np.array_equal(got, want), (name, approximate, metric, r)
                    assert len(set(got.tolist())) == len(got)   # emitted once
                seen["allg"] += info["all_guaranteed"]
                seen["tested"] += info["tested"]
                seen["emitted"] += len(want)
    assert min(seen.values()) > 0, seen


@pytest.mark.parametrize("okind,qkind", PCS.PAIRS)
def test_degenerate_edges_and_boxes_in_the_restatement(okind, qkind, grid, oracle_mod):
    """zero-length edges inside rings and chains: the scalar loop, the numpy form and the closed form agree;
    the zero-width and zero-height boxes realize the argument order of the bbox-bbox function"""
    case = PCS.degenerate(okind)
    swapped = 0
    for qname, by_kind in case["queries"].items():
        q = by_kind[qkind][0]
        for o in case["objs"]:
            for metric in (0, 1):
                assert R.facet_distance(qkind, q, okind, o, metric) == R.facet_distance_np(qkind, q, okind, o, metric)
            qb, ob = GR.bbox(qkind, q), GR.bbox(okind, o)
            swapped += R.bbox_bbox_distance(qb, ob) != R.bbox_bbox_distance(ob, qb)
        for approximate, metric in ((False, 0), (False, 1), (True, 0)):
            for r in R.case_radii(case, qkind, by_kind[qkind], metric, approximate, limit=6):
                assert np.array_equal(R.range_literal(grid, okind, case["objs"], qkind, by_kind[qkind], r, approximate, metric),
                                      R.range_closed_form(grid, okind, case["objs"], qkind, by_kind[qkind], r, approximate, metric))
    assert swapped > 0


def test_the_segment_window_holds_every_pair(grid, oracle_mod):
    case, queries = PCS.segment_window()
    assert len(case["objs"]) == len(queries) == len(PCS.SEGMENT_PAIRS) + 400
    assert all(GR.valid(LINESTRING, o) and len(o) == 2 for o in case["objs"])
    for i, (name, a, b, c, d, want) in enumerate(PCS.SEGMENT_PAIRS):
        got = R.distance(LINESTRING, queries[i], LINESTRING, case["objs"][i])
        assert got == R.segment_to_segment(a, b, c, d) and (want is None or got == want), name


def test_knn_literal_is_the_sorted_deduplicated_candidates(grid, oracle_mod):
    for okind, qkind in PCS.PAIRS:
        case = PCS.pairs(okind)
        q = PCS.QUERY_SETS["holed"][qkind][0]
        for k in (1, 7, 50, 600):
            o, d, i = R.knn_literal(grid, okind, case["objs"], case["keys"], qkind, q, 3.0, k)
            assert len(o) <= k and len(set(o.tolist())) == len(o)
            rows = list(zip(d.tolist(), o.tolist(), i.tolist()))
            assert rows == sorted(rows) and all(v <= 3.0 for v in d)
        assert (d == 0.0).sum() > 1    # ties at d = 0, ordered by key then idx
        assert len(o) < 600            # a short record


# ---- the pure host part under the sanitizers ------------------------------------------------------------------
def test_rectangle_marked_tables_under_the_host_sanitizers(tmp_path):
    exe = str(tmp_path / "geompair_plan_main")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-I/opt/rocm/include",
                    "-D__HIP_PLATFORM_AMD__", os.path.join(ROOT, "tests", "native", "geompair_plan_main.cpp"), "-o", exe],
                   check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1")
    run = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert run.returncode == 0, run.stderr[-2000:]
    assert run.stdout.startswith("ok ") and int(run.stdout.split()[1]) > 100000


# ---- the C ABI and the mirror, without a device ---------------------------------------------------------------
NEW_SYMBOLS = ("gf_geom_query_create_polygons", "gf_geom_query_create_linestrings", "gf_geom_query_set_chain_mode")
NEW_CLASSES = ("PolygonPolygonRangeQuery", "PolygonLineStringRangeQuery", "LineStringPolygonRangeQuery",
               "LineStringLineStringRangeQuery", "PolygonPolygonKNNQuery", "PolygonLineStringKNNQuery",
               "LineStringPolygonKNNQuery", "LineStringLineStringKNNQuery")


def test_the_new_symbols_are_declared_exported_and_bound():
    from spatialflink_amd import _lib

    header = open(os.path.join(ROOT, "include", "geoflink_hip.h")).read()
    L = _lib.lib()
    for s in NEW_SYMBOLS:
        assert s + "(" in header and s in _lib.EXPORTS and hasattr(L, s), s
    assert L.gf_abi_version() == 2


def test_the_constructors_refuse_before_any_device_call():
    import spatialflink_amd as sf
    from spatialflink_amd import _lib

    L = _lib.lib()
    E = _lib.GF_ERR_ARG
    g = sf.UniformGrid(*[PCS.UNIT[0], *PCS.UNIT[1]])
    h = C.c_void_p()
    ps = sf.PolygonSet([sf.Polygon([PCS.square(5.2, 5.2, 0.5)])]).c_struct()
    ls = sf.LineStringSet([sf.LineString([(5.2, 5.2), (5.7, 5.6)])]).c_struct()
    # a null context, output, grid or set
    assert L.gf_geom_query_create_polygons(None, C.byref(g.c_grid), C.byref(ps), 1.0, 0, 0, C.byref(h)) == E
    assert L.gf_geom_query_create_linestrings(None, C.byref(g.c_grid), C.byref(ls), 1.0, 0, 0, C.byref(h)) == E
    assert L.gf_geom_query_create_polygons(None, C.byref(g.c_grid), None, 1.0, 0, 0, C.byref(h)) == E
    assert L.gf_geom_query_create_linestrings(None, None, C.byref(ls), 1.0, 0, 0, C.byref(h)) == E
    assert L.gf_geom_query_create_polygons(None, C.byref(g.c_grid), C.byref(ps), 1.0, 0, 0, None) == E
    assert L.gf_geom_query_create_polygons(None, C.byref(g.c_grid), C.byref(ps), 1.0, 0, 2, C.byref(h)) == E  # bad metric
    assert L.gf_geom_query_set_chain_mode(None, 0) == E
    assert not h.value


def test_the_mirror_classes_follow_their_siblings():
    import spatialflink_amd as sf

    grid = sf.UniformGrid(PCS.UNIT[0], *PCS.UNIT[1])
    for name in NEW_CLASSES:
        cls = getattr(sf, name)
        assert issubclass(cls, sf.spatialOperators._GeomWindowQuery) and name in sf.__all__
        op = cls(sf.QueryConfiguration(sf.QueryType.RealTime), grid)
        with pytest.raises(ValueError, match="Not yet support"):
            op.query(0, [sf.Polygon([PCS.square(5.2, 5.2, 0.5)])], 1.0)
        window_kind = sf._lib.GEOM_POLYGON if name.startswith("Polygon") else sf._lib.GEOM_LINESTRING
        query_polygon = name[len("Polygon" if name.startswith("Polygon") else "LineString"):].startswith("Polygon")
        assert cls._kind == window_kind
        assert cls._query_kind == (sf._lib.GEOM_POLYGON if query_polygon else sf._lib.GEOM_LINESTRING)
