"""GPU: polygon and linestring windows against polygon and linestring queries (gf_geom_query_create_polygons /
_linestrings through gf_geom_range_run and gf_geom_knn_enqueue; the eight
{Polygon,LineString}{Polygon,LineString}{Range,KNN}Query operators) against the restatement of
tests/geompair_ref.py, exactly: bitmaps equal, kNN objIDs, indices and distance bits equal -- for the four
pairs, exact and approximate, both metrics, every wide_vertices threshold (every object by waves, the middle,
the default, lanes only), at the layer regimes, r = 0 and realized distances with their ulp neighbours.
Small shapes only: the 10 x 10 unit grid."""
import ctypes as C

import numpy as np
import pytest

import spatialflink_amd as sf
from spatialflink_amd import _lib

import geomwin_cases as GC
import geompair_cases as PCS
import geompair_ref as R
import geomwin_ref as GR

pytestmark = pytest.mark.gpu

POLYGON, LINESTRING = R.POLYGON, R.LINESTRING
DEFAULT = 0  # gf_geom_index_set_thresholds: the library's default wide_vertices
THRESHOLDS = (1, 64, DEFAULT, GC.INT32_MAX)
RANGE_OPS = {(POLYGON, POLYGON): sf.PolygonPolygonRangeQuery, (POLYGON, LINESTRING): sf.PolygonLineStringRangeQuery,
             (LINESTRING, POLYGON): sf.LineStringPolygonRangeQuery, (LINESTRING, LINESTRING): sf.LineStringLineStringRangeQuery}
KNN_OPS = {(POLYGON, POLYGON): sf.PolygonPolygonKNNQuery, (POLYGON, LINESTRING): sf.PolygonLineStringKNNQuery,
           (LINESTRING, POLYGON): sf.LineStringPolygonKNNQuery, (LINESTRING, LINESTRING): sf.LineStringLineStringKNNQuery}
MODES = ((False, 0), (False, 1), (True, 0), (True, 1))


def _grid():
    return sf.UniformGrid(PCS.UNIT[0], *PCS.UNIT[1])


def _window(case, gpu):
    ro, vo, vx, vy = GC.csr(case)
    return sf.GeometryWindow.from_csr(case["kind"], ro, vo, vx, vy, case["keys"], device=gpu.index)


def _conf(approximate=False, metric=0):
    conf = sf.QueryConfiguration(sf.QueryType.WindowBased)
    conf.setApproximateQuery(approximate)
    conf.distanceMetric = metric
    return conf


def _ops(okind, qkind, approximate=False, metric=0, chain_mode=0):
    rop, kop = RANGE_OPS[(okind, qkind)](_conf(approximate, metric), _grid()), KNN_OPS[(okind, qkind)](_conf(approximate, metric), _grid())
    rop.chain_mode = kop.chain_mode = chain_mode
    return rop, kop


def _qobjs(qkind, geoms):
    return [sf.Polygon(q) if qkind == POLYGON else sf.LineString(q) for q in geoms]


def _bits(a):
    return np.asarray(a, np.float64).view(np.int64)


def _same_record(got, ref):
    o, d, i = ref
    return np.array_equal(got.objID, o) and np.array_equal(got.idx, i) and np.array_equal(_bits(got.dist), _bits(d))


@pytest.mark.parametrize("approximate", [False, True])
@pytest.mark.parametrize("okind,qkind", PCS.PAIRS)
def test_range_equals_the_restatement_at_every_threshold(okind, qkind, approximate, gpu, oracle_mod):
    """the hand-built geometry pairs, the query sets (g = -1, 0, > 0, r = 0, overlapping rectangles) and the
    out-of-grid corner of G, with the invalid objects and a background object per cell"""
    case = PCS.pairs(okind)
    w = _window(case, gpu)
    g = GR.grid_of(*case["grid"])
    ix = sf.GeometryIndex(w, _grid())
    expected = {}
    for metric in (0, 1):
        for qname, by_kind in case["queries"].items():
            for r in R.case_radii(case, qkind, by_kind[qkind], metric, approximate):
                info = {}
                exp = R.range_literal(g, okind, case["objs"], qkind, by_kind[qkind], r, approximate, metric, info=info)
                expected[(metric, qname, r)] = (exp, info)
    waved = emitted = 0
    for thr in THRESHOLDS:
        ix.set_thresholds(thr)
        for metric in (0, 1):
            op, _ = _ops(okind, qkind, approximate, metric)
            for qname, by_kind in case["queries"].items():
                qs = _qobjs(qkind, by_kind[qkind])
                for r in R.case_radii(case, qkind, by_kind[qkind], metric, approximate):
                    exp, info = expected[(metric, qname, r)]
                    res = op.run(w, qs, r, index=ix)
                    got = res.indices().astype(np.int64)
                    assert np.array_equal(got, exp), (thr, metric, qname, r)
                    assert res.count() == len(exp) and res.multiset_size() == info["all_guaranteed"]
                    gi = op.info()
                    assert {k: gi[k] for k in info} == info, (thr, metric, qname, r, gi)
                    assert thr != 1 or approximate or gi["wave_path"] == gi["tested"]
                    assert thr != GC.INT32_MAX or gi["wave_path"] == 0
                    waved += gi["wave_path"]
                    emitted += len(exp)
    assert emitted > 0 and (approximate or waved > 0)
    ix.close()


@pytest.mark.parametrize("okind,qkind", PCS.PAIRS)
def test_knn_on_the_hand_built_pairs(okind, qkind, gpu, oracle_mod):
    """duplicate keys, ties at d = 0 (several objects inside or crossing the query), short records, k on both
    sides of the one-block select's 512"""
    case = PCS.pairs(okind)
    w = _window(case, gpu)
    g = GR.grid_of(*case["grid"])
    ix = sf.GeometryIndex(w, _grid())
    ties = short = 0
    for thr in THRESHOLDS:
        ix.set_thresholds(thr)
        for approximate, metric in MODES:
            _, kop = _ops(okind, qkind, approximate, metric)
            for qname, by_kind in case["queries"].items():
                for q in by_kind[qkind]:  # every geometry of every query set, one at a time
                    for k, r in ((1, 3.0), (7, 3.0), (50, 3.0), (50, 0.75), (600, 1.6), (600, 3.0), (5, 0.0)):
                        ref = R.knn_literal(g, okind, case["objs"], case["keys"], qkind, q, r, k, approximate, metric)
                        got = kop.run(w, _qobjs(qkind, [q])[0], r, k, index=ix)
                        assert _same_record(got, ref), (thr, approximate, metric, qname, k, r)
                        ties += int((ref[1] == 0.0).sum() > 1)
                        short += int(0 < len(ref[0]) < k)
    assert ties > 0 and short > 0
    ix.close()


@pytest.mark.parametrize("metric", [0, 1])
def test_every_segment_pair_on_the_device(metric, gpu, oracle_mod):
    """segment_to_segment itself: every hand-built pair (crossing, touching at r or s = 0 or 1, collinear,
    parallel, A == B, C == D, both, envelope-disjoint, near-parallel) and the lattice pairs as 2-vertex
    linestring objects against 2-vertex linestring queries; the recorded d of EVERY object against the query is
    R.segment_to_segment's bit for bit, by lanes and by waves, and the bitmaps at r = d and one ulp below agree"""
    case, queries = PCS.segment_window()
    w = _window(case, gpu)
    g = GR.grid_of(*case["grid"])
    ix = sf.GeometryIndex(w, _grid())
    nhand = len(PCS.SEGMENT_PAIRS)
    n = len(case["objs"])
    rop, kop = _ops(LINESTRING, LINESTRING, False, metric)
    R_ALL = 9.0  # nine candidate layers: every cell of the grid, every distance of the window
    zero = degenerate = 0
    for thr in (1, GC.INT32_MAX):
        ix.set_thresholds(thr)
        for qi in list(range(nhand)) + list(range(nhand, nhand + 60)):
            a, b = queries[qi]
            ref = R.knn_literal(g, LINESTRING, case["objs"], case["keys"], LINESTRING, queries[qi], R_ALL, 512, False, metric)
            assert len(ref[0]) == n   # every object is a candidate, so every pair's d is in the record
            got = kop.run(w, sf.LineString(queries[qi]), R_ALL, 512, index=ix)
            assert _same_record(got, ref), (thr, qi)
            own = R.segment_to_segment(a, b, case["objs"][qi][0], case["objs"][qi][1], metric)
            assert _bits(got.dist[got.idx == qi])[0] == _bits([own])[0], (thr, qi)
            zero += own == 0.0
            degenerate += a == b or case["objs"][qi][0] == case["objs"][qi][1]
            if qi < nhand and own > 0.0:
                for r in (own, float(np.nextafter(own, 0.0))):
                    exp = R.range_literal(g, LINESTRING, case["objs"], LINESTRING, [queries[qi]], r, False, metric)
                    res = rop.run(w, [sf.LineString(queries[qi])], r, index=ix)
                    assert np.array_equal(res.indices().astype(np.int64), exp), (thr, qi, r)
    assert zero > 10 and degenerate > 6
    ix.close()


@pytest.mark.parametrize("okind,qkind", PCS.PAIRS)
def test_degenerate_edges_and_boxes(okind, qkind, gpu, oracle_mod):
    """zero-length edges inside rings and chains on both sides (the A == B and C == D branches among ordinary
    edges), and boxes of zero width or height, where getBBoxBBoxMinEuclideanDistance depends on which box comes
    first: the query's"""
    case = PCS.degenerate(okind)
    w = _window(case, gpu)
    g = GR.grid_of(*case["grid"])
    ix = sf.GeometryIndex(w, _grid())
    swapped = 0
    for qname, by_kind in case["queries"].items():
        q = by_kind[qkind][0]
        for o in case["objs"]:
            if GR.valid(okind, o):
                qb, ob = GR.bbox(qkind, q), GR.bbox(okind, o)
                swapped += R.bbox_bbox_distance(qb, ob) != R.bbox_bbox_distance(ob, qb)
    assert swapped > 0   # a swapped call on the device would show below
    for thr in THRESHOLDS:
        ix.set_thresholds(thr)
        for approximate, metric in MODES:
            rop, kop = _ops(okind, qkind, approximate, metric)
            for qname, by_kind in case["queries"].items():
                qs = _qobjs(qkind, by_kind[qkind])
                for r in R.case_radii(case, qkind, by_kind[qkind], metric, approximate, limit=6):
                    exp = R.range_literal(g, okind, case["objs"], qkind, by_kind[qkind], r, approximate, metric)
                    res = rop.run(w, qs, r, index=ix)
                    assert np.array_equal(res.indices().astype(np.int64), exp), (thr, approximate, metric, qname, r)
                ref = R.knn_literal(g, okind, case["objs"], case["keys"], qkind, by_kind[qkind][0], 9.0, 50, approximate, metric)
                assert len(ref[0]) == sum(GR.valid(okind, o) for o in case["objs"])
                assert _same_record(kop.run(w, qs[0], 9.0, 50, index=ix), ref), (thr, approximate, metric, qname)
    ix.close()


@pytest.mark.parametrize("n", (0, 1, 63, 64, 65, 3001))
@pytest.mark.parametrize("okind,qkind", PCS.PAIRS)
def test_window_sizes(okind, qkind, n, gpu, oracle_mod):
    case = PCS.sized(okind, n)
    w = _window(case, gpu)
    g = GR.grid_of(*case["grid"])
    rop, kop = _ops(okind, qkind)
    ix = sf.GeometryIndex(w, _grid())
    for thr in (1, DEFAULT):
        ix.set_thresholds(thr)
        for qname, r in (("overlapping", GC.R_G0), ("holed", GC.R_GM1), ("leaving", GC.R_G0)):
            queries = case["queries"][qname][qkind]
            exp = R.range_literal(g, okind, case["objs"], qkind, queries, r)
            res = rop.run(w, _qobjs(qkind, queries), r, index=ix)
            assert np.array_equal(res.indices().astype(np.int64), exp), (n, thr, qname)
            assert res.count() == len(exp)
        q = case["queries"]["small"][qkind][0]
        ref = R.knn_literal(g, okind, case["objs"], case["keys"], qkind, q, GC.R_G1, 7)
        assert _same_record(kop.run(w, _qobjs(qkind, [q])[0], GC.R_G1, 7, index=ix), ref), (n, thr)
    ix.close()


@pytest.mark.parametrize("okind,qkind", PCS.PAIRS)
def test_knn_depths_ties_and_duplicates(okind, qkind, gpu, oracle_mod):
    case = PCS.sized(okind, 3001)
    w = _window(case, gpu)
    g = GR.grid_of(*case["grid"])
    ix = sf.GeometryIndex(w, _grid())
    q = case["queries"]["holed"][qkind][0]
    for approximate, metric in MODES:
        _, kop = _ops(okind, qkind, approximate, metric)
        for thr in (1, DEFAULT):
            ix.set_thresholds(thr)
            for k, r in ((1, GC.R_G1), (7, GC.R_G1), (50, GC.R_G1), (600, GC.R_G1), (600, GC.R_GM1), (513, 0.0)):
                ref = R.knn_literal(g, okind, case["objs"], case["keys"], qkind, q, r, k, approximate, metric)
                got = kop.run(w, _qobjs(qkind, [q])[0], r, k, index=ix)
                assert _same_record(got, ref), (approximate, metric, thr, k, r)
                if (k, r) == (600, GC.R_G1):
                    assert len(ref[0]) == 600  # the sorted path filled the record
    ix.close()


@pytest.mark.parametrize("okind,qkind", PCS.PAIRS)
def test_a_long_query_pruned_against_plain(okind, qkind, gpu, oracle_mod):
    """a query of about 2,000 segments: the run envelopes prune, chain mode 1 consults none, the restatement
    (its numpy form) walks every pair -- all three agree, range and kNN, lanes and waves"""
    case = PCS.sized(okind, 257)
    w = _window(case, gpu)
    g = GR.grid_of(*case["grid"])
    ix = sf.GeometryIndex(w, _grid())
    q = PCS.long_queries()[qkind]
    assert sum(len(l) - 1 for l in R.lines_of(qkind, q[0])) >= 2000
    qs = _qobjs(qkind, q)
    for r in (GC.R_GM1, 0.3):
        exp = R.range_literal(g, okind, case["objs"], qkind, q, r)
        ref = R.knn_literal(g, okind, case["objs"], case["keys"], qkind, q[0], r, 50)
        assert 0 < len(exp) < 257
        for thr in (1, GC.INT32_MAX):
            ix.set_thresholds(thr)
            for mode in (0, 1):
                rop, kop = _ops(okind, qkind, chain_mode=mode)
                res = rop.run(w, qs, r, index=ix)
                assert np.array_equal(res.indices().astype(np.int64), exp), (r, thr, mode)
                assert _same_record(kop.run(w, qs[0], r, 50, index=ix), ref), (r, thr, mode)
    ix.close()


@pytest.mark.parametrize("okind,qkind", PCS.PAIRS)
def test_a_long_object_is_taken_by_a_wave(okind, qkind, gpu, oracle_mod):
    case = PCS.with_long_object(okind)
    big = len(case["objs"]) - 1
    w = _window(case, gpu)
    g = GR.grid_of(*case["grid"])
    ix = sf.GeometryIndex(w, _grid())
    assert ix.info()["wide"] == 1
    rop, kop = _ops(okind, qkind)
    waved = 0
    for qname in ("small", "overlapping", "holed"):
        queries = case["queries"][qname][qkind]
        for r in (GC.R_GM1, 0.2):
            exp = R.range_literal(g, okind, case["objs"], qkind, queries, r)
            alone = {}  # the long object by itself: is its distance evaluated (filtered and not all-G)?
            R.range_literal(g, okind, [case["objs"][big]], qkind, queries, r, info=alone)
            ix.set_thresholds(DEFAULT)
            res = rop.run(w, _qobjs(qkind, queries), r, index=ix)
            assert np.array_equal(res.indices().astype(np.int64), exp), (qname, r)
            assert rop.info()["wave_path"] == alone["tested"], (qname, r)
            waved += alone["tested"]
            ix.set_thresholds(GC.INT32_MAX)
            res = rop.run(w, _qobjs(qkind, queries), r, index=ix)
            assert np.array_equal(res.indices().astype(np.int64), exp) and rop.info()["wave_path"] == 0
    assert waved > 0
    q = case["queries"]["small"][qkind][0]
    d_big = R.distance(qkind, q, okind, case["objs"][big])
    ref = R.knn_literal(g, okind, case["objs"], case["keys"], qkind, q, GC.R_G1, 600)
    assert big in ref[2].tolist() or d_big > GC.R_G1 or int(case["keys"][big]) in ref[0].tolist()
    for thr in (DEFAULT, GC.INT32_MAX):
        ix.set_thresholds(thr)
        assert _same_record(kop.run(w, _qobjs(qkind, [q])[0], GC.R_G1, 600, index=ix), ref), thr
    ix.close()


def test_a_record_merges_with_a_point_window_record(gpu, oracle_mod):
    import torch

    case = PCS.sized(POLYGON, 257)
    w = _window(case, gpu)
    grid = _grid()
    k, r = 7, GC.R_G1
    _, kop = _ops(POLYGON, POLYGON)
    ix = sf.GeometryIndex(w, grid)
    q = case["queries"]["small"][POLYGON][0]
    nb = sf.spatialOperators.knn_record_bytes(k)
    recs = torch.zeros(2 * nb, dtype=torch.uint8, device=gpu)
    ctx = kop.enqueue(w, sf.Polygon(q), r, k, recs[:nb], ix)
    rnd = np.random.default_rng(3)
    px, py = rnd.uniform(3.0, 8.0, 500), rnd.uniform(3.0, 8.0, 500)
    pobj = np.arange(500, dtype=np.int64) % 300 + 100   # some keys shared with the geometry window
    pw = sf.PointWindow.from_numpy(px, py, pobj, device=gpu.index)
    sf.PointPointKNNQuery(_conf(), grid).enqueue(pw, sf.Point("q", 5.5, 5.5, 0, grid), r, k, recs[nb:])
    out = torch.zeros(nb, dtype=torch.uint8, device=gpu)
    _lib.check(_lib.lib().gf_knn_merge_dev(ctx.handle, k, C.c_void_p(recs.data_ptr()), 2, C.c_void_p(out.data_ptr())),
               ctx.handle, "gf_knn_merge_dev")
    parts = [sf.spatialOperators.decode_knn_record(recs[j * nb:(j + 1) * nb].cpu().numpy().tobytes(), k) for j in (0, 1)]
    assert parts[0][0] == 0 and parts[1][0] == 0
    rows = sorted((float(d), int(o), int(i)) for _, oo, dd, ii in parts for o, d, i in zip(oo, dd, ii))
    seen, exp = set(), []
    for d, o, i in rows:
        if o not in seen:
            seen.add(o)
            exp.append((d, o, i))
    exp = exp[:k]
    st, o, d, i = sf.spatialOperators.decode_knn_record(out.cpu().numpy().tobytes(), k)
    assert st == 0 and [(float(a), int(b), int(c)) for a, b, c in zip(d, o, i)] == exp
    eo, ed, ei = R.knn_literal(GR.grid_of(*case["grid"]), POLYGON, case["objs"], case["keys"], POLYGON, q, r, k)
    assert np.array_equal(parts[0][1], eo) and np.array_equal(_bits(parts[0][2]), _bits(ed)) and np.array_equal(parts[0][3], ei)
    ix.close()


@pytest.mark.parametrize("okind", [POLYGON, LINESTRING])
def test_one_index_under_a_point_query_and_a_geometry_query_in_turn(okind, gpu, oracle_mod):
    case = PCS.sized(okind, 3001)
    w = _window(case, gpu)
    g = GR.grid_of(*case["grid"])
    ix = sf.GeometryIndex(w, _grid())
    pop = (sf.PolygonPointRangeQuery if okind == POLYGON else sf.LineStringPointRangeQuery)(_conf(), _grid())
    qx, qy = GC.QUERIES_UNIT["five"]
    pexp = GR.range_literal(g, okind, case["objs"], qx, qy, GC.R_G0)
    points = [sf.Point("q", float(a), float(b)) for a, b in zip(qx, qy)]
    for _ in range(2):
        for qkind in (POLYGON, LINESTRING):
            rop, kop = _ops(okind, qkind)
            queries = case["queries"]["overlapping"][qkind]
            exp = R.range_literal(g, okind, case["objs"], qkind, queries, GC.R_G0)
            res_p = pop.run(w, points, GC.R_G0, index=ix)
            res_g = rop.run(w, _qobjs(qkind, queries), GC.R_G0, index=ix)
            res_p2 = pop.run(w, points, GC.R_G0, index=ix)
            assert np.array_equal(res_p.indices().astype(np.int64), pexp) and np.array_equal(res_p2.indices().astype(np.int64), pexp)
            assert np.array_equal(res_g.indices().astype(np.int64), exp)
    ix.close()


def test_refusals(gpu, oracle_mod):
    import torch

    L = _lib.lib()
    E = _lib.GF_ERR_ARG
    case = PCS.sized(POLYGON, 65)
    w = _window(case, gpu)
    grid, other = _grid(), sf.UniformGrid(20, 0.0, 10.0, 0.0, 10.0)
    ix = sf.GeometryIndex(w, grid)
    ctx = ix.ctx
    keep = []

    def create(qkind, geoms, g=grid, r=1.0, approximate=0, metric=0, raw=None):
        ro, vo, vx, vy = raw if raw is not None else PCS.query_csr(qkind, geoms)
        keep.append((ro, vo, vx, vy))
        h = C.c_void_p()
        if qkind == POLYGON:
            s = _lib.GfPolygons(len(ro) - 1, ro.ctypes.data, vo.ctypes.data, vx.ctypes.data, vy.ctypes.data)
            st = L.gf_geom_query_create_polygons(ctx.handle, C.byref(g.c_grid), C.byref(s), r, approximate, metric, C.byref(h))
        else:
            s = _lib.GfLineStrings(len(vo) - 1, vo.ctypes.data, vx.ctypes.data, vy.ctypes.data)
            st = L.gf_geom_query_create_linestrings(ctx.handle, C.byref(g.c_grid), C.byref(s), r, approximate, metric, C.byref(h))
        return st, h

    i32, f64 = (lambda v: np.array(v, np.int32)), (lambda v: np.array(v, np.float64))
    # illegal query geometry: an unclosed ring, a 3-vertex ring, a polygon without a ring, a 1-vertex chain, no query
    for raw in ((i32([0, 1]), i32([0, 4]), f64([0, 1, 1, 0]), f64([0, 0, 1, 1])),
                (i32([0, 1]), i32([0, 3]), f64([0, 1, 0]), f64([0, 0, 0])),
                (i32([0, 0]), i32([0]), f64([0]), f64([0])),
                (i32([0]), i32([0]), f64([0]), f64([0]))):
        st, h = create(POLYGON, None, raw=raw)
        assert st == E and not h.value
    for raw in ((None, i32([0, 1]), f64([0]), f64([0])), (None, i32([0]), f64([0]), f64([0])), (None, i32([1, 3]), f64([0, 1, 2]), f64([0, 1, 2]))):
        st, h = create(LINESTRING, None, raw=raw)
        assert st == E and not h.value
    good = PCS.QUERY_SETS["small"]
    assert create(POLYGON, good[POLYGON], metric=2)[0] == E
    assert create(POLYGON, good[POLYGON], g=sf.UniformGrid(46341, 0.0, 10.0, 0.0, 10.0))[0] == E
    # the documented deviation: guaranteed layers 0, several queries, a rectangle leaving the grid -- and only that
    for qkind in (POLYGON, LINESTRING):
        bad = PCS.REFUSED_SETS["leaving_set"][qkind]
        assert create(qkind, bad, r=GC.R_G0)[0] == E
        for r in (GC.R_G1, GC.R_GM1, 0.0):     # other layers: accepted
            st, h = create(qkind, bad, r=r)
            assert st == _lib.GF_OK
            L.gf_geom_query_destroy(h)
        st, h = create(qkind, PCS.QUERY_SETS["leaving"][qkind], r=GC.R_G0)   # one query: exact, accepted
        assert st == _lib.GF_OK
        L.gf_geom_query_destroy(h)
    # no GF_ERR_LAYERS: a negative radius is an empty N
    st, qneg = create(POLYGON, good[POLYGON], r=-1.0)
    assert st == _lib.GF_OK
    st, q1 = create(POLYGON, good[POLYGON])
    st2, q3 = create(LINESTRING, PCS.QUERY_SETS["overlapping"][LINESTRING], r=GC.R_G1)
    st3, qo = create(POLYGON, good[POLYGON], g=other)
    assert st == st2 == st3 == _lib.GF_OK
    rec = torch.zeros(sf.spatialOperators.knn_record_bytes(5), dtype=torch.uint8, device=gpu)
    bm = torch.zeros(2, dtype=torch.int64, device=gpu)
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    assert L.gf_geom_knn_enqueue(q3, ix.handle, 5, ptr(rec)) == E      # a kNN query takes one geometry
    assert L.gf_geom_knn_enqueue(q1, ix.handle, 0, ptr(rec)) == E      # k < 1
    assert L.gf_geom_knn_enqueue(q1, ix.handle, 5, None) == E
    assert L.gf_geom_knn_enqueue(qo, ix.handle, 5, ptr(rec)) == E      # prepared on another grid
    assert L.gf_geom_range_run(qo, ix.handle, ptr(bm), None) == E
    assert L.gf_geom_range_run(q1, ix.handle, None, None) == E
    assert L.gf_geom_range_run(q1, None, ptr(bm), None) == E
    assert L.gf_geom_query_set_chain_mode(q1, 2) == E and L.gf_geom_query_set_chain_mode(q1, 1) == _lib.GF_OK
    qx, qy = (C.c_double * 1)(5.5), (C.c_double * 1)(5.5)
    qp = C.c_void_p()
    assert L.gf_geom_query_create(ctx.handle, C.byref(grid.c_grid), qx, qy, 1, 1.0, 0, 0, C.byref(qp)) == _lib.GF_OK
    assert L.gf_geom_query_set_chain_mode(qp, 1) == E                  # a point query has no runs
    assert L.gf_geom_range_run(q1, ix.handle, ptr(bm), None) == _lib.GF_OK
    assert L.gf_geom_range_run(qneg, ix.handle, ptr(bm), None) == _lib.GF_OK
    ctx.synchronize()
    assert int(bm.cpu().numpy().view(np.uint64).sum()) == 0            # r < 0 selects nothing
    for q in (q1, q3, qo, qneg, qp):
        L.gf_geom_query_destroy(q)
    with pytest.raises(ValueError):   # the operator of the other window kind
        sf.LineStringPolygonRangeQuery(_conf(), grid).run(w, _qobjs(POLYGON, good[POLYGON]), 1.0, index=ix)
    with pytest.raises(ValueError, match="Not yet support"):
        sf.PolygonPolygonRangeQuery(sf.QueryConfiguration(sf.QueryType.RealTime), grid).run(w, _qobjs(POLYGON, good[POLYGON]), 1.0, index=ix)
    ix.close()
