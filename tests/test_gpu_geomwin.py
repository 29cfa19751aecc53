"""GPU: polygon and linestring windows against query points (gf_geom_*; PolygonPoint / LineStringPoint
{Range,KNN}Query) against the restatement of tests/geomwin_ref.py, exactly: bitmaps equal, kNN objIDs,
indices and distance bits equal -- for every wide_vertices threshold (every object by waves, the middle,
lanes only), exact and approximate, both metrics, at the layer regimes, r = 0 and realized distances with
their ulp neighbours.  Small shapes only: a 10 x 10 unit grid and the 100 x 100 Beijing grid."""
import ctypes as C

import numpy as np
import pytest

import spatialflink_amd as sf
from spatialflink_amd import _lib

import geomwin_cases as GC
import geomwin_ref as R

pytestmark = pytest.mark.gpu

CASES = {"rules": GC.rules, "holes": GC.holes, "rings": GC.rings, "lines": GC.lines}
DEFAULT = 0  # gf_geom_index_set_thresholds: the library's default wide_vertices


def _grid(case):
    n, box = case["grid"]
    return sf.UniformGrid(n, *box)


def _window(case, gpu):
    ro, vo, vx, vy = GC.csr(case)
    return sf.GeometryWindow.from_csr(case["kind"], ro, vo, vx, vy, case["keys"], device=gpu.index)


def _conf(approximate=False, metric=0):
    conf = sf.QueryConfiguration(sf.QueryType.WindowBased)
    conf.setApproximateQuery(approximate)
    conf.distanceMetric = metric
    return conf


def _ops(case, approximate=False, metric=0):
    rq = sf.PolygonPointRangeQuery if case["kind"] == GC.POLYGON else sf.LineStringPointRangeQuery
    kq = sf.PolygonPointKNNQuery if case["kind"] == GC.POLYGON else sf.LineStringPointKNNQuery
    g = _grid(case)
    return rq(_conf(approximate, metric), g), kq(_conf(approximate, metric), g)


def _points(qx, qy):
    return [sf.Point("q", float(a), float(b)) for a, b in zip(qx, qy)]


def _bits(a):
    return np.asarray(a, np.float64).view(np.int64)


@pytest.mark.parametrize("name", sorted(CASES))
def test_prepare_matches_numpy_bit_for_bit(name, gpu, oracle_mod):
    case = CASES[name]()
    w = _window(case, gpu)
    ix = sf.GeometryIndex(w, _grid(case))
    env_ref, ok = GC.numpy_index(case)
    g = R.grid_of(*case["grid"])
    cx1, cy1 = oracle_mod.assign_cells(g, env_ref[:, 0], env_ref[:, 1])
    cx2, cy2 = oracle_mod.assign_cells(g, env_ref[:, 2], env_ref[:, 3])
    nvert = np.array([sum(len(r) for r in o) if case["kind"] == GC.POLYGON else len(o) for o in case["objs"]])
    for thr in (DEFAULT, 64, 1, 65, 63, GC.INT32_MAX):
        ix.set_thresholds(thr)
        env, cells = ix.read()
        assert np.array_equal(_bits(env), _bits(env_ref)), (name, thr)
        assert np.array_equal(cells, np.stack([cx1, cy1, cx2, cy2], axis=1)), (name, thr)
        info = ix.info()
        t = 384 if thr == DEFAULT else thr
        assert info == dict(nobj=len(ok), nvert=int(nvert.sum()), invalid=int((~ok).sum()), wide=int((nvert >= t).sum()))
    ix.close()


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("approximate", [False, True])
def test_range_equals_the_restatement_at_every_threshold(name, approximate, gpu, oracle_mod):
    case = CASES[name]()
    w = _window(case, gpu)
    g = R.grid_of(*case["grid"])
    ix = sf.GeometryIndex(w, _grid(case))
    expected = {}
    for metric in (0, 1):
        for qname, (qx, qy) in case["queries"].items():
            for r in R.case_radii(case, qx, qy, metric, approximate):
                info = {}
                exp = R.range_literal(g, case["kind"], case["objs"], qx, qy, r, approximate, metric, info=info)
                expected[(metric, qname, r)] = (exp, info)
    waved = 0
    for thr in GC.THRESHOLDS + (DEFAULT,):
        ix.set_thresholds(thr)
        for metric in (0, 1):
            op, _ = _ops(case, approximate, metric)
            for qname, (qx, qy) in case["queries"].items():
                for r in R.case_radii(case, qx, qy, metric, approximate):
                    exp, info = expected[(metric, qname, r)]
                    res = op.run(w, _points(qx, qy), r, index=ix)
                    got = res.indices().astype(np.int64)
                    assert np.array_equal(got, exp), (name, thr, metric, qname, r)
                    assert res.count() == len(exp) and res.multiset_size() == info["all_guaranteed"]
                    gi = op.info()
                    assert {k: gi[k] for k in info} == info, (name, thr, metric, qname, r, gi)
                    assert gi["wave_path"] == (gi["tested"] if thr == 1 and not approximate else gi["wave_path"])
                    assert thr != GC.INT32_MAX or gi["wave_path"] == 0
                    waved += gi["wave_path"]
    assert approximate or waved > 0
    ix.close()


def test_the_default_threshold_sends_the_long_ring_to_a_wave(gpu, oracle_mod):
    case = GC.rings()
    w = _window(case, gpu)
    ix = sf.GeometryIndex(w, _grid(case))
    nvert = np.array([sum(len(r) for r in o) for o in case["objs"]])
    assert nvert[len(GC.RING_SIZES)] == 5066 and ix.info()["wide"] == int((nvert >= 384).sum()) >= 1
    op, _ = _ops(case)
    qx, qy = case["queries"]["p1"]  # inside the long ring's hole
    r = 1.6 * GC.PC.CL
    res = op.run(w, _points(qx, qy), r, index=ix)
    exp = R.range_literal(R.grid_of(*case["grid"]), case["kind"], case["objs"], qx, qy, r)
    assert np.array_equal(res.indices().astype(np.int64), exp) and len(GC.RING_SIZES) in exp.tolist()
    info = {}
    R.range_literal(R.grid_of(*case["grid"]), case["kind"], case["objs"], qx, qy, r, info=info)
    gi = op.info()
    assert {k: gi[k] for k in info} == info and 1 <= gi["wave_path"] <= gi["tested"]
    ix.set_thresholds(GC.INT32_MAX)
    res = op.run(w, _points(qx, qy), r, index=ix)
    assert np.array_equal(res.indices().astype(np.int64), exp) and op.info()["wave_path"] == 0
    ix.close()


@pytest.mark.parametrize("kind", [GC.POLYGON, GC.LINESTRING])
@pytest.mark.parametrize("n", GC.SIZES)
def test_window_sizes(kind, n, gpu, oracle_mod):
    case = GC.sized(kind, n)
    w = _window(case, gpu)
    g = R.grid_of(*case["grid"])
    rop, kop = _ops(case)
    ix = sf.GeometryIndex(w, _grid(case))
    for thr in (1, DEFAULT):
        ix.set_thresholds(thr)
        for qname in ("five", "borders"):
            qx, qy = case["queries"][qname]
            exp = R.range_literal(g, kind, case["objs"], qx, qy, GC.R_G0)
            res = rop.run(w, _points(qx, qy), GC.R_G0, index=ix)
            assert np.array_equal(res.indices().astype(np.int64), exp), (n, thr, qname)
            assert res.count() == len(exp)
        o, d, i = R.knn_literal(g, kind, case["objs"], case["keys"], 5.5, 5.5, GC.R_G1, 7)
        got = kop.run(w, sf.Point("q", 5.5, 5.5), GC.R_G1, 7, index=ix)
        assert np.array_equal(got.objID, o) and np.array_equal(got.idx, i) and np.array_equal(_bits(got.dist), _bits(d))
    ix.close()


@pytest.mark.parametrize("kind", [GC.POLYGON, GC.LINESTRING])
def test_knn_depths_ties_and_duplicates(kind, gpu, oracle_mod):
    """k on both sides of the one-block select's 512; duplicate objIDs keep their smaller distance once; fewer
    than k candidates; both metrics, exact and approximate"""
    case = GC.sized(kind, 3001)
    w = _window(case, gpu)
    g = R.grid_of(*case["grid"])
    ix = sf.GeometryIndex(w, _grid(case))
    for approximate, metric in ((False, 0), (False, 1), (True, 0)):
        _, kop = _ops(case, approximate, metric)
        for thr in (1, DEFAULT):
            ix.set_thresholds(thr)
            for k, r in ((1, GC.R_G1), (7, GC.R_G1), (50, GC.R_G1), (600, 4.5), (600, GC.R_GM1), (513, 0.0)):
                o, d, i = R.knn_literal(g, kind, case["objs"], case["keys"], 5.5, 5.5, r, k, approximate, metric)
                got = kop.run(w, sf.Point("q", 5.5, 5.5), r, k, index=ix)
                assert np.array_equal(got.objID, o), (approximate, metric, thr, k, r)
                assert np.array_equal(got.idx, i) and np.array_equal(_bits(got.dist), _bits(d)), (approximate, metric, thr, k, r)
                if (k, r) == (600, 4.5):
                    assert len(o) == 600  # the sorted path filled the record
                if (k, r) == (600, GC.R_GM1):
                    assert 0 < len(o) < 600
    ix.close()


@pytest.mark.parametrize("name", ["holes", "rings", "lines"])
def test_knn_on_the_hand_built_cases(name, gpu, oracle_mod):
    case = CASES[name]()
    w = _window(case, gpu)
    g = R.grid_of(*case["grid"])
    ix = sf.GeometryIndex(w, _grid(case))
    cl = (case["grid"][1][1] - case["grid"][1][0]) / case["grid"][0]
    ties = 0
    for thr in GC.THRESHOLDS:
        ix.set_thresholds(thr)
        for approximate, metric in ((False, 0), (False, 1), (True, 0)):
            _, kop = _ops(case, approximate, metric)
            for qname, (qx, qy) in case["queries"].items():
                if len(qx) != 1:
                    continue
                for k, r in ((1, 3.0 * cl), (3, 3.0 * cl), (50, 3.0 * cl), (50, 0.75 * cl), (600, 1.6 * cl)):
                    o, d, i = R.knn_literal(g, case["kind"], case["objs"], case["keys"], qx[0], qy[0], r, k, approximate, metric)
                    got = kop.run(w, sf.Point("q", qx[0], qy[0]), r, k, index=ix)
                    assert np.array_equal(got.objID, o) and np.array_equal(got.idx, i), (name, thr, qname, k, r)
                    assert np.array_equal(_bits(got.dist), _bits(d)), (name, thr, qname, k, r)
                    ties += int((d == 0.0).sum() > 1)
    assert name != "holes" or ties > 0  # several polygons contain the query point: ordered by key, then idx
    ix.close()


@pytest.mark.parametrize("kind", [GC.POLYGON, GC.LINESTRING])
def test_an_object_within_r_but_with_no_cell_in_N_is_dropped(kind, gpu, oracle_mod):
    """across a cell corner on a grid of cell length fl(0.3): the reference's cell filter drops it, so must the kernel"""
    case = GC.corner(kind)
    w = _window(case, gpu)
    g = R.grid_of(*case["grid"])
    ix = sf.GeometryIndex(w, _grid(case))
    qx, qy = case["queries"]["corner"]
    for thr in GC.THRESHOLDS:
        ix.set_thresholds(thr)
        for approximate, metric in ((False, 0), (False, 1), (True, 0)):
            assert R.distance(kind, case["objs"][0], qx[0], qy[0], metric, approximate) <= GC.CORNER_R
            rop, kop = _ops(case, approximate, metric)
            exp = R.range_literal(g, kind, case["objs"], qx, qy, GC.CORNER_R, approximate, metric)
            res = rop.run(w, _points(qx, qy), GC.CORNER_R, index=ix)
            assert exp.tolist() == [1] and np.array_equal(res.indices().astype(np.int64), exp), (thr, approximate, metric)
            assert rop.info()["filtered"] == 1
            o, d, i = R.knn_literal(g, kind, case["objs"], case["keys"], qx[0], qy[0], GC.CORNER_R, 5, approximate, metric)
            got = kop.run(w, sf.Point("q", qx[0], qy[0]), GC.CORNER_R, 5, index=ix)
            assert np.array_equal(got.idx, i) and np.array_equal(got.objID, o) and np.array_equal(_bits(got.dist), _bits(d))
            assert got.idx.tolist() == [1]
    ix.close()


def test_one_index_prepared_again_for_every_window(gpu, oracle_mod):
    """the per-window path of a continuous query: one index through windows of both growing and shrinking size
    (its arrays grow only), polygons with several rings, an empty window and a window without a vertex"""
    g = R.grid_of(*GC.UNIT)
    grid = sf.UniformGrid(GC.UNIT[0], *GC.UNIT[1])
    rop, kop = _ops(GC.sized(GC.POLYGON, 65))
    qx, qy = GC.QUERIES_UNIT["five"]
    ix = None
    for n in (65, 3001, 0, 257, 3001, 1):
        case = GC.sized(GC.POLYGON, n)
        w = _window(case, gpu)
        if ix is None:
            ix = sf.GeometryIndex(w, grid)
            ix.set_thresholds(8)
        else:
            ix.prepare(w)
        env_ref, ok = GC.numpy_index(case)
        env, _ = ix.read()
        assert np.array_equal(_bits(env), _bits(env_ref)) and ix.info()["invalid"] == int((~ok).sum()), n
        exp = R.range_literal(g, GC.POLYGON, case["objs"], qx, qy, GC.R_G0)
        res = rop.run(w, _points(qx, qy), GC.R_G0, index=ix)
        assert np.array_equal(res.indices().astype(np.int64), exp), n
        o, d, i = R.knn_literal(g, GC.POLYGON, case["objs"], case["keys"], 5.5, 5.5, GC.R_G1, 7)
        got = kop.run(w, sf.Point("q", 5.5, 5.5), GC.R_G1, 7, index=ix)
        assert np.array_equal(got.objID, o) and np.array_equal(got.idx, i) and np.array_equal(_bits(got.dist), _bits(d)), n
    hollow = sf.PolygonWindow.from_polygons([[], []], device=gpu.index)  # objects without a ring: no vertex at all
    ix.prepare(hollow)
    assert ix.info() == dict(nobj=2, nvert=0, invalid=2, wide=0)
    assert rop.run(hollow, _points(qx, qy), GC.R_G0, index=ix).count() == 0
    ix.close()


def test_a_record_merges_with_a_point_window_record(gpu, oracle_mod):
    import torch

    case = GC.sized(GC.POLYGON, 257)
    w = _window(case, gpu)
    grid = _grid(case)
    k, r = 7, GC.R_G1
    _, kop = _ops(case)
    ix = sf.GeometryIndex(w, grid)
    nb = sf.spatialOperators.knn_record_bytes(k)
    recs = torch.zeros(2 * nb, dtype=torch.uint8, device=gpu)
    ctx = kop.enqueue(w, sf.Point("q", 5.5, 5.5), r, k, recs[:nb], ix)
    rnd = np.random.default_rng(3)
    px, py = rnd.uniform(3.0, 8.0, 500), rnd.uniform(3.0, 8.0, 500)
    pobj = np.arange(500, dtype=np.int64) % 300 + 100   # some keys shared with the geometry window
    pw = sf.PointWindow.from_numpy(px, py, pobj, device=gpu.index)
    pop = sf.PointPointKNNQuery(_conf(), grid)
    pop.enqueue(pw, sf.Point("q", 5.5, 5.5, 0, grid), r, k, recs[nb:])
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
    g = R.grid_of(*case["grid"])
    eo, ed, ei = R.knn_literal(g, GC.POLYGON, case["objs"], case["keys"], 5.5, 5.5, r, k)
    assert np.array_equal(parts[0][1], eo) and np.array_equal(_bits(parts[0][2]), _bits(ed)) and np.array_equal(parts[0][3], ei)
    ix.close()


def test_one_index_many_queries_and_one_query_many_windows(gpu, oracle_mod):
    small, large = GC.sized(GC.POLYGON, 65), GC.sized(GC.POLYGON, 3001)
    g = R.grid_of(*small["grid"])
    rop, kop = _ops(small)
    qx, qy = small["queries"]["one"]
    for _ in range(2):  # the same cached queries over a small window, then a larger one, then both again
        for case in (small, large):
            w = _window(case, gpu)
            ix = sf.GeometryIndex(w, _grid(case))
            res = rop.run(w, _points(qx, qy), GC.R_G0, index=ix)
            got = kop.run(w, sf.Point("q", 5.5, 5.5), GC.R_G1, 50, index=ix)
            res2 = rop.run(w, _points(qx, qy), GC.R_G0, index=ix)
            exp = R.range_literal(g, GC.POLYGON, case["objs"], qx, qy, GC.R_G0)
            assert np.array_equal(res.indices().astype(np.int64), exp) and np.array_equal(res2.indices().astype(np.int64), exp)
            o, d, i = R.knn_literal(g, GC.POLYGON, case["objs"], case["keys"], 5.5, 5.5, GC.R_G1, 50)
            assert np.array_equal(got.objID, o) and np.array_equal(got.idx, i) and np.array_equal(_bits(got.dist), _bits(d))
            ix.close()
    assert len(rop._plans) == 1 and len(kop._plans) == 1


def test_refusals_that_need_handles(gpu, oracle_mod):
    import torch

    L = _lib.lib()
    case = GC.sized(GC.POLYGON, 65)
    w = _window(case, gpu)
    grid, other = _grid(case), sf.UniformGrid(20, 0.0, 10.0, 0.0, 10.0)
    ix = sf.GeometryIndex(w, grid)
    ctx = ix.ctx
    qx, qy = (C.c_double * 2)(5.5, 6.5), (C.c_double * 2)(5.5, 5.5)

    def query(g, nq, r=1.0):
        h = C.c_void_p()
        assert L.gf_geom_query_create(ctx.handle, C.byref(g.c_grid), qx, qy, nq, r, 0, 0, C.byref(h)) == _lib.GF_OK
        return h
    q1, q2, qo = query(grid, 1), query(grid, 2), query(other, 1)
    rec = torch.zeros(sf.spatialOperators.knn_record_bytes(5), dtype=torch.uint8, device=gpu)
    bm = torch.zeros(2, dtype=torch.int64, device=gpu)
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    assert L.gf_geom_knn_enqueue(q2, ix.handle, 5, ptr(rec)) == _lib.GF_ERR_ARG      # a kNN query takes one point
    assert L.gf_geom_knn_enqueue(q1, ix.handle, 0, ptr(rec)) == _lib.GF_ERR_ARG      # k < 1
    assert L.gf_geom_knn_enqueue(q1, ix.handle, 5, None) == _lib.GF_ERR_ARG
    assert L.gf_geom_knn_enqueue(qo, ix.handle, 5, ptr(rec)) == _lib.GF_ERR_ARG      # prepared on another grid
    assert L.gf_geom_range_run(qo, ix.handle, ptr(bm), None) == _lib.GF_ERR_ARG
    assert L.gf_geom_range_run(q1, ix.handle, None, None) == _lib.GF_ERR_ARG
    assert L.gf_geom_range_run(q1, None, ptr(bm), None) == _lib.GF_ERR_ARG
    assert L.gf_geom_index_set_thresholds(ix.handle, -1) == _lib.GF_ERR_ARG
    g = w.c_struct()
    g.objID = None
    h = C.c_void_p()
    assert L.gf_geom_prepare(ctx.handle, C.byref(grid.c_grid), C.byref(g), C.byref(h)) == _lib.GF_OK
    assert L.gf_geom_knn_enqueue(q1, h, 5, ptr(rec)) == _lib.GF_ERR_ARG              # kNN needs the objID keys
    assert L.gf_geom_range_run(q1, h, ptr(bm), None) == _lib.GF_OK                   # range does not
    assert L.gf_geom_range_run(q1, ix.handle, ptr(bm), None) == _lib.GF_OK
    ctx.synchronize()
    L.gf_geom_index_destroy(h)
    for q in (q1, q2, qo):
        L.gf_geom_query_destroy(q)
    with pytest.raises(ValueError):  # the operator of the other kind
        sf.LineStringPointRangeQuery(_conf(), grid).run(w, _points([5.5], [5.5]), 1.0, index=ix)
    with pytest.raises(_lib.CandidateLayersError):
        sf.PolygonPointRangeQuery(_conf(), grid).run(w, _points([5.5], [5.5]), -1.0, index=ix)
    ix.close()
