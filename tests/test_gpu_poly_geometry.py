"""GPU: every polygon kernel family (the range kernels inline, deferred and behind the span
prefilter; join_ppoly_{count,write}_kernel with its worklist; the polygon-query kNN scan, fused,
refine and sample kernels) on the catalogue of tests/poly_cases.py -- degenerate and many-vertex
polygons with probes on and around every vertex, edge, vertex ordinate and envelope side, and the
near-collinear lattice family that only the exact orientation sign answers.  Expected values come
from the C oracle, which tests/test_poly_geometry.py ties to the independent reference; for the
collinear families, the holed shape and the comb also from that reference directly.  Everything is
bit-exact: index lists, sorted pair lists, kNN (objID, distance bits, index)."""
import ctypes as C

import numpy as np
import pytest

import edge_cases as E
import poly_cases as PC

pytestmark = pytest.mark.gpu

METRICS = (0, 1)
REF_NAMES = ("collinear_tiled", "collinear_stacked", "holed", "comb")   # also checked against the reference
KNN_NAMES = ("comb", "star", "holed", "spike_dup", "ngon", "collinear_tiled")


@pytest.fixture(scope="module")
def sf(gpu):
    import spatialflink_amd

    return spatialflink_amd


@pytest.fixture(scope="module")
def hyp(oracle_mod):
    f = np.frompyfunc(oracle_mod.lib().orc_hypot, 2, 1)

    def hypot(a, b):
        with np.errstate(all="ignore"):
            return f(a, b).astype(np.float64)
    return hypot


def conf(sf, approximate=False, metric=0):
    c = sf.QueryConfiguration(sf.QueryType.WindowBased)
    c.setApproximateQuery(approximate)
    c.distanceMetric = metric
    return c


def win(sf, x, y, obj=None, ts=None):
    copy = lambda a: None if a is None else np.array(a)   # noqa: E731  (the catalogue's arrays are read-only)
    return sf.PointWindow.from_numpy(np.array(x, np.float64), np.array(y, np.float64), copy(obj), copy(ts))


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def grids(sf, oracle_mod, n=PC.GRID_N):
    return sf.UniformGrid(n, *PC.BEIJING), oracle_mod.grid(n, *PC.BEIJING)


def sf_polygons(sf, name, g):
    """The package's polygons from the rings as a caller lists them (Polygon orders them)."""
    return [sf.Polygon(p, g) for p in PC.raw_polygons(name)]


def variants(name):
    """(approximate, metric) of the entry: exact under both metrics, approximate once."""
    return [(False, 0), (False, 1), (True, 0)]


def expected_range(name, oracle_mod, og, hyp, r, approximate, metric):
    """The expected index list: the oracle's; on REF_NAMES the reference's too (equal, or the test
    fails here).  The tiled family asks the oracle at TINY only (1536 overlapping polygons)."""
    x, y, _, _ = PC.window(name)
    polys = PC.polygons(name)
    exp = None
    if name in REF_NAMES:
        D = PC.window_distances(name, metric, hyp, approximate=approximate)
        exp = PC.ref_range_ppoly(PC.Grid(), x, y, polys, r, D)
    if name != "collinear_tiled" or r == PC.TINY:
        orc = oracle_mod.range_ppoly(og, x, y, oracle_mod.Polygons(polys), r, approximate, metric)
        if exp is not None:
            np.testing.assert_array_equal(orc, exp, err_msg=f"oracle != reference: {name} r {r!r}")
        exp = orc
    return exp


# ---------------------------------------------------------------------------------------------
# range
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PC.NAMES)
def test_range_every_variant(sf, oracle_mod, hyp, name):
    """PointPolygonRangeQuery on the entry's window: exact under both metrics and approximate, every
    radius of the entry at the default plan; TINY (d <= 0), realized radii with their lower
    neighbours and the 2.5-cell radius with the candidate tests inline (1), deferred (2) and behind
    the span prefilter (3), modes 1 and 3 also drained by 1 and by 37 lanes of every wave."""
    g, og = grids(sf, oracle_mod)
    x, y, _, _ = PC.window(name)
    w = win(sf, x, y)
    polys = sf_polygons(sf, name, g)
    tunings = [(None, None)] + [((0, m), None) for m in (1, 2, 3)] + [((0, m), ln) for m in (1, 3) for ln in (1, 37)]
    for approximate, metric in variants(name):
        every = PC.radii(name, metric, hyp)
        some = PC.gpu_radii(name, metric, hyp)
        if approximate and name == "collinear_tiled":
            every = some = [PC.TINY]
        for r in every:
            exp = expected_range(name, oracle_mod, og, hyp, r, approximate, metric)
            assert r == 0.0 or len(exp) > 0
            for tuning, lanes in (tunings if r in some else tunings[:1]):
                op = sf.PointPolygonRangeQuery(conf(sf, approximate, metric), g)
                if tuning is not None:
                    op.tuning = tuning
                if lanes is not None:
                    op.drain_lanes = lanes
                res = op.run(w, polys, r)
                msg = f"{name} approximate {approximate} metric {metric} r {r!r} tuning {tuning} lanes {lanes}"
                np.testing.assert_array_equal(res.indices().astype(np.int64), exp, err_msg=msg)
                assert res.count() == len(exp), msg


def test_range_near_rectangles_one_by_one(sf, oracle_mod, hyp):
    """Every near-rectangle as a query of its own: the true rectangles with 6 vertices or given
    clockwise answer exactly as the plain 5-vertex rectangle of the same box; the bow-tie, the
    three-corner ring and the zero-width ring answer as the oracle, and differently from their
    bounding box's rectangle (the rectangle shortcut applied to them would show here)."""
    g, og = grids(sf, oracle_mod)
    x, y, _, _ = PC.window("near_rects")
    w = win(sf, x, y)
    raw = dict(zip(PC.NEAR_RECTS, PC.raw_polygons("near_rects")))
    rr = PC.realized_radii("near_rects", 0, hyp)
    for r in (PC.TINY, rr[0], rr[-1], E.toward0(rr[-1])):
        got = {}
        for k, p in raw.items():
            res = sf.PointPolygonRangeQuery(conf(sf), g).run(w, [sf.Polygon(p, g)], r)
            got[k] = res.indices().astype(np.int64)
            exp = oracle_mod.range_ppoly(og, x, y, oracle_mod.Polygons([PC.ordered(p)]), r)
            np.testing.assert_array_equal(got[k], exp, err_msg=f"{k} r {r!r}")
        for k in PC.TRUE_RECTS:
            np.testing.assert_array_equal(got[k], got["plain"], err_msg=f"{k} r {r!r}")
        if r == PC.TINY:
            for k in PC.NON_RECTS:
                x1, y1, x2, y2 = PC.shell_bbox(PC.ordered(raw[k]))
                if x1 < x2:
                    box = oracle_mod.range_ppoly(og, x, y, oracle_mod.Polygons([[PC._rect(x1, y1, x2, y2)]]), r)
                    assert not np.array_equal(got[k], box), k


def test_rectangle_detection_in_plan_stats(sf, hyp):
    """gf_range_plan_stats: cells wholly inside the shape are marked inside (accepted untested) only
    for the 5-vertex axis-aligned rectangles -- never for the 6-vertex ones, the bow-tie, the
    three-corner ring, the zero-width ring or the staircase, whose edges are all axis-aligned."""
    from spatialflink_amd import _lib

    g = sf.UniformGrid(PC.GRID_N, *PC.BEIJING)
    L = _lib.lib()
    ctx = _lib.context(0)

    def inside_cells(poly):
        ps = sf.PolygonSet([sf.Polygon(poly, g)])
        cs = ps.c_struct()
        h = C.c_void_p()
        _lib.check(L.gf_range_ppoly_plan_create(ctx.handle, C.byref(g.c_grid), C.byref(cs), PC.CL, 0, 0, C.byref(h)),
                   ctx.handle, "plan")
        try:
            cells = [C.c_int64() for _ in range(4)]
            _lib.check(L.gf_range_plan_stats(h, *[C.byref(c) for c in cells]), ctx.handle, "stats")
            return cells[3].value
        finally:
            L.gf_range_plan_destroy(h)
    raw = dict(zip(PC.NEAR_RECTS, PC.raw_polygons("near_rects")))
    for k in ("plain", "cw0", "cw1", "cw2", "cw3"):
        assert inside_cells(raw[k]) == inside_cells(raw["plain"]) > 0, k
    for k in ("mid_vertex", "dup_corner") + PC.NON_RECTS:
        assert inside_cells(raw[k]) == 0, k
    assert inside_cells(PC.raw_polygons("staircase")[0]) == 0


def catalogue_set(sf, g):
    """The whole catalogue as one polygon set (the tiled family's first 256 triangles)."""
    raw = []
    for name in PC.NAMES:
        raw += PC.raw_polygons(name)[:256]
    return raw, [sf.Polygon(p, g) for p in raw]


def catalogue_window():
    """The probes of the small shapes and of 300 tiled cases, shuffled."""
    xs, ys = [], []
    for name in ("comb", "star", "staircase", "near_rects", "holed", "spike_dup", "sliver", "collinear_stacked"):
        x, y, _, pi = PC.window(name)
        xs.append(x[pi])
        ys.append(y[pi])
    x, y, _, pi = PC.window("collinear_tiled")
    xs.append(x[pi[:300]])
    ys.append(y[pi[:300]])
    x, y = np.concatenate(xs), np.concatenate(ys)
    perm = np.random.default_rng(7).permutation(len(x))
    return x[perm], y[perm]


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_range_whole_catalogue_one_plan(sf, oracle_mod, hyp, mode):
    """Every polygon of the catalogue in one plan: a cell's candidate list holds several polygons,
    whose envelopes hold the point or not and lie near or far (test_point's two passes, env_far)."""
    g, og = grids(sf, oracle_mod)
    raw, polys = catalogue_set(sf, g)
    OP = oracle_mod.Polygons([PC.ordered(p) for p in raw])
    x, y = catalogue_window()
    w = win(sf, x, y)
    d = PC.realized_radii("comb", 0, hyp)[1]
    for metric in METRICS:
        for r in (PC.TINY, d, E.toward0(d), PC.CL):
            op = sf.PointPolygonRangeQuery(conf(sf, False, metric), g)
            if mode:
                op.tuning = (0, mode)
            res = op.run(w, polys, r)
            exp = oracle_mod.range_ppoly(og, x, y, OP, r, False, metric)
            assert 0 < len(exp) < len(x)
            np.testing.assert_array_equal(res.indices().astype(np.int64), exp, err_msg=f"metric {metric} r {r!r}")


def test_range_run_batch_two_windows(sf, oracle_mod, hyp):
    """gf_range_run_batch over two of the windows (the comb's and the holed shape's) on one plan of
    both polygons: each window's counts, bitmap and index list equal the oracle's."""
    import torch
    from spatialflink_amd import _lib

    L = _lib.lib()
    g, og = grids(sf, oracle_mod)
    ctx = _lib.context(0)
    raw = PC.raw_polygons("comb") + PC.raw_polygons("holed")
    OP = oracle_mod.Polygons([PC.ordered(p) for p in raw])
    ps = sf.PolygonSet([sf.Polygon(p, g) for p in raw])
    cs = ps.c_struct()
    data = [PC.window(n)[:2] for n in ("comb", "holed")]
    wins = [win(sf, x, y) for x, y in data]
    sizes = [len(x) for x, _ in data]
    for r in (PC.TINY, PC.realized_radii("holed", 0, hyp)[-1]):
        h = C.c_void_p()
        _lib.check(L.gf_range_ppoly_plan_create(ctx.handle, C.byref(g.c_grid), C.byref(cs), r, 0, 0, C.byref(h)),
                   ctx.handle, "plan")
        try:
            B = 2
            pts = (_lib.GfPoints * B)(*[w.c_struct() for w in wins])
            bms = [torch.zeros((n + 63) // 64, dtype=torch.int64, device="cuda") for n in sizes]
            cnts = [torch.full((2,), -1, dtype=torch.int64, device="cuda") for _ in sizes]
            idxs = [torch.full((n,), -1, dtype=torch.int32, device="cuda") for n in sizes]
            icnt = [torch.full((1,), -1, dtype=torch.int64, device="cuda") for _ in sizes]
            P_ = C.c_void_p
            st = L.gf_range_run_batch(h, B, pts, (P_ * B)(*[b.data_ptr() for b in bms]),
                                      (P_ * B)(*[c.data_ptr() for c in cnts]), (P_ * B)(*[i.data_ptr() for i in idxs]),
                                      (C.c_int64 * B)(*sizes), (P_ * B)(*[c.data_ptr() for c in icnt]))
            _lib.check(st, ctx.handle, "gf_range_run_batch")
            torch.cuda.synchronize()
            for j, (x, y) in enumerate(data):
                exp = oracle_mod.range_ppoly(og, x, y, OP, r)
                assert int(cnts[j][0]) == len(exp) == int(icnt[j][0]) > 0
                np.testing.assert_array_equal(idxs[j][:len(exp)].cpu().numpy().astype(np.int64), exp)
                got = sf.spatialOperators.bitmap_indices(ctx, bms[j], sizes[j]).astype(np.int64)
                np.testing.assert_array_equal(got, exp)
        finally:
            L.gf_range_plan_destroy(h)


# ---------------------------------------------------------------------------------------------
# join
# ---------------------------------------------------------------------------------------------
def expected_join(name, oracle_mod, og, hyp, r, approximate, metric, G=None):
    """The expected sorted pairs: the oracle's; on REF_NAMES the reference's too (equal, or the test
    fails here).  The tiled family asks the oracle at TINY under the sqrt metric only."""
    x, y, _, _ = PC.window(name)
    polys = PC.polygons(name)
    G = G or PC.Grid()
    exp = None
    if name in REF_NAMES:
        if G.n == PC.GRID_N:
            D = PC.window_distances(name, metric, hyp, approximate=approximate)
        else:
            D = PC.distance_matrix(G, x, y, polys, metric, hyp, approximate=approximate)
        exp = PC.ref_join_ppoly(G, x, y, polys, r, D, approximate)
    if name != "collinear_tiled" or (r == PC.TINY and metric == 0 and not approximate):
        orc = E.sorted_pairs(oracle_mod.join_ppoly(og, og, x, y, oracle_mod.Polygons(polys), r, approximate, metric))
        if exp is not None:
            np.testing.assert_array_equal(orc, exp, err_msg=f"oracle != reference: {name} r {r!r}")
        exp = orc
    return exp


@pytest.mark.parametrize("name", PC.NAMES)
def test_join_same_grid(sf, oracle_mod, hyp, name):
    """PointPolygonJoinQuery with ugrid == qgrid (n = 100) on the entry's window: r = 0 (no cells: no
    pairs), TINY, realized radii with their lower neighbours, 2.5 cell lengths; exact under both
    metrics, approximate at TINY and at the last radius."""
    g, og = grids(sf, oracle_mod)
    x, y, _, _ = PC.window(name)
    w = win(sf, x, y)
    polys = sf_polygons(sf, name, g)
    for approximate, metric in variants(name):
        radii = [0.0] + PC.gpu_radii(name, metric, hyp)
        if approximate:
            radii = [radii[1]] if name == "collinear_tiled" else [radii[1], radii[-1]]
        for r in radii:
            exp = expected_join(name, oracle_mod, og, hyp, r, approximate, metric)
            assert (len(exp) == 0) == (r == 0.0)
            got = sf.PointPolygonJoinQuery(conf(sf, approximate, metric), g, g).run(w, polys, r)
            np.testing.assert_array_equal(got, exp, err_msg=f"{name} approximate {approximate} metric {metric} r {r!r}")


def test_join_tiled_pairs_are_the_exact_sign_answers(sf, oracle_mod, hyp):
    """The tiled family as one join of >= 1000 polygons at d <= 0: the pair (probe q, polygon q)
    exists exactly where the exact orientation sign puts the probe inside its triangle -- in >= 40
    cases not where the plain-double sign would."""
    g, og = grids(sf, oracle_mod)
    x, y, _, pi = PC.window("collinear_tiled")
    polys = PC.polygons("collinear_tiled")
    assert len(polys) >= 1000
    got = sf.PointPolygonJoinQuery(conf(sf), g, g).run(win(sf, x, y), sf_polygons(sf, "collinear_tiled", g), PC.TINY)
    have = set(map(tuple, got.tolist()))
    own = np.array([(int(pi[q]), q) in have for q in range(len(polys))])
    exact = np.array([PC.polygon_distance(x[pi[q]:pi[q] + 1], y[pi[q]:pi[q] + 1], polys[q])[0][0] <= 0
                      for q in range(len(polys))])
    plain = np.array([PC.polygon_distance(x[pi[q]:pi[q] + 1], y[pi[q]:pi[q] + 1], polys[q], exact=False)[0][0] <= 0
                      for q in range(len(polys))])
    np.testing.assert_array_equal(own, exact)
    assert (exact != plain).sum() >= 40
    assert 0 < own.sum() < len(polys)


def test_join_stacked_overflows_keep_and_worklist(sf, oracle_mod, hyp):
    """The stacked family as one join: the shared probe pairs with more than kJoinKeep (4) polygons
    (the write pass walks its list again), and the window's pairs -- none of them answered by the
    rectangle shortcut -- outnumber 1024 per round of 256 queued points, so a round's worklist
    overflows (pigeonhole) and its points are recounted by their own walk.  Also the counting call
    (no pair buffer): the exact pair count with GF_ERR_CAPACITY."""
    from spatialflink_amd import _lib

    g, og = grids(sf, oracle_mod)
    x, y, _, pi = PC.window("collinear_stacked")
    w = win(sf, x, y)
    polys = sf_polygons(sf, "collinear_stacked", g)
    for metric in METRICS:
        exp = expected_join("collinear_stacked", oracle_mod, og, hyp, PC.TINY, False, metric)
        assert (exp[:, 0] == pi[0]).sum() > PC.JOIN_KEEP
        assert len(exp) > PC.JOIN_WORK * -(-len(x) // PC.JOIN_ROUND)
        got = sf.PointPolygonJoinQuery(conf(sf, False, metric), g, g).run(w, polys, PC.TINY)
        np.testing.assert_array_equal(got, exp)
    L = _lib.lib()
    ctx = _lib.context(0)
    ps = sf.PolygonSet(polys)
    cs = ps.c_struct()
    pts = w.c_struct()
    n = C.c_int64()
    exp = expected_join("collinear_stacked", oracle_mod, og, hyp, PC.TINY, False, 0)
    st = L.gf_join_ppoly(ctx.handle, C.byref(g.c_grid), C.byref(g.c_grid), C.byref(pts), C.byref(cs), PC.TINY, 0, 0,
                         None, 0, C.byref(n))
    assert st == _lib.GF_ERR_CAPACITY and n.value == len(exp)


@pytest.mark.parametrize("name", ["holed", "comb"])
def test_join_other_grid(sf, oracle_mod, hyp, name):
    """The same join on a 37 x 37 grid (cells of 2.7 times the size: other keys, other lists)."""
    g, og = grids(sf, oracle_mod, 37)
    G = PC.Grid(37)
    x, y, _, _ = PC.window(name)
    w = win(sf, x, y)
    polys = sf_polygons(sf, name, g)
    for metric in METRICS:
        for r in [0.0] + PC.gpu_radii(name, metric, hyp):
            exp = expected_join(name, oracle_mod, og, hyp, r, False, metric, G)
            got = sf.PointPolygonJoinQuery(conf(sf, False, metric), g, g).run(w, polys, r)
            np.testing.assert_array_equal(got, exp, err_msg=f"{name} metric {metric} r {r!r}")


# ---------------------------------------------------------------------------------------------
# polygon-query kNN
# ---------------------------------------------------------------------------------------------
def check_knn(res, exp, msg):
    eo, ed, ei = exp
    np.testing.assert_array_equal(res.objID, eo, err_msg=msg)
    np.testing.assert_array_equal(bits(res.dist), bits(ed), err_msg=msg)
    np.testing.assert_array_equal(res.idx, ei, err_msg=msg)


def expected_knn(name, q, oracle_mod, og, hyp, k, approximate, metric):
    x, y, obj, _ = PC.window(name)
    rings = PC.polygons(name)[q]
    m, oo, od, oi = oracle_mod.knn_ppoly(og, x, y, obj, oracle_mod.Polygons([rings]), PC.KNN_R, k, approximate, metric)
    if name in REF_NAMES:
        D = PC.window_distances(name, metric, hyp, approximate=approximate)
        eo, ed, ei = PC.ref_knn_ppoly(PC.Grid(), x, y, obj, rings, PC.KNN_R, k, D[q])
        assert np.array_equal(oo, eo) and np.array_equal(bits(od), bits(ed)) and np.array_equal(oi, ei), (name, q, k)
    return oo, od, oi


@pytest.mark.parametrize("name", KNN_NAMES)
def test_polyknn_every_distance(sf, oracle_mod, hyp, name):
    """PointPolygonKNNQuery at r = 2 cell lengths with k = 7 and with k above the number of
    candidates (every distance is compared), objIDs with duplicates: exact under both metrics and
    approximate, pipeline depths 1 and 2, and once with a scan capacity of 64 (the exact fallback
    computes the same distances).  One query polygon at a time: the entry's (the tiled family's
    first 8)."""
    import torch

    g, og = grids(sf, oracle_mod)
    x, y, obj, _ = PC.window(name)
    w = win(sf, x, y, obj)
    raw = PC.raw_polygons(name)[:8]
    for q, poly in enumerate(raw):
        P = sf.Polygon(poly, g)
        for approximate, metric in variants(name):
            full = expected_knn(name, q, oracle_mod, og, hyp, len(x), approximate, metric)
            assert len(full[0]) > 7
            for k in (7, len(full[0]) + 3):
                exp = tuple(a[:k] for a in full)
                msg = f"{name} polygon {q} approximate {approximate} metric {metric} k {k}"
                op = sf.PointPolygonKNNQuery(conf(sf, approximate, metric), g)
                check_knn(op.run(w, P, PC.KNN_R, k), exp, msg)
                op.set_pipeline(0, P, PC.KNN_R, k, 2)
                rec = sf.PinnedRecords(2, k)
                for i in range(2):
                    op.enqueue(w, P, PC.KNN_R, k, rec.ptr(i))
                op.flush(0, P, PC.KNN_R, k)
                torch.cuda.synchronize()
                for i in range(2):
                    check_knn(op.finish(w, P, PC.KNN_R, k, rec.raw(i)), exp, msg + " depth 2")
                op.set_pipeline(0, P, PC.KNN_R, k, 1)
                if q == 0 and not approximate:
                    op2 = sf.PointPolygonKNNQuery(conf(sf, approximate, metric), g)
                    op2.set_capacity(0, P, PC.KNN_R, k, 64)
                    check_knn(op2.run(w, P, PC.KNN_R, k), exp, msg + " capacity 64")


def test_polyknn_sampled_window(sf, oracle_mod, hyp):
    """The holed shape with 2^20 + 3 random points around its probes: the sample kernel picks the
    threshold (every other window of this file is below its size)."""
    g, og = grids(sf, oracle_mod)
    x, y, obj, _ = PC.window("holed")
    n = (1 << 20) + 3
    rx, ry = oracle_mod.java_random_points(20, n, *PC.BEIJING)
    x, y = np.concatenate([x, rx]), np.concatenate([y, ry])
    obj = (np.arange(len(x)) % (len(x) // 3)).astype(np.int64)
    P = sf.Polygon(PC.raw_polygons("holed")[0], g)
    OP = oracle_mod.Polygons([PC.polygons("holed")[0]])
    w = win(sf, x, y, obj)
    for metric in METRICS:
        for k in (7, 400):
            res = sf.PointPolygonKNNQuery(conf(sf, False, metric), g).run(w, P, PC.KNN_R, k)
            m, oo, od, oi = oracle_mod.knn_ppoly(og, x, y, obj, OP, PC.KNN_R, k, False, metric)
            assert m == k
            check_knn(res, (oo, od, oi), f"metric {metric} k {k}")


# ---------------------------------------------------------------------------------------------
# sliding windows and shards: per-pane and per-shard plans with these shapes
# ---------------------------------------------------------------------------------------------
def stream_points(names, extra, seed):
    xs, ys = zip(*[PC.window(n)[:2] for n in names])
    rng = np.random.default_rng(seed)
    x = np.concatenate(list(xs) + [rng.uniform(PC.BEIJING[0], PC.BEIJING[1], extra)])
    y = np.concatenate(list(ys) + [rng.uniform(PC.BEIJING[2], PC.BEIJING[3], extra)])
    perm = rng.permutation(len(x))
    return x[perm], y[perm]


def test_sliding_range_over_holed_and_comb(sf, oracle_mod, hyp):
    """SlidingRangeQuery (size 3000, slide 1000) over the holed shape and the comb: every fired
    window's hits equal the oracle over that window's points."""
    g, og = grids(sf, oracle_mod)
    raw = PC.raw_polygons("holed") + PC.raw_polygons("comb")
    OP = oracle_mod.Polygons([PC.ordered(p) for p in raw])
    polys = [sf.Polygon(p, g) for p in raw]
    x, y = stream_points(("holed", "comb"), 17_000, 3)
    ts = np.sort(np.random.default_rng(4).integers(0, 9_000, len(x))).astype(np.int64)
    r = PC.realized_radii("holed", 0, hyp)[-1]
    op = sf.SlidingRangeQuery(sf.PointPolygonRangeQuery(conf(sf), g), polys, r, 3000, 1000)
    got = []
    cuts = [0, len(x) // 3, 2 * len(x) // 3, len(x)]
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        op.push(win(sf, x[lo:hi], y[lo:hi], None, ts[lo:hi]))
        got += op.results()
    op.flush()
    got += op.results()
    assert len(got) >= 9
    for s, e, hits in got:
        m = (ts >= s) & (ts < e)
        exp = oracle_mod.range_ppoly(og, x[m], y[m], OP, r)
        np.testing.assert_array_equal(hits, exp, err_msg=f"window {s}..{e}")
    assert sum(len(h) for _, _, h in got) > 0


@pytest.mark.parametrize("kind", ["range", "knn"])
def test_sliding_engine_outlives_its_operator(sf, kind):
    """The operator of a sliding query finalized before the query itself, as the collector may do
    when both die in one cycle (a failed test's traceback holds them): the pane engine's plan stays
    until the engine is destroyed."""
    g = sf.UniformGrid(PC.GRID_N, *PC.BEIJING)
    x, y, obj, _ = PC.window("comb")
    ts = np.sort(np.random.default_rng(6).integers(0, 5_000, len(x))).astype(np.int64)
    if kind == "range":
        polys = [sf.Polygon(p, g) for p in PC.raw_polygons("comb")]
        q = sf.SlidingRangeQuery(sf.PointPolygonRangeQuery(conf(sf), g), polys, PC.CL, 3000, 1000)
    else:
        q = sf.SlidingKNNQuery(conf(sf), g, sf.Point("q", 116.0, 40.0, 0, g), PC.KNN_R, 7, size_ms=3000, slide_ms=1000)
    q.push(win(sf, x, y, obj, ts))
    assert len(q.results()) >= 1
    q.op.__del__()          # closes the operator's plans, all but the one the engine holds
    q.flush()
    assert len(q.results()) >= 1
    q.close()
    assert len(q.op._plans._orphans) == 0 and len(q.op._plans._held) == 0


def test_sharded_range_three_bands(sf, oracle_mod, hyp):
    """The shapes' polygons over three column bands balanced by candidate work: per-shard hits
    concatenated equal the oracle over the whole window."""
    from spatialflink_amd import sharding

    g, og = grids(sf, oracle_mod)
    raw = []
    for name in PC.SHAPES:
        raw += PC.raw_polygons(name)
    OP = oracle_mod.Polygons([PC.ordered(p) for p in raw])
    polys = [sf.Polygon(p, g) for p in raw]
    x, y = stream_points(("comb", "star", "holed", "near_rects", "sliver"), 5_000, 5)
    cx, cy = oracle_mod.assign_cells(og, x, y)
    r = PC.realized_radii("comb", 0, hyp)[1]
    bb = [(p.boundingBox[0][0], p.boundingBox[0][1], p.boundingBox[1][0], p.boundingBox[1][1]) for p in polys]
    cand = sharding.candidate_columns(g, cx, cy, bb, r)
    pts = np.bincount(np.clip(cx, 0, PC.GRID_N - 1), minlength=PC.GRID_N)
    bands = sharding.work_bands(PC.GRID_N, 3, pts, cand, candidate_cost=8.0)
    assert len(bands) == 3
    perm, off = sharding.shard_order(cx, bands)
    got = []
    for s in range(3):
        ix = perm[off[s]:off[s + 1]]
        assert len(ix) > 0
        res = sf.PointPolygonRangeQuery(conf(sf), g).run(win(sf, x[ix], y[ix]), polys, r)
        got.append(ix[res.indices().astype(np.int64)])
    exp = oracle_mod.range_ppoly(og, x, y, OP, r)
    assert len(exp) > 0
    np.testing.assert_array_equal(np.sort(np.concatenate(got)), exp)
