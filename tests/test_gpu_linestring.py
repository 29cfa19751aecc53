"""GPU: the linestring queries over point windows -- PointLineStringRangeQuery, PointLineStringKNNQuery,
PointLineStringJoinQuery and the C entry points behind them -- on the catalogue of
tests/linestring_cases.py, against its numpy restatement (tests/test_linestring_ref.py pins that to
the C oracle).  Every comparison is exact: equal index sets, equal pair sets, bit-equal (d, objID)
lists."""
import ctypes as C

import numpy as np
import pytest

import linestring_cases as LC
import poly_cases as PC

pytestmark = pytest.mark.gpu

METRICS = (0, 1)
VARIANTS = [(False, 0), (False, 1), (True, 0), (True, 1)]
KS = (1, 7, 50, 600)                     # 600 > 512: the sorted path
CHAIN_NAMES = LC.ZIGZAGS + ("many",)


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


def grid(sf):
    return sf.UniformGrid(LC.GRID_N, *LC.BEIJING)


def sf_lines(sf, name, g):
    return [sf.LineString(c, g) for c in LC.lines(name)]


def expected_range(name, hyp, r, approximate, metric):
    x, y, _, _ = LC.window(name)
    D = LC.window_distances(name, metric, hyp, approximate)
    return LC.ref_range_pls(PC.Grid(), x, y, LC.lines(name), r, D)


def plan_stats(L, plan):
    cells = [C.c_int64() for _ in range(4)]
    assert L.gf_range_plan_stats(plan, *[C.byref(c) for c in cells]) == 0
    return [c.value for c in cells]


# ---------------------------------------------------------------------------------------------
# range
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("approximate,metric", VARIANTS)
@pytest.mark.parametrize("name", LC.NAMES)
def test_range(sf, hyp, name, approximate, metric):
    """PointLineStringRangeQuery on the entry's window at every radius of the entry (0, each realized
    distance and its two neighbours, half a cell, 2.5 cells) against ref_range_pls; in exact mode
    gf_range_plan_stats reports no inside cell."""
    from spatialflink_amd import _lib

    g = grid(sf)
    x, y, _, _ = LC.window(name)
    w = win(sf, x, y)
    lines = sf_lines(sf, name, g)
    op = sf.PointLineStringRangeQuery(conf(sf, approximate, metric), g)
    for r in LC.radii(name, metric, hyp):
        exp = expected_range(name, hyp, r, approximate, metric)
        assert r == 0.0 or 0 < len(exp) < len(x)
        res = op.run(w, lines, r)
        msg = f"{name} approximate {approximate} metric {metric} r {r!r}"
        np.testing.assert_array_equal(res.indices().astype(np.int64), exp, err_msg=msg)
        assert res.count() == len(exp), msg
        if not approximate:
            _, plan = op.plan(0, lines, r)
            assert plan_stats(_lib.lib(), plan)[3] == 0, msg


@pytest.mark.parametrize("metric", METRICS)
def test_closed_square_rejects_interior_points(sf, hyp, metric):
    """A closed chain encloses nothing: the lattice of points inside the square (whole cells lie inside
    it) farther than r from its border is rejected, the points within r of the border are selected.
    Fails if the rectangle shortcut, the containment test or an inside-cell region survived."""
    g = grid(sf)
    name = "closed_square"
    x, y, _, _ = LC.window(name)
    sx, sy, ss = LC.SQUARE
    inside = (x > sx) & (x < sx + ss) & (y > sy) & (y < sy + ss)
    d = LC.window_distances(name, metric, hyp)[0]
    w = win(sf, x, y)
    for r in (0.3 * LC.CL, LC.CL):
        res = sf.PointLineStringRangeQuery(conf(sf, False, metric), g).run(w, sf_lines(sf, name, g), r)
        got = np.zeros(len(x), bool)
        got[res.indices().astype(np.int64)] = True
        far = inside & (d > r)
        assert far.sum() >= 30 and (inside & (d <= r)).sum() >= 30
        assert not got[far].any()
        assert got[inside & (d <= r)].all()
        np.testing.assert_array_equal(np.flatnonzero(got), expected_range(name, hyp, r, False, metric))


@pytest.mark.parametrize("name", CHAIN_NAMES)
def test_chain_modes_agree(sf, hyp, name):
    """Sub-chain envelopes (mode 0) and the plain segment loop (mode 1) give identical bitmaps and
    identical kNN records, both equal to the reference: lines of CHAIN_RUN - 1 and CHAIN_RUN segments
    (one run) and CHAIN_RUN + 1 (a second run of one segment) -- at most CHAIN_PLAIN_RUNS runs: the plain
    loop either way --, 2 CHAIN_RUN + 1 (the shortest line whose runs the range kernels skip: two whole
    runs and a third of one segment), 4 CHAIN_RUN and 4 CHAIN_RUN + 1 (the same threshold of the kNN
    kernels), 4097 (129 runs), and 300 short lines in one plan."""
    assert 2 * LC.CHAIN_RUN + 1 > LC.CHAIN_PLAIN_RUNS * LC.CHAIN_RUN >= LC.CHAIN_RUN + 1
    g = grid(sf)
    x, y, obj, _ = LC.window(name)
    w = win(sf, x, y, obj)
    lines = sf_lines(sf, name, g)
    for metric in METRICS:
        for r in LC.radii(name, metric, hyp)[1:]:
            exp = expected_range(name, hyp, r, False, metric)
            for mode in (0, 1):
                op = sf.PointLineStringRangeQuery(conf(sf, False, metric), g)
                op.chain_mode = mode
                res = op.run(w, lines, r)
                np.testing.assert_array_equal(res.indices().astype(np.int64), exp, err_msg=f"{name} mode {mode} r {r!r}")
        d = LC.window_distances(name, metric, hyp)[0]
        for k in (7, 600):
            exp = LC.ref_knn_pls(PC.Grid(), x, y, obj, LC.lines(name)[0], LC.KNN_R, k, d)
            assert len(exp[0]) > 0
            for mode in (0, 1):
                op = sf.PointLineStringKNNQuery(conf(sf, False, metric), g)
                op.chain_mode = mode
                check_knn(op.run(w, lines[0], LC.KNN_R, k), exp, f"{name} mode {mode} metric {metric} k {k}")


@pytest.mark.parametrize("how", ["defer1", "defer2", "defer3", "drain5"])
def test_range_plumbing_tuning(sf, hyp, how):
    """One case through the candidate tests inline (1), deferred (2), behind the span prefilter (3), and
    the deferred drain on 5 lanes of every wave: zigzag_65 (two runs and a third of one segment)."""
    g = grid(sf)
    name = "zigzag_65"
    x, y, _, _ = LC.window(name)
    w = win(sf, x, y)
    for r in LC.radii(name, 0, hyp)[1:]:
        op = sf.PointLineStringRangeQuery(conf(sf), g)
        op.tuning = (0, int(how[-1])) if how.startswith("defer") else (0, 2)
        if how == "drain5":
            op.drain_lanes = 5
        res = op.run(w, sf_lines(sf, name, g), r)
        np.testing.assert_array_equal(res.indices().astype(np.int64), expected_range(name, hyp, r, False, 0),
                                      err_msg=f"{how} r {r!r}")


def test_range_run_batch_three_windows(sf, hyp):
    """gf_range_run_batch over three windows (those of zigzag_65, zigzag_33 and dup_vertex) on one plan
    of the three lines: each window's counts, bitmap and index list equal the reference."""
    import torch
    from spatialflink_amd import _lib

    L = _lib.lib()
    g = grid(sf)
    ctx = _lib.context(0)
    names = ("zigzag_65", "zigzag_33", "dup_vertex")
    chains = [LC.lines(n)[0] for n in names]
    ls = sf.LineStringSet([sf.LineString(c, g) for c in chains])
    cs = ls.c_struct()
    data = [LC.window(n)[:2] for n in names]
    wins = [win(sf, x, y) for x, y in data]
    sizes = [len(x) for x, _ in data]
    r = LC.CL
    h = C.c_void_p()
    _lib.check(L.gf_range_pls_plan_create(ctx.handle, C.byref(g.c_grid), C.byref(cs), r, 0, 0, C.byref(h)), ctx.handle, "plan")
    try:
        B = 3
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
            D = LC.distance_matrix(PC.Grid(), x, y, chains, 0, hyp)
            exp = LC.ref_range_pls(PC.Grid(), x, y, chains, r, D)
            assert int(cnts[j][0]) == len(exp) == int(icnt[j][0]) > 0
            np.testing.assert_array_equal(idxs[j][:len(exp)].cpu().numpy().astype(np.int64), exp)
            got = sf.spatialOperators.bitmap_indices(ctx, bms[j], sizes[j]).astype(np.int64)
            np.testing.assert_array_equal(got, exp)
    finally:
        L.gf_range_plan_destroy(h)


def test_sliding_range_over_a_line(sf, hyp):
    """SlidingRangeQuery (windows of 3 panes, slide 1 pane) over zigzag_65: every fired window's hits
    equal the reference over that window's points."""
    g = grid(sf)
    name = "zigzag_65"
    x, y, _, _ = LC.window(name)
    chains = LC.lines(name)
    ts = np.sort(np.random.default_rng(4).integers(0, 6_000, len(x))).astype(np.int64)
    r = LC.CL
    D = LC.window_distances(name, 0, hyp)
    op = sf.SlidingRangeQuery(sf.PointLineStringRangeQuery(conf(sf), g), sf_lines(sf, name, g), r, 3000, 1000)
    op.push(win(sf, x, y, None, ts))
    got = op.results()
    op.flush()
    got += op.results()
    assert len(got) >= 6
    total = 0
    for s, e, hits in got:
        m = np.flatnonzero((ts >= s) & (ts < e))
        exp = LC.ref_range_pls(PC.Grid(), x[m], y[m], chains, r, D[:, m])
        np.testing.assert_array_equal(hits, exp, err_msg=f"window {s}..{e}")
        total += len(exp)
    assert total > 0
    op.close()


# ---------------------------------------------------------------------------------------------
# kNN
# ---------------------------------------------------------------------------------------------
def check_knn(res, exp, msg):
    eo, ed, ei = exp
    np.testing.assert_array_equal(res.objID, eo, err_msg=msg)
    np.testing.assert_array_equal(bits(res.dist), bits(ed), err_msg=msg)
    np.testing.assert_array_equal(res.idx, ei, err_msg=msg)


@pytest.mark.parametrize("name", LC.SINGLE)
def test_knn_every_k(sf, hyp, name):
    """PointLineStringKNNQuery at r = 2 cell lengths with k = 1, 7, 50 and 600 (above 512: the sorted
    path), objIDs with duplicates: exact under both metrics and approximate; the record is the
    reference's (objID, distance bits, index)."""
    g = grid(sf)
    x, y, obj, _ = LC.window(name)
    w = win(sf, x, y, obj)
    chain = LC.lines(name)[0]
    line = sf.LineString(chain, g)
    for approximate, metric in VARIANTS[:3]:
        d = LC.window_distances(name, metric, hyp, approximate)[0]
        for k in KS:
            exp = LC.ref_knn_pls(PC.Grid(), x, y, obj, chain, LC.KNN_R, k, d)
            assert len(exp[0]) == k or k == 600
            op = sf.PointLineStringKNNQuery(conf(sf, approximate, metric), g)
            check_knn(op.run(w, line, LC.KNN_R, k), exp, f"{name} approximate {approximate} metric {metric} k {k}")


def continuous_windows(name, count):
    """`count` windows cut from the entry's window (each drops another 97 points from its front)."""
    x, y, obj, _ = LC.window(name)
    return [(x[97 * i:], y[97 * i:], obj[97 * i:]) for i in range(count)]


@pytest.mark.parametrize("depth", [1, 2])
def test_knn_continuous_windows_with_the_hint(sf, hyp, depth):
    """Six windows in a row on one plan with the threshold hint on (the default), at pipeline depths 1
    and 2: every window's record equals its own reference."""
    import torch

    g = grid(sf)
    name = "zigzag_65"
    chain = LC.lines(name)[0]
    line = sf.LineString(chain, g)
    k = 50
    wins = continuous_windows(name, 6)
    exps = []
    for x, y, obj in wins:
        d = LC.distance_matrix(PC.Grid(), x, y, [chain], 0, hyp)[0]
        exps.append(LC.ref_knn_pls(PC.Grid(), x, y, obj, chain, LC.KNN_R, k, d))
    op = sf.PointLineStringKNNQuery(conf(sf), g)
    dev = [win(sf, *w) for w in wins]
    if depth == 1:
        for i, w in enumerate(dev):
            check_knn(op.run(w, line, LC.KNN_R, k), exps[i], f"window {i}")
        return
    op.set_pipeline(0, line, LC.KNN_R, k, 2)
    rec = sf.PinnedRecords(len(dev), k)
    for i, w in enumerate(dev):
        op.enqueue(w, line, LC.KNN_R, k, rec.ptr(i))
    op.flush(0, line, LC.KNN_R, k)
    torch.cuda.synchronize()
    for i, w in enumerate(dev):
        check_knn(op.finish(w, line, LC.KNN_R, k, rec.raw(i)), exps[i], f"window {i} depth 2")
    op.set_pipeline(0, line, LC.KNN_R, k, 1)


def test_knn_capacity_fallback_and_short_records(sf, hyp):
    """A candidate capacity of 64 forces the exact fallback (the same record); and a window where fewer
    than k objIDs lie within r returns them all."""
    g = grid(sf)
    name = "zigzag_65"
    x, y, obj, _ = LC.window(name)
    w = win(sf, x, y, obj)
    chain = LC.lines(name)[0]
    line = sf.LineString(chain, g)
    for metric in METRICS:
        d = LC.window_distances(name, metric, hyp)[0]
        exp = LC.ref_knn_pls(PC.Grid(), x, y, obj, chain, LC.KNN_R, 50, d)
        op = sf.PointLineStringKNNQuery(conf(sf, False, metric), g)
        op.set_capacity(0, line, LC.KNN_R, 50, 64)
        check_knn(op.run(w, line, LC.KNN_R, 50), exp, f"capacity 64 metric {metric}")
    name = "two"
    x, y, obj, _ = LC.window(name)
    chain = LC.lines(name)[0]
    r = 0.3 * LC.CL
    d = LC.window_distances(name, 0, hyp)[0]
    for k in (50, 600):
        exp = LC.ref_knn_pls(PC.Grid(), x, y, obj, chain, r, k, d)
        assert k == 50 or 50 < len(exp[0]) < 600
        res = sf.PointLineStringKNNQuery(conf(sf), g).run(win(sf, x, y, obj), sf.LineString(chain, g), r, k)
        check_knn(res, exp, f"fewer than k = {k} within r")


def test_sliding_knn_over_a_line(sf, hyp):
    """SlidingKNNQuery on a PointLineStringKNNQuery plan (windows of 3 panes, slide 1): every fired
    window's record equals the reference over that window's points."""
    g = grid(sf)
    name = "zigzag_65"
    x, y, obj, _ = LC.window(name)
    chain = LC.lines(name)[0]
    line = sf.LineString(chain, g)
    ts = np.sort(np.random.default_rng(8).integers(0, 6_000, len(x))).astype(np.int64)
    k = 7
    d = LC.window_distances(name, 0, hyp)[0]
    c = conf(sf)
    q = sf.SlidingKNNQuery(c, g, line, LC.KNN_R, k, size_ms=3000, slide_ms=1000, op=sf.PointLineStringKNNQuery(c, g))
    q.push(win(sf, x, y, obj, ts))
    got = q.results()
    q.flush()
    got += q.results()
    assert len(got) >= 6
    for res in got:
        m = np.flatnonzero((ts >= res.windowStart) & (ts < res.windowEnd))
        exp = LC.ref_knn_pls(PC.Grid(), x[m], y[m], obj[m], chain, LC.KNN_R, k, d[m])
        check_knn(res, exp, f"window {res.windowStart}..{res.windowEnd}")
    q.close()


# ---------------------------------------------------------------------------------------------
# join
# ---------------------------------------------------------------------------------------------
def join_case(which, hyp):
    """(x, y, chains, D(metric, approximate)): `many` on its window (the shared distance matrix), or
    closed_square + dup_vertex as a 2-line set on both their windows."""
    if which == "many":
        x, y, _, _ = LC.window("many")
        return x, y, LC.lines("many"), lambda m, ap: LC.window_distances("many", m, hyp, ap)
    a, b = LC.window("closed_square"), LC.window("dup_vertex")
    x, y = np.concatenate([a[0], b[0]]), np.concatenate([a[1], b[1]])
    chains = LC.lines("closed_square") + LC.lines("dup_vertex")
    return x, y, chains, lambda m, ap: LC.distance_matrix(PC.Grid(), x, y, chains, m, hyp, ap)


@pytest.mark.parametrize("approximate", [False, True])
@pytest.mark.parametrize("which", ["many", "square_and_dup"])
def test_join(sf, hyp, which, approximate):
    """PointLineStringJoinQuery against ref_join_pls (pairs: point index, line index) under both
    metrics; the one-shot gf_join_pls gives the same pairs as plan + gf_join_ppoly_run, and a short
    pair buffer gives GF_ERR_CAPACITY with the required count."""
    import torch
    from spatialflink_amd import _lib

    L = _lib.lib()
    g = grid(sf)
    ctx = _lib.context(0)
    x, y, chains, dist = join_case(which, hyp)
    w = win(sf, x, y)
    lines = [sf.LineString(c, g) for c in chains]
    G = PC.Grid()
    for metric in METRICS:
        D = dist(metric, approximate)
        for r in (0.0, LC.SMALL_R, LC.CL, LC.BIG_R):
            exp = LC.ref_join_pls(G, x, y, chains, r, D, approximate)
            assert (len(exp) == 0) == (r == 0.0)
            got = sf.PointLineStringJoinQuery(conf(sf, approximate, metric), g, g).run(w, lines, r)
            np.testing.assert_array_equal(got, exp, err_msg=f"{which} approximate {approximate} metric {metric} r {r!r}")
    r = LC.CL
    exp = LC.ref_join_pls(G, x, y, chains, r, dist(0, approximate), approximate)
    if which == "many":
        assert np.bincount(exp[:, 0]).max() > LC.JOIN_KEEP      # a point with more pairs than the count pass keeps
    ls = sf.LineStringSet(lines)
    cs = ls.c_struct()
    pts = w.c_struct()
    n = C.c_int64()
    gp = C.byref(g.c_grid)
    pairs = torch.empty(2 * len(exp), dtype=torch.int32, device="cuda")
    st = L.gf_join_pls(ctx.handle, gp, gp, C.byref(pts), C.byref(cs), r, int(approximate), 0, pairs.data_ptr(), len(exp),
                       C.byref(n))
    _lib.check(st, ctx.handle, "gf_join_pls")
    assert n.value == len(exp)
    one = pairs.cpu().numpy().view(np.uint32).astype(np.int64).reshape(-1, 2)
    np.testing.assert_array_equal(one[np.lexsort((one[:, 1], one[:, 0]))], exp)
    st = L.gf_join_pls(ctx.handle, gp, gp, C.byref(pts), C.byref(cs), r, int(approximate), 0, pairs.data_ptr(),
                       len(exp) - 1, C.byref(n))
    assert st == _lib.GF_ERR_CAPACITY and n.value == len(exp)
    st = L.gf_join_pls(ctx.handle, gp, gp, C.byref(pts), C.byref(cs), r, int(approximate), 0, None, 0, C.byref(n))
    assert st == _lib.GF_ERR_CAPACITY and n.value == len(exp)


# ---------------------------------------------------------------------------------------------
# argument errors with a context; plans side by side
# ---------------------------------------------------------------------------------------------
def test_argument_errors_and_empty_set(sf):
    """With a real context: a line of one vertex, a bad metric, two lines for kNN and a chain mode on a
    polygon plan are GF_ERR_ARG; an empty set is a valid plan that matches nothing."""
    from spatialflink_amd import _lib

    L = _lib.lib()
    g = grid(sf)
    ctx = _lib.context(0)
    gp = C.byref(g.c_grid)
    h = C.c_void_p()
    vo = np.array([0, 2, 3], np.int32)
    vx = np.array([116.0, 116.1, 116.2])
    vy = np.array([40.0, 40.1, 40.2])
    short = _lib.GfLineStrings(2, vo.ctypes.data, vx.ctypes.data, vy.ctypes.data)
    ok = _lib.GfLineStrings(1, vo.ctypes.data, vx.ctypes.data, vy.ctypes.data)
    vo2 = np.array([0, 2, 4], np.int32)
    vx2 = np.array([116.0, 116.1, 116.2, 116.3])
    two = _lib.GfLineStrings(2, vo2.ctypes.data, vx2.ctypes.data, vx2.ctypes.data)
    E_ = _lib.GF_ERR_ARG
    assert L.gf_range_pls_plan_create(ctx.handle, gp, C.byref(short), 0.1, 0, 0, C.byref(h)) == E_
    assert L.gf_join_pls_plan_create(ctx.handle, gp, C.byref(short), 0.1, 0, 0, C.byref(h)) == E_
    assert L.gf_range_pls_plan_create(ctx.handle, gp, C.byref(ok), 0.1, 0, 2, C.byref(h)) == E_
    assert L.gf_knn_pls_plan_create(ctx.handle, gp, C.byref(two), 0.1, 5, 0, 0, C.byref(h)) == E_
    assert L.gf_knn_pls_plan_create(ctx.handle, gp, C.byref(short), 0.1, 5, 0, 0, C.byref(h)) == E_
    assert h.value is None
    x, y, _, _ = LC.window("two")
    w = win(sf, x, y)
    assert len(sf.PointLineStringRangeQuery(conf(sf), g).run(w, [], LC.CL).indices()) == 0
    assert len(sf.PointLineStringJoinQuery(conf(sf), g, g).run(w, [], LC.CL)) == 0
    poly = sf.PolygonSet([sf.Polygon(PC.raw_polygons("comb")[0], g)])
    pc = poly.c_struct()
    _lib.check(L.gf_range_ppoly_plan_create(ctx.handle, gp, C.byref(pc), 0.1, 0, 0, C.byref(h)), ctx.handle, "plan")
    try:
        assert L.gf_range_plan_set_chain_mode(h, 1) == E_
    finally:
        L.gf_range_plan_destroy(h)
    h = C.c_void_p()
    _lib.check(L.gf_range_pls_plan_create(ctx.handle, gp, C.byref(ok), 0.1, 0, 0, C.byref(h)), ctx.handle, "plan")
    try:
        assert L.gf_range_plan_set_chain_mode(h, 2) == E_
        assert L.gf_range_plan_set_chain_mode(h, 1) == 0 and L.gf_range_plan_set_chain_mode(h, 0) == 0
    finally:
        L.gf_range_plan_destroy(h)


def test_polygon_and_linestring_plans_side_by_side(sf, oracle_mod, hyp):
    """A polygon plan and a linestring plan on one context, run alternately on one window: neither
    disturbs the other, and the polygon result still equals the committed oracle's."""
    g = grid(sf)
    og = oracle_mod.grid(LC.GRID_N, *LC.BEIJING)
    sx, sy, ss = LC.SQUARE
    x, y, _, _ = LC.window("closed_square")
    w = win(sf, x, y)
    ring = LC.lines("closed_square")[0]
    r = 0.3 * LC.CL
    exp_poly = oracle_mod.range_ppoly(og, x, y, oracle_mod.Polygons([[ring]]), r)
    exp_line = expected_range("closed_square", hyp, r, False, 0)
    assert len(exp_poly) > len(exp_line) > 0        # the polygon also holds the square's interior
    pop = sf.PointPolygonRangeQuery(conf(sf), g)
    lop = sf.PointLineStringRangeQuery(conf(sf), g)
    poly, line = [sf.Polygon([ring], g)], sf_lines(sf, "closed_square", g)
    for _ in range(3):
        np.testing.assert_array_equal(pop.run(w, poly, r).indices().astype(np.int64), exp_poly)
        np.testing.assert_array_equal(lop.run(w, line, r).indices().astype(np.int64), exp_line)
