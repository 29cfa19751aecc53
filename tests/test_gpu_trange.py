"""GPU: tRange (gf_trange_points, gf_trange_run) and tFilter (gf_tfilter_run) against the plain-Python
restatement of tests/trange_ref.py.  Everything is exact: keys, offsets, x / y / ts by bits, idx, counts and
the point bitmap.  The polygon catalogue, its probes and windows are tests/poly_cases.py's (a few thousand
to 40k points each); tests/test_trange_ref.py holds the census that keeps them meaningful.

The boundary split compares with the closed-polygon range route.  PointPolygonRangeQuery at radius 0 has no
cells at all (guaranteed layers -1, candidate layers 0: it returns nothing, asserted below), so the route
is taken at poly_cases.TINY, the catalogue's stand-in for `distance <= 0` with one candidate layer."""
import ctypes as C
import functools

import numpy as np
import pytest

import spatialflink_amd as sf
from spatialflink_amd import _lib

import poly_cases as PC
import tjoin_cases as JC
import traj_ref as TR
import trange_cases as TC
import trange_ref as R

pytestmark = pytest.mark.gpu


def grid(case="beijing"):
    n, box = TC.grid_of(case)
    return sf.UniformGrid(n, *box)


def win(x, y, obj, ts):
    return sf.PointWindow.from_numpy(np.ascontiguousarray(x), np.ascontiguousarray(y), np.ascontiguousarray(obj),
                                     np.ascontiguousarray(ts), start=1_000, end=11_000)


def sf_polys(polys, g):
    return [sf.Polygon([list(r) for r in rings], g) for rings in polys]


def csr(s):
    return s.objID, s.off, s.x, s.y, s.ts, s.idx


def ctx0():
    return _lib.context(0)


@functools.lru_cache(maxsize=None)
def contains_of(name):
    """contains_matrix of a named case, computed once and shared (read-only)"""
    x, y, _, _, polys = TC.shape_case(name, "each") if name in PC.NAMES else TC.extra_cases()[name]
    Cm = R.contains_matrix(x, y, polys)
    Cm.setflags(write=False)
    return Cm


def check_window(plan, g, x, y, obj, ts, polys, Cm, G=None, groups=None):
    """gf_trange_points against the closed form, gf_trange_run against the literal reference"""
    w = win(x, y, obj, ts)
    res = plan.points(w)
    exp_pts = R.trange_points(x, y, polys, Cm)
    np.testing.assert_array_equal(res.indices().astype(np.int64), exp_pts)
    assert res.count() == len(exp_pts)
    own = groups is None
    tg = sf.TrajectoryGroups(w) if own else groups.regroup(w)
    try:
        got = tg.trange(g, None, plan=plan)
        R.assert_csr_equal(csr(got), R.trange_literal(G or PC.Grid(), x, y, obj, ts, polys, True, Cm))
        assert got.totals == (len(got.objID), len(got.idx))
    finally:
        if own:
            tg.close()
    return exp_pts, got


@pytest.mark.parametrize("name", PC.NAMES)
def test_shapes_every_objid_assignment(gpu, name):
    g = grid()
    polys = PC.polygons(name)
    plan = sf.TRangePlan(ctx0(), g, sf_polys(polys, g))
    Cm = contains_of(name)
    try:
        for mode in TC.MODES:
            x, y, obj, ts, _ = TC.shape_case(name, mode)
            exp_pts, _ = check_window(plan, g, x, y, obj, ts, polys, Cm)
        # the probes poly_cases appends last: NaN x, NaN y, both, outside the grid -- never contained
        pidx = PC.window(name)[3]
        assert not np.isin(pidx[-4:], exp_pts).any()
    finally:
        plan.close()


def _run_with_wide(name, wide_ring, mode="mod"):
    g = grid()
    polys = PC.polygons(name)
    plan = sf.TRangePlan(ctx0(), g, sf_polys(polys, g))
    try:
        plan.set_thresholds(wide_ring)
        x, y, obj, ts, _ = TC.shape_case(name, mode)
        w = win(x, y, obj, ts)
        pts = plan.points(w)
        tg = sf.TrajectoryGroups(w)
        try:
            got = tg.trange(g, None, plan=plan)
        finally:
            tg.close()
        return dict(plan.stats(), **plan.info()), pts.indices().astype(np.int64), pts.count(), csr(got)
    finally:
        plan.close()


def test_ngon_wave_path_equals_lane_path(gpu):
    st_w, pw, cw, tw = _run_with_wide("ngon", 4)
    st_l, pl, cl, tl = _run_with_wide("ngon", 1002)
    assert st_w["wide_polygons"] > 0 and st_l["wide_polygons"] == 0
    assert st_w["wave_path"] == 1 and st_l["wave_path"] == 0 and (st_w["wide_ring"], st_l["wide_ring"]) == (4, 1002)
    np.testing.assert_array_equal(pw, pl)
    assert cw == cl
    R.assert_csr_equal(tw, tl)
    x, y, obj, ts, polys = TC.shape_case("ngon", "mod")
    np.testing.assert_array_equal(pw, R.trange_points(x, y, polys, contains_of("ngon")))
    R.assert_csr_equal(tw, R.trange_closed(x, y, obj, ts, polys, contains_of("ngon")))
    # one objID per point: every worklist entry decides a row alone
    _, pe, _, te = _run_with_wide("ngon", 4, "each")
    x, y, obj, ts, polys = TC.shape_case("ngon", "each")
    np.testing.assert_array_equal(pe, pw)
    R.assert_csr_equal(te, R.trange_closed(x, y, obj, ts, polys, contains_of("ngon")))


@pytest.mark.parametrize("name", ["near_rects", "holed", "collinear_tiled"])
def test_every_polygon_on_the_wave_path(gpu, name):
    st, p, c, t = _run_with_wide(name, 4, "each")
    assert st["wide_polygons"] == len(PC.polygons(name))
    x, y, obj, ts, polys = TC.shape_case(name, "each")
    np.testing.assert_array_equal(p, R.trange_points(x, y, polys, contains_of(name)))
    assert c == len(p)
    R.assert_csr_equal(t, R.trange_closed(x, y, obj, ts, polys, contains_of(name)))


def test_inside_cells(gpu):
    g = grid()
    x, y, obj, ts, polys = TC.inside_case()
    plan = sf.TRangePlan(ctx0(), g, sf_polys(polys, g))
    try:
        st = plan.stats()
        assert st["inside_cells"] >= 15 + 1  # 5 x 3 cells of the rectangle, cell (0, 0) of the other
        exp_pts, _ = check_window(plan, g, x, y, obj, ts, polys, contains_of("inside"))
        info = plan.info()
        cx, cy = PC.Grid().cells(x, y)
        in_r = (cx >= 21) & (cx <= 25) & (cy >= 31) & (cy <= 33)
        in_z = (cx == 0) & (cy == 0) & (x == x) & (y == y)
        assert info["inside_points"] == int((in_r | in_z).sum()) and info["inside_points"] > 500
        assert info["cell_points"] == int(R.cell_filter(PC.Grid(), x, y, polys).sum())
        assert not np.isin(np.flatnonzero(~(x == x) | ~(y == y)), exp_pts).any()  # the NaN points of cell (0, 0)
    finally:
        plan.close()


def test_grid_edges(gpu):
    g = grid()
    x, y, obj, ts, polys = TC.grid_edge_case()
    plan = sf.TRangePlan(ctx0(), g, sf_polys(polys, g))
    try:
        exp_pts, _ = check_window(plan, g, x, y, obj, ts, polys, contains_of("grid_edge"))
        cx, cy = PC.Grid().cells(x, y)
        out = ~PC.Grid().valid(cx, cy)
        assert out[exp_pts].sum() >= 40 and (~out[exp_pts]).sum() >= 40
        # the wave path over the polygons that leave the grid
        plan.set_thresholds(4)
        assert plan.stats()["wide_polygons"] == 3
        check_window(plan, g, x, y, obj, ts, polys, contains_of("grid_edge"))
    finally:
        plan.close()


def test_hand_vector(gpu):
    g = grid("hand")
    x, y, obj, ts, polys = TC.hand_case()
    plan = sf.TRangePlan(ctx0(), g, sf_polys(polys, g))
    try:
        exp_pts, got = check_window(plan, g, x, y, obj, ts, polys, R.contains_matrix(x, y, polys), G=PC.Grid(*TC.HAND_GRID))
        assert exp_pts.tolist() == TC.HAND_EXPECT["points"]
        assert got.objID.tolist() == TC.HAND_EXPECT["keys"] and got.idx.tolist() == TC.HAND_EXPECT["idx"]
    finally:
        plan.close()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 257])
def test_wave_and_block_boundaries(gpu, n):
    g = grid()
    polys = PC.polygons("holed")
    minx, maxx, miny, maxy = PC.extent("holed")
    rng = np.random.default_rng(n)
    plan = sf.TRangePlan(ctx0(), g, sf_polys(polys, g))
    try:
        x, y = rng.uniform(minx - PC.CL, maxx + PC.CL, n), rng.uniform(miny - PC.CL, maxy + PC.CL, n)
        obj, ts = (np.arange(n) % 5).astype(np.int64), TC.ts_of(n)
        check_window(plan, g, x, y, obj, ts, polys, R.contains_matrix(x, y, polys))
        # a window whose only contained point is its last: a fixed point interior to the shell and outside
        # the holes (the reference says so below), every other point left of the shape
        cand_x, cand_y = np.linspace(minx, maxx, 41)[1:-1], np.linspace(miny, maxy, 41)[1:-1]
        gx, gy = (v.ravel() for v in np.meshgrid(cand_x, cand_y))
        k = int(np.flatnonzero(R.polygon_contains(gx, gy, polys[0]))[0])  # the catalogue's shape has interior lattice points
        x2 = np.full(n, minx - 3 * PC.CL)
        y2 = np.full(n, miny)
        x2[-1], y2[-1] = gx[k], gy[k]
        exp_pts, got = check_window(plan, g, x2, y2, np.zeros(n, np.int64), ts, polys, R.contains_matrix(x2, y2, polys))
        assert exp_pts.tolist() == [n - 1] and len(got.idx) == n and got.objID.tolist() == [0]
    finally:
        plan.close()


def test_early_exit_changes_no_result(gpu):
    g = grid()
    polys = PC.polygons("star")
    minx, maxx, miny, maxy = PC.extent("star")
    rng = np.random.default_rng(3)
    m = 20_000
    # rejection-sample m points inside the star (reference verdicts), m others around it
    cx, cy = rng.uniform(minx, maxx, 8 * m), rng.uniform(miny, maxy, 8 * m)
    inner = np.flatnonzero(R.polygon_contains(cx, cy, polys[0]))[:m]
    assert len(inner) == m
    ox, oy = rng.uniform(minx - 5 * PC.CL, maxx + 5 * PC.CL, m), rng.uniform(miny - 5 * PC.CL, maxy + 5 * PC.CL, m)
    x, y = np.concatenate([cx[inner], ox]), np.concatenate([cy[inner], oy])
    perm = rng.permutation(2 * m)
    hot = np.concatenate([np.ones(m, bool), np.zeros(m, bool)])[perm]
    x, y = x[perm], y[perm]
    others = 10_000_000 + np.arange(2 * m, dtype=np.int64)
    obj_hot = np.where(hot, 7, others)
    obj_each = np.where(hot, 1_000 + np.arange(2 * m), others)
    ts = TC.ts_of(2 * m)
    plan = sf.TRangePlan(ctx0(), g, sf_polys(polys, g))
    try:
        def run(obj):
            w = win(x, y, obj, ts)
            tg = sf.TrajectoryGroups(w)
            try:
                return csr(tg.trange(g, None, plan=plan)), plan.info()
            finally:
                tg.close()
        (a, ia), (b, ib), (c, ic) = run(obj_hot), run(obj_hot), run(obj_each)
        R.assert_csr_equal(a, b)
        assert ia == ib == ic  # the counters do not depend on the flags
        Cm = R.contains_matrix(x, y, polys)
        R.assert_csr_equal(a, R.trange_closed(x, y, obj_hot, ts, polys, Cm))
        R.assert_csr_equal(c, R.trange_closed(x, y, obj_each, ts, polys, Cm))
        # restricted to the shared rows (the other objIDs): the same trajectories either way
        ka, kc = a[0][a[0] >= 10_000_000], c[0][c[0] >= 10_000_000]
        np.testing.assert_array_equal(ka, kc)
        assert 7 in a[0] and (a[1][1:] - a[1][:-1]).max() == m
    finally:
        plan.close()


def test_empty_cases_and_capacities(gpu):
    g = grid()
    x, y, obj, ts, polys = TC.shape_case("comb", "mod")
    w = win(x, y, obj, ts)
    tg = sf.TrajectoryGroups(w)
    try:
        empty = sf.TRangePlan(ctx0(), g, [])
        assert empty.stats()["test_cells"] == 0
        assert len(tg.trange(g, None, plan=empty)) == 0 and empty.points(w).count() == 0
        assert len(empty.points(w).indices()) == 0
        far = sf.TRangePlan(ctx0(), g, sf_polys([[[(10.0, 10.0), (11.0, 10.0), (11.0, 11.0), (10.0, 10.0)]]], g))
        got = tg.trange(g, None, plan=far)
        assert len(got) == 0 and len(got.idx) == 0 and got.off.tolist() == [0] and far.points(w).count() == 0
        plan = sf.TRangePlan(ctx0(), g, sf_polys(polys, g))
        full = tg.trange(g, None, plan=plan)
        assert len(full) > 10
        cut = tg.trange(g, None, plan=plan, cap_traj=3, cap_pts=5)
        assert cut.totals == (len(full), len(full.idx))
        np.testing.assert_array_equal(cut.objID, full.objID[:3])
        np.testing.assert_array_equal(cut.off, full.off[:4])
        np.testing.assert_array_equal(cut.idx, full.idx[:5])
        np.testing.assert_array_equal(cut.x.view(np.uint64), full.x[:5].view(np.uint64))
        # an empty window
        w0 = win(np.empty(0), np.empty(0), np.empty(0, np.int64), np.empty(0, np.int64))
        t0 = sf.TrajectoryGroups(w0)
        assert len(t0.trange(g, None, plan=plan)) == 0 and plan.points(w0).count() == 0 and len(t0.tfilter([])) == 0
        t0.close()
        for p in (empty, far, plan):
            p.close()
    finally:
        tg.close()


def test_plan_and_groups_reused_across_windows(gpu):
    g = grid()
    names = ("holed", "comb", "star")
    polys = [p for nme in names for p in PC.polygons(nme)]
    plan = sf.TRangePlan(ctx0(), g, sf_polys(polys, g))
    tg = None
    try:
        for nme, mode in zip(names, ("mod", "each", "one")):
            x, y, obj, ts, _ = TC.shape_case(nme, mode)
            Cm = R.contains_matrix(x, y, polys)
            w = win(x, y, obj, ts)
            tg = sf.TrajectoryGroups(w) if tg is None else tg
            _, reused = check_window(plan, g, x, y, obj, ts, polys, Cm, groups=tg)
            fresh_plan = sf.TRangePlan(ctx0(), g, sf_polys(polys, g))
            fresh_tg = sf.TrajectoryGroups(w)
            try:
                R.assert_csr_equal(csr(reused), csr(fresh_tg.trange(g, None, plan=fresh_plan)))
            finally:
                fresh_tg.close()
                fresh_plan.close()
    finally:
        if tg is not None:
            tg.close()
        plan.close()


def test_boundary_split_against_the_closed_polygon_route(gpu):
    """The closed-polygon range route (distance <= 0) = the contained points + exactly the boundary-only
    points: the difference this operator exists for."""
    g = grid()
    x, y, obj, ts, polys = TC.shape_case("comb", "each")
    w = win(x, y, obj, ts)
    sp = sf_polys(polys, g)
    op = sf.PointPolygonRangeQuery(sf.QueryConfiguration(sf.QueryType.WindowBased), g)
    assert len(op.run(w, sp, 0.0).indices()) == 0  # radius 0: no candidate cells at all
    closed = op.run(w, sp, PC.TINY).indices().astype(np.int64)
    plan = sf.TRangePlan(ctx0(), g, sp)
    try:
        inner = plan.points(w).indices().astype(np.int64)
    finally:
        plan.close()
    bnd = np.zeros(len(x), bool)
    for rings in polys:
        bnd |= R.on_boundary(x, y, rings)
    bnd_only = np.flatnonzero(bnd & ~contains_of("comb").any(axis=0))
    print(f"comb: closed route {len(closed)}, contained {len(inner)}, boundary-only {len(bnd_only)}")
    assert len(bnd_only) >= 50 and len(inner) >= 50
    assert not np.isin(bnd_only, inner).any()
    np.testing.assert_array_equal(closed, np.union1d(inner, bnd_only))
    # the operator classes end to end: RealTime = the contained points, WindowBased = their trajectories
    rt = sf.PointPolygonTRangeQuery(sf.QueryConfiguration(sf.QueryType.RealTime), g).run(w, sp)
    np.testing.assert_array_equal(rt.indices().astype(np.int64), inner)
    q = sf.PointPolygonTRangeQuery(sf.QueryConfiguration(sf.QueryType.WindowBased), g)
    wb = q.run(w, sp)
    np.testing.assert_array_equal(wb.idx.astype(np.int64), inner)  # one objID per point
    assert len(q._plans) == 1 and len(q.run(w, sf_polys(polys, g))) == len(wb) and len(q._plans) == 1  # cached by digest


@pytest.mark.parametrize("seed", [1, 2])
def test_traj_select_bytes_unchanged(gpu, seed):
    """gf_traj_select (whose tail is now shared) against a NumPy restatement, with a random bitmap"""
    import torch

    x, y, obj, ts = JC.walks(seed, 30_001, 2_000, JC.BEIJING, 0.002)
    w = JC.device_window((x, y, obj, ts))
    rng = np.random.default_rng(seed)
    hit = rng.random(len(x)) < 0.0007
    words = np.zeros((len(x) + 63) // 64, np.uint64)
    np.bitwise_or.at(words, np.flatnonzero(hit) >> 6, np.uint64(1) << (np.flatnonzero(hit) & 63).astype(np.uint64))
    bitmap = torch.as_tensor(words.view(np.int64)).cuda()
    tg = sf.TrajectoryGroups(w)
    try:
        got = tg.select(bitmap)
        keys, off, perm = TR.group_ref(obj)
        exp = TR.subtraj_ref(x, y, ts, keys, off, perm, hit)
        assert 0 < len(exp[0]) < len(keys)
        R.assert_csr_equal(csr(got), exp)
    finally:
        tg.close()


def test_tfilter(gpu):
    x, y, obj, ts = JC.walks(5, 20_003, 1_500, JC.BEIJING, 0.002)  # numeric, dictionary and the null key
    w = JC.device_window((x, y, obj, ts))
    keys = TR.group_ref(obj)[0]
    rng = np.random.default_rng(9)
    pick = rng.choice(keys, 200, replace=False)
    sets = {
        "some": pick.tolist(),
        "absent": pick[:50].tolist() + [123_456_789_012, -(1 << 63) + 999_999_999, (1 << 62) - 1],
        "duplicates": pick[:80].tolist() * 3,
        "empty": [],
        "null": [_lib.OBJID_NULL, int(keys[0])],
        "only_absent": [987_654_321_987],
    }
    assert JC.NULL_KEY in keys.tolist() and (keys < _lib.OBJID_NUMERIC_MIN).any()
    tg = sf.TrajectoryGroups(w)
    try:
        for name, ids in sets.items():
            got = tg.tfilter(ids)
            exp = R.tfilter_ref(x, y, obj, ts, ids)
            R.assert_csr_equal(csr(got), exp)
            if name == "empty":
                assert len(got) == len(keys) and len(got.idx) == len(x)
            if name == "only_absent":
                assert len(got) == 0
        cut = tg.tfilter(sets["some"], cap_traj=7, cap_pts=9)
        full = tg.tfilter(sets["some"])
        assert cut.totals == (len(full), len(full.idx)) and cut.idx.tolist() == full.idx[:9].tolist()
    finally:
        tg.close()


def test_tfilter_query_with_dictionary_strings(gpu):
    g = grid()
    names = ["bus-7", "12", "taxi:3", "bus-7", "12", "tram A", "taxi:3", "bus-7", None, "012"]
    pts = [sf.Point(nm, 116.0 + 0.01 * i, 40.0 + 0.005 * i, 1_000 + i, g) for i, nm in enumerate(names)]
    w = sf.PointWindow.from_points(pts)
    q = sf.PointTFilterQuery(sf.QueryConfiguration(sf.QueryType.WindowBased))
    got = q.run(w, ["taxi:3", "12", "never seen", "bus-7"])
    assert got.objid_strings() == ["bus-7", "12", "taxi:3"]
    assert got.off.tolist() == [0, 3, 5, 7] and got.idx.tolist() == [0, 3, 7, 1, 4, 2, 6]
    assert len(q.run(w, ["never seen"])) == 0
    assert len(q.run(w, [])) == 6 and len(q.run(w, []).idx) == len(names)
    assert q.run(w, [None]).idx.tolist() == [8]
    tg = sf.TrajectoryGroups(w)
    try:
        assert q.run(w, ["012"], groups=tg).idx.tolist() == [9]
    finally:
        tg.close()


def test_bad_arguments_with_a_live_context(gpu):
    """Every refusal is GF_ERR_ARG before any device work, with the context, plan and groups all valid."""
    L = _lib.lib()
    g = grid()
    ctx = ctx0()
    h = C.c_void_p()
    neg = _lib.GfPolygons(-1, None, None, None, None)
    assert L.gf_trange_plan_create(ctx.handle, C.byref(g.c_grid), C.byref(neg), C.byref(h)) == _lib.GF_ERR_ARG
    assert L.gf_trange_plan_create(ctx.handle, C.byref(g.c_grid), None, C.byref(h)) == _lib.GF_ERR_ARG
    assert L.gf_trange_plan_create(ctx.handle, None, C.byref(neg), C.byref(h)) == _lib.GF_ERR_ARG
    assert h.value is None
    open_ring = sf.PolygonSet(sf_polys(PC.polygons("star"), g))
    open_ring.vx = open_ring.vx.copy()
    open_ring.vx[0] += 1.0  # the shell no longer closes
    cs = open_ring.c_struct()
    assert L.gf_trange_plan_create(ctx.handle, C.byref(g.c_grid), C.byref(cs), C.byref(h)) == _lib.GF_ERR_ARG and h.value is None
    x, y, obj, ts, polys = TC.shape_case("star", "mod")
    w = win(x, y, obj, ts)
    w_short = win(x[:100], y[:100], obj[:100], ts[:100])
    plan = sf.TRangePlan(ctx, g, sf_polys(polys, g))
    tg = sf.TrajectoryGroups(w)
    other = _lib.Context(0)
    other_plan = sf.TRangePlan(other, g, sf_polys(polys, g))
    try:
        assert L.gf_trange_plan_set_thresholds(plan.handle, -1) == _lib.GF_ERR_ARG
        m, q = C.c_int64(), C.c_int64()
        pts, short = w.c_struct(), w_short.c_struct()
        run = lambda p, t, ps, ct, cp, a=C.byref(m), b=C.byref(q): L.gf_trange_run(  # noqa: E731
            p, t, ps, None, None, ct, None, None, None, None, cp, a, b)
        assert run(plan.handle, tg.handle, C.byref(pts), 0, 0) == _lib.GF_OK and m.value > 0  # counting only
        assert run(plan.handle, tg.handle, C.byref(pts), -1, 0) == _lib.GF_ERR_ARG
        assert run(plan.handle, tg.handle, C.byref(pts), 0, -1) == _lib.GF_ERR_ARG
        assert run(plan.handle, tg.handle, C.byref(pts), 0, 0, None) == _lib.GF_ERR_ARG
        assert run(plan.handle, tg.handle, C.byref(pts), 0, 0, C.byref(m), None) == _lib.GF_ERR_ARG
        assert run(plan.handle, tg.handle, None, 0, 0) == _lib.GF_ERR_ARG
        assert run(plan.handle, tg.handle, C.byref(short), 0, 0) == _lib.GF_ERR_ARG          # not the grouped window
        assert run(other_plan.handle, tg.handle, C.byref(pts), 0, 0) == _lib.GF_ERR_ARG       # another context's plan
        assert run(plan.handle, None, C.byref(pts), 0, 0) == _lib.GF_ERR_ARG
        no_xy = _lib.GfPoints(None, None, pts.objID, pts.ts, pts.n)
        assert L.gf_trange_points(plan.handle, C.byref(no_xy), None, None) == _lib.GF_ERR_ARG
        assert L.gf_trange_points(plan.handle, C.byref(pts), None, None) == _lib.GF_ERR_ARG    # no bitmap
        assert L.gf_trange_points(plan.handle, None, None, None) == _lib.GF_ERR_ARG
        flt = lambda ps, ids, ns, ct, cp: L.gf_tfilter_run(tg.handle, ps, ids, ns, None, None, ct, None, None, None, None,  # noqa: E731
                                                           cp, C.byref(m), C.byref(q))
        assert flt(C.byref(pts), None, 0, 0, 0) == _lib.GF_OK and m.value == tg.ntraj
        assert flt(C.byref(pts), None, 3, 0, 0) == _lib.GF_ERR_ARG
        assert flt(C.byref(pts), None, -1, 0, 0) == _lib.GF_ERR_ARG
        assert flt(C.byref(pts), None, 0, -1, 0) == _lib.GF_ERR_ARG
        assert flt(C.byref(pts), None, 0, 0, -1) == _lib.GF_ERR_ARG
        assert flt(C.byref(short), None, 0, 0, 0) == _lib.GF_ERR_ARG
        # the objects still work after the refusals
        R.assert_csr_equal(csr(tg.trange(g, None, plan=plan)), R.trange_closed(x, y, obj, ts, polys))
    finally:
        tg.close()
        plan.close()
        other_plan.close()
