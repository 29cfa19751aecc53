"""GPU parity at the numeric edges: every operator, through the product API, on the grid catalogue
of tests/edge_cases.py -- negative coordinates, grids straddling 0, exact binary cell lengths, a
large origin offset, cells 5 doubles and half a double wide, both sides of the division-free switch
(n = 2048 / 2049) -- with window points on and around every cell edge and radii that are realized
distances (points exactly at r) and their lower neighbours.  Every comparison is exact; expected
values come from the C oracle, which tests/test_numeric_edges.py ties to an independent numpy /
rational reference on exactly these cases."""
import ctypes as C

import numpy as np
import pytest

import edge_cases as E

pytestmark = pytest.mark.gpu
GRID_NAMES = list(E.GRIDS)
_memo = {}


def memo(key, fn):
    """Oracle expectations computed once and shared by the parametrized variants."""
    if key not in _memo:
        _memo[key] = fn()
    return _memo[key]


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


def grids(sf, oracle_mod, name):
    return sf.UniformGrid(*E.GRIDS[name]), oracle_mod.grid(*E.GRIDS[name])


def dev_window(sf, name, second=False):
    def make():
        x, y, obj = E.second_window(name) if second else E.window(name)
        return x, y, obj, sf.PointWindow.from_numpy(np.array(x), np.array(y), np.array(obj))
    return memo(("win", name, second), make)


def conf(sf, approximate=False, metric=0):
    c = sf.QueryConfiguration(sf.QueryType.WindowBased)
    c.setApproximateQuery(approximate)
    c.distanceMetric = metric
    return c


def u32(t):
    return t.cpu().numpy().view(np.uint32).astype(np.int64)


# ------------------------------------------------------------------ K1 / K2 / sharding
@pytest.mark.parametrize("name", GRID_NAMES)
def test_cells_bucket_shard(sf, oracle_mod, name):
    """assign_cells, the exact stable bucket permutation with its cell starts, and the column-band
    router with 3 bands whose starts sit on tested edges (the query corner's column among them)."""
    from spatialflink_amd import sharding

    g, og = grids(sf, oracle_mod, name)
    n = E.GRIDS[name][0]
    x, y, _, w = dev_window(sf, name)
    ocx, ocy = oracle_mod.assign_cells(og, x, y)
    cx, cy = sf.assign_cells(w, g)
    np.testing.assert_array_equal(cx.cpu().numpy(), ocx)
    np.testing.assert_array_equal(cy.cpu().numpy(), ocy)
    # keyBy(gridID): bucket = valid cell cy*n + cx, out-of-grid last, arrival order inside a bucket
    c64x, c64y = ocx.astype(np.int64), ocy.astype(np.int64)
    valid = (c64x >= 0) & (c64y >= 0) & (c64x < n) & (c64y < n)
    key = np.where(valid, c64y * n + c64x, n * n)
    eperm = np.argsort(key, kind="stable")
    estart = np.searchsorted(key[eperm], np.arange(n * n + 2), side="left")
    perm, start = sf.bucket_by_cell(w, g)
    np.testing.assert_array_equal(u32(perm), eperm)
    np.testing.assert_array_equal(u32(start), estart)
    cols = np.sort(c64x[valid])   # band starts at the terciles of the occupied columns (subulp: the first 660)
    a, b = int(cols[len(cols) // 3]), int(cols[2 * len(cols) // 3])
    assert 0 < a < b < n
    bands = [(0, a), (a, b), (b, n)]
    sperm, soff = sharding.shard_window(w, g, bands)
    eperm, eoff = sharding.shard_order(ocx, bands)
    np.testing.assert_array_equal(soff, eoff)
    np.testing.assert_array_equal(u32(sperm), eperm)
    assert (np.diff(eoff) > 0).all()   # every band holds points


# ------------------------------------------------------------------ range, point queries
@pytest.mark.parametrize("defer", [1, 2, 3])
@pytest.mark.parametrize("name", GRID_NAMES)
def test_range_pp(sf, oracle_mod, hyp, name, defer):
    """One query point (arithmetic path) and three (table path) -- on a cell corner, at a cell
    centre, in the grid's last cell --, exact and approximate, both metrics, every defer mode, at
    realized radii, their lower neighbours, the radii where the layer counts change and r = 0."""
    g, og = grids(sf, oracle_mod, name)
    x, y, _, w = dev_window(sf, name)
    ops = {}
    for ap in (False, True):
        for metric in (0, 1):
            ops[ap, metric] = sf.PointPointRangeQuery(conf(sf, ap, metric), g)
            ops[ap, metric].tuning = (0, defer)
    hits = 0
    for tag, qx, qy, r, metric in E.range_cases(name, hyp):
        qs = [sf.Point(str(i), a, b, 0, g) for i, (a, b) in enumerate(zip(qx, qy))]
        for ap in (False, True):
            exp = memo(("range", name, tag, r, metric if not ap else 0, ap),
                       lambda: oracle_mod.range_pp(og, x, y, qx, qy, r, ap, 0 if ap else metric))
            res = ops[ap, metric].run(w, qs, r)
            msg = f"{name} {tag} r={r!r} metric {metric} approximate {ap} defer {defer}"
            np.testing.assert_array_equal(res.indices().astype(np.int64), np.unique(exp), err_msg=msg)
            assert res.count() == len(np.unique(exp)), msg
            if ap and len(qx) > 1:
                np.testing.assert_array_equal(res.multiset_indices(), exp, err_msg=msg)
                assert res.multiset_size() == len(exp), msg
            hits += len(exp)
    assert hits > 0


# ------------------------------------------------------------------ range and join, polygons
def polygon_cases(name):
    """(polygons, radii): an axis-aligned rectangle whose sides lie on cell edges and a triangle with
    a vertex on a cell corner (lattice vertices on the lattice grids)."""
    n, x0, _, y0, _ = E.GRIDS[name]
    cl = E.cell_length(name)
    if name in E.LATTICE:
        u = E.U
        # subulp: 2 cells per U -- smaller shapes and radii keep the oracle's per-cell sets small
        w, h, t, big = (15, 10, 3, [25 * u]) if name == "ulp5" else (3, 2, 1, [])
        rect = [(x0 + 100 * u, y0 + 150 * u), (x0 + (100 + w) * u, y0 + 150 * u), (x0 + (100 + w) * u, y0 + (150 + h) * u),
                (x0 + 100 * u, y0 + (150 + h) * u), (x0 + 100 * u, y0 + 150 * u)]
        tri = [(x0 + 200 * u, y0 + 50 * u), (x0 + (200 + 10 * t) * u, y0 + (50 + 2 * t) * u),
               (x0 + (200 + 4 * t) * u, y0 + (50 + 11 * t) * u), (x0 + 200 * u, y0 + 50 * u)]
        radii = [0.0, 5 * u, E.toward0(5 * u)] + big
    else:
        a0, a1, b0, b1 = n // 3, n // 3 + 2, n // 2, n // 2 + 1
        ex = lambda c: x0 + c * cl  # noqa: E731
        ey = lambda c: y0 + c * cl  # noqa: E731
        rect = [(ex(a0), ey(b0)), (ex(a1), ey(b0)), (ex(a1), ey(b1)), (ex(a0), ey(b1)), (ex(a0), ey(b0))]
        vx, vy = ex(a1 + 1), ey(b0 - 2)
        tri = [(vx, vy), (vx + 1.7 * cl, vy + 0.4 * cl), (vx + 0.6 * cl, vy + 1.9 * cl), (vx, vy)]
        radii = [0.0, 0.3 * cl, E.prev(cl), cl, E.nxt(cl), 1.5 * cl]
    return [[rect], [tri]], radii


@pytest.mark.parametrize("name", GRID_NAMES)
def test_range_and_join_ppoly(sf, oracle_mod, name):
    """Point-polygon range and join: a rectangle on cell edges (cells inside it are accepted
    untested) and a triangle (every pair takes the exact distance), exact and approximate, both
    metrics, r = 0, around r = cl where the layer counts change, and on the lattice at 5 U -- points
    exactly at r from a side -- and its lower neighbour."""
    g, og = grids(sf, oracle_mod, name)
    x, y, _, w = dev_window(sf, name)
    raw, radii = polygon_cases(name)
    polys = [sf.Polygon(p, g) for p in raw]
    OP = oracle_mod.Polygons(raw)
    hits = 0
    for ap in (False, True):
        for metric in (0, 1):
            rop = sf.PointPolygonRangeQuery(conf(sf, ap, metric), g)
            jop = sf.PointPolygonJoinQuery(conf(sf, ap, metric), g, g)
            for r in radii:
                msg = f"{name} r={r!r} metric {metric} approximate {ap}"
                exp = oracle_mod.range_ppoly(og, x, y, OP, r, ap, metric)
                res = rop.run(w, polys, r)
                np.testing.assert_array_equal(res.indices().astype(np.int64), exp, err_msg=msg)
                assert res.count() == len(exp), msg
                pexp = E.sorted_pairs(oracle_mod.join_ppoly(og, og, x, y, OP, r, ap, metric))
                np.testing.assert_array_equal(jop.run(w, polys, r), pexp, err_msg="join " + msg)
                hits += len(exp) + len(pexp)
    assert hits > 0


# ------------------------------------------------------------------ kNN, point queries
def check_knn(res, exp, msg):
    st, oo, od, oi = exp
    assert st == 0
    np.testing.assert_array_equal(res.objID, oo, err_msg=msg)
    np.testing.assert_array_equal(res.idx, oi, err_msg=msg)
    np.testing.assert_array_equal(res.dist.view(np.uint64), od.view(np.uint64), err_msg=msg)


@pytest.mark.parametrize("depth", [1, 2])
@pytest.mark.parametrize("name", GRID_NAMES)
def test_knn_pp(sf, oracle_mod, hyp, name, depth):
    """k in {1, 7, 50} (the lattice: also k = 20, which ends inside a pair of tied distances), both
    metrics, r at realized distances and their lower neighbours, two consecutive windows with the
    threshold hint on and off, pipeline depth 1 (synchronous) and 2 (records enqueued back to back)."""
    import torch

    from spatialflink_amd import _lib

    g, og = grids(sf, oracle_mod, name)
    wins = [dev_window(sf, name), dev_window(sf, name, True)]
    ops = {m: sf.PointPointKNNQuery(conf(sf, False, m), g) for m in (0, 1)}
    found = 0
    for qx, qy, r, metric, k in E.knn_cases(name, hyp):
        q = sf.Point("q", qx, qy, 0, g)
        op = ops[metric]
        exps = [memo(("knn", name, j, qx, qy, r, metric, k),
                     lambda j=j: oracle_mod.knn(og, wins[j][0], wins[j][1], wins[j][2], qx, qy, r, k, metric))
                for j in (0, 1)]
        found += len(exps[0][1])
        ctx, plan = op.plan(0, q, r, k)
        for hint in (1, 0):
            msg = f"{name} q=({qx!r}, {qy!r}) r={r!r} metric {metric} k={k} hint {hint} depth {depth}"
            _lib.check(_lib.lib().gf_knn_plan_set_hint(plan, hint), ctx.handle, "hint")
            order = [0, 1, 1, 0]
            if depth == 1:
                for j in order:
                    check_knn(op.run(wins[j][3], q, r, k), exps[j], msg)
            else:
                op.set_pipeline(0, q, r, k, 2)
                rec = sf.PinnedRecords(len(order), k)
                for i, j in enumerate(order):
                    op.enqueue(wins[j][3], q, r, k, rec.ptr(i))
                op.flush(0, q, r, k)
                torch.cuda.synchronize()
                for i, j in enumerate(order):
                    check_knn(op.finish(wins[j][3], q, r, k, rec.raw(i)), exps[j], msg)
                op.set_pipeline(0, q, r, k, 1)
    assert found > 0


def test_knn_forced_fallback_on_lattice(sf, oracle_mod):
    """A candidate buffer far smaller than the 13,273 points within r = 65 U of ulp5: the exact
    partitioned fallback, among thousands of exactly tied distances."""
    name = "ulp5"
    g, og = grids(sf, oracle_mod, name)
    x, y, obj, w = dev_window(sf, name)
    qx, qy = E.queries(name)[0]
    q = sf.Point("q", qx, qy, 0, g)
    for metric in (0, 1):
        for r in (65 * E.U, E.toward0(65 * E.U)):
            for k in (20, 50):
                op = sf.PointPointKNNQuery(conf(sf, False, metric), g)
                op.set_capacity(0, q, r, k, 1024)
                check_knn(op.run(w, q, r, k), oracle_mod.knn(og, x, y, obj, qx, qy, r, k, metric),
                          f"r={r!r} metric {metric} k={k}")


# ------------------------------------------------------------------ join, point-point
@pytest.mark.parametrize("name", GRID_NAMES)
def test_join_pp(sf, oracle_mod, hyp, name):
    """200 query points taken from the window itself (the catalogue queries, NaN / inf / 1e300, an
    even sample): the default path, the legacy probe, the cell (coarse) variant and the streaming
    variant, both metrics, and the async entry once per grid; pair sets compared after sorting."""
    import torch

    from spatialflink_amd import _lib

    L = _lib.lib()
    g, og = grids(sf, oracle_mod, name)
    x, y, _, w = dev_window(sf, name)
    qi = E.join_query_side(name)
    qx, qy = x[qi], y[qi]
    wq = sf.PointWindow.from_numpy(np.array(qx), np.array(qy), None)
    ctx = _lib.context(0)
    flags = (_lib.FLAG_JOIN_LEGACY, _lib.FLAG_JOIN_COARSE, _lib.FLAG_JOIN_STREAM)
    cases = E.join_cases(name, hyp)
    total = 0
    for r, metric in cases:
        st, pairs = oracle_mod.join_pp(og, og, x, y, qx, qy, r, False, metric)
        assert st == 0
        exp = E.sorted_pairs(pairs)
        total += len(exp)
        for flag in (0,) + flags:
            try:
                if flag:
                    _lib.check(L.gf_ctx_set_flag(ctx.handle, flag, 1), ctx.handle, "flag")
                got = sf.PointPointJoinQuery(conf(sf, False, metric), g, g).run(w, wq, r)
            finally:
                for f in flags:
                    L.gf_ctx_set_flag(ctx.handle, f, 0)
            np.testing.assert_array_equal(got, exp, err_msg=f"{name} r={r!r} metric {metric} flag {flag}")
    assert total > 0
    # approximate: every co-located pair
    r = cases[0][0]
    st, pairs = oracle_mod.join_pp(og, og, x, y, qx, qy, r, True, 0)
    np.testing.assert_array_equal(sf.PointPointJoinQuery(conf(sf, True, 0), g, g).run(w, wq, r), E.sorted_pairs(pairs))
    # the async entry: the same pairs, the count in device memory
    r, metric = next((c for c in cases if c[0] > 0 and c[1] == 1))
    st, pairs = oracle_mod.join_pp(og, og, x, y, qx, qy, r, False, metric)
    exp = E.sorted_pairs(pairs)
    cap = len(exp) + 16
    buf = torch.zeros(2 * cap, dtype=torch.int32, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    po, pq = w.c_struct(), wq.c_struct()
    _lib.check(L.gf_join_pp_async(ctx.handle, C.byref(g.c_grid), C.byref(g.c_grid), C.byref(po), C.byref(pq), r, 0, metric,
                                  buf.data_ptr(), cap, cnt.data_ptr()), ctx.handle, "gf_join_pp_async")
    ctx.synchronize()
    m = int(cnt.item())
    assert m == len(exp)
    np.testing.assert_array_equal(E.sorted_pairs(u32(buf[: 2 * m])), exp)
