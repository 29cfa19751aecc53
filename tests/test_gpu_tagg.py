"""GPU: tAggregate -- gf_tagg_group / gf_tagg_run, the per-cell table, the ALL CSR and the rows of the
five aggregates through PointTAggregateQuery -- against the literal transcription of
TimeWindowProcessFunction.process (tests/tagg_ref.py).  Everything is compared exactly: integers, keys,
order.  The windows are the smallest that reach every path: a wave boundary, one (cell, objID) group
over many tiles (short and long group paths), one hot cell over ~5k objIDs (lane and block cell paths),
the highest table load (every point its own group) and 200k points of every kind of key with common
timestamp ties, out-of-grid cells and non-finite coordinates."""
import ctypes as C
import functools

import numpy as np
import pytest

import spatialflink_amd as sf
from spatialflink_amd import _lib
from conftest import BEIJING

import tagg_ref as R

pytestmark = pytest.mark.gpu

I64_MIN = -(1 << 63)
EMPTY_MARK = (1 << 63) - 2  # the grouping table's own empty marker: a legal key like any other
NAMES = ["ALL", "SUM", "AVG", "MIN", "MAX"]
COLS = ("cx", "cy", "count", "multi", "sum", "minLen", "minKey", "maxLen", "maxKey")


def grid_of(name):
    return sf.UniformGrid(100, *BEIJING)


@functools.lru_cache(maxsize=None)
def window_data(name):
    """(x, y, obj, ts) of the named window, with its reference (computed once, shared)."""
    w, h = BEIJING[1] - BEIJING[0], BEIJING[3] - BEIJING[2]
    cl = w / 100
    if name == "one1":
        x, y = np.array([116.4]), np.array([39.9])
        obj, ts = np.array([I64_MIN + 5], np.int64), np.array([77])
    elif name == "one65":  # one cell, one objID, 65 points: crosses a wave
        rng = np.random.default_rng(21)
        n = 65
        x, y = np.full(n, 116.4001), np.full(n, 39.9001)
        obj, ts = np.full(n, 42, np.int64), rng.integers(0, 40, n)
    elif name == "hot20k":  # one (cell, objID) group holds ~95 %: its segment spans many tiles and blocks
        rng = np.random.default_rng(22)
        n = 20_000
        hot = rng.random(n) < 0.95
        x = np.where(hot, 116.4001, rng.uniform(BEIJING[0], BEIJING[1], n))
        y = np.where(hot, 39.9001, rng.uniform(BEIJING[2], BEIJING[3], n))
        obj = np.where(hot, 7, rng.integers(0, 40, n)).astype(np.int64)
        ts = rng.integers(1000, 3000, n)
        ts[rng.random(n) < 0.3] = 1000  # the minimum and the maximum are both held by many points
        ts[rng.random(n) < 0.3] = 2999
    elif name == "hotcell20k":  # one cell over ~5k objIDs
        rng = np.random.default_rng(23)
        n = 20_000
        x, y = 116.41 + rng.uniform(0, cl * 0.4, n), 39.9 + rng.uniform(0, cl * 0.4, n)
        obj = (rng.integers(0, 5000, n) * 7919 - 9_000_000).astype(np.int64)
        ts = rng.integers(0, 12, n)  # lengths, first steps and their positions tie all over
    elif name == "distinct100k":  # every point its own (cell, objID): the highest table load
        rng = np.random.default_rng(24)
        n = 100_000
        x, y = rng.uniform(BEIJING[0], BEIJING[1], n), rng.uniform(BEIJING[2], BEIJING[3], n)
        obj = (rng.permutation(n).astype(np.int64) - 40_000) * 7919
        ts = rng.integers(1, 1 << 40, n)
    elif name == "mix200k":  # ~20k objIDs of every kind of key, each around a home inside 30 x 30 cells
        rng = np.random.default_rng(25)
        n = 200_000
        pool = np.concatenate([rng.integers(-(1 << 40), 1 << 40, 12_000), rng.integers(0, 5000, 2_000),
                               I64_MIN + rng.integers(0, 20_000, 5_996),
                               [_lib.OBJID_NULL, EMPTY_MARK, I64_MIN, -1]]).astype(np.int64)
        pool = np.unique(pool)
        hx = BEIJING[0] + w * rng.uniform(0.3, 0.6, len(pool))
        hy = BEIJING[2] + h * rng.uniform(0.3, 0.6, len(pool))
        who = rng.integers(0, len(pool), n)
        who[:4000] = rng.integers(len(pool) - 4, len(pool), 4000)  # (unique sorted: NULL / the marker are last)
        who[4000:8000] = rng.integers(0, 2, 4000)                  # INT64_MIN and its neighbour
        rng.shuffle(who)
        obj = pool[who]
        x = hx[who] + rng.normal(0, cl * 0.6, n)
        y = hy[who] + rng.normal(0, cl * 0.6, n)
        out = rng.random(n) < 0.04  # out of grid on every side: cells like any other
        side = rng.integers(0, 4, n)
        x = np.where(out & (side == 0), BEIJING[0] - rng.uniform(0, 3 * cl, n), x)
        x = np.where(out & (side == 1), BEIJING[1] + rng.uniform(0, 3 * cl, n), x)
        y = np.where(out & (side == 2), BEIJING[2] - rng.uniform(0, 3 * cl, n), y)
        y = np.where(out & (side == 3), BEIJING[3] + rng.uniform(0, 3 * cl, n), y)
        bad = rng.choice(n, 40, replace=False)
        x[bad[:10]] = np.nan
        y[bad[10:20]] = np.nan
        x[bad[20:25]] = np.inf
        y[bad[25:30]] = -np.inf
        x[bad[30:35]] = -1e300
        y[bad[35:40]] = 1e300
        ts = rng.integers(0, 30, n)
    else:
        raise KeyError(name)
    ts = np.asarray(ts, np.int64)
    obj = np.asarray(obj, np.int64)
    cx, cy = R.cells_of(grid_of(name), x, y)
    table, csr, cells = R.tagg_ref(cx, cy, obj, ts)
    for a in (x, y, obj, ts, *table.values(), *csr):
        a.setflags(write=False)
    return x, y, obj, ts, table, csr, cells


def device_window(name):
    x, y, obj, ts = (a.copy() for a in window_data(name)[:4])  # (the shared arrays are read-only)
    return sf.PointWindow.from_numpy(x, y, obj, ts, start=1_000, end=11_000)


def check_run(g, name):
    """the per-cell table and the ALL CSR of a run TAggregateGroups against the reference; -> their bytes"""
    table, csr = window_data(name)[4:6]
    got = g.cells()
    assert (g.ncells, g.ngroups, g.n) == (len(table["cx"]), len(csr[1]), len(window_data(name)[0]))
    for k in COLS:
        assert got[k].dtype == table[k].dtype, k
        np.testing.assert_array_equal(got[k], table[k], err_msg=k)
    off, keys, lens = g.all_rows()
    np.testing.assert_array_equal(off, csr[0])
    np.testing.assert_array_equal(keys, csr[1])
    np.testing.assert_array_equal(lens, csr[2])
    return b"".join(got[k].tobytes() for k in COLS) + off.tobytes() + keys.tobytes() + lens.tobytes()


def check_query(name, groups=None):
    """the rows of each aggregate through PointTAggregateQuery against the reference's emission code"""
    table, csr, cells = window_data(name)[4:]
    w = device_window(name)
    q = sf.PointTAggregateQuery(sf.QueryConfiguration(sf.QueryType.WindowBased), grid_of(name))
    for fn in NAMES + ["mAx", "heatmap"]:
        exp = R.rows_ref(fn, table, cells)
        res = q.run(w, fn, "TIME", groups=groups)
        assert res.kind == exp["kind"] and len(res) == len(exp["keep"])
        assert (res.start, res.end) == (1_000, 11_000)
        for k in ("cx", "cy", "count", "key"):
            np.testing.assert_array_equal(getattr(res, k), exp[k], err_msg=f"{fn} {k}")
        np.testing.assert_array_equal(res.value, exp["value"], err_msg=fn)
        if exp["kind"] == "ALL":
            np.testing.assert_array_equal(res.off, csr[0])
            np.testing.assert_array_equal(res.keys, csr[1])
            np.testing.assert_array_equal(res.lens, csr[2])


def test_empty_window(gpu):
    e = np.empty(0)
    w = sf.PointWindow.from_numpy(e, e, e.astype(np.int64), e.astype(np.int64))
    g = sf.TAggregateGroups(w, grid_of("empty")).run()
    assert (g.ncells, g.ngroups, g.n) == (0, 0, 0)
    assert all(len(v) == 0 for v in g.cells().values())
    off, keys, lens = g.all_rows()
    assert off.tolist() == [0] and len(keys) == 0 and len(lens) == 0
    q = sf.PointTAggregateQuery(sf.QueryConfiguration(sf.QueryType.WindowBased), grid_of("empty"))
    for fn in NAMES:
        res = q.run(w, fn)
        assert len(res) == 0 and res.tuples() == []


@pytest.mark.parametrize("name", ["one1", "one65", "distinct100k", "mix200k"])
def test_table_csr_and_rows_match_the_reference(gpu, name):
    g = sf.TAggregateGroups(device_window(name), grid_of(name)).run()
    check_run(g, name)
    check_query(name, groups=g)
    if name == "distinct100k":  # nothing repeats: MIN / MAX and SUM / AVG emit nothing
        t = g.cells()
        assert g.ngroups == 100_000 and not t["multi"].any() and not t["sum"].any()
        q = sf.PointTAggregateQuery(sf.QueryConfiguration(sf.QueryType.WindowBased), grid_of(name))
        assert all(len(q.run(g.window, fn, groups=g)) == 0 for fn in NAMES[1:])
    if name == "mix200k":
        t = window_data(name)[4]
        n = 100
        assert ((t["cx"] < 0) | (t["cx"] >= n) | (t["cy"] < 0) | (t["cy"] >= n)).sum() > 50  # out-of-grid cells
        assert (t["multi"] > 1).sum() > 500 and (t["sum"] > 0).sum() > 500
    g.close()


def test_one_group_over_many_tiles_on_both_group_paths(gpu):
    g = sf.TAggregateGroups(device_window("hot20k"), grid_of("hot20k"))
    x, y, obj = window_data("hot20k")[:3]
    assert ((x == 116.4001) & (y == 39.9001) & (obj == 7)).sum() > 18_000  # the hot group
    seen = set()
    for long_group in (0, 1, 1 << 31):  # the default (block path for the hot group), every group, none
        g.set_thresholds(long_group, 0)
        seen.add(check_run(g.run(), "hot20k"))
    assert len(seen) == 1
    g.set_thresholds(0, 0)
    check_query("hot20k", groups=g)
    g.close()


def test_one_hot_cell_on_both_cell_paths(gpu):
    g = sf.TAggregateGroups(device_window("hotcell20k"), grid_of("hotcell20k"))
    t = window_data("hotcell20k")[4]
    assert len(t["cx"]) == 1 and t["count"][0] > 4000 and t["multi"][0] > 3000
    seen = set()
    for big_cell in (0, 1, 1 << 31):  # the default (block path), every cell, none (one lane walks ~5k groups)
        g.set_thresholds(0, big_cell)
        seen.add(check_run(g.run(), "hotcell20k"))
    assert len(seen) == 1
    g.set_thresholds(0, 0)
    check_query("hotcell20k", groups=g)
    g.close()


def test_block_paths_for_every_group_and_cell(gpu):
    g = sf.TAggregateGroups(device_window("mix200k"), grid_of("mix200k"))
    g.set_thresholds(1, 1)
    a = check_run(g.run(), "mix200k")
    g.set_thresholds(1 << 31, 1 << 31)
    assert check_run(g.run(), "mix200k") == a
    g.close()


def test_reused_object_after_a_larger_window_gives_the_same_bytes(gpu):
    fresh = sf.TAggregateGroups(device_window("hot20k"), grid_of("hot20k")).run()
    a = check_run(fresh, "hot20k")
    fresh.close()
    g = sf.TAggregateGroups(device_window("mix200k"), grid_of("mix200k")).run()
    check_run(g, "mix200k")
    for _ in range(2):
        g.regroup(device_window("hot20k"), grid_of("hot20k")).run()
        assert check_run(g, "hot20k") == a
    g.close()


def test_tuples_carry_cell_ids_window_bounds_and_objid_strings(gpu):
    grid = grid_of("t")
    pts = [sf.Point("bus-7", 116.4001, 39.9001, 10), sf.Point("12", 116.4002, 39.9002, 50),
           sf.Point("bus-7", 116.4003, 39.9003, 40), sf.Point("12", 116.4001, 39.9001, 20),
           sf.Point("tram", 115.0, 39.0, 5), sf.Point("bus-7", 116.4002, 39.9001, 10)]
    w = sf.PointWindow.from_points(pts, start=0, end=10_000)
    q = sf.PointTAggregateQuery(sf.QueryConfiguration(sf.QueryType.WindowBased), grid)
    cid = grid.assignGridCellID(116.4001, 39.9001)
    oid = grid.assignGridCellID(115.0, 39.0)  # out of the grid: a cell like any other
    allr = q.run(w, "all").tuples()
    assert [(t[0], t[1], t[2], t[3]) for t in allr] == [(cid, 2, 0, 10_000), (oid, 1, 0, 10_000)]
    assert list(allr[0][4].items()) == [("bus-7", 30), ("12", 30)] and dict(allr[1][4]) == {"tram": 0}
    assert q.run(w, "SUM").tuples() == [(cid, 2, 0, 10_000, {"": 60})]
    assert q.run(w, "avg").tuples() == [(cid, 2, 0, 10_000, {"": 30})]
    assert q.run(w, "MIN").tuples() == [(cid, 2, 0, 10_000, {"bus-7": 30})]  # first steps: both 30, bus-7's came first
    assert q.run(w, "MAX").tuples() == [(cid, 2, 0, 10_000, {"bus-7": 30})]


def test_argument_errors_with_a_device(gpu):
    L = _lib.lib()
    name = "one65"
    w = device_window(name)
    grid = grid_of(name)
    g = sf.TAggregateGroups(w, grid)
    with pytest.raises(ValueError, match="no gf_tagg_run"):
        g.cells()
    with pytest.raises(ValueError, match="no gf_tagg_run"):
        g.all_rows()
    ctx = g.ctx.handle
    pts = w.c_struct()
    h = C.c_void_p()
    for col in ("x", "y", "objID"):
        bad = w.c_struct()
        setattr(bad, col, None)
        assert L.gf_tagg_group(ctx, C.byref(grid.c_grid), C.byref(bad), C.byref(h)) == _lib.GF_ERR_ARG
        assert b"null x / y / objID" in L.gf_ctx_last_error(ctx) and h.value is None
    flat = _lib.GfGrid(100, 0, 1.0, 1.0, 0.0, 1.0, 0.0)  # cellLength 0
    assert L.gf_tagg_group(ctx, C.byref(flat), C.byref(pts), C.byref(h)) == _lib.GF_ERR_ARG
    other = _lib.Context(0)
    assert L.gf_tagg_group(other.handle, C.byref(grid.c_grid), C.byref(pts), C.byref(g.handle)) == _lib.GF_ERR_ARG
    assert b"another context" in L.gf_ctx_last_error(other.handle)
    short_w = sf.PointWindow.from_numpy(*(a[:64].copy() for a in window_data(name)[:4]))
    shorter = short_w.c_struct()
    assert L.gf_tagg_run(g.handle, C.byref(shorter)) == _lib.GF_ERR_ARG
    assert b"not the grouped window" in L.gf_ctx_last_error(ctx)
    nots = w.c_struct()
    nots.ts = None
    assert L.gf_tagg_run(g.handle, C.byref(nots)) == _lib.GF_ERR_ARG
    assert L.gf_tagg_set_thresholds(g.handle, -1, 0) == _lib.GF_ERR_ARG
    check_run(g.run(), name)  # the object is still good
    cells = C.c_int64()
    cx = np.full(4, -7, np.int32)
    assert L.gf_tagg_read_cells(g.handle, cx.ctypes.data, *([None] * 8), 0, C.byref(cells)) == _lib.GF_OK
    assert cells.value == 1 and cx[0] == -7  # cap 0: the count only
    assert L.gf_tagg_read_cells(g.handle, *([None] * 9), -1, C.byref(cells)) == _lib.GF_ERR_ARG
    g.close()
