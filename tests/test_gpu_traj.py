"""GPU: the trajectory operators -- gf_traj_group (a window grouped by objID), gf_tstats_run
(TStatsQuery.java:154-188) and gf_traj_select (sub-trajectories) -- against the plain-Python
restatement of tests/traj_ref.py.  Everything is compared exactly: keys, offsets, perm and the
temporal lengths as integers, the spatial lengths bit for bit (the sequential left-to-right fp64
sum), speeds equal or both NaN.  The windows are the smallest that reach every path: a wave
boundary, a hot objID over many tiles and blocks (short and long tStats paths), every kind of key
at 200k points over ~50k objIDs, and the highest table load (every point its own objID)."""
import ctypes as C
import functools

import numpy as np
import pytest

import spatialflink_amd as sf
from spatialflink_amd import _lib
from conftest import BEIJING, QPOINT

import traj_ref as R

pytestmark = pytest.mark.gpu

I64_MIN = -(1 << 63)
EMPTY_MARK = (1 << 63) - 2  # the grouping table's own empty marker: a legal key like any other


def _xy(rng, n):
    return rng.uniform(BEIJING[0], BEIJING[1], n), rng.uniform(BEIJING[2], BEIJING[3], n)


@functools.lru_cache(maxsize=None)
def window_data(name):
    """(x, y, obj, ts) of the named window, with its restatement (computed once, shared)."""
    if name == "hot20k":  # 3 objIDs, one holding ~95 %: its segment spans many tiles and blocks
        rng = np.random.default_rng(11)
        n = 20_000
        obj = np.where(rng.random(n) < 0.95, 7, np.where(rng.random(n) < 0.6, I64_MIN + 2, _lib.OBJID_NULL)).astype(np.int64)
        ts = 1_600_000_000_000 + np.arange(n) * 5 + rng.integers(-12, 12, n)  # mostly rising, some late / equal
        ts[rng.random(n) < 0.01] = 0
        ts[:3] = 0  # leading ts-0 points
    elif name == "mix200k":  # ~50k objIDs of every kind of key; ts unsorted with duplicates and zeros
        rng = np.random.default_rng(12)
        n = 200_000
        pool = np.concatenate([rng.integers(-(1 << 40), 1 << 40, 30_000), rng.integers(0, 5000, 4_000),
                               I64_MIN + rng.integers(0, 20_000, 15_996),
                               [_lib.OBJID_NULL, EMPTY_MARK, I64_MIN, -1]]).astype(np.int64)
        obj = pool[rng.integers(0, len(pool), n)]
        ts = rng.integers(0, 4000, n)
        ts[rng.random(n) < 0.02] = 0
    elif name == "distinct100k":  # every point its own objID: the highest table load
        rng = np.random.default_rng(13)
        n = 100_000
        obj = (rng.permutation(n).astype(np.int64) - 40_000) * 7919
        ts = rng.integers(1, 1 << 40, n)
    elif name == "one65":  # one objID over 65 points: crosses a wave
        rng = np.random.default_rng(14)
        n = 65
        obj = np.full(n, 42, np.int64)
        ts = np.cumsum(rng.integers(0, 3, n))
    elif name == "one1":
        rng = np.random.default_rng(15)
        n = 1
        obj = np.array([I64_MIN + 5], np.int64)
        ts = np.array([77], np.int64)
    else:
        raise KeyError(name)
    x, y = _xy(rng, n)
    ts = ts.astype(np.int64)
    keys, off, perm = R.group_ref(obj)
    stats = R.tstats_ref(x, y, ts, keys, off, perm)
    return x, y, obj, ts, (keys, off, perm), stats


def device_window(name):
    x, y, obj, ts = window_data(name)[:4]
    return sf.PointWindow.from_numpy(x, y, obj, ts)


def check_groups(g, ref):
    keys, off, perm = g.read()
    np.testing.assert_array_equal(keys, ref[0])
    np.testing.assert_array_equal(off, ref[1])
    np.testing.assert_array_equal(perm, ref[2])
    assert (g.ntraj, g.n) == (len(ref[0]), len(ref[2]))


def test_empty_window(gpu):
    e = np.empty(0)
    w = sf.PointWindow.from_numpy(e, e, e.astype(np.int64), e.astype(np.int64))
    g = sf.TrajectoryGroups(w)
    keys, off, perm = g.read()
    assert (g.ntraj, g.n, len(keys), off.tolist(), len(perm)) == (0, 0, 0, [0], 0)
    cnt, k, S, T, V = g.tstats()
    assert cnt == 0 and len(k) == 0
    import torch
    sub = g.select(torch.zeros(1, dtype=torch.int64, device=gpu))
    assert len(sub) == 0 and sub.off.tolist() == [0] and len(sub.idx) == 0
    assert len(sf.PointTStatsQuery(sf.QueryConfiguration(sf.QueryType.WindowBased)).run(w)) == 0


@pytest.mark.parametrize("name", ["one1", "one65", "distinct100k", "mix200k"])
def test_grouping_and_tstats_match_the_restatement(gpu, name):
    ref, stats = window_data(name)[4:]
    g = sf.TrajectoryGroups(device_window(name))
    check_groups(g, ref)
    cnt, *got = g.tstats()
    assert cnt == len(ref[0])
    R.assert_stats_equal(got, stats)
    if name == "distinct100k":
        np.testing.assert_array_equal(g.read()[2], np.arange(100_000, dtype=np.uint32))
        assert not got[1].any() and not got[2].any() and np.isnan(got[3]).all()
    if name == "mix200k":  # every trajectory of two points or more through the block path as well
        g.set_long_threshold(2)
        R.assert_stats_equal(g.tstats()[1:], stats)


@pytest.mark.parametrize("threshold", [0, 256, 1 << 31], ids=["default", "long256", "lane-only"])
def test_hot_objid_short_and_long_paths(gpu, threshold):
    """20k points, 3 objIDs, one with ~95 %.  Default: the hot objID takes the block path, the two
    small ones (~600 and ~400 points) a lane each; 256: all three take the block path; 2^31: one lane
    walks even the hot one.  All bit for bit the restatement."""
    ref, stats = window_data("hot20k")[4:]
    sizes = np.diff(ref[1])
    assert len(sizes) == 3 and sizes.max() > 18_000 and 256 < sizes.min() < 2048
    g = sf.TrajectoryGroups(device_window("hot20k"))
    check_groups(g, ref)
    g.set_long_threshold(threshold)
    assert stats[1].min() > 0.0 and stats[2].min() > 0  # the vector exercises the sums
    R.assert_stats_equal(g.tstats()[1:], stats)


def test_traj_id_set(gpu):
    ref, stats = window_data("mix200k")[4:]
    keys = ref[0]
    g = sf.TrajectoryGroups(device_window("mix200k"))
    present = keys[[5, len(keys) // 2, 3, 17, len(keys) - 1]]
    absent = np.array([(1 << 62) - 5, I64_MIN + 999_999, 123_456_789_123], np.int64)
    assert not np.isin(absent, keys).any()
    want = np.isin(keys, present)
    cnt, *got = g.tstats(np.concatenate([absent[:2], present, present[:2], absent[2:]]))
    assert cnt == 5
    R.assert_stats_equal(got, tuple(a[want] for a in stats))  # only the present rows, in first-occurrence order
    cnt, *got = g.tstats(absent)
    assert cnt == 0 and len(got[0]) == 0
    cnt, *got = g.tstats(())  # the empty set: everything
    assert cnt == len(keys)
    R.assert_stats_equal(got, stats)


@pytest.mark.parametrize("filtered", [False, True])
def test_tstats_capacity(gpu, filtered):
    """cap < count: the full count comes back, exactly cap rows are written, nothing beyond them."""
    ref, stats = window_data("mix200k")[4:]
    keys = ref[0]
    w = device_window("mix200k")
    g = sf.TrajectoryGroups(w)
    ids = np.ascontiguousarray(keys[::3]) if filtered else np.empty(0, np.int64)
    want = np.isin(keys, ids) if filtered else np.ones(len(keys), bool)
    cap, guard = 1000, 64
    ok = np.full(cap + guard, -7, np.int64)
    oS, oV = np.full(cap + guard, -7.0), np.full(cap + guard, -7.0)
    oT = np.full(cap + guard, -7, np.int64)
    cnt = C.c_int64()
    pts = w.c_struct()
    st = _lib.lib().gf_tstats_run(g.handle, C.byref(pts), ids.ctypes.data if filtered else None, len(ids), ok.ctypes.data,
                                  oS.ctypes.data, oT.ctypes.data, oV.ctypes.data, cap, C.byref(cnt))
    assert st == _lib.GF_OK and cnt.value == int(want.sum()) > cap
    R.assert_stats_equal((ok[:cap], oS[:cap], oT[:cap], oV[:cap]), tuple(a[want][:cap] for a in stats))
    assert (ok[cap:] == -7).all() and (oS[cap:] == -7.0).all() and (oT[cap:] == -7).all() and (oV[cap:] == -7.0).all()
    # cap 0 with null outputs only counts
    st = _lib.lib().gf_tstats_run(g.handle, C.byref(pts), None, 0, None, None, None, None, 0, C.byref(cnt))
    assert st == _lib.GF_OK and cnt.value == len(keys)


def check_sub(sub, exp):
    for got, e in zip((sub.objID, sub.off, sub.x, sub.y, sub.ts, sub.idx), exp):
        np.testing.assert_array_equal(got, e)


def test_sub_trajectories_of_a_range_query(gpu):
    x, y, obj, ts, ref, _ = window_data("mix200k")
    w = device_window("mix200k")
    grid = sf.UniformGrid(100, *BEIJING)
    conf = sf.QueryConfiguration(sf.QueryType.WindowBased)
    rr = sf.PointPointRangeQuery(conf, grid).run(w, [sf.Point("q", *QPOINT, 0, grid)], 0.02)
    hits = rr.indices().astype(np.int64)
    assert 10 < len(hits) < 2000
    hit = np.zeros(len(x), bool)
    hit[hits] = True
    exp = R.subtraj_ref(x, y, ts, *ref, hit)
    assert 10 < len(exp[0]) and (np.diff(exp[1]) == 1).any() and (np.diff(exp[1]) > 1).any()  # single points too
    sub = sf.sub_trajectories(w, rr)
    check_sub(sub, exp)
    check_sub(sf.sub_trajectories(w, rr.bitmap), exp)


def test_sub_trajectory_of_one_flagged_point(gpu):
    """one flagged point of the hot objID gives that whole trajectory (19k points); no flag, nothing"""
    import torch

    x, y, obj, ts, ref, _ = window_data("hot20k")
    w = device_window("hot20k")
    keys, off, perm = ref
    hot = int(np.argmax(np.diff(off)))
    i = int(perm[off[hot] + 12_345])
    hit = np.zeros(len(x), bool)
    hit[i] = True
    words = np.zeros((len(x) + 63) // 64, np.uint64)
    words[i >> 6] = np.uint64(1) << np.uint64(i & 63)
    g = sf.TrajectoryGroups(w)
    sub = g.select(torch.as_tensor(words.view(np.int64)).to(gpu))
    exp = R.subtraj_ref(x, y, ts, *ref, hit)
    assert exp[0].tolist() == [int(keys[hot])] and exp[1][-1] == off[hot + 1] - off[hot]
    check_sub(sub, exp)
    none = g.select(torch.zeros(len(words), dtype=torch.int64, device=gpu))
    assert len(none) == 0 and none.off.tolist() == [0] and len(none.idx) == 0
    # capacity: the counts are complete, the arrays cut
    m, npts = C.c_int64(), C.c_int64()
    oi = np.full(100 + 8, 0xFFFFFFFF, np.uint32)
    pts = w.c_struct()
    st = _lib.lib().gf_traj_select(g.handle, C.byref(pts), torch.as_tensor(words.view(np.int64)).to(gpu).data_ptr(), None,
                                   None, 0, None, None, None, oi.ctypes.data, 100, C.byref(m), C.byref(npts))
    assert st == _lib.GF_OK and (m.value, npts.value) == (1, int(exp[1][-1]))
    np.testing.assert_array_equal(oi[:100], exp[5][:100])
    assert (oi[100:] == 0xFFFFFFFF).all()


def test_results_are_identical_from_run_to_run(gpu):
    """the 200k window twice through ONE groups object (its workspace reused), a smaller window in
    between: every output byte-identical"""
    import torch

    w = device_window("mix200k")
    rng = np.random.default_rng(5)
    bm = torch.as_tensor(rng.integers(-(1 << 63), 1 << 63, (w.n + 63) // 64, dtype=np.int64) &
                         rng.integers(-(1 << 63), 1 << 63, (w.n + 63) // 64, dtype=np.int64) &
                         rng.integers(-(1 << 63), 1 << 63, (w.n + 63) // 64, dtype=np.int64)).to(gpu)
    g = sf.TrajectoryGroups(w)

    def outputs():
        sub = g.select(bm)
        return [a.tobytes() for a in (*g.read(), *g.tstats()[1:], sub.objID, sub.off, sub.x, sub.y, sub.ts, sub.idx)]

    first = outputs()
    g.regroup(device_window("hot20k"))
    check_groups(g, window_data("hot20k")[4])
    g.regroup(w)
    assert outputs() == first
    check_groups(g, window_data("mix200k")[4])


def test_argument_errors_on_the_device(gpu):
    w = device_window("one65")
    g = sf.TrajectoryGroups(w)
    L = _lib.lib()
    cnt, cnt2 = C.c_int64(), C.c_int64()
    pts = w.c_struct()
    no_ts = _lib.GfPoints(pts.x, pts.y, pts.objID, None, pts.n)
    other_n = _lib.GfPoints(pts.x, pts.y, pts.objID, pts.ts, pts.n - 1)
    for p in (no_ts, other_n):
        assert L.gf_tstats_run(g.handle, C.byref(p), None, 0, None, None, None, None, 0, C.byref(cnt)) == _lib.GF_ERR_ARG
        assert L.gf_traj_select(g.handle, C.byref(p), w.x.data_ptr(), None, None, 0, None, None, None, None, 0,
                                C.byref(cnt), C.byref(cnt2)) == _lib.GF_ERR_ARG
    assert L.gf_tstats_run(g.handle, C.byref(pts), None, 3, None, None, None, None, 0, C.byref(cnt)) == _lib.GF_ERR_ARG
    assert L.gf_tstats_run(g.handle, C.byref(pts), None, 0, None, None, None, None, -1, C.byref(cnt)) == _lib.GF_ERR_ARG
    assert L.gf_traj_groups_set_long_threshold(g.handle, -1) == _lib.GF_ERR_ARG
    h = C.c_void_p()
    for p in (_lib.GfPoints(pts.x, pts.y, pts.objID, pts.ts, -1), _lib.GfPoints(pts.x, pts.y, pts.objID, pts.ts, 1 << 32),
              _lib.GfPoints(pts.x, pts.y, None, pts.ts, pts.n)):
        assert L.gf_traj_group(g.ctx.handle, C.byref(p), C.byref(h)) == _lib.GF_ERR_ARG
        assert h.value is None


def test_python_mirror_with_string_objids(gpu):
    """PointWindow.from_points with String objIDs: the decoded Strings of the tStats rows match the
    restatement keyed by String; trajIDSet takes Strings."""
    rng = np.random.default_rng(21)
    names = ["dev-17", "42", "007", "tram 9", None, "-12", "bus/é"]
    n = 700
    who = rng.integers(0, len(names), n)
    x, y = _xy(rng, n)
    ts = np.cumsum(rng.integers(0, 4, n)) + rng.integers(0, 3, n)
    points = [sf.Point(names[who[i]], x[i], y[i], int(ts[i])) for i in range(n)]
    w = sf.PointWindow.from_points(points)
    exp = {}
    for nm in names:
        exp.setdefault(nm, R.tstats_one((p.x, p.y, p.timeStampMillisec) for p in points if p.objID == nm))
    order = list(dict.fromkeys(names[j] for j in who))  # first-occurrence order
    conf = sf.QueryConfiguration(sf.QueryType.WindowBased)
    res = sf.PointTStatsQuery(conf).run(w)
    assert res.objid_strings() == order

    def same(rows, want):
        assert [r[0] for r in rows] == want
        for nm, S, T, V in rows:
            eS, eT, eV = exp[nm]
            assert (S, T) == (eS, eT) and (V == eV or (V != V and eV != eV))

    same(res.tuples(), order)
    sel = ["tram 9", "42", "no such device", "007"]
    same(sf.PointTStatsQuery(conf).run(w, sel).tuples(), [nm for nm in order if nm in sel])
    assert len(sf.PointTStatsQuery(conf).run(w, ["no such device"])) == 0
    keys, off, perm = sf.group_by_objid(w)
    assert w.objid_strings(keys) == order and off[-1] == n
    for t, nm in enumerate(order):
        np.testing.assert_array_equal(perm[off[t]:off[t + 1]], np.flatnonzero([names[j] == nm for j in who]))
