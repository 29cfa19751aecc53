"""GPU: the sliding pane ENGINES (gf_knn_sliding_*, gf_range_sliding_*, gf_pane_bounds; _PaneStream,
SlidingKNNQuery, SlidingRangeQuery) at small shapes and pane edges.  Everything is bit-exact against the
oracle evaluated from scratch on each window's points (objID, distance bits, in-window index, hit
positions); the fired windows are Flink's assignment by brute force (sliding_cases.expected_windows).
The streams, cuts and gaps come from tests/sliding_cases.py; tests/test_sliding_cases.py shows on the CPU,
from the oracle alone, that they hold what the cases here claim (full, short and empty records, windows
only the merge decides, points on p * pane - 1 and p * pane that are rank 0 of their windows, ...)."""
import ctypes as C
import math

import numpy as np
import pytest

import sliding_cases as SC
from conftest import BEIJING, QPOINT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sf(gpu):
    import spatialflink_amd

    return spatialflink_amd


def conf(sf):
    return sf.QueryConfiguration(sf.QueryType.WindowBased)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def dev_batches(sf, s, cuts):
    for x, y, o, t in SC.batches_of(s, cuts):
        yield sf.PointWindow.from_numpy(x, y, o, t)


def even_cuts(s, count=7):
    n = len(s.ts)
    return [0] + sorted({(n * j) // count | 1 for j in range(1, count)} - {n}) + [n]


def knn_engine(sf, s, k, depth, grid_n=100, cap=None):
    g = sf.UniformGrid(grid_n, *BEIJING)
    q = sf.Point("q", *QPOINT, 0, g)
    op = sf.SlidingKNNQuery(conf(sf), g, q, SC.R_KNN, k, size_ms=s.size, slide_ms=s.slide, pipeline=depth)
    if cap:
        op.op.set_capacity(0, q, SC.R_KNN, k, cap)
    return op


def drive(op, batches, lazy=False, statuses=None):
    """Push every batch; results() after every push, or (lazy) only once after flush()."""
    import torch

    got = []
    for b in batches:
        op.push(b)
        if statuses is not None:  # the raw records' status words, before they are decoded
            torch.cuda.synchronize()
            done = op.closed[:-1] if op.pending else op.closed
            statuses.update(op.records.decode(slot)[0] for _, slot, _ in done)
        if not lazy:
            got += op.results()
    op.flush()
    got += op.results()
    return got


def run_knn(sf, s, cuts, k, depth, grid_n=100, cap=None, lazy=False, statuses=None):
    op = knn_engine(sf, s, k, depth, grid_n, cap)
    try:
        return drive(op, dev_batches(sf, s, cuts), lazy, statuses)
    finally:
        op.close()


def check_knn(got, ref, what=""):
    assert [(r.windowStart, r.windowEnd) for r in got] == [w for w, *_ in ref], what
    for r, (w, st, o, d, i) in zip(got, ref):
        msg = f"{what} window {w}"
        assert st == 0
        np.testing.assert_array_equal(r.objID, o, err_msg=msg)
        np.testing.assert_array_equal(bits(r.dist), bits(d), err_msg=msg)
        np.testing.assert_array_equal(r.idx, i, err_msg=msg)


def same_records(a, b, shift=0):
    assert [(r.windowStart + shift, r.windowEnd + shift) for r in a] == [(r.windowStart, r.windowEnd) for r in b]
    for r, t in zip(a, b):
        np.testing.assert_array_equal(r.objID, t.objID)
        np.testing.assert_array_equal(bits(r.dist), bits(t.dist))
        np.testing.assert_array_equal(r.idx, t.idx)


def range_engine(sf, s, poly, op=None):
    g = sf.UniformGrid(100, *BEIJING)
    if poly:
        op = op or sf.PointPolygonRangeQuery(conf(sf), g)
        return sf.SlidingRangeQuery(op, [sf.Polygon(r, g) for r in SC.POLYGONS], SC.R_POLY, s.size, s.slide)
    op = op or sf.PointPointRangeQuery(conf(sf), g)
    return sf.SlidingRangeQuery(op, [sf.Point("q", *QPOINT, 0, g)], SC.R_RANGE, s.size, s.slide)


def run_range(sf, s, cuts, poly, lazy=False):
    op = range_engine(sf, s, poly)
    try:
        return drive(op, dev_batches(sf, s, cuts), lazy)
    finally:
        op.close()


def check_range(got, ref, what=""):
    assert [(a, b) for a, b, _ in got] == [w for w, _ in ref], what
    for (a, b, hits), (w, h) in zip(got, ref):
        np.testing.assert_array_equal(hits, h, err_msg=f"{what} window {w}")


# ---------------------------------------------------------------------------------------------
# geometry x origin
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [1, 2])
@pytest.mark.parametrize("case", SC.MATRIX, ids=SC.case_id)
def test_knn_geometry_and_origin(sf, oracle_mod, case, depth):
    """Tumbling, slide > size, W = 3, 7, 63, 64 (the maximum) and 100 ms panes, on streams that start at
    0, cross zero from -7500 and sit at an epoch-scale origin: the fired windows are Flink's, every record
    is the oracle's on that window's points."""
    s = SC.case_stream(oracle_mod, case)
    got = run_knn(sf, s, even_cuts(s), case[3], depth)
    check_knn(got, SC.knn_reference(oracle_mod, s, case[3]), SC.case_id(case))


@pytest.mark.parametrize("poly", [False, True])
@pytest.mark.parametrize("case", SC.MATRIX, ids=SC.case_id)
def test_range_geometry_and_origin(sf, oracle_mod, case, poly):
    s = SC.case_stream(oracle_mod, case)
    got = run_range(sf, s, even_cuts(s), poly)
    check_range(got, SC.range_reference(oracle_mod, s, poly), SC.case_id(case))


@pytest.mark.parametrize("size,slide", [(1000, 3000), (3000, 2000), (7000, 2000), (6400, 100)])
def test_shifted_stream_gives_the_same_records(sf, oracle_mod, size, slide):
    """The same stream 1000 * lcm(size, slide) ms later: the same records and hit lists, byte for byte,
    in windows shifted by that amount."""
    s = SC.case_stream(oracle_mod, (size, slide, "negative", SC.MATRIX_K))
    by = 1000 * math.lcm(size, slide)
    t = SC.shifted(s, by)
    cuts = even_cuts(s)
    for depth in (1, 2):
        a, b = run_knn(sf, s, cuts, SC.MATRIX_K, depth), run_knn(sf, t, cuts, SC.MATRIX_K, depth)
        assert [(r.windowStart, r.windowEnd) for r in b] == SC.expected_windows(t.ts, size, slide)
        same_records(a, b, by)
    a, b = run_range(sf, s, cuts, False), run_range(sf, t, cuts, False)
    assert [(w0 + by, w1 + by) for w0, w1, _ in a] == [(w0, w1) for w0, w1, _ in b] == SC.expected_windows(t.ts, size, slide)
    for (_, _, h), (_, _, g) in zip(a, b):
        np.testing.assert_array_equal(h, g)


def test_65_panes_are_refused_and_the_context_lives_on(sf, oracle_mod):
    """size / gcd = 65 panes: GF_ERR_ARG at creation, the message names the 64-pane limit; a refused
    engine borrows nothing, so the next one on the same operator (and context) works and is exact."""
    from spatialflink_amd import _lib

    L = _lib.lib()
    g = sf.UniformGrid(100, *BEIJING)
    q = sf.Point("q", *QPOINT, 0, g)
    k = SC.MATRIX_K
    kop = sf.PointPointKNNQuery(conf(sf), g)
    ctx, plan = kop.plan(0, q, SC.R_KNN, k)
    h = C.c_void_p()
    assert L.gf_knn_sliding_create(plan, 65000, 1000, C.byref(h)) == _lib.GF_ERR_ARG and not h.value
    assert "64 panes" in L.gf_ctx_last_error(ctx.handle).decode()
    with pytest.raises(ValueError, match="64 panes"):
        sf.SlidingKNNQuery(conf(sf), g, q, SC.R_KNN, k, size_ms=65000, slide_ms=1000, op=kop)
    assert kop._plans.holds(plan) == 0
    s = SC.case_stream(oracle_mod, (3000, 2000, "zero", k))
    op = sf.SlidingKNNQuery(conf(sf), g, q, SC.R_KNN, k, size_ms=3000, slide_ms=2000, op=kop)
    check_knn(drive(op, dev_batches(sf, s, even_cuts(s))), SC.knn_reference(oracle_mod, s, k), "after the refusal")
    op.close()

    rop = sf.PointPointRangeQuery(conf(sf), g)
    ctx, rplan = rop.plan(0, [q], SC.R_RANGE)
    assert L.gf_range_sliding_create(rplan, 65000, 1000, C.byref(h)) == _lib.GF_ERR_ARG and not h.value
    assert "64 panes" in L.gf_ctx_last_error(ctx.handle).decode()
    bad = sf.SlidingRangeQuery(rop, [q], SC.R_RANGE, 65000, 1000)
    with pytest.raises(ValueError, match="64 panes"):
        drive(bad, dev_batches(sf, s, even_cuts(s)))
    assert rop._plans.holds(rplan) == 0
    good = range_engine(sf, s, False, op=rop)
    check_range(drive(good, dev_batches(sf, s, even_cuts(s))), SC.range_reference(oracle_mod, s, False))
    good.close()


# ---------------------------------------------------------------------------------------------
# cuts and gaps
# ---------------------------------------------------------------------------------------------
def cut_case(oracle_mod, size, slide):
    return SC.case_stream(oracle_mod, (size, slide, "negative", SC.CUT_K))


def all_engines(sf, oracle_mod, s, cuts, what):
    for depth in (1, 2):
        check_knn(run_knn(sf, s, cuts, SC.CUT_K, depth), SC.knn_reference(oracle_mod, s, SC.CUT_K), f"{what} depth {depth}")
    check_range(run_range(sf, s, cuts, False), SC.range_reference(oracle_mod, s, False), what)


@pytest.mark.parametrize("cut", list(SC.CUTS))
@pytest.mark.parametrize("size,slide", SC.CUT_GEOMETRIES)
def test_batch_cuts(sf, oracle_mod, size, slide, cut):
    """One batch; cuts exactly on panes' first points; a pane over three batches; a run of one-point
    batches across a pane's end; pane slices at odd (copied) and even (viewed) offsets."""
    s = cut_case(oracle_mod, size, slide)
    all_engines(sf, oracle_mod, s, SC.CUTS[cut](s), cut)


@pytest.mark.parametrize("straddle", [False, True], ids=["inside", "on_cut"])
@pytest.mark.parametrize("kind", ["bridge", "exact", "ring"])
@pytest.mark.parametrize("size,slide", SC.CUT_GEOMETRIES)
def test_gaps(sf, oracle_mod, size, slide, kind, straddle):
    """W - 1 panes without a point (the bridging window fires), exactly W on a window start (that window
    does not fire), 2W + S + 3 (more than the record ring: stale slots are reused); inside one batch
    and with a cut on the gap."""
    g, cuts, _ = SC.with_gap(cut_case(oracle_mod, size, slide), kind, straddle)
    all_engines(sf, oracle_mod, g, cuts, f"gap {kind}")


@pytest.mark.parametrize("size,slide", SC.CUT_GEOMETRIES)
def test_single_point_first_batch_and_last_pane(sf, oracle_mod, size, slide):
    s = cut_case(oracle_mod, size, slide)
    last_pane = int(s.ts[-1]) // s.pane
    keep = np.flatnonzero(s.ts < last_pane * s.pane)
    keep = np.r_[keep, len(s.ts) - 1]            # the last pane keeps one point
    t = SC.subset(s, keep)
    assert np.count_nonzero(t.ts // t.pane == last_pane) == 1
    n = len(t.ts)
    all_engines(sf, oracle_mod, t, [0, 1, n // 2 | 1, n - 1, n], "single points")


# ---------------------------------------------------------------------------------------------
# k on both sides of every path change
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [1, 2])
@pytest.mark.parametrize("case", SC.K_CASES, ids=SC.case_id)
def test_k_boundaries(sf, oracle_mod, case, depth):
    """k = 1, 128 | 129 (the merge fused into the scan launch), 256 | 257 (the fused select), 512 | 513
    (the one-block select | the sorted path and the rank merge)."""
    s = SC.case_stream(oracle_mod, case)
    got = run_knn(sf, s, SC.cut_on_panes(s), case[3], depth)
    check_knn(got, SC.knn_reference(oracle_mod, s, case[3]), SC.case_id(case))


# ---------------------------------------------------------------------------------------------
# polling cadence and the overflow decode
# ---------------------------------------------------------------------------------------------
def every_pane(s):
    return SC._cuts(s, SC.pane_starts(s))


@pytest.mark.parametrize("depth", [1, 2])
@pytest.mark.parametrize("size,slide,cap", [(3000, 2000, None), (6400, 100, None), (3000, 2000, 2), (7000, 2000, 2)])
def test_polling_cadence(sf, oracle_mod, size, slide, cap, depth):
    """results() after every pane == results() once after flush(), over >= 3 rings of panes; with the
    candidate capacity at 2 the flagged windows are re-evaluated from their panes, so the engine's own
    trigger must decode each before its panes leave the ring."""
    k = SC.MATRIX_K
    s = SC.case_stream(oracle_mod, (size, slide, "negative", k))
    op = knn_engine(sf, s, k, depth)
    ring = C.c_int32()
    from spatialflink_amd import _lib

    assert _lib.lib().gf_knn_sliding_geometry(op.handle, None, None, None, C.byref(ring)) == 0
    op.close()
    assert ring.value == 2 * s.W + s.S + 2 and s.npanes >= 3 * ring.value
    cuts = every_pane(s)
    eager = run_knn(sf, s, cuts, k, depth, cap=cap)
    lazy = run_knn(sf, s, cuts, k, depth, cap=cap, lazy=True)
    same_records(eager, lazy)
    check_knn(lazy, SC.knn_reference(oracle_mod, s, k), "lazy")


@pytest.mark.parametrize("depth", [1, 2])
@pytest.mark.parametrize("k,cap", [(7, 2), (300, 64)])
def test_overflow_decode(sf, oracle_mod, k, cap, depth):
    """A candidate capacity that some panes overflow and others do not: flagged windows are re-evaluated
    pane by pane, exactly -- from a negative origin (floor_div of negative window ends), the first
    windows reaching before the stream's first pane (its first pane holds k + 2 neighbours)."""
    s = SC.case_stream(oracle_mod, (3000, 1000, "negative", k))
    statuses = set()
    got = run_knn(sf, s, every_pane(s), k, depth, cap=cap, statuses=statuses)
    check_knn(got, SC.knn_reference(oracle_mod, s, k), f"cap {cap}")
    assert 0 in statuses and statuses - {0}, statuses


# ---------------------------------------------------------------------------------------------
# range: a pane slot that regrows
# ---------------------------------------------------------------------------------------------
def test_range_slot_regrows_twice(sf, oracle_mod):
    """W = 3: slot 0 first holds 10 points (capacity 4096), then 6000, then 9000; every window before and
    after each regrow is exact."""
    sizes = [10, 10, 10, 6000, 10, 10, 9000, 10, 10, 10, 10]
    n = sum(sizes)
    x, y = oracle_mod.java_random_points(91, n, *BEIJING)
    rng = np.random.default_rng(91)
    ts = np.concatenate([j * 1000 + np.sort(rng.integers(0, 1000, m)) for j, m in enumerate(sizes)]).astype(np.int64)
    s = SC.Stream(x, y, np.arange(n, dtype=np.int64), ts, [], 3000, 1000, 1000, 3, 1, 0, len(sizes))
    ref = SC.range_reference(oracle_mod, s, False)
    assert sum(len(h) for _, h in ref) > 100
    check_range(run_range(sf, s, [0, 25, 3000, 6035, n - 7, n], False), ref, "regrow")
    check_range(run_range(sf, s, [0, n], True), SC.range_reference(oracle_mod, s, True), "regrow, polygons")


# ---------------------------------------------------------------------------------------------
# a sampled pane inside the engine (the one large case)
# ---------------------------------------------------------------------------------------------
_BIG = {}


def big_stream(oracle_mod):
    if not _BIG:
        sizes = [300, 400, (1 << 20) + 3, 350, 250]
        n = sum(sizes)
        x, y = oracle_mod.java_random_points(17, n, *BEIJING)
        rng = np.random.default_rng(17)
        ts = np.concatenate([j * 1000 + np.sort(rng.integers(0, 1000, m)) for j, m in enumerate(sizes)]).astype(np.int64)
        obj = (rng.permutation(n) % (n // 2)).astype(np.int64)
        s = SC.Stream(x, y, obj, ts, [], 2000, 1000, 1000, 2, 1, 0, len(sizes))
        _BIG["s"] = s
        _BIG["ref"] = SC.knn_reference(oracle_mod, s, 50, grid_n=500)
    return _BIG["s"], _BIG["ref"]


@pytest.mark.parametrize("depth", [1, 2])
def test_sampled_pane_inside_the_engine(sf, oracle_mod, depth):
    """(2000, 1000): a pane of 2^20 + 3 points (the smallest that takes the sampled threshold) between
    panes of a few hundred; at depth 2 the hint chain runs from an unsampled pane into the sampled one
    and back.  k = 50; the windows before, with and after that pane."""
    s, ref = big_stream(oracle_mod)
    got = run_knn(sf, s, [0, 500, len(s.ts) - 450, len(s.ts)], 50, depth, grid_n=500)
    assert len(got) == 6
    check_knn(got, ref, "sampled pane")


# ---------------------------------------------------------------------------------------------
# polygon and linestring plans under the engine
# ---------------------------------------------------------------------------------------------
def spread(n, seed):
    """n timestamps over (5000, 3000) panes from the negative origin, every pane populated."""
    rng = np.random.default_rng(seed)
    return np.sort(rng.integers(-7_500, 14_500, n)).astype(np.int64)


@pytest.mark.parametrize("depth", [1, 2])
def test_polygon_plan_under_the_engine(sf, oracle_mod, depth):
    import poly_cases as PC

    g = sf.UniformGrid(PC.GRID_N, *PC.BEIJING)
    og = oracle_mod.grid(PC.GRID_N, *PC.BEIJING)
    x, y, obj, _ = (np.array(a) for a in PC.window("star"))
    rings = PC.raw_polygons("star")[0]
    P = oracle_mod.Polygons([PC.polygons("star")[0]])
    ts = spread(len(x), 3)
    k = 20
    c = conf(sf)
    op = sf.SlidingKNNQuery(c, g, sf.Polygon(rings, g), PC.KNN_R, k, size_ms=5000, slide_ms=3000, pipeline=depth,
                            op=sf.PointPolygonKNNQuery(c, g))
    s = SC.Stream(x, y, obj, ts, [], 5000, 3000, 1000, 5, 3, -8, 22)
    got = drive(op, dev_batches(sf, s, even_cuts(s)))
    op.close()
    assert [(r.windowStart, r.windowEnd) for r in got] == SC.expected_windows(ts, 5000, 3000) and len(got) >= 7
    full = 0
    for r, (w, m) in zip(got, SC.window_masks(s)):
        n, eo, ed, ei = oracle_mod.knn_ppoly(og, x[m], y[m], obj[m], P, PC.KNN_R, k)
        full += n == k
        np.testing.assert_array_equal(r.objID, eo, err_msg=str(w))
        np.testing.assert_array_equal(bits(r.dist), bits(ed), err_msg=str(w))
        np.testing.assert_array_equal(r.idx, ei, err_msg=str(w))
    assert full > 0


@pytest.mark.parametrize("depth", [1, 2])
def test_linestring_plan_under_the_engine(sf, oracle_mod, depth):
    import linestring_cases as LC
    import poly_cases as PC

    f = np.frompyfunc(oracle_mod.lib().orc_hypot, 2, 1)

    def hyp(a, b):
        with np.errstate(all="ignore"):
            return f(a, b).astype(np.float64)

    name = "zigzag_65"
    g = sf.UniformGrid(LC.GRID_N, *LC.BEIJING)
    x, y, obj, _ = (np.array(a) for a in LC.window(name))
    chain = LC.lines(name)[0]
    d = LC.window_distances(name, 0, hyp)[0]
    ts = spread(len(x), 4)
    k = 7
    c = conf(sf)
    op = sf.SlidingKNNQuery(c, g, sf.LineString(chain, g), LC.KNN_R, k, size_ms=5000, slide_ms=3000, pipeline=depth,
                            op=sf.PointLineStringKNNQuery(c, g))
    s = SC.Stream(x, y, obj, ts, [], 5000, 3000, 1000, 5, 3, -8, 22)
    got = drive(op, dev_batches(sf, s, even_cuts(s)))
    op.close()
    assert [(r.windowStart, r.windowEnd) for r in got] == SC.expected_windows(ts, 5000, 3000) and len(got) >= 7
    for r, (w, m) in zip(got, SC.window_masks(s)):
        eo, ed, ei = LC.ref_knn_pls(PC.Grid(), x[m], y[m], obj[m], chain, LC.KNN_R, k, d[m])
        np.testing.assert_array_equal(r.objID, eo, err_msg=str(w))
        np.testing.assert_array_equal(bits(r.dist), bits(ed), err_msg=str(w))
        np.testing.assert_array_equal(r.idx, ei, err_msg=str(w))


# ---------------------------------------------------------------------------------------------
# several engines on one context
# ---------------------------------------------------------------------------------------------
def interleave(sf, engines):
    """engines: [(op, stream, cuts)]; push batch by batch, alternating; -> each engine's results."""
    its = [iter(list(dev_batches(sf, s, cuts))) for _, s, cuts in engines]
    got = [[] for _ in engines]
    live = list(range(len(engines)))
    while live:
        for j in list(live):
            b = next(its[j], None)
            if b is None:
                engines[j][0].flush()
                live.remove(j)
            else:
                engines[j][0].push(b)
            got[j] += engines[j][0].results()
    return got


def test_two_engines_of_each_kind_interleaved(sf, oracle_mod):
    """Two SlidingKNNQuery and two SlidingRangeQuery, each on its own operator, at different geometries on
    one context, fed alternately: each equals its single-engine reference."""
    k = SC.MATRIX_K
    a = SC.case_stream(oracle_mod, (3000, 2000, "negative", k))
    b = SC.case_stream(oracle_mod, (7000, 2000, "epoch", k))
    engines = [(knn_engine(sf, a, k, 2), a, even_cuts(a, 11)), (knn_engine(sf, b, k, 1), b, even_cuts(b, 9)),
               (range_engine(sf, a, False), a, even_cuts(a, 5)), (range_engine(sf, b, True), b, even_cuts(b, 13))]
    got = interleave(sf, engines)
    for e, _, _ in engines:
        e.close()
    check_knn(got[0], SC.knn_reference(oracle_mod, a, k), "knn a")
    check_knn(got[1], SC.knn_reference(oracle_mod, b, k), "knn b")
    check_range(got[2], SC.range_reference(oracle_mod, a, False), "range a")
    check_range(got[3], SC.range_reference(oracle_mod, b, True), "range b")


def test_range_engines_share_one_plan(sf, oracle_mod):
    """Two SlidingRangeQuery on ONE PointPointRangeQuery and one query set (one cached plan, held twice) at
    two geometries, interleaved; the first is closed half way and the operator's cache is then driven
    past its limit: the second still owns the plan and stays exact."""
    k = SC.MATRIX_K
    a = SC.case_stream(oracle_mod, (3000, 2000, "negative", k))
    b = SC.case_stream(oracle_mod, (7000, 2000, "negative", k))
    g = sf.UniformGrid(100, *BEIJING)
    rop = sf.PointPointRangeQuery(conf(sf), g)
    ea, eb = range_engine(sf, a, False, op=rop), range_engine(sf, b, False, op=rop)
    ba, bb = list(dev_batches(sf, a, even_cuts(a, 8))), list(dev_batches(sf, b, even_cuts(b, 8)))
    got_a, got_b = [], []
    for j in range(4):
        ea.push(ba[j]); got_a += ea.results()
        eb.push(bb[j]); got_b += eb.results()
    assert ea.plan.value == eb.plan.value and rop._plans.holds(eb.plan) == 2
    ea.close()
    assert rop._plans.holds(eb.plan) == 1
    for j in range(rop._plans.limit + 2):           # other queries: the LRU evicts, never the held plan
        rop.plan(0, [sf.Point("p", 116.0 + 0.01 * j, 40.0, 0, g)], 0.02)
    for j in range(4, len(bb)):
        eb.push(bb[j]); got_b += eb.results()
    eb.flush()
    got_b += eb.results()
    eb.close()
    assert rop._plans.holds(eb.plan) == 0
    check_range(got_b, SC.range_reference(oracle_mod, b, False), "the surviving engine")
    ref_a = SC.range_reference(oracle_mod, a, False)
    assert 0 < len(got_a) < len(ref_a)
    check_range(got_a, ref_a[:len(got_a)], "the closed engine, up to its close")


# ---------------------------------------------------------------------------------------------
# the engines' C ABI
# ---------------------------------------------------------------------------------------------
class Raw:
    """One stream cut into device panes, for pushing through the C entry points by hand."""

    def __init__(self, sf, s):
        from spatialflink_amd import _lib

        self.lib, self.L, self.s = _lib, _lib.lib(), s
        self.panes = {}
        ids = s.ts // s.pane
        for p in np.unique(ids):
            m = ids == p
            self.panes[int(p)] = sf.PointWindow.from_numpy(s.x[m], s.y[m], s.obj[m], s.ts[m])
        self.first, self.last = min(self.panes), max(self.panes)
        self.empty = _lib.GfPoints(None, None, None, None, 0)

    def cs(self, p):
        return self.panes[p].c_struct() if p in self.panes else self.empty


def err(raw, ctx):
    return raw.L.gf_ctx_last_error(ctx.handle).decode()


@pytest.mark.parametrize("origin,first", [("negative", -5), ("epoch", 1_700_000_000)])
def test_knn_engine_abi(sf, oracle_mod, origin, first):
    """gf_knn_sliding_push refuses, before any device work: a non-consecutive pane, n = -1, a plan at
    depth 3, a closing window without a record.  After each refusal the engine goes on and every window
    is exact.  The first pane pushed is -5 / 1 700 000 000."""
    import torch
    from spatialflink_amd import _lib

    k, size, slide = SC.MATRIX_K, 3000, 1000
    s0 = SC.case_stream(oracle_mod, (size, slide, "zero", k))
    s = SC.shifted(s0, first * 1000)
    raw = Raw(sf, s)
    assert raw.first == first
    L = raw.L
    g = sf.UniformGrid(100, *BEIJING)
    q = sf.Point("q", *QPOINT, 0, g)
    kop = sf.PointPointKNNQuery(conf(sf), g)
    ctx, plan = kop.plan(0, q, SC.R_KNN, k)
    kop.set_pipeline(0, q, SC.R_KNN, k, 3)
    h = C.c_void_p()
    assert L.gf_knn_sliding_create(plan, size, slide, C.byref(h)) == 0
    pane, W, S, ring = C.c_int64(), C.c_int32(), C.c_int32(), C.c_int32()
    assert L.gf_knn_sliding_geometry(h, C.byref(pane), C.byref(W), C.byref(S), C.byref(ring)) == 0
    assert (pane.value, W.value, S.value, ring.value) == (1000, 3, 1, 9)
    recs = sf.PinnedRecords(ring.value, k)
    closed, end = C.c_int32(), C.c_int64()

    def push(p, cs, slot, rec=True):
        return L.gf_knn_sliding_push(h, p, C.byref(cs), C.c_void_p(recs.ptr(slot)) if rec else None,
                                     C.byref(closed), C.byref(end))

    # depth 3 is refused; at depth 2 the same pane goes in
    assert push(first, raw.cs(first), 0) == _lib.GF_ERR_ARG and "depth" in err(raw, ctx)
    kop.set_pipeline(0, q, SC.R_KNN, k, 2)
    got, nclosed, fired = [], 0, []
    ref = SC.knn_reference(oracle_mod, s, k)
    last_end = ref[-1][0][1]
    p = first
    while p * 1000 < last_end:
        cs = raw.cs(p)
        if p == first + 3:      # out of order, then a negative n, then a closing window without a record
            assert push(p + 1, raw.cs(p + 1), nclosed) == _lib.GF_ERR_ARG and "consecutively" in err(raw, ctx)
            bad = _lib.GfPoints(cs.x, cs.y, cs.objID, cs.ts, -1)
            assert push(p, bad, nclosed) == _lib.GF_ERR_ARG
            assert push(p, cs, nclosed, rec=False) == _lib.GF_ERR_ARG and "null" in err(raw, ctx)
        assert push(p, cs, nclosed) == 0
        if closed.value:
            fired.append((end.value, nclosed % ring.value))
            nclosed += 1
        if len(fired) == 3 or (p + 1) * 1000 >= last_end:   # while the windows' panes are in the ring
            assert L.gf_knn_sliding_flush(h) == 0
            torch.cuda.synchronize()
            for e, slot in fired:
                o, d, i, n = np.empty(k, np.int64), np.empty(k, np.float64), np.empty(k, np.int64), C.c_int32()
                buf = C.create_string_buffer(recs.raw(slot), recs.bytes)
                assert L.gf_knn_sliding_decode(h, e, buf, o.ctypes.data, d.ctypes.data, i.ctypes.data, C.byref(n)) == 0
                got.append((e, o[:n.value].copy(), d[:n.value].copy(), i[:n.value].copy()))
            fired = []
        p += 1
    L.gf_knn_sliding_destroy(h)
    assert [(e - size, e) for e, *_ in got] == [w for w, *_ in ref]
    for (e, o, d, i), (w, _, eo, ed, ei) in zip(got, ref):
        base = int(np.searchsorted(s.ts, w[0]))
        np.testing.assert_array_equal(o, eo, err_msg=str(w))
        np.testing.assert_array_equal(bits(d), bits(ed), err_msg=str(w))
        np.testing.assert_array_equal(i - base, ei, err_msg=str(w))


@pytest.mark.parametrize("origin,first", [("negative", -5), ("epoch", 1_700_000_000)])
def test_range_engine_abi(sf, oracle_mod, origin, first):
    """gf_range_sliding_push: a non-consecutive pane and n = -1 are GF_ERR_ARG; an index buffer below the
    closing window's point count is GF_ERR_CAPACITY with *window_n set, *closed == 0 and nothing enqueued
    -- the same pane pushed again with cap = window_n succeeds and the hits are the oracle's."""
    import torch
    from spatialflink_amd import _lib

    k, size, slide = SC.MATRIX_K, 3000, 2000
    s0 = SC.case_stream(oracle_mod, (size, slide, "zero", k))
    s = SC.shifted(s0, first * 1000)
    raw = Raw(sf, s)
    assert raw.first == first
    L = raw.L
    g = sf.UniformGrid(100, *BEIJING)
    rop = sf.PointPointRangeQuery(conf(sf), g)
    ctx, plan = rop.plan(0, [sf.Point("q", *QPOINT, 0, g)], SC.R_RANGE)
    h = C.c_void_p()
    assert L.gf_range_sliding_create(plan, size, slide, C.byref(h)) == 0
    pane, W, S = C.c_int64(), C.c_int32(), C.c_int32()
    assert L.gf_range_sliding_geometry(h, C.byref(pane), C.byref(W), C.byref(S)) == 0
    assert (pane.value, W.value, S.value) == (1000, 3, 2)
    closed, end, wn = C.c_int32(), C.c_int64(), C.c_int64()
    ref = SC.range_reference(oracle_mod, s, False)
    last_end = ref[-1][0][1]
    got, refused = [], 0

    def push(p, cs, idx, cnt):
        return L.gf_range_sliding_push(h, p, C.byref(cs), idx.data_ptr(), idx.numel(), cnt.data_ptr(), C.byref(closed),
                                       C.byref(end), C.byref(wn))

    one = torch.empty(1, dtype=torch.int32, device="cuda")
    p = first
    while p * 1000 < last_end:
        cs = raw.cs(p)
        cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
        if p == first + 4:
            assert push(p + 1, raw.cs(p + 1), one, cnt) == _lib.GF_ERR_ARG and "consecutively" in err(raw, ctx)
            bad = _lib.GfPoints(cs.x, cs.y, cs.objID, cs.ts, -1)
            assert push(p, bad, one, cnt) == _lib.GF_ERR_ARG
        st = push(p, cs, one, cnt)
        idx = one
        if st == _lib.GF_ERR_CAPACITY:
            w = (int((p + 1) * 1000 - size), int((p + 1) * 1000))
            npts = int(np.count_nonzero((s.ts >= w[0]) & (s.ts < w[1])))
            assert closed.value == 0 and wn.value == npts > 1
            refused += 1
            if npts > 2:   # still too small by one: refused again, nothing changes
                small = torch.empty(npts - 1, dtype=torch.int32, device="cuda")
                assert push(p, cs, small, cnt) == _lib.GF_ERR_CAPACITY and closed.value == 0
            idx = torch.empty(npts, dtype=torch.int32, device="cuda")
            st = push(p, cs, idx, cnt)
        assert st == 0
        if closed.value:
            torch.cuda.synchronize()
            m = int(cnt.item())
            got.append((end.value - size, end.value, idx[:m].cpu().numpy().view(np.uint32).astype(np.int64)))
        p += 1
    L.gf_range_sliding_destroy(h)
    assert refused > 10
    check_range(got, ref, "by hand")


def test_pane_bounds_edges(sf):
    """gf_pane_bounds == np.searchsorted on an epoch-scale column of runs of equal timestamps that straddle
    pane edges (pane - 1, pane, pane repeated), on n = 1 and with npanes = 0."""
    from spatialflink_amd.windows import pane_bounds

    rng = np.random.default_rng(12)
    pane = 1000
    p0 = 1_700_000_000_123 // pane
    edges = (p0 + np.arange(1, 40)) * pane
    ts = np.sort(np.concatenate([np.repeat(edges - 1, 7), np.repeat(edges, 9), np.repeat(edges[::3] + 1, 3),
                                 p0 * pane + rng.integers(0, 40 * pane, 2000) // 50 * 50])).astype(np.int64)
    w = sf.PointWindow.from_numpy(np.zeros(len(ts)), np.zeros(len(ts)), None, ts)
    for pn, first, npanes in ((pane, p0 - 2, 45), (pane, p0 + 5, 0), (50, p0 * 20 + 3, 700), (7, ts[0] // 7, 64)):
        exp = np.searchsorted(ts, (first + np.arange(npanes + 1)) * pn, side="left")
        np.testing.assert_array_equal(pane_bounds(w, pn, first, npanes), exp)
    for t in (edges[0] - 1, edges[0]):
        one = sf.PointWindow.from_numpy(np.zeros(1), np.zeros(1), None, np.array([t], np.int64))
        for first, npanes in ((p0, 3), (p0 + 1, 1), (p0 + 1, 0), (p0 + 2, 0)):
            exp = np.searchsorted([t], (first + np.arange(npanes + 1)) * pane, side="left")
            np.testing.assert_array_equal(pane_bounds(one, pane, first, npanes), exp)
