"""GPU: the kNN scan reads x first and y only for lanes whose x lies inside the threshold band
(knn_scan_body, shared by knn_fused_kernel at depths 2-4 and knn_scan_kernel at depth 1).  The
band test is exact -- fl(dx*dx) <= fl(fl(dx*dx) + fl(dy*dy)) without contraction -- so the set of
appended candidates, and with it every record, is what reading both columns gave.  Checked here
bit-exactly against the oracle on hinted windows (a tight T needs n >= 2^20 points): points
exactly on the band edge, per-lane shapes, every loop shape (main loop, checked tail, odd last
element) under every tuning the kernels instantiate, and every consumer of the loop."""
import ctypes as C

import numpy as np
import pytest

from conftest import BEIJING, QPOINT

pytestmark = pytest.mark.gpu

N0 = 1 << 20  # kSampleMinN: the smallest window that takes a threshold below r
R = 0.5
QD = (116.5, 40.0)  # dyadic query point: q - x is exact for dyadic x
ORIGIN = (-1.05, 1.05, -0.75, 0.75)  # a grid around (0, 0): room for -0.0 coordinates
LANES = {1: 1, 2: 2, 3: 4, 4: 6}  # hint lanes of a plan per pipeline depth


@pytest.fixture(scope="module")
def sf(gpu):
    import spatialflink_amd

    return spatialflink_amd


def conf(sf, metric=0):
    c = sf.QueryConfiguration(sf.QueryType.WindowBased)
    c.distanceMetric = metric
    return c


def filler(oracle_mod, seed, n, bounds, q, clear=0.06):
    """n uniform points, none within `clear` (Chebyshev) of q: far beyond any hinted T."""
    x, y = oracle_mod.java_random_points(seed, n, *bounds)
    near = (np.abs(x - q[0]) < clear) & (np.abs(y - q[1]) < clear)
    y[near] += 0.2
    return x, y


def header(raw):
    from spatialflink_amd import _lib

    return _lib.GfKnnHeader.from_buffer_copy(raw[: C.sizeof(_lib.GfKnnHeader)])


def check(res, ref):
    st, oo, od, oi = ref
    assert st == 0
    np.testing.assert_array_equal(res.objID, oo)
    np.testing.assert_array_equal(res.dist.view(np.int64), od.view(np.int64))
    np.testing.assert_array_equal(res.idx, oi)


def check_raw(sf, raw, k, ref):
    st, o, d, i = sf.spatialOperators.decode_knn_record(raw, k)
    assert st == 0
    np.testing.assert_array_equal(o, ref[1])
    np.testing.assert_array_equal(d.view(np.int64), ref[2].view(np.int64))
    np.testing.assert_array_equal(i, ref[3])


def run_ring(sf, op, q, k, depth, wins, order):
    """enqueue wins[j] for j in order at the given depth -> the raw records"""
    import torch

    op.set_pipeline(0, q, R, k, depth)
    rec = sf.PinnedRecords(len(order), k)
    try:
        for i, j in enumerate(order):
            op.enqueue(wins[j], q, R, k, rec.ptr(i))
        op.flush(0, q, R, k)
        torch.cuda.synchronize()
        return [rec.raw(i) for i in range(len(order))]
    finally:
        op.set_pipeline(0, q, R, k, 1)


def n_candidates(x, y, q, T):
    """points within T of q (metric 0: s <= smax(T) <=> sqrt(s) <= T; numpy never contracts)"""
    dx, dy = q[0] - x, q[1] - y
    with np.errstate(invalid="ignore", over="ignore"):
        return int(np.count_nonzero(np.sqrt(dx * dx + dy * dy) <= T))


K = 16
T2 = 2.0 ** -7  # the hint the first window leaves: 2 x its k-th distance 2^-8


def hint_window(oracle_mod, n, bounds=BEIJING, q=QD, seed=11):
    """k-th neighbour exactly at 2^-8, the others closer, everything else far."""
    x, y = filler(oracle_mod, seed, n, bounds, q)
    at = np.arange(K) * 4099 + 77
    x[at[:-1]] = q[0] + np.arange(1, K) * 2.0 ** -12
    y[at[:-1]] = q[1]
    x[at[-1]], y[at[-1]] = q[0] + 2.0 ** -8, q[1]
    return x, y, np.arange(n, dtype=np.int64)


@pytest.fixture(scope="module")
def hint_win(sf, oracle_mod):
    x, y, obj = hint_window(oracle_mod, N0 + 1234)
    return sf.PointWindow.from_numpy(x, y, obj)


@pytest.mark.parametrize("outward", [False, True])
@pytest.mark.parametrize("depth", [1, 2, 3])
def test_points_exactly_on_the_band_edge(sf, oracle_mod, hint_win, depth, outward):
    """Second window: k - 3 objIDs well inside T = 2^-7 and three points exactly at distance T,
    at (qx +- T, qy) -- dx*dx == T*T, the edge of the x band -- and (qx, qy + T).  The raw record
    is final (status 0) BEFORE decode and equals the oracle's.  With the three moved outward by
    one ulp only k - 3 lie below T: the record is flagged, and decode's re-evaluation equals the
    oracle."""
    g = sf.UniformGrid(500, *BEIJING)
    og = oracle_mod.grid(500, *BEIJING)
    q = sf.Point("q", *QD, 0, g)
    n = N0 + 4321
    x, y = filler(oracle_mod, 12, n, BEIJING, QD)
    obj = np.arange(n, dtype=np.int64)
    inner = np.arange(K - 3) * 70001 + 5
    x[inner] = QD[0] - np.arange(1, K - 2) * 2.0 ** -12
    y[inner] = QD[1] + np.arange(1, K - 2) * 2.0 ** -13
    edge = np.array([640_000, 640_001, n - 1])  # an even/odd pair of one lane, and the last point
    ex = np.array([QD[0] + T2, QD[0] - T2, QD[0]])
    ey = np.array([QD[1], QD[1], QD[1] + T2])
    if outward:
        ex = np.array([np.nextafter(ex[0], np.inf), np.nextafter(ex[1], -np.inf), ex[2]])
        ey[2] = np.nextafter(ey[2], np.inf)
    x[edge], y[edge] = ex, ey
    assert n_candidates(x, y, QD, T2) == (K - 3 if outward else K)
    w2 = sf.PointWindow.from_numpy(x, y, obj)
    ref = oracle_mod.knn(og, x, y, obj, *QD, R, K)
    op = sf.PointPointKNNQuery(conf(sf), g)
    lanes = LANES[depth]
    raws = run_ring(sf, op, q, K, depth, [hint_win, w2], [0] * lanes + [1] * lanes)
    for raw in raws[:lanes]:
        assert header(raw).status == 0
    for raw in raws[lanes:]:
        h = header(raw)
        assert h.threshold == T2, "the first window must leave the hint 2^-7"
        if outward:
            assert h.status != 0 and h.candidates == K - 3
        else:
            assert h.status == 0 and h.candidates == K
            check_raw(sf, raw, K, ref)
        check(op.finish(w2, q, R, K, raw), ref)


@pytest.mark.parametrize("where", ["beijing", "origin"])
@pytest.mark.parametrize("depth", [1, 2])
def test_per_lane_shapes(sf, oracle_mod, where, depth):
    """Lanes whose even or odd point alone is in the band, a vertical line x = qx (every lane
    loads y, nearly all fail), a horizontal line y = qy (x alone decides), NaN / +-inf in either
    column next to an in-band value in the other, and -0.0 coordinates around a query at 0."""
    bounds, qp = (BEIJING, QD) if where == "beijing" else (ORIGIN, (0.0, 0.0))
    g = sf.UniformGrid(500, *bounds)
    og = oracle_mod.grid(500, *bounds)
    q = sf.Point("q", *qp, 0, g)
    n = N0 + 2 * 4097 + 1
    x1, y1, o1 = hint_window(oracle_mod, n, bounds, qp, seed=21)
    w1 = sf.PointWindow.from_numpy(x1, y1, o1)
    x, y = filler(oracle_mod, 22, n, bounds, qp)
    obj = np.arange(n, dtype=np.int64)
    nan, inf = np.nan, np.inf
    e = 2.0 ** -10
    for j in range(40):  # only the even / only the odd point of a lane's pair
        i = 2 * (3000 + 129 * j) + (j & 1)
        x[i], y[i] = qp[0] + (j + 1) * 2.0 ** -14, qp[1] - (j + 1) * 2.0 ** -15
    m = 2048
    v0, h0 = 200_000, 500_001  # whole waves of line points; the horizontal line starts odd
    x[v0:v0 + m], y[v0:v0 + m] = qp[0], qp[1] + np.linspace(-0.3, 0.3, m)
    obj[v0:v0 + m] = 7_000_000 + np.arange(m) % 40  # duplicated objIDs among the nearest
    x[h0:h0 + m], y[h0:h0 + m] = qp[0] + np.linspace(-0.3, 0.3, m), qp[1]
    sp = [(qp[0] + e, nan), (qp[0], inf), (qp[0] - e, -inf), (nan, qp[1]), (inf, qp[1]), (-inf, qp[1] + e),
          (nan, nan), (qp[0] + e, qp[1] + e)]
    if where == "origin":
        sp += [(-0.0, e), (e, -0.0), (-0.0, -0.0), (-e, -0.0), (-0.0, nan)]
    for j, (sx, sy) in enumerate(sp):
        i = 800_000 + 3 * j  # alternating parity
        x[i], y[i] = sx, sy
    x[n - 1], y[n - 1] = qp[0] - 3 * 2.0 ** -11, qp[1]  # the odd last element, in the band
    w = sf.PointWindow.from_numpy(x, y, obj)
    ref = oracle_mod.knn(og, x, y, obj, *qp, R, K)
    op = sf.PointPointKNNQuery(conf(sf), g)
    lanes = LANES[depth]
    raws = run_ring(sf, op, q, K, depth, [w1, w], [0] * lanes + [1] * lanes)
    for raw in raws[lanes:]:
        h = header(raw)
        assert h.threshold == T2 and h.status == 0
        assert h.candidates == n_candidates(x, y, qp, T2)
        check_raw(sf, raw, K, ref)
        check(op.finish(w, q, R, K, raw), ref)


# every tile size the kernels instantiate (512 * unroll * scan_blocks points) divides TILES
TILES = 512 * 8 * 3 * 86  # 1,056,768 >= 2^20


@pytest.mark.parametrize("n", [N0, N0 + 1, TILES + 1, TILES + 2 * 37])
def test_loop_shapes(sf, oracle_mod, n):
    """scan_blocks 1 and 3, every unroll (the fused kernel runs 1, 2, 4; the scan kernel also 8),
    nontemporal loads on and off, depth 1 (knn_scan_kernel) and 2 (knn_fused_kernel).  In-band
    points sit in the main loop, in the checked tail, in a partial last wave and in the odd last
    element.  The window is evaluated twice per lane: cold, then under its own hint."""
    from spatialflink_amd import _lib

    g = sf.UniformGrid(500, *BEIJING)
    og = oracle_mod.grid(500, *BEIJING)
    q = sf.Point("q", *QD, 0, g)
    x, y = filler(oracle_mod, 31, n, BEIJING, QD)
    obj = np.arange(n, dtype=np.int64)
    rng = np.random.default_rng(n)
    at = np.concatenate([rng.choice(n - 200, 24, replace=False), np.arange(n - 40, n)])
    x[at] = QD[0] + rng.integers(-31, 32, len(at)) * 2.0 ** -13
    y[at] = QD[1] + rng.integers(-31, 32, len(at)) * 2.0 ** -13
    obj[at[::3]] = 9_000_000 + np.arange(len(at[::3])) % 5  # some duplicated objIDs
    w = sf.PointWindow.from_numpy(x, y, obj)
    ref = oracle_mod.knn(og, x, y, obj, *QD, R, K)
    dk = ref[2][K - 1]
    op = sf.PointPointKNNQuery(conf(sf), g)
    ctx, plan = op.plan(0, q, R, K)
    L = _lib.lib()
    try:
        for depth in (1, 2):
            lanes = LANES[depth]
            for blocks in (1, 3):
                for unroll in (1, 2, 4, 8):
                    for nt in (0, 1):
                        _lib.check(L.gf_knn_plan_set_tuning(plan, blocks, unroll, nt), ctx.handle, "tuning")
                        raws = run_ring(sf, op, q, K, depth, [w], [0] * (2 * lanes))
                        for raw in raws[lanes:]:
                            h = header(raw)
                            what = (depth, blocks, unroll, nt)
                            assert h.status == 0 and h.threshold == 2.0 * dk, what
                            assert h.candidates == n_candidates(x, y, QD, 2.0 * dk), what
                            check_raw(sf, raw, K, ref)
    finally:
        _lib.check(L.gf_knn_plan_set_tuning(plan, 0, 2, 1), ctx.handle, "tuning")


@pytest.fixture(scope="module")
def ring(sf, oracle_mod):
    """three distinct uniform windows with duplicated objIDs, and their oracle records per metric"""
    og = oracle_mod.grid(500, *BEIJING)
    data, refs = [], {}
    for j in range(3):
        n = N0 + 1000 * j + j
        x, y = oracle_mod.java_random_points(50 + j, n, *BEIJING)
        obj = (np.random.default_rng(j).permutation(n) % (2 * n // 3)).astype(np.int64)
        data.append((x, y, obj, sf.PointWindow.from_numpy(x, y, obj)))
        for metric in (0, 1):
            refs[j, metric] = oracle_mod.knn(og, x, y, obj, *QPOINT, R, 50, metric=metric)
    return data, refs


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("depth", [1, 2, 3, 4])
def test_every_depth_and_metric(sf, ring, depth, metric):
    """A ring of three distinct windows: every lane's hint is validated on fresh data.  Once each
    lane carries a hint the raw records are final, and every record equals the oracle's."""
    data, refs = ring
    g = sf.UniformGrid(500, *BEIJING)
    q = sf.Point("q", *QPOINT, 0, g)
    op = sf.PointPointKNNQuery(conf(sf, metric), g)
    lanes = LANES[depth]
    order = [(i % lanes + i // lanes) % 3 for i in range(3 * lanes)]  # a lane never meets a window twice in a row
    raws = run_ring(sf, op, q, 50, depth, [d[3] for d in data], order)
    for i, j in enumerate(order):
        if i >= lanes:
            assert header(raws[i]).status == 0, f"window {i} was not final under its lane's hint"
            assert header(raws[i]).threshold < R
            check_raw(sf, raws[i], 50, refs[j, metric])
        check(op.finish(data[j][3], q, R, 50, raws[i]), refs[j, metric])


def test_cold_plan(sf, ring):
    """Hints off: every window takes its threshold from the sample kernel (use_state 2)."""
    from spatialflink_amd import _lib

    data, refs = ring
    g = sf.UniformGrid(500, *BEIJING)
    q = sf.Point("q", *QPOINT, 0, g)
    op = sf.PointPointKNNQuery(conf(sf), g)
    ctx, plan = op.plan(0, q, R, 50)
    _lib.check(_lib.lib().gf_knn_plan_set_hint(plan, 0), ctx.handle, "hint")
    for depth in (1, 3):
        order = [0, 1, 2, 1, 0, 2]
        raws = run_ring(sf, op, q, 50, depth, [d[3] for d in data], order)
        for i, j in enumerate(order):
            assert header(raws[i]).threshold < R
            check(op.finish(data[j][3], q, R, 50, raws[i]), refs[j, 0])
