"""GPU: the end of the point kNN scan's loop (knn_scan_body: knn_fused_kernel at depths 2-4,
knn_scan_kernel at depth 1 and in the exact re-evaluation).  Every wave runs the same number of
unchecked U-pair tiles; what is left of the window goes through the bounds-checked tail.  Exact
records (status, objID, distance bits, index) are compared with the oracle's on windows whose sizes
walk the tile boundaries:

    n = 2 (U 512 m + r) + e,  m in {0, 1, 2},  r in {0, 1, 63, 64, 65, 511, 512, U 512 - 1},  e in {0, 1}

and n in {0, 1, 2, 3}, at 2 scanning blocks (512 pairs per step), U in {1, 2, 4} tiles per iteration,
nontemporal loads on and off, depths 1 to 4, hints on and off (T = r).  In every window the nearest
points sit on the very last point, in the tail and in the last unchecked tile; points lie exactly
at distance T on the x axis (the edge of the x band) for the hinted T = 2^-7 and for T = r; a NaN,
a +inf and a -inf x lie in the tail next to an in-band y."""
import ctypes as C

import numpy as np
import pytest

from conftest import BEIJING

pytestmark = pytest.mark.gpu

R = 0.5
K = 8
QD = (116.5, 40.0)  # dyadic query point: q - x is exact for dyadic x
BLOCKS = 2
WSTRIDE = BLOCKS * 256  # pairs per step of the scanning blocks
LANES = {1: 1, 2: 2, 3: 4, 4: 6}
NROLES = K + 8


def sizes(U):
    out = [0, 1, 2, 3]
    for m in (0, 1, 2):
        for r in (0, 1, 63, 64, 65, 511, 512, U * WSTRIDE - 1):
            for e in (0, 1):
                out.append(2 * (U * WSTRIDE * m + r) + e)
    return sorted(set(out))


def make_window(oracle_mod, n, U, seed, obj_base=0):
    """n points, all farther than r from q (y >= qy + 0.6) except the placed ones."""
    x, y = oracle_mod.java_random_points(seed, n, BEIJING[0], BEIJING[1], 40.6, 41.1)
    obj = obj_base + np.arange(n, dtype=np.int64)
    tile = 2 * U * WSTRIDE  # points per tile
    m = (n // 2) // (U * WSTRIDE)
    pt0 = m * tile  # first point of the tail
    rng = np.random.default_rng(seed)

    def uniq(seq, taken=()):
        out = []
        for i in seq:
            i = int(i)
            if 0 <= i < n and i not in out and i not in taken:
                out.append(i)
        return out

    pp = uniq([n - 1, pt0, pt0 + 1] + (list(rng.integers(pt0, n, 12)) if n > pt0 else []))[:9]
    lf = [pt0 - 1, pt0 - 2, 0] + (list(rng.integers(pt0 - tile, pt0, 6)) if m >= 1 else [])
    op = uniq(lf + (list(rng.integers(0, n, 24)) if n else []), pp)
    near = [("near", j) for j in range(K + 1)]
    edge = [("edge", s * t) for t in (2.0 ** -7, R) for s in (1.0, -1.0)]
    roles_pp = [near[0], ("x", np.nan), near[1], ("x", np.inf), edge[0], near[2], ("x", -np.inf), edge[2], near[3]]
    roles_op = near[4:] + [edge[1], edge[3]]
    assert len(roles_pp) + len(roles_op) == NROLES
    roles = roles_pp[:len(pp)] + roles_op + roles_pp[len(pp):]
    for i, (kind, v) in zip(pp + op, roles):
        if kind == "near":  # the K + 1 nearest, the last of them at 2^-8: the next window's hint is 2^-7
            d = 2.0 ** -8 if v == K else (v + 1) * 2.0 ** -12
            x[i], y[i] = (QD[0] + d, QD[1]) if v % 2 == 0 else (QD[0], QD[1] - d)
            if v == 1:
                obj[i] = obj_base + (pp + op)[0]  # the two nearest share an objID: K distinct among K + 1
        elif kind == "edge":  # dx*dx == T*T exactly, dy == 0
            x[i], y[i] = QD[0] + v, QD[1]
        else:
            x[i], y[i] = v, QD[1]
    return x, y, obj


def distinct_within_r(x, y, obj):
    with np.errstate(invalid="ignore", over="ignore"):
        dx, dy = QD[0] - x, QD[1] - y
        return len(np.unique(obj[np.sqrt(dx * dx + dy * dy) <= R]))


@pytest.fixture(scope="module")
def sf(gpu):
    import spatialflink_amd

    return spatialflink_amd


class Windows:
    """Per U: the windows, uploaded once, and the oracle's records, computed once and read-only."""

    def __init__(self, sf, oracle_mod):
        self.sf, self.O = sf, oracle_mod
        self.grid = sf.UniformGrid(500, *BEIJING)
        self.og = oracle_mod.grid(500, *BEIJING)
        self._sets = {}

    def get(self, U):
        if U not in self._sets:
            wins, refs = {}, {}
            for n in sizes(U):
                x, y, obj = make_window(self.O, n, U, 1000 * U + n % 991)
                ref = self.O.knn(self.og, x, y, obj, *QD, R, K)
                assert ref[0] == 0
                # the oracle alone fills the record wherever the window holds the placed points
                assert len(ref[1]) == min(K, distinct_within_r(x, y, obj))
                if n >= 2 * NROLES:
                    assert len(ref[1]) == K and ref[2][K - 1] == 2.0 ** -8
                for a in ref[1:]:
                    a.setflags(write=False)
                wins[n] = self.sf.PointWindow.from_numpy(x, y, obj)
                refs[n] = ref
            self._sets[U] = (wins, refs)
        return self._sets[U]


@pytest.fixture(scope="module")
def windows(sf, oracle_mod):
    return Windows(sf, oracle_mod)


def header(raw):
    from spatialflink_amd import _lib

    return _lib.GfKnnHeader.from_buffer_copy(raw[: C.sizeof(_lib.GfKnnHeader)])


def check(res, ref, what):
    np.testing.assert_array_equal(res.objID, ref[1], err_msg=str(what))
    np.testing.assert_array_equal(res.dist.view(np.int64), ref[2].view(np.int64), err_msg=str(what))
    np.testing.assert_array_equal(res.idx, ref[3], err_msg=str(what))


def lane_order(ns, lanes):
    """every size once; a lane (every lanes-th window) sees a long window, then a short one"""
    ns = sorted(ns)
    short, long_ = ns[: len(ns) // 2], ns[len(ns) // 2:][::-1]
    out = []
    while short or long_:
        for src in (long_, short):
            out += [src.pop(0) for _ in range(min(lanes, len(src)))]
    return out


@pytest.mark.parametrize("depth", [1, 2, 3, 4])
@pytest.mark.parametrize("U", [1, 2, 4])
def test_tile_boundaries(sf, windows, U, depth):
    import torch
    from spatialflink_amd import _lib

    wins, refs = windows.get(U)
    q = sf.Point("q", *QD, 0, windows.grid)
    op = sf.PointPointKNNQuery(sf.QueryConfiguration(sf.QueryType.WindowBased), windows.grid)
    ctx, plan = op.plan(0, q, R, K)
    L = _lib.lib()
    order = lane_order(list(wins), LANES[depth])
    assert len(order) >= 2 * (depth - 1) + 1 and sorted(order) == sorted(wins)
    rec = sf.PinnedRecords(len(order), K)
    try:
        for nt in (0, 1):
            for hint in (1, 0):
                _lib.check(L.gf_knn_plan_set_tuning(plan, BLOCKS, U, nt), ctx.handle, "tuning")
                op.set_pipeline(0, q, R, K, depth)
                _lib.check(L.gf_knn_plan_set_hint(plan, hint), ctx.handle, "hint")
                for i, n in enumerate(order):
                    op.enqueue(wins[n], q, R, K, rec.ptr(i))
                op.flush(0, q, R, K)
                torch.cuda.synchronize()
                final = 0
                for i, n in enumerate(order):
                    what = (U, depth, nt, hint, i, n)
                    raw = rec.raw(i)
                    h = header(raw)
                    if h.status == 0:  # final as written: the raw record itself
                        final += 1
                        st, o, d, ix = sf.spatialOperators.decode_knn_record(raw, K)
                        np.testing.assert_array_equal(o, refs[n][1], err_msg=str(what))
                        np.testing.assert_array_equal(d.view(np.int64), refs[n][2].view(np.int64), err_msg=str(what))
                        np.testing.assert_array_equal(ix, refs[n][3], err_msg=str(what))
                    if not hint or depth == 1:  # T = r: nothing is ever flagged
                        assert h.status == 0 and h.threshold == R, what
                    # a flagged record (a hint below a window that holds fewer than K points) is
                    # re-evaluated exactly, through knn_scan_kernel under the same tuning
                    check(op.finish(wins[n], q, R, K, raw), refs[n], what)
                if hint and depth > 1:  # every window that holds the K nearest within 2^-7 of a warm lane
                    assert final >= len([n for n in order if n >= 2 * NROLES]) - 2 * LANES[depth], (U, depth, nt, final)
    finally:
        op.set_pipeline(0, q, R, K, 1)
        op._plans.close()
        rec.__del__()


@pytest.mark.parametrize("U", [1, 2, 4])
def test_odd_panes_through_the_sliding_engine(sf, oracle_mod, windows, U):
    """The pane engine scans sub-ranges of the stream: panes of odd sizes, so every later pane
    starts at an odd stream position (its index base), each scanned once at depth 2 and merged
    into the windows that hold it."""
    from spatialflink_amd import _lib

    g = windows.grid
    q = sf.Point("q", *QD, 0, g)
    ns = [2 * (U * WSTRIDE + 65) + 1, 2 * 511 + 1, 3, 2 * (2 * U * WSTRIDE + U * WSTRIDE - 1) + 1, 1,
          2 * (U * WSTRIDE + 512) + 1, 2 * 63 + 1]
    data = [make_window(oracle_mod, n, U, 77 + j, obj_base=100_000 * (j + 1)) for j, n in enumerate(ns)]
    for nt in (0, 1):
        op = sf.SlidingKNNQuery(sf.QueryConfiguration(sf.QueryType.WindowBased), g, q, R, K, size_ms=3000,
                                slide_ms=1000, pipeline=2)
        _lib.check(_lib.lib().gf_knn_plan_set_tuning(op.plan, BLOCKS, U, nt), op.ctx.handle, "tuning")
        for p, (x, y, obj) in enumerate(data):
            op.push_pane(10 + p, sf.PointWindow.from_numpy(x, y, obj))
        op.flush()
        got = op.results()
        assert len(got) == len(ns) + 2
        for r in got:
            panes = [p for p in range(len(ns)) if r.windowStart <= 1000 * (10 + p) < r.windowEnd]
            x, y, obj = (np.concatenate([data[p][c] for p in panes]) for c in range(3))
            st, eo, ed, ei = oracle_mod.knn(windows.og, x, y, obj, *QD, R, K)
            assert st == 0 and len(eo) == K
            what = (U, nt, r.windowStart)
            np.testing.assert_array_equal(r.objID, eo, err_msg=str(what))
            np.testing.assert_array_equal(r.dist.view(np.int64), ed.view(np.int64), err_msg=str(what))
            np.testing.assert_array_equal(r.idx, ei, err_msg=str(what))
