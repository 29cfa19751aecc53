"""GPU: the window-based tJoin -- gf_tjoin_run / gf_tjoin_read_* through TrajectoryGroups.tjoin and
PointPointTJoinQuery -- against the closed form of tests/tjoin_ref.py over the C oracle's point-point join
pairs.  Everything is compared exactly: every row field, both CSRs and gf_tjoin_info's counts.  The windows
(tests/tjoin_cases.py) are the smallest that reach every path: the hand vector, 65 trajectories in one cell
against one (a wave boundary) and its mirror image, the grid's edges, 200k x 50k points of every kind of
key on three grids / radii, a table grown from 16 slots, one cell holding both windows, SINGLE, and one
object reused across windows."""
import ctypes as C
import math

import numpy as np
import pytest

import spatialflink_amd as sf
from spatialflink_amd import _lib

import tjoin_cases as W
import tjoin_ref as R

pytestmark = pytest.mark.gpu

ROW_COLS = ("okey", "qkey", "p_first", "q_latest", "emit", "oslot", "qslot")
CSR_COLS = ("keys", "off", "x", "y", "ts", "idx")
_CACHE = {}


def shared(name, make):
    """a window or an expectation computed once and shared (never written to)"""
    if name not in _CACHE:
        _CACHE[name] = make()
    return _CACHE[name]


def as_bytes(res):
    rows = b"".join(np.ascontiguousarray(getattr(res, c)).tobytes() for c in ROW_COLS)
    csr = b"".join(np.ascontiguousarray(getattr(side, "objID" if c == "keys" else c)).tobytes()
                   for side in (res.ordinary, res.query) for c in CSR_COLS)
    return rows + csr


def check(res, exp):
    """a TJoinResult against tjoin_closed's dict, exactly; -> the result's bytes"""
    info = res.info
    assert (info["rows"], info["emitted"]) == (exp["rows"], exp["emitted"])
    assert (info["otraj"], info["opoints"]) == (len(exp["ordinary"]["keys"]), len(exp["ordinary"]["idx"]))
    assert (info["qtraj"], info["qpoints"]) == (len(exp["query"]["keys"]), len(exp["query"]["idx"]))
    for c in ROW_COLS:
        got = getattr(res, c)
        assert got.dtype == exp[c].dtype, c
        np.testing.assert_array_equal(got, exp[c], err_msg=c)
    for side, e in ((res.ordinary, exp["ordinary"]), (res.query, exp["query"])):
        for c in CSR_COLS:
            got = getattr(side, "objID" if c == "keys" else c)
            assert got.dtype == e[c].dtype, c
            a, b = (got.view(np.int64), e[c].view(np.int64)) if got.dtype == np.float64 else (got, e[c])  # NaN: by bits
            np.testing.assert_array_equal(a, b, err_msg=c)
    assert res.first_point == R.first_point(exp)
    return as_bytes(res)


def oracle_grid(oracle_mod, grid):
    g = grid.c_grid
    return oracle_mod.grid(g.n, g.minX, g.maxX, g.minY, g.maxY)


def expected(oracle_mod, grid, O, Q, r, single=False):
    st, pairs = oracle_mod.join_pp(oracle_grid(oracle_mod, grid), oracle_grid(oracle_mod, grid), O[0], O[1], Q[0], Q[1], r)
    assert st == 0
    return R.tjoin_closed(pairs, O, Q, single), len(pairs)


def groups_of(*windows):
    return [sf.TrajectoryGroups(W.device_window(w)) for w in windows]


def close(*groups):
    for g in groups:
        g.close()


def test_hand_vector(gpu, oracle_mod):
    g = W.small_grid()
    go, gq = groups_of(W.HAND_O, W.HAND_Q)
    res = go.tjoin(gq, g, W.HAND_R)
    got = list(zip(*(getattr(res, c).tolist() for c in ROW_COLS)))
    assert got == [tuple(r) for r in W.HAND_ROWS]
    for side, exp in ((res.ordinary, W.HAND_ORDINARY), (res.query, W.HAND_QUERY)):
        assert {"keys": side.objID.tolist(), "off": side.off.tolist(), "idx": side.idx.tolist()} == exp
    assert res.first_point == W.HAND_FIRST_POINT
    assert res.trajectory_pairs() == [(0, 0), (0, 1), (1, 1)]
    assert res.point_pairs() == [(0, 1), (0, 10), (4, 3), (3, 6), (3, 5)]
    check(res, expected(oracle_mod, g, W.HAND_O, W.HAND_Q, W.HAND_R)[0])
    # the operator class, grouping the windows itself
    q = sf.PointPointTJoinQuery(sf.QueryConfiguration(sf.QueryType.WindowBased), g)
    assert as_bytes(q.run(W.device_window(W.HAND_O), W.device_window(W.HAND_Q), W.HAND_R)) == as_bytes(res)
    close(go, gq)


def _wave65():
    """65 two-point trajectories in cell (3, 3) of the small grid, and one two-point trajectory next to them"""
    rng = np.random.default_rng(65)
    many = (3.2 + 0.6 * rng.random(130), 3.2 + 0.6 * rng.random(130), np.repeat(np.arange(65, dtype=np.int64) * 2 + 1, 2)[rng.permutation(130)],
            rng.integers(0, 9, 130).astype(np.int64))
    one = (np.array([3.5, 3.4]), np.array([3.5, 3.6]), np.array([400, 400], np.int64), np.array([7, 7], np.int64))
    return many, one


@pytest.mark.parametrize("mirror", [False, True])
def test_65_trajectories_in_one_cell_cross_a_wave(gpu, oracle_mod, mirror):
    many, one = _wave65()
    O, Q = (many, one) if mirror else (one, many)
    g = W.small_grid()
    exp, _ = expected(oracle_mod, g, O, Q, 0.5)
    assert exp["rows"] == exp["emitted"] == 65
    go, gq = groups_of(O, Q)
    check(go.tjoin(gq, g, 0.5), exp)
    close(go, gq)


def test_grid_edges(gpu, oracle_mod):
    g = W.small_grid()
    nan = math.nan
    #            outside, on a query point | inside at the border | coincident pairs in two cells | near, not coincident | NaN
    O = (np.array([-0.25, -0.25, 0.25, 0.25, 2.5, 2.5, 6.5, 6.5, 4.5, 4.5, nan, 5.5]),
         np.array([4.5, 4.5, 4.5, 4.5, 2.5, 2.5, 1.5, 1.5, 4.5, 4.5, 5.5, nan]),
         np.array([1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6], np.int64), np.arange(12, dtype=np.int64))
    Q = (np.array([-0.25, -0.25, 2.5, 2.5, 6.5, 6.5, 4.5, 4.5, nan, 5.5, 5.5, 5.5]),
         np.array([4.5, 4.5, 2.5, 2.5, 1.5, 1.5, 4.5000001, 4.5000001, 5.5, nan, 5.5, 5.5]),
         np.array([11, 11, 13, 13, 14, 14, 15, 15, 16, 16, 17, 17], np.int64), np.arange(12, dtype=np.int64) % 5)
    go, gq = groups_of(O, Q)
    for r in (0.75, 0.0):
        exp, _ = expected(oracle_mod, g, O, Q, r)
        res = go.tjoin(gq, g, r)
        check(res, exp)
        rows = list(zip(res.okey.tolist(), res.qkey.tolist()))
        assert all(a != 1 for a, _ in rows)  # the ordinary point outside the grid never matches, even at distance 0
        assert all(a != 6 and b != 16 for a, b in rows)  # NaN never matches
        if r == 0.75:
            assert (2, 11) in rows and (5, 15) in rows  # a query point outside matches across the border
        else:
            assert rows == [(3, 13), (4, 14)]  # only coincident points, whatever their cells
    with pytest.raises(_lib.CandidateLayersError):
        go.tjoin(gq, g, -1.0)
    check(go.tjoin(gq, g, 0.75), expected(oracle_mod, g, O, Q, 0.75)[0])  # the object is usable afterwards
    close(go, gq)


PARITY = {  # grid (bounds, n), r
    "L1": ((W.BEIJING, 100), 0.01),
    "L2": ((W.BEIJING, 200), 0.0106),
    "corner_clipped": (((116.55, 117.6, 40.35, 41.1), 50), 0.012),  # the windows reach far outside this grid
}


def _parity_windows():
    return (shared("O200k", lambda: W.walks(1, 200_000, 20_000, W.BEIJING, 0.004)),
            shared("Q50k", lambda: W.walks(2, 50_000, 6_000, W.BEIJING, 0.004)))


def _parity_expected(oracle_mod, name):
    (bounds, n), r = PARITY[name]
    grid = sf.UniformGrid(n, *bounds)
    O, Q = _parity_windows()
    return grid, r, shared("exp_" + name, lambda: expected(oracle_mod, grid, O, Q, r))


@pytest.mark.parametrize("name", list(PARITY))
def test_oracle_parity_200k_x_50k(gpu, oracle_mod, name):
    grid, r, (exp, npairs) = _parity_expected(oracle_mod, name)
    assert grid.getCandidateNeighboringLayers(r) == (2 if name == "L2" else 1)
    assert 100_000 < npairs < 6_000_000 and exp["rows"] > 10_000 and 0 < exp["emitted"] < exp["rows"]
    go, gq = shared("parity_groups", lambda: groups_of(*_parity_windows()))
    check(go.tjoin(gq, grid, r), exp)


def test_the_plain_joins_pairs_reduce_to_the_same_rows(gpu, oracle_mod):
    grid, r, (exp, npairs) = _parity_expected(oracle_mod, "L1")
    O, Q = _parity_windows()
    go, gq = shared("parity_groups", lambda: groups_of(*_parity_windows()))
    pairs = sf.PointPointJoinQuery(sf.QueryConfiguration(sf.QueryType.WindowBased), grid).run(go.window, gq.window, r)
    assert len(pairs) == npairs
    clo = R.tjoin_closed(pairs, O, Q)
    res = go.tjoin(gq, grid, r)
    for c in ROW_COLS:
        np.testing.assert_array_equal(getattr(res, c), clo[c], err_msg=c)


def test_table_growth_from_16_slots(gpu, oracle_mod):
    O = shared("O6k", lambda: W.walks(3, 6_000, 900, W.BEIJING, 0.004, keys="plain"))
    Q = shared("Q3k", lambda: W.walks(4, 3_000, 500, W.BEIJING, 0.004, keys="plain"))
    grid = W.beijing_grid(20)
    r = 0.1
    exp, _ = expected(oracle_mod, grid, O, Q, r)
    assert 2_000 < exp["rows"] < 60_000
    go, gq = groups_of(O, Q)
    first = go.tjoin(gq, grid, r)
    base = check(first, exp)
    assert first.info["probe_passes"] == 1
    small = go.tjoin(gq, grid, r, table_slots=16)
    assert small.info["probe_passes"] > 1 and check(small, exp) == base
    again = go.tjoin(gq, grid, r, table_slots=0)  # the default again
    assert again.info["probe_passes"] == 1 and as_bytes(again) == base
    close(go, gq)


@pytest.mark.parametrize("ntraj", [4, 300])
def test_one_cell_holds_both_windows(gpu, oracle_mod, ntraj):
    """20k + 20k points in one cell: as 4 x 4 trajectories every insert hits one of 16 rows"""
    O = W.one_cell(10 + ntraj, 20_000, ntraj)
    Q = W.one_cell(20 + ntraj, 20_000, ntraj)
    grid = W.beijing_grid(100)
    r = 0.0005
    exp, npairs = expected(oracle_mod, grid, O, Q, r)
    assert npairs > 300_000 and 0.9 * ntraj * ntraj < exp["rows"] == exp["emitted"] <= ntraj * ntraj
    go, gq = groups_of(O, Q)
    check(go.tjoin(gq, grid, r), exp)
    close(go, gq)


def test_single(gpu, oracle_mod):
    B = W.BEIJING
    inner = (B[0] + 0.1, B[1] - 0.1, B[2] + 0.1, B[3] - 0.1)

    def make():
        x, y, obj, ts = W.walks(5, 20_000, 2_500, inner, 0.003, keys="plain")
        return np.nan_to_num(x, nan=116.5), np.nan_to_num(y, nan=40.3), obj, ts

    Wn = shared("S20k", make)
    grid = W.beijing_grid(100)
    r = 0.015
    assert np.all((Wn[0] > B[0]) & (Wn[0] < B[1]) & (Wn[1] > B[2]) & (Wn[1] < B[3]))  # inside: the join is symmetric
    exp, _ = expected(oracle_mod, grid, Wn, Wn, r, single=True)
    full, _ = expected(oracle_mod, grid, Wn, Wn, r, single=False)
    assert 1_000 < exp["rows"] == full["rows"] - len(np.unique(Wn[2]))  # every trajectory matches itself
    g, g2 = groups_of(Wn, Wn)
    res = g.tjoin(g, grid, r, single=True)
    check(res, exp)
    rows = set(zip(res.okey.tolist(), res.qkey.tolist()))
    assert all(a != b and (b, a) in rows for a, b in rows)
    q = sf.PointPointTJoinQuery(sf.QueryConfiguration(sf.QueryType.WindowBased), grid)
    assert as_bytes(q.runSingle(g.window, r, groups=g)) == as_bytes(res)
    with pytest.raises(ValueError):  # two different groups objects, though of the same window
        g.tjoin(g2, grid, r, single=True)
    check(g.tjoin(g2, grid, r), full)  # PAIR takes them, and the object is usable after the error
    close(g, g2)


def test_reuse_and_determinism(gpu, oracle_mod):
    grid, r, (exp, _) = _parity_expected(oracle_mod, "L1")
    big_o, big_q = (W.device_window(w) for w in _parity_windows())
    go, gq = sf.TrajectoryGroups(big_o), sf.TrajectoryGroups(big_q)
    first = check(go.tjoin(gq, grid, r), exp)
    assert as_bytes(go.tjoin(gq, grid, r)) == first and as_bytes(go.tjoin(gq, grid, r)) == first
    go.regroup(W.device_window(W.HAND_O))
    gq.regroup(W.device_window(W.HAND_Q))
    small = go.tjoin(gq, W.small_grid(), W.HAND_R)
    assert list(zip(*(getattr(small, c).tolist() for c in ROW_COLS))) == [tuple(r_) for r_ in W.HAND_ROWS]
    go.regroup(big_o)
    gq.regroup(big_q)
    assert as_bytes(go.tjoin(gq, grid, r)) == first
    # an empty window on either side: no rows
    empty = tuple(a[:0] for a in W.HAND_O)
    ge = sf.TrajectoryGroups(W.device_window(empty))
    for a, b in ((ge, gq), (go, ge)):
        res = a.tjoin(b, grid, r)
        assert len(res) == 0 and res.info["rows"] == res.info["otraj"] == res.info["qpoints"] == 0
        assert res.ordinary.off.tolist() == [0] and res.query.off.tolist() == [0]
    close(go, gq, ge)


def test_argument_errors_leave_the_object_usable(gpu, oracle_mod):
    g = W.small_grid()
    go, gq = groups_of(W.HAND_O, W.HAND_Q)
    base = as_bytes(go.tjoin(gq, g, W.HAND_R))
    L = _lib.lib()
    h = go._tjoin
    po, pq = go.window.c_struct(), gq.window.c_struct()

    def run(go_=go.handle, po_=po, gq_=gq.handle, pq_=pq, grid=g.c_grid, r=W.HAND_R, mode=_lib.TJOIN_PAIR, out=h):
        return L.gf_tjoin_run(go_, C.byref(po_) if po_ is not None else None, gq_, C.byref(pq_) if pq_ is not None else None,
                              C.byref(grid) if grid is not None else None, r, mode, C.byref(out) if out is not None else None)

    def without(p, col):
        q = _lib.GfPoints(p.x, p.y, p.objID, p.ts, p.n)
        setattr(q, col, None)
        return q

    assert run(r=math.nan) == _lib.GF_ERR_ARG
    assert run(mode=2) == _lib.GF_ERR_ARG and run(mode=-1) == _lib.GF_ERR_ARG
    assert run(go_=None) == _lib.GF_ERR_ARG and run(gq_=None) == _lib.GF_ERR_ARG
    assert run(grid=None) == _lib.GF_ERR_ARG and run(po_=None) == _lib.GF_ERR_ARG and run(pq_=None) == _lib.GF_ERR_ARG
    assert run(out=None) == _lib.GF_ERR_ARG
    for col in ("x", "y", "objID", "ts"):
        assert run(po_=without(po, col)) == _lib.GF_ERR_ARG and run(pq_=without(pq, col)) == _lib.GF_ERR_ARG
    assert run(po_=pq) == _lib.GF_ERR_ARG and run(pq_=po) == _lib.GF_ERR_ARG  # not the grouped windows
    assert run(mode=_lib.TJOIN_SINGLE) == _lib.GF_ERR_ARG  # SINGLE with two groups objects
    other = _lib.Context(0)  # the query window grouped in another context
    h2 = C.c_void_p()
    _lib.check(L.gf_traj_group(other.handle, C.byref(pq), C.byref(h2)), other.handle, "gf_traj_group")
    assert run(gq_=h2) == _lib.GF_ERR_ARG
    L.gf_traj_groups_destroy(h2)
    assert L.gf_tjoin_set_table_slots(h, 24) == _lib.GF_ERR_ARG and L.gf_tjoin_set_table_slots(h, 8) == _lib.GF_ERR_ARG
    assert run() == _lib.GF_OK
    assert as_bytes(go.tjoin(gq, g, W.HAND_R)) == base
    close(go, gq)
