"""CPU: tAggregate's closed forms (include/geoflink_hip.h, what the kernels compute) against the literal
transcription of TimeWindowProcessFunction.process (tests/tagg_ref.py), the pure-host row rules
(gf_tagg_rows) against the reference's emission code for every aggregate name, and the argument
checks of the entry points that need no device."""
import ctypes as C
import random

import numpy as np
import pytest

import spatialflink_amd as sf
from spatialflink_amd import _lib

import tagg_ref as R


def _random_cell(rng):
    """a small cell with few objIDs and a tiny ts range: ties of every kind are the rule"""
    m = rng.randint(1, 14)
    nobj = rng.randint(1, 5)
    span = rng.choice([1, 2, 3, 6, 50])
    return [(rng.randint(0, nobj - 1) * 7 - 3, rng.randint(0, span)) for _ in range(m)]


def test_closed_forms_match_the_literal_loop():
    rng = random.Random(20240611)
    for _ in range(4000):
        pts = _random_cell(rng)
        base = rng.randint(0, 1000)  # window indices: ascending, not contiguous
        idx = sorted(rng.sample(range(base, base + 3 * len(pts)), len(pts)))
        lit = R.cell_loop(pts)
        clo = R.cell_closed([(i, o, t) for i, (o, t) in zip(idx, pts)])
        for k in ("count", "sum", "minLen", "minKey", "maxLen", "maxKey"):
            assert lit[k] == clo[k], (k, pts)
        assert list(lit["lengths"].items()) == list(clo["lengths"].items()), pts
        assert (clo["multi"] > 0) == (lit["minLen"] != R.LONG_MAX) == (lit["maxLen"] != R.LONG_MIN)


def test_hand_vector():
    # objID 5: ts 10, 10, 40 -> e = 0 (second point), L = 30 reached at its third point (index 4)
    # objID 9: ts 50, 20     -> e = L = 30 reached at its second point (index 3): the MAX winner
    pts = [(5, 10), (9, 50), (5, 10), (9, 20), (5, 40), (7, 99)]
    lit = R.cell_loop(pts)
    assert (lit["count"], lit["sum"]) == (3, 60)
    assert (lit["minLen"], lit["minKey"]) == (0, 5)
    assert (lit["maxLen"], lit["maxKey"]) == (30, 9)
    assert list(lit["lengths"].items()) == [(5, 30), (9, 30), (7, 0)]
    assert R.rows_of("avg", lit) == ("AVG", None, 20)
    assert R.rows_of("Min", lit) == ("MIN", 5, 0)


def _table(cells, multi):
    z = lambda k: np.array([c[k] if c[k] is not None else 0 for c in cells], np.int64)  # noqa: E731
    return dict(count=z("count"), multi=np.array(multi, np.int64), sum=z("sum"), minLen=z("minLen"), minKey=z("minKey"),
                maxLen=z("maxLen"), maxKey=z("maxKey"))


@pytest.mark.parametrize("name", ["ALL", "SUM", "AVG", "MIN", "MAX", "sum", "aVg", "Min", "mAX", "all", "median", ""])
def test_rows_function_matches_the_reference(name):
    rng = random.Random(7)
    cells_pts = [_random_cell(rng) for _ in range(600)]
    cells_pts += [
        [(1, 5)],                                   # one point: sum 0, no repeat
        [(1, 5), (2, 5), (3, 9)],                   # no repeat objID
        [(1, 5), (1, 5)],                           # a repeat with length 0: sum 0 but MIN / MAX emit
        [(1, 0), (1, 5), (2, 0)],                   # 5 / 2 = 2.5 -> 3
        [(1, 0), (1, 7), (2, 0)],                   # 3.5 -> 4
        [(1, 0), (1, 1), (2, 0)],                   # 0.5 -> 1
        [(1, 0), (1, 1), (2, 0), (3, 0)],           # 1 / 3 -> 0
        [(1, 0), (1, (1 << 53) + 1), (2, 0)],       # (2^53 + 1) / 2: (double)sum rounds first
        [(1, 0), (1, 9007199254740993), (2, 3), (2, 4), (3, 0)],
    ]
    cells = [R.cell_loop(p) for p in cells_pts]
    multi = [R.cell_closed([(i, o, t) for i, (o, t) in enumerate(p)])["multi"] for p in cells_pts]
    kind, emit, value, key = sf.tagg_rows(name, _table(cells, multi))
    exp = [R.rows_of(name, c) for c in cells]
    assert kind == (name.upper() if name.upper() in ("SUM", "AVG", "MIN", "MAX") else "ALL")
    assert emit.tolist() == [r is not None for r in exp]
    for j, r in enumerate(exp):
        if r is None:
            assert (value[j], key[j]) == (0, 0)
        elif r[0] == "ALL":
            assert (value[j], key[j]) == (cells[j]["sum"], 0)
        else:
            assert (r[0], value[j], key[j]) == (kind, r[2], r[1] or 0), (name, cells_pts[j])


def test_avg_rounds_half_up_of_the_binary64_quotient():
    # quotients ending exactly in .5, just below and just above (the quotient itself is rounded to binary64 first)
    cases = [(5, 2), (7, 2), (1, 2), (2**52 + 1, 2), (2**53 - 1, 2), (10, 4), (9999999999999999, 2),
             (4999999999999999, 10000000000000000), (1, 3), (2, 3), (2**62, 3), (2**63 - 1, 1), (2**63 - 1, 2)]
    t = dict(count=[c for _, c in cases], multi=[0] * len(cases), sum=[s for s, _ in cases], minLen=[0] * len(cases),
             minKey=[0] * len(cases), maxLen=[0] * len(cases), maxKey=[0] * len(cases))
    kind, emit, value, _ = sf.tagg_rows("AVG", t)
    assert kind == "AVG" and emit.all()
    for (s, c), v in zip(cases, value.tolist()):
        assert v == min(R.java_round(float(s) / float(c)), R.LONG_MAX), (s, c)
    assert value[0] == 3 and value[1] == 4 and value[2] == 1 and value[7] == 0


def _pts(n, x=16, y=16, objid=16, ts=16):
    return _lib.GfPoints(x, y, objid, ts, n)


def test_entry_points_reject_bad_arguments_without_a_device():
    L = _lib.lib()
    h = C.c_void_p()
    grid = sf.UniformGrid(10, 0.0, 1.0, 0.0, 1.0)
    g = C.byref(grid.c_grid)
    assert L.gf_tagg_group(None, g, C.byref(_pts(0)), C.byref(h)) == _lib.GF_ERR_ARG  # a null context is refused first
    assert h.value is None
    assert L.gf_tagg_group(None, g, None, C.byref(h)) == _lib.GF_ERR_ARG
    assert L.gf_tagg_group(None, None, C.byref(_pts(0)), C.byref(h)) == _lib.GF_ERR_ARG
    assert L.gf_tagg_group(None, g, C.byref(_pts(0)), None) == _lib.GF_ERR_ARG
    assert L.gf_tagg_group(None, g, C.byref(_pts(-1)), C.byref(h)) == _lib.GF_ERR_ARG
    assert L.gf_tagg_group(None, g, C.byref(_pts(1 << 32)), C.byref(h)) == _lib.GF_ERR_ARG
    for col in ("x", "y", "objid"):
        assert L.gf_tagg_group(None, g, C.byref(_pts(5, **{col: None})), C.byref(h)) == _lib.GF_ERR_ARG
    assert L.gf_tagg_run(None, C.byref(_pts(0))) == _lib.GF_ERR_ARG
    a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
    assert L.gf_tagg_info(None, C.byref(a), C.byref(b), C.byref(c)) == _lib.GF_ERR_ARG
    assert L.gf_tagg_set_thresholds(None, 1, 1) == _lib.GF_ERR_ARG
    assert L.gf_tagg_read_cells(None, *([None] * 9), 0, C.byref(a)) == _lib.GF_ERR_ARG
    assert L.gf_tagg_read_all(None, None, None, None, 0, 0, C.byref(a), C.byref(b)) == _lib.GF_ERR_ARG
    L.gf_tagg_destroy(None)  # a no-op
    # gf_tagg_rows: null name / outputs / the columns its aggregate reads
    z = np.zeros(2, np.int64)
    e = np.zeros(2, np.uint8)
    p = z.ctypes.data
    assert L.gf_tagg_rows(None, 2, p, p, p, p, p, p, p, e.ctypes.data, p, p, None) == _lib.GF_ERR_ARG
    assert L.gf_tagg_rows(b"SUM", 2, p, p, p, p, p, p, p, None, p, p, None) == _lib.GF_ERR_ARG
    assert L.gf_tagg_rows(b"SUM", -1, p, p, p, p, p, p, p, e.ctypes.data, p, p, None) == _lib.GF_ERR_ARG
    assert L.gf_tagg_rows(b"SUM", 2, p, p, None, p, p, p, p, e.ctypes.data, p, p, None) == _lib.GF_ERR_ARG
    assert L.gf_tagg_rows(b"AVG", 2, None, p, p, p, p, p, p, e.ctypes.data, p, p, None) == _lib.GF_ERR_ARG
    assert L.gf_tagg_rows(b"MIN", 2, p, p, p, None, p, p, p, e.ctypes.data, p, p, None) == _lib.GF_ERR_ARG
    assert L.gf_tagg_rows(b"MAX", 2, p, p, p, p, p, p, None, e.ctypes.data, p, p, None) == _lib.GF_ERR_ARG
    assert L.gf_tagg_rows(b"SUM", 0, None, None, None, None, None, None, None, e.ctypes.data, p, p, None) == _lib.GF_OK


def test_kernel_id_and_mirror_are_exported():
    assert _lib.K_TAGG == 15
    for name in ("PointTAggregateQuery", "TAggregateResult", "TAggregateGroups", "tagg_rows"):
        assert hasattr(sf, name) and name in sf.__all__
        assert name in sf.spatialOperators.__all__


@pytest.mark.parametrize("qt", [sf.QueryType.RealTime, sf.QueryType.CountBased, sf.QueryType.RealTimeNaive])
def test_taggregate_is_window_based_only(qt):
    with pytest.raises(ValueError, match="Not yet support"):
        sf.PointTAggregateQuery(sf.QueryConfiguration(qt)).run(None, "ALL")


@pytest.mark.parametrize("wt", ["COUNT", "count", "Count"])
def test_count_windows_are_refused(wt):
    with pytest.raises(ValueError, match="Not yet support"):
        sf.PointTAggregateQuery(sf.QueryConfiguration(sf.QueryType.WindowBased)).run(None, "ALL", wt)
