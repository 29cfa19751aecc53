"""CPU: the tRange / tFilter restatement (tests/trange_ref.py) on a hand vector; literal == closed form and
the cell filter a pure prune on every case; the census of the cases (so a later edit cannot hollow the GPU
tests out); the plan builder's host part under the host sanitizers (a stand-alone program); the mirror's
names, and the entry points refusing bad arguments before any device call (no GPU in this container)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import spatialflink_amd as sf
from spatialflink_amd import _lib

import poly_cases as PC
import trange_cases as TC
import trange_ref as R
from conftest import ROOT


def _grid(case_name):
    n, box = TC.grid_of(case_name)
    return PC.Grid(n, box)


def _all_cases():
    out = dict(TC.extra_cases())
    for name in PC.NAMES:
        out[name] = TC.shape_case(name, "mod")
    return out


CASES = _all_cases()


@pytest.fixture(scope="module")
def contains():
    """contains_matrix per case, computed once and shared"""
    return {k: R.contains_matrix(c[0], c[1], c[4]) for k, c in CASES.items()}


def test_hand_vector():
    x, y, obj, ts, polys = TC.hand_case()
    G = _grid("hand")
    exp = TC.HAND_EXPECT
    assert R.trange_points(x, y, polys).tolist() == exp["points"]
    for got in (R.trange_literal(G, x, y, obj, ts, polys), R.trange_closed(x, y, obj, ts, polys)):
        keys, off, gx, gy, gts, idx = got
        assert keys.tolist() == exp["keys"] and off.tolist() == exp["off"] and idx.tolist() == exp["idx"]
        assert gx.tolist() == [9.0, 1.0, 4.0] and gy.tolist() == [9.0, 1.0, 4.0] and gts.tolist() == [100, 103, 107]
    # the closed polygon (distance <= 0) would also emit 5 and 9, which only touch an edge
    rings = polys[0]
    d0 = PC.polygon_distance(x, y, rings)[0] <= 0.0
    assert sorted(set(obj[d0].tolist())) == [5, 7, 9]
    # tFilter: the set's trajectories whole, in first-occurrence order; absent ids match nothing; empty = all
    keys, off, _, _, _, idx = R.tfilter_ref(x, y, obj, ts, [9, 5, 1234, 9])
    assert keys.tolist() == [5, 9] and off.tolist() == [0, 3, 6] and idx.tolist() == [1, 5, 9, 2, 6, 10]
    assert R.tfilter_ref(x, y, obj, ts, [])[0].tolist() == [7, 5, 9, 3]


@pytest.mark.parametrize("name", sorted(CASES))
def test_literal_equals_closed_form_and_the_filter_removes_nothing(name, contains):
    x, y, obj, ts, polys = CASES[name]
    G, Cm = _grid(name), contains[name]
    lit = R.trange_literal(G, x, y, obj, ts, polys, True, Cm)
    R.assert_csr_equal(lit, R.trange_closed(x, y, obj, ts, polys, Cm))
    R.assert_csr_equal(lit, R.trange_literal(G, x, y, obj, ts, polys, False, Cm))
    # per point too: every contained point passes the cell filter
    assert not (Cm.any(axis=0) & ~R.cell_filter(G, x, y, polys)).any()


def test_grid_edge_case_has_contained_points_outside_the_grid(contains):
    x, y, obj, ts, polys = CASES["grid_edge"]
    G = _grid("grid_edge")
    cx, cy = G.cells(x, y)
    out = ~G.valid(cx, cy)
    Cm = contains["grid_edge"]
    assert (Cm[0] & out).sum() >= 20 and (Cm[0] & ~out).sum() >= 20   # the straddling polygon, both sides
    assert (Cm[1] & out).sum() >= 20 and not (Cm[1] & ~out).any()     # the polygon wholly outside
    assert (Cm[2] & ~out).sum() >= 20
    assert not Cm[:, ~np.isfinite(x) | ~np.isfinite(y)].any()


def test_census():
    """A condition on the cases, not a measurement: with one objID per point every probe decides a row."""
    for name in PC.SHAPES:
        px, py = PC.probes(name)
        polys = PC.polygons(name)
        inside = R.contains_matrix(px, py, polys).any(axis=0)
        bnd = np.zeros(len(px), bool)
        hole = np.zeros(len(px), bool)
        for rings in polys:
            bnd |= R.on_boundary(px, py, rings)
            hole |= R.in_hole_only(px, py, rings)
        assert inside.sum() >= 50, (name, int(inside.sum()))
        assert (bnd & ~inside).sum() >= 50, (name, int((bnd & ~inside).sum()))
        if name in ("holed", "holed_rev", "ngon"):
            assert (hole & ~inside & ~bnd).sum() >= 200, (name, int((hole & ~inside & ~bnd).sum()))
        assert not inside[-4:].any()  # NaN x, NaN y, both, outside the grid
    # collinear_tiled: the probes whose location in their own triangle changes under the plain-double sign
    P, _ = PC.collinear_tiled()
    polys = PC.polygons("collinear_tiled")
    changed = 0
    for q, rings in enumerate(polys):
        a, b = np.array([P[q][0]]), np.array([P[q][1]])
        changed += int(PC.ring_locate(a, b, rings[0])[0] != PC.ring_locate(a, b, rings[0], exact=False)[0])
    assert changed >= 100, changed


# ---- the plan builder's host part, stand-alone under ASan + UBSan ---------------------------------
def _is_rect(rings):
    if len(rings) != 1 or len(rings[0]) != 5:
        return False
    ring = rings[0]
    x1, x2, y1, y2 = PC.envelope(ring)
    if not (x1 < x2 and y1 < y2):
        return False
    corners = set()
    for i, (X, Y) in enumerate(ring):
        if X not in (x1, x2) or Y not in (y1, y2):
            return False
        if i > 0 and (X == ring[i - 1][0]) == (Y == ring[i - 1][1]):
            return False
        if i < 4:
            corners.add((X == x2, Y == y2))
    return len(corners) == 4


def _expected_counts(n, box, polys):
    G = PC.Grid(n, box)
    test = np.zeros((n, n), bool)
    inside = np.zeros((n, n), bool)
    count = np.zeros((n, n), np.int64)
    extras = 0
    for rings in polys:
        bb = PC.shell_bbox(rings)
        (x1, x2), (y1, y2) = (a.tolist() for a in G.cells(np.array([bb[0], bb[2]]), np.array([bb[1], bb[3]])))
        extras += x1 < 0 or y1 < 0 or x2 >= n or y2 >= n
        ys, xs = slice(max(y1, 0), max(min(y2, n - 1) + 1, 0)), slice(max(x1, 0), max(min(x2, n - 1) + 1, 0))
        test[ys, xs] = True
        count[ys, xs] += 1
        if _is_rect(rings):
            inside[slice(max(y1 + 1, 0), max(min(y2 - 1, n - 1) + 1, 0)), slice(max(x1 + 1, 0), max(min(x2 - 1, n - 1) + 1, 0))] = True
    test &= ~inside
    return (int(n * n - test.sum() - inside.sum()), int(test.sum()), int(inside.sum()), int(count[test].sum()), int(extras),
            int(count[test].max()) if test.any() else 0)


def _plan_sets():
    sets = [(name, PC.GRID_N, PC.BEIJING, PC.polygons(name)) for name in PC.SHAPES]
    sets += [(k, *TC.grid_of(k), c[4]) for k, c in TC.extra_cases().items()]
    sets.append(("empty", 7, PC.BEIJING, []))
    sets.append(("one_cell_grid", 1, PC.BEIJING, PC.polygons("holed")))
    return sets


def test_plan_builder_host_part_under_the_host_sanitizers(tmp_path):
    exe = str(tmp_path / "trange_plan_main")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-I/opt/rocm/include",
                    "-D__HIP_PLATFORM_AMD__", os.path.join(ROOT, "tests", "native", "trange_plan_main.cpp"), "-o", exe],
                   check=True)
    sets = _plan_sets()
    lines = [str(len(sets) + 1)]
    for _, n, box, polys in sets:
        lines.append(" ".join([str(n)] + [float(v).hex() for v in box] + [str(len(polys))]))
        for rings in polys:
            lines.append(str(len(rings)))
            for ring in rings:
                lines.append(" ".join([str(len(ring))] + [float(c).hex() for v in ring for c in v]))
    lines.append("4 0x0p+0 0x1p+2 0x0p+0 0x1p+2 1 1 3 0x1p+0 0x1p+0 0x1p+1 0x1p+0 0x1p+0 0x1p+0")  # a 3-vertex ring: refused
    src = tmp_path / "sets.txt"
    src.write_text("\n".join(lines) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1")
    run = subprocess.run([exe, str(src)], capture_output=True, text=True, env=env)
    assert run.returncode == 0, run.stderr[-2000:]
    rows = [tuple(int(v) for v in ln.split()) for ln in run.stdout.strip().splitlines()]
    assert len(rows) == len(sets) + 1
    for (name, n, box, polys), row in zip(sets, rows):
        assert row[0] == 0, name
        assert row[1:] == _expected_counts(n, box, polys), (name, row)
    assert rows[-1][0] == 2
    by_name = {s[0]: r for s, r in zip(sets, rows)}
    assert by_name["inside"][3] > 0 and by_name["grid_edge"][5] >= 2


# ---- the ABI and the mirror --------------------------------------------------------------------------
def _pts(n, objid=1, ts=1):
    return _lib.GfPoints(None, None, objid, ts, n)


def test_entry_points_reject_bad_arguments_without_a_device():
    L = _lib.lib()
    h = C.c_void_p()
    g = sf.UniformGrid(10, *PC.BEIJING)
    empty = _lib.GfPolygons(0, None, None, None, None)
    neg = _lib.GfPolygons(-1, None, None, None, None)
    assert L.gf_trange_plan_create(None, C.byref(g.c_grid), C.byref(empty), C.byref(h)) == _lib.GF_ERR_ARG
    assert L.gf_trange_plan_create(None, C.byref(g.c_grid), C.byref(neg), C.byref(h)) == _lib.GF_ERR_ARG
    assert L.gf_trange_plan_create(None, None, None, None) == _lib.GF_ERR_ARG
    assert h.value is None
    c = [C.c_int64() for _ in range(5)]
    assert L.gf_trange_plan_stats(None, *(C.byref(v) for v in c)) == _lib.GF_ERR_ARG
    assert L.gf_trange_plan_set_thresholds(None, 4) == _lib.GF_ERR_ARG
    assert L.gf_trange_info(None, C.byref(c[0]), C.byref(c[1]), C.byref(c[2]), C.byref(c[3])) == _lib.GF_ERR_ARG
    assert L.gf_trange_points(None, C.byref(_pts(0)), None, None) == _lib.GF_ERR_ARG
    assert L.gf_trange_run(None, None, C.byref(_pts(0)), None, None, 0, None, None, None, None, 0, C.byref(c[0]),
                           C.byref(c[1])) == _lib.GF_ERR_ARG
    assert L.gf_tfilter_run(None, C.byref(_pts(0)), None, 0, None, None, 0, None, None, None, None, 0, C.byref(c[0]),
                            C.byref(c[1])) == _lib.GF_ERR_ARG
    L.gf_trange_plan_destroy(None)  # a no-op


def test_kernel_id_and_mirror_are_exported():
    assert _lib.K_TRANGE == 18
    for name in ("PointPolygonTRangeQuery", "PointTFilterQuery", "TRangePlan"):
        assert hasattr(sf, name) and name in sf.__all__
    assert hasattr(sf.TrajectoryGroups, "trange") and hasattr(sf.TrajectoryGroups, "tfilter")
    for fn in ("gf_trange_plan_create", "gf_trange_points", "gf_trange_run", "gf_tfilter_run"):
        assert fn in _lib.EXPORTS


@pytest.mark.parametrize("qt", [sf.QueryType.CountBased, sf.QueryType.RealTimeNaive])
def test_trange_query_types(qt):
    with pytest.raises(ValueError, match="Not yet support"):
        sf.PointPolygonTRangeQuery(sf.QueryConfiguration(qt), sf.UniformGrid(10, *PC.BEIJING)).run(None, [])
    with pytest.raises(ValueError, match="Not yet support"):
        sf.PointTFilterQuery(sf.QueryConfiguration(qt)).run(None, [])


def test_tfilter_is_window_based_only():
    with pytest.raises(ValueError, match="Not yet support"):
        sf.PointTFilterQuery(sf.QueryConfiguration(sf.QueryType.RealTime)).run(None, [])
