"""CPU: the geometry-window restatement (tests/geomwin_ref.py) -- literal == closed form on every case, the
HashSet walk independent of its iteration order, the rectangle rules on hand-built objects; the
summed-area rectangle sums of gf_geom_plan.hpp against brute force under the host sanitizers (a
stand-alone program); the entry points refusing bad arguments before any device call (no GPU in this
container); the exports, the mirror's names and its host-side offset validation."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import spatialflink_amd as sf
from spatialflink_amd import _lib
from spatialflink_amd.spatialObjects import validate_geom_offsets

import geomwin_cases as GC
import geomwin_ref as R
from conftest import ROOT

CASES = {"rules": GC.rules, "holes": GC.holes, "rings": GC.rings, "lines": GC.lines,
         "poly_257": lambda: GC.sized(GC.POLYGON, 257), "line_257": lambda: GC.sized(GC.LINESTRING, 257)}


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("approximate", [False, True])
def test_literal_equals_closed_form_in_any_cell_order(name, approximate, oracle_mod):
    case = CASES[name]()
    g = R.grid_of(*case["grid"])
    rnd = random.Random(5)
    for qname, (qx, qy) in case["queries"].items():
        for metric in (0, 1):
            for r in R.case_radii(case, qx, qy, metric, approximate):
                lit = R.range_literal(g, case["kind"], case["objs"], qx, qy, r, approximate, metric)
                closed = R.range_closed_form(g, case["kind"], case["objs"], qx, qy, r, approximate, metric)
                assert np.array_equal(lit, closed), (name, qname, metric, r)
                assert len(set(lit.tolist())) == len(lit)  # each object once
                shuffled = R.range_literal(g, case["kind"], case["objs"], qx, qy, r, approximate, metric, order=rnd.shuffle)
                assert np.array_equal(lit, shuffled), (name, qname, metric, r)


def test_rectangle_rules_on_the_hand_built_objects(oracle_mod):
    case = GC.rules()
    g = R.grid_of(*case["grid"])
    run = lambda q, r, **kw: set(R.range_literal(g, GC.POLYGON, case["objs"], *case["queries"][q], r, **kw).tolist())  # noqa: E731
    info = {}
    one = set(R.range_literal(g, GC.POLYGON, case["objs"], *case["queries"]["one"], GC.R_G1, info=info).tolist())
    assert 0 in one and info["all_guaranteed"] > 0          # inside G cells: emitted untested
    assert 1 not in one                                     # spans G and non-G cells, its geometry 3.39 > r away
    assert R.distance(GC.POLYGON, case["objs"][1], 5.5, 5.5) > GC.R_G1
    borders = run("borders", GC.R_G0)
    assert {2, 3, 4, 5} <= borders                          # leave the grid: filtered in through their in-grid cells
    assert 6 not in borders and R.distance(GC.POLYGON, case["objs"][6], 0.5, 5.5) <= GC.R_G0  # wholly outside: never
    for q in case["queries"]:
        for r in (GC.R_G1, GC.R_G0, GC.R_GM1, 0.0):
            got = run(q, r)
            assert not got & {6, 10, 11, 14, 15}, (q, r)    # outside the grid, invalid: never selected
    assert 12 in run("one", GC.R_G0)                        # the invalid objects' neighbour is unaffected
    zero = run("one", 0.0)                                  # r == 0: N is the whole grid, emitted iff d <= 0
    assert zero == {i for i, o in enumerate(case["objs"]) if R.valid(GC.POLYGON, o) and i != 6
                    and R.distance(GC.POLYGON, o, 5.5, 5.5) == 0.0} and {0, 13} <= zero
    with pytest.raises(R.LayersError):
        run("one", -1.0)


@pytest.mark.parametrize("kind", [GC.POLYGON, GC.LINESTRING])
def test_an_object_within_r_but_with_no_cell_in_N_is_dropped(kind, oracle_mod):
    case = GC.corner(kind)
    g = R.grid_of(*case["grid"])
    qx, qy = case["queries"]["corner"]
    assert oracle_mod.layers(g, GC.CORNER_R)[1] == 3
    assert R.cell_rect(g, R.bbox(kind, case["objs"][0]))[0] == 4 and oracle_mod.assign_cells(g, qx, qy)[0][0] == 0
    for approximate, metric in ((False, 0), (False, 1), (True, 0)):
        assert R.distance(kind, case["objs"][0], qx[0], qy[0], metric, approximate) <= GC.CORNER_R  # within r ...
        lit = R.range_literal(g, kind, case["objs"], qx, qy, GC.CORNER_R, approximate, metric)
        assert lit.tolist() == [1]                                                                  # ... and dropped
        assert np.array_equal(lit, R.range_closed_form(g, kind, case["objs"], qx, qy, GC.CORNER_R, approximate, metric))
        o, d, i = R.knn_literal(g, kind, case["objs"], case["keys"], qx[0], qy[0], GC.CORNER_R, 5, approximate, metric)
        assert i.tolist() == [1] and o.tolist() == [6]


def test_knn_contract_on_ties_and_duplicates(oracle_mod):
    case = GC.holes()
    g = R.grid_of(*case["grid"])
    qx, qy = case["queries"]["in_shell"]
    o, d, i = R.knn_literal(g, GC.POLYGON, case["objs"], case["keys"], qx[0], qy[0], GC.R_G1, 50)
    assert len(set(o.tolist())) == len(o) and np.all(np.diff(d) >= 0)
    zero = d == 0.0
    assert zero.sum() >= 3 and np.all(np.diff(o[zero]) > 0)   # ties at d = 0 ordered by key
    assert i[o == 1][0] == 4                                   # key 1 twice at d = 0: the smaller index
    o1, d1, _ = R.knn_literal(g, GC.POLYGON, case["objs"], case["keys"], qx[0], qy[0], GC.R_G1, 2)
    assert np.array_equal(o1, o[:2]) and np.array_equal(d1, d[:2])


# ---- the summed-area tables under the host sanitizers ------------------------------------------------
def _sat_sets():
    rnd = random.Random(11)
    sets = []
    for n in (1, 2, 7, 100):
        for nq, gl, cl, whole in ((1, 0, 2, 0), (3, 1, 3, 0), (3, -1, 1, 0), (1, -1, 0, 1), (3, 0, 1, 0)):
            qc = [(rnd.randint(-2, n + 1), rnd.randint(-2, n + 1)) for _ in range(nq)]
            if nq == 3:
                qc[1] = (qc[0][0] + 1, qc[0][1])  # overlapping squares
            rects = [(-3, -3, n + 2, n + 2), (0, 0, n - 1, n - 1), (-5, 0, -1, n - 1), (n, n, n + 3, n + 3), (0, 0, 0, 0),
                     (-1, -1, 0, 0), (n - 1, n - 1, n, n)]
            for _ in range(40):
                x1, y1 = rnd.randint(-3, n + 1), rnd.randint(-3, n + 1)
                rects.append((x1, y1, x1 + rnd.randint(0, max(1, n // 2)), y1 + rnd.randint(0, max(1, n // 2))))
            sets.append((n, nq, gl, cl, whole, qc, rects))
    return sets


def _brute_masks(n, gl, cl, whole, qc):
    inN, inG = np.zeros((n, n), bool), np.zeros((n, n), bool)
    for x in range(n):
        for y in range(n):
            inN[x, y] = bool(whole) or (cl > 0 and any(abs(x - a) <= cl and abs(y - b) <= cl for a, b in qc))
            inG[x, y] = gl >= 0 and any(abs(x - a) <= gl and abs(y - b) <= gl for a, b in qc)
    return inN, inG


def test_summed_area_rectangle_sums_under_the_host_sanitizers(tmp_path):
    exe = str(tmp_path / "geom_plan_main")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-I/opt/rocm/include",
                    "-D__HIP_PLATFORM_AMD__", os.path.join(ROOT, "tests", "native", "geom_plan_main.cpp"), "-o", exe],
                   check=True)
    sets = _sat_sets()
    lines = [str(len(sets) + 2)]
    for n, nq, gl, cl, whole, qc, rects in sets:
        lines.append(" ".join(map(str, [n, nq, gl, cl, whole] + [v for c in qc for v in c] + [len(rects)] +
                                  [v for r in rects for v in r])))
    lines.append("46341 1 0 1 0 0 0 0")  # refused: the tables would leave int32
    lines.append("0 1 0 1 0 0 0 0")
    src = tmp_path / "sets.txt"
    src.write_text("\n".join(lines) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1")
    run = subprocess.run([exe, str(src)], capture_output=True, text=True, env=env)
    assert run.returncode == 0, run.stderr[-2000:]
    rows = [tuple(int(v) for v in ln.split()) for ln in run.stdout.strip().splitlines()]
    at = 0
    for n, nq, gl, cl, whole, qc, rects in sets:
        inN, inG = _brute_masks(n, gl, cl, whole, qc)
        assert rows[at] == (0, int(inN.sum()), int(inG.sum())), (n, qc)
        at += 1
        for rect in rects:
            cn, (cg, area) = R.rect_counts(inN, rect)[0], R.rect_counts(inG, rect)
            assert rows[at] == (cn, cg, area), (n, qc, rect, rows[at])
            at += 1
    assert rows[at] == (1, 0, 0) and rows[at + 1] == (1, 0, 0) and at + 2 == len(rows)


# ---- the ABI and the mirror --------------------------------------------------------------------------
def test_entry_points_reject_bad_arguments_without_a_device():
    L = _lib.lib()
    h = C.c_void_p()
    g = sf.UniformGrid(10, 0.0, 10.0, 0.0, 10.0)
    qx, qy = (C.c_double * 2)(5.5, 6.5), (C.c_double * 2)(5.5, 5.5)
    geoms = lambda kind, nobj: _lib.GfGeoms(kind, 0, nobj, None, None, None, None, None, None)  # noqa: E731
    # gf_geom_prepare: null context / grid / geoms / out, nobj < 0, a kind other than the two
    assert L.gf_geom_prepare(None, C.byref(g.c_grid), C.byref(geoms(1, 0)), C.byref(h)) == _lib.GF_ERR_ARG
    assert L.gf_geom_prepare(None, None, None, None) == _lib.GF_ERR_ARG
    for kind, nobj in ((1, -1), (3, 0), (0, 0), (2, -5)):
        assert L.gf_geom_prepare(None, C.byref(g.c_grid), C.byref(geoms(kind, nobj)), C.byref(h)) == _lib.GF_ERR_ARG
    assert h.value is None
    c = [C.c_int64() for _ in range(4)]
    assert L.gf_geom_index_info(None, *(C.byref(v) for v in c)) == _lib.GF_ERR_ARG
    assert L.gf_geom_index_read(None, None, None) == _lib.GF_ERR_ARG
    assert L.gf_geom_index_set_thresholds(None, 64) == _lib.GF_ERR_ARG
    # gf_geom_query_create: nq <= 0, null points / out / grid, a bad metric, a grid the tables cannot hold
    create = lambda grid, x, y, nq, r, metric=0, out=C.byref(h): L.gf_geom_query_create(None, grid, x, y, nq, r, 0, metric, out)  # noqa: E731
    assert create(C.byref(g.c_grid), qx, qy, 0, 1.0) == _lib.GF_ERR_ARG
    assert create(C.byref(g.c_grid), qx, qy, -1, 1.0) == _lib.GF_ERR_ARG
    assert create(C.byref(g.c_grid), None, qy, 1, 1.0) == _lib.GF_ERR_ARG
    assert create(C.byref(g.c_grid), qx, None, 1, 1.0) == _lib.GF_ERR_ARG
    assert create(None, qx, qy, 1, 1.0) == _lib.GF_ERR_ARG
    assert create(C.byref(g.c_grid), qx, qy, 1, 1.0, metric=2) == _lib.GF_ERR_ARG
    assert create(C.byref(g.c_grid), qx, qy, 1, 1.0, out=None) == _lib.GF_ERR_ARG
    big = sf.UniformGrid(46341, 0.0, 10.0, 0.0, 10.0)
    assert create(C.byref(big.c_grid), qx, qy, 1, 1.0) == _lib.GF_ERR_ARG
    # candidate layers <= 0 (r != 0): the reference's System.exit(1)
    for r in (-1.0, float("nan"), -0.001):
        assert create(C.byref(g.c_grid), qx, qy, 2, r) == _lib.GF_ERR_LAYERS
    # a well-formed query without a context (r == 0 is legal: N is the whole grid)
    assert create(C.byref(g.c_grid), qx, qy, 2, 0.0) == _lib.GF_ERR_ARG
    assert create(C.byref(g.c_grid), qx, qy, 2, 1.0) == _lib.GF_ERR_ARG
    assert h.value is None
    # the runs: null handles (k, nq and the pairing are checked on the GPU, where handles exist)
    assert L.gf_geom_range_run(None, None, None, None) == _lib.GF_ERR_ARG
    assert L.gf_geom_knn_enqueue(None, None, 5, None) == _lib.GF_ERR_ARG
    assert L.gf_geom_knn_enqueue(None, None, 0, None) == _lib.GF_ERR_ARG
    assert L.gf_geom_info(None, *(C.byref(v) for v in c)) == _lib.GF_ERR_ARG
    L.gf_geom_index_destroy(None)  # no-ops
    L.gf_geom_query_destroy(None)


def test_exports_kernel_id_and_mirror_names():
    L = _lib.lib()
    assert L.gf_abi_version() == 2
    with open(os.path.join(ROOT, "include", "geoflink_hip.h")) as f:
        header = f.read()
    assert "#define GF_ABI_VERSION 2" in header and "#define GF_K_GEOM        19" in header
    assert _lib.K_GEOM == 19 and _lib.GEOM_POLYGON == 1 and _lib.GEOM_LINESTRING == 2
    for fn in ("gf_geom_prepare", "gf_geom_index_destroy", "gf_geom_index_info", "gf_geom_index_read",
               "gf_geom_index_set_thresholds", "gf_geom_query_create", "gf_geom_query_destroy", "gf_geom_range_run",
               "gf_geom_knn_enqueue", "gf_geom_info"):
        assert fn in _lib.EXPORTS and hasattr(L, fn) and fn in header
    for name in ("GeometryWindow", "PolygonWindow", "LineStringWindow", "GeometryIndex", "PolygonPointRangeQuery",
                 "LineStringPointRangeQuery", "PolygonPointKNNQuery", "LineStringPointKNNQuery"):
        assert hasattr(sf, name) and name in sf.__all__
    assert "geom_cpp" in L.gf_build_info().decode() or L.gf_build_is_product() == 1


def test_the_mirror_validates_offsets_on_the_host():
    ok = validate_geom_offsets
    ok(_lib.GEOM_POLYGON, 2, [0, 1, 3], [0, 4, 8, 12], 12)
    ok(_lib.GEOM_LINESTRING, 2, None, [0, 2, 5], 5)
    ok(_lib.GEOM_POLYGON, 0, [0], [0], 0)
    bad = [
        (_lib.GEOM_POLYGON, 2, [0, 1, 3], [0, 4, 8, 12], 11),      # the vertices end elsewhere
        (_lib.GEOM_POLYGON, 2, [0, 1, 4], [0, 4, 8, 12], 12),      # the rings end elsewhere
        (_lib.GEOM_POLYGON, 2, [0, 2, 1], [0, 4, 8], 8),           # decreasing
        (_lib.GEOM_POLYGON, 2, [1, 1, 2], [0, 4, 8], 8),           # does not start at 0
        (_lib.GEOM_POLYGON, 2, [0, 1], [0, 4], 4),                 # nobj + 1 entries
        (_lib.GEOM_POLYGON, 1, None, [0, 4], 4),                   # polygons need ring_off
        (_lib.GEOM_LINESTRING, 2, None, [0, 5, 2], 2),             # decreasing
        (_lib.GEOM_LINESTRING, 2, [0, 1, 2], [0, 2, 5], 5),        # linestrings have none
        (_lib.GEOM_LINESTRING, 1, None, [0, -1], -1),
        (3, 1, None, [0, 2], 2),                                   # another kind
    ]
    for args in bad:
        with pytest.raises(ValueError):
            ok(*args)
