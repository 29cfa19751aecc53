"""CPU: the numpy restatement of the point-linestring geometry and operators
(tests/linestring_cases.py) pinned to the C oracle where the two must agree, its invariances, and the
C ABI / Python mirror of the linestring queries as far as they run without a device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import linestring_cases as LC
import poly_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
METRICS = (0, 1)


@pytest.fixture(scope="module")
def hyp(oracle_mod):
    f = np.frompyfunc(oracle_mod.lib().orc_hypot, 2, 1)

    def hypot(a, b):
        with np.errstate(all="ignore"):
            return f(a, b).astype(np.float64)
    return hypot


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def hole_free(name):
    return [rings for rings in PC.polygons(name) if len(rings) == 1]


# ---------------------------------------------------------------------------------------------
# 1. the restatement is pinned to the oracle
# ---------------------------------------------------------------------------------------------
HOLE_FREE = tuple(n for n in PC.SHAPES if hole_free(n))   # every entry but the two holed ones (ngon: its first)


@pytest.mark.parametrize("name", HOLE_FREE)
def test_chain_distance_equals_the_oracle_outside_the_shell(oracle_mod, hyp, name):
    """Every hole-free polygon of the catalogue entry, its shell taken as a closed chain, on the
    entry's probes under both metrics: where the shell location is EXTERIOR the chain distance equals
    the oracle's polygon distance bit for bit; the bbox distance equals the oracle's approximate
    distance on every probe.  The oracle exports no location: the shell location is
    poly_cases.ring_locate's (tests/test_poly_geometry.py ties it to the oracle), and wherever it is
    not EXTERIOR the oracle's distance must be 0 -- asserted, so the two agree on what is compared.
    No probe is left out for any other reason (the compared count equals the EXTERIOR count), and the
    entry has interior probes at chain distance > 0 and polygon distance 0 (the difference between
    the two geometries is exercised, not assumed)."""
    px, py = PC.probes(name)
    polys = hole_free(name)
    assert polys and set(PC.SHAPES) - set(HOLE_FREE) == {"holed", "holed_rev"}
    interior_seen = 0
    for metric in METRICS:
        for rings in polys:
            shell = rings[0]
            OP = oracle_mod.Polygons([rings])
            orc = np.array([oracle_mod.point_polygon_distance(a, b, OP, 0, metric) for a, b in zip(px, py)])
            loc = np.where(px == px, PC.ring_locate(px, py, shell), PC.LOC_E)
            ext = loc == PC.LOC_E
            d = LC.chain_distance(px, py, shell, metric, hyp)
            assert (orc[~ext] == 0.0).all()
            compared = np.flatnonzero(ext)
            np.testing.assert_array_equal(bits(d[compared]), bits(orc[compared]), err_msg=f"{name} metric {metric}")
            assert len(compared) == int(ext.sum()) > 0
            interior_seen += int(((loc == PC.LOC_I) & (d > 0) & (orc == 0.0)).sum())
            x1, y1, x2, y2 = LC.bbox(shell)
            ob = np.array([oracle_mod.point_bbox_distance(a, b, x1, y1, x2, y2) for a, b in zip(px, py)])
            np.testing.assert_array_equal(bits(LC.bbox_distance(px, py, shell)), bits(ob), err_msg=f"{name} bbox")
    assert interior_seen >= 1, name


# ---------------------------------------------------------------------------------------------
# 2. the there-and-back polygon through the oracle == the chain through the restatement
# ---------------------------------------------------------------------------------------------
# A segment walked backwards rounds its projection and cross product differently: the ring's minimum
# over both directions can differ from the chain's by the rounding of one pointToSegment, which is
# below 64 eps x (|x| + |y|) < 2.3e-12 here (the same bound env_far's margin rests on).  The two routes
# are therefore compared at radii no window point's distance comes that close to -- asserted per
# radius -- which leaves out only the radii EQUAL to a realized distance and their ulp neighbours
# (those belong to the GPU tests, where both sides walk the chain forwards).
BAND = 2.3e-12


def baseline_radii(name, hyp):
    out = [0.0, LC.SMALL_R, LC.CL, LC.KNN_R, LC.BIG_R]
    for d in LC.realized_radii(name, 0, hyp)[1:]:     # about 0.3 and 1.2 cell lengths
        out += [d * (1 - 2.0 ** -20), d * (1 + 2.0 ** -20)]
    return out


@pytest.mark.parametrize("name", LC.OPEN)
def test_there_and_back_polygon_through_the_oracle(oracle_mod, hyp, name):
    """The zero-area there-and-back ring of every open shape, as a polygon through the ORACLE's range
    query, selects what ref_range_pls selects on the chain -- exact and approximate, on the probe
    window: the route a user has without linestring queries is a fair baseline for them.  Radii: none,
    half a cell, one, two and 2.5 cells, and just below / above the realized distances near 0.3 and 1.2
    cells (see BAND)."""
    x, y, _, _ = LC.window(name)
    og = oracle_mod.grid(LC.GRID_N, *LC.BEIJING)
    chains = LC.lines(name)
    OP = oracle_mod.Polygons([[LC.there_and_back(c)] for c in chains])
    G = PC.Grid()
    for approximate in (False, True):
        D = LC.window_distances(name, 0, hyp, approximate)
        for r in baseline_radii(name, hyp):
            if not approximate and r > 0.0:   # (r == 0 has no cells: nothing is asked of any distance)
                assert not (np.abs(D[np.isfinite(D)] - r) <= BAND).any(), (name, r)
            exp = LC.ref_range_pls(G, x, y, chains, r, D)
            got = oracle_mod.range_ppoly(og, x, y, OP, r, approximate, 0)
            np.testing.assert_array_equal(got, exp, err_msg=f"{name} approximate {approximate} r {r!r}")
            assert r == 0.0 or len(exp) > 0


# ---------------------------------------------------------------------------------------------
# 3. invariances of the kNN restatement
# ---------------------------------------------------------------------------------------------
def test_knn_reference_invariant_under_reversal_and_exact_split(hyp):
    """ref_knn_pls does not change when the chain is reversed, nor when a segment is split at an
    interior vertex lying exactly on it (a dyadic midpoint).  Vertices and points lie on the 2^-10
    lattice, so every product and sum of pointToSegment's projections is exact in double: reversal only
    flips the cross product's sign, the split halves it and quarters len2 -- the records are equal bit
    for bit, not merely close."""
    G = PC.Grid()
    chain = [(116.0, 40.0), (116.125, 40.0625), (116.25, 40.0), (116.375, 40.125)]
    mid = ((chain[1][0] + chain[2][0]) / 2, (chain[1][1] + chain[2][1]) / 2)
    assert mid == (116.1875, 40.03125)
    split = chain[:2] + [mid] + chain[2:]
    rng = np.random.default_rng(11)
    n = 3001
    x = 115.875 + rng.integers(0, 640, n) / 1024.0
    y = 39.875 + rng.integers(0, 400, n) / 1024.0
    obj = (np.arange(n) % 700).astype(np.int64)
    for metric in METRICS:
        recs = []
        for c in (chain, chain[::-1], split):
            d = LC.distance_matrix(G, x, y, [c], metric, hyp)[0]
            recs.append(LC.ref_knn_pls(G, x, y, obj, c, LC.KNN_R, 50, d))
        base = recs[0]
        assert len(base[0]) == 50 and (base[1] > 0).any()
        for other in recs[1:]:
            np.testing.assert_array_equal(other[0], base[0])
            np.testing.assert_array_equal(bits(other[1]), bits(base[1]))
            np.testing.assert_array_equal(other[2], base[2])


def test_plan_builder_host_part_under_the_host_sanitizers(tmp_path):
    """gf_chain_plan.hpp (validation, bboxes, the runs of CHAIN_RUN segments and their envelopes) driven
    by a stand-alone program built with ASan + UBSan: every catalogue entry at run lengths 1, 3 and
    CHAIN_RUN, an empty set, and the sets it must refuse (a line of one vertex, a line of none)."""
    exe = str(tmp_path / "chain_plan_main")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-I/opt/rocm/include",
                    "-D__HIP_PLATFORM_AMD__", os.path.join(ROOT, "tests", "native", "chain_plan_main.cpp"), "-o", exe],
                   check=True)
    sets = [(run, LC.lines(name)) for name in LC.NAMES for run in (1, 3, LC.CHAIN_RUN)] + [(LC.CHAIN_RUN, [])]
    bad = [(LC.CHAIN_RUN, [[(1.0, 1.0), (2.0, 2.0)], [(3.0, 3.0)]]), (LC.CHAIN_RUN, [[]])]
    rows_in = [str(len(sets) + len(bad))]
    for run, chains in sets + bad:
        rows_in.append(f"{run} {len(chains)}")
        for c in chains:
            rows_in.append(" ".join([str(len(c))] + [float(v).hex() for p in c for v in p]))
    src = tmp_path / "sets.txt"
    src.write_text("\n".join(rows_in) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1")
    out = subprocess.run([exe, str(src)], capture_output=True, text=True, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = [ln.split() for ln in out.stdout.strip().splitlines()]
    assert len(rows) == len(sets) + len(bad)
    for (run, chains), row in zip(sets, rows):
        assert row[0] == "1"
        assert int(row[1]) == sum(-(-(len(c) - 1) // run) for c in chains)
        got = [float.fromhex(v) for v in row[2:]]
        assert got == [v for c in chains for v in LC.bbox(c)]
    assert [r[0] for r in rows[len(sets):]] == ["0", "0"]


# ---------------------------------------------------------------------------------------------
# 4. ABI and the Python mirror (no device)
# ---------------------------------------------------------------------------------------------
NEW_EXPORTS = ("gf_range_pls_plan_create", "gf_knn_pls_plan_create", "gf_join_pls_plan_create", "gf_join_pls",
               "gf_range_plan_set_chain_mode", "gf_knn_plan_set_chain_mode")


def test_exports_are_listed_declared_and_resolvable():
    from spatialflink_amd import _lib

    header = open(os.path.join(ROOT, "include", "geoflink_hip.h")).read()
    L = _lib.lib()
    for name in NEW_EXPORTS:
        assert name in _lib.EXPORTS
        assert name + "(" in header
        assert getattr(L, name) is not None
    assert "gf_linestrings;" in header
    assert "#define GF_ABI_VERSION 2" in header and L.gf_abi_version() == 2


def _ls(vert_off, vx, vy, nline=None):
    from spatialflink_amd import _lib

    vo, ax, ay = np.asarray(vert_off, np.int32), np.asarray(vx, np.float64), np.asarray(vy, np.float64)
    s = _lib.GfLineStrings(len(vo) - 1 if nline is None else nline, vo.ctypes.data, ax.ctypes.data, ay.ctypes.data)
    return s, (vo, ax, ay)


def test_argument_errors_without_a_device():
    """Null, short-line, nline != 1 and bad-metric arguments give GF_ERR_ARG before any device call (the
    creators validate first: no context is needed to be refused)."""
    import spatialflink_amd as sf
    from spatialflink_amd import _lib

    L = _lib.lib()
    g = sf.UniformGrid(LC.GRID_N, *LC.BEIJING)
    gp = C.byref(g.c_grid)
    h = C.c_void_p()
    ok, keep0 = _ls([0, 2], [116.0, 116.1], [40.0, 40.1])
    short, keep1 = _ls([0, 2, 3], [116.0, 116.1, 116.2], [40.0, 40.1, 40.2])
    two, keep2 = _ls([0, 2, 4], [116.0, 116.1, 116.2, 116.3], [40.0, 40.1, 40.2, 40.3])
    neg = _lib.GfLineStrings(-1, None, None, None)
    null = _lib.GfLineStrings(1, None, None, None)
    E_ = _lib.GF_ERR_ARG
    for bad in (short, neg, null):
        assert L.gf_range_pls_plan_create(None, gp, C.byref(bad), 0.1, 0, 0, C.byref(h)) == E_
        assert L.gf_join_pls_plan_create(None, gp, C.byref(bad), 0.1, 0, 0, C.byref(h)) == E_
        assert L.gf_knn_pls_plan_create(None, gp, C.byref(bad), 0.1, 5, 0, 0, C.byref(h)) == E_
    assert L.gf_range_pls_plan_create(None, gp, None, 0.1, 0, 0, C.byref(h)) == E_
    assert L.gf_range_pls_plan_create(None, gp, C.byref(ok), 0.1, 0, 7, C.byref(h)) == E_
    assert L.gf_knn_pls_plan_create(None, gp, C.byref(ok), 0.1, 5, 0, 7, C.byref(h)) == E_
    assert L.gf_knn_pls_plan_create(None, gp, C.byref(two), 0.1, 5, 0, 0, C.byref(h)) == E_
    assert L.gf_knn_pls_plan_create(None, gp, C.byref(ok), 0.1, 0, 0, 0, C.byref(h)) == E_
    n = C.c_int64()
    assert L.gf_join_pls(None, gp, gp, None, C.byref(short), 0.1, 0, 0, None, 0, C.byref(n)) == E_
    assert L.gf_range_plan_set_chain_mode(None, 0) == E_ and L.gf_knn_plan_set_chain_mode(None, 1) == E_
    assert h.value is None
    del keep0, keep1, keep2


def test_mirror_names_and_unsupported_query_types():
    import spatialflink_amd as sf
    from spatialflink_amd import spatialOperators as SO

    names = ("LineString", "LineStringSet", "PointLineStringRangeQuery", "PointLineStringKNNQuery",
             "PointLineStringJoinQuery")
    for n in names:
        assert n in sf.__all__ and n in SO.__all__ and getattr(sf, n) is getattr(SO, n)
    g = sf.UniformGrid(LC.GRID_N, *LC.BEIJING)
    line = sf.LineString(LC.lines("two")[0], g)
    for qt in (sf.QueryType.CountBased, sf.QueryType.RealTimeNaive):
        conf = sf.QueryConfiguration(qt)
        with pytest.raises(ValueError, match="Not yet support"):
            sf.PointLineStringRangeQuery(conf, g).run(None, [line], 0.1)
        with pytest.raises(ValueError, match="Not yet support"):
            sf.PointLineStringRangeQuery(conf, g).plan(0, [line], 0.1)
        with pytest.raises(ValueError, match="Not yet support"):
            sf.PointLineStringJoinQuery(conf, g).run(None, [line], 0.1)
        with pytest.raises(ValueError, match="Not yet support"):
            sf.PointLineStringKNNQuery(conf, g).run(None, line, 0.1, 3)
    with pytest.raises(ValueError):
        sf.LineString([(116.0, 40.0)], g)
    s1, s2 = sf.LineStringSet([line]), sf.LineStringSet([sf.LineString(LC.lines("two")[0][::-1], g)])
    assert s1.digest() == sf.LineStringSet([line]).digest() != s2.digest()
    cs = s1.c_struct()
    assert cs.nline == 1 and list(s1.vert_off) == [0, 2]


@pytest.mark.parametrize("name", LC.SINGLE[:8])
def test_grid_cell_sets_of_a_linestring_equal_a_polygons_of_the_same_bbox(name):
    """UniformGrid's G / C sets for a LineString equal those of a Polygon with the same bbox -- for the
    zero-width, zero-height and point bboxes too (a row, a column, one cell: never empty)."""
    import spatialflink_amd as sf

    g = sf.UniformGrid(LC.GRID_N, *LC.BEIJING)
    chain = LC.lines(name)[0]
    x1, y1, x2, y2 = LC.bbox(chain)
    line = sf.LineString(chain, g)
    poly = sf.Polygon([[(x1, y1), (x2, y1), (x2, y2), (x1, y2), (x1, y1)]], g)
    assert line.boundingBox == poly.boundingBox == ((x1, y1), (x2, y2))
    assert line.gridIDsSet == poly.gridIDsSet and len(line.gridIDsSet) >= 1
    for r in (LC.SMALL_R, LC.CL, LC.BIG_R, 4.5 * LC.CL):
        G1, G2 = g.getGuaranteedNeighboringCells(r, line), g.getGuaranteedNeighboringCells(r, poly)
        assert G1 == G2
        assert g.getCandidateNeighboringCells(r, line, G1) == g.getCandidateNeighboringCells(r, poly, G2)
