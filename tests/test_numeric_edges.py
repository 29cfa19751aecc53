"""CPU: the numeric shortcuts of the window path against an independent reference.

1. The C oracle (the GPU tests' checker) equals tests/edge_cases.py's numpy / rational reference on
   every case of the grid catalogue -- cells, layers, range, kNN, join -- so the GPU is later held
   to a proven reference, and the generator's cases are not vacuous (points exactly at r, on both
   sides of every cell edge).
2. A host build of spatialflink_amd/csrc/gf_numerics.hpp (tests/native/numerics_core.cpp):
   fdlibm_hypot bit for bit against the oracle and within 1 ulp of the rational value, smax_for,
   the exact cell thresholds, and the device's multiply-by-reciprocal cell_index_fast against the
   division on the catalogue windows and on 10^7 triples next to cell edges."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import edge_cases as E
from conftest import NATIVE_FLAGS, ROOT

GRID_NAMES = list(E.GRIDS)


@pytest.fixture(scope="module")
def hyp(oracle_mod):
    """The oracle's hypot as an array function (tied to rational arithmetic below)."""
    f = np.frompyfunc(oracle_mod.lib().orc_hypot, 2, 1)

    def hypot(a, b):
        with np.errstate(all="ignore"):
            return f(a, b).astype(np.float64)
    return hypot


@pytest.fixture(scope="module")
def core(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("core") / "numerics_core.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-I/opt/rocm/include",
                    "-D__HIP_PLATFORM_AMD__", *NATIVE_FLAGS, os.path.join(ROOT, "tests", "native", "numerics_core.cpp"),
                    "-o", out], check=True)
    L = C.CDLL(out)
    P = C.c_void_p
    L.core_hypot_many.argtypes = [P, P, C.c_int64, P]
    L.core_smax_many.argtypes = [P, C.c_int64, P]
    L.core_s_prefilter_many.argtypes = [P, C.c_int64, C.c_int, P]
    L.core_cell_div_many.argtypes = [P, P, P, C.c_int64, P]
    L.core_cell_fast_many.argtypes = [P, P, P, C.c_int64, P, P]
    L.core_jint_many.argtypes = [P, C.c_int64, P]
    L.core_layers.argtypes = [C.c_double, C.c_double, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    return L


def _f64(a):
    return np.ascontiguousarray(a, np.float64)


def core_hypot(core, a, b):
    a, b = _f64(a), _f64(b)
    out = np.empty(len(a))
    core.core_hypot_many(a.ctypes.data, b.ctypes.data, len(a), out.ctypes.data)
    return out


def core_cells(core, v, mn, cl):
    """(division cells, fast cells, decided) of the host build, element-wise."""
    v = _f64(v)
    mn = _f64(np.broadcast_to(mn, v.shape))
    cl = _f64(np.broadcast_to(cl, v.shape))
    div = np.empty(len(v), np.int32)
    fast = np.empty(len(v), np.int32)
    dec = np.empty(len(v), np.uint8)
    core.core_cell_div_many(v.ctypes.data, mn.ctypes.data, cl.ctypes.data, len(v), div.ctypes.data)
    core.core_cell_fast_many(v.ctypes.data, mn.ctypes.data, cl.ctypes.data, len(v), fast.ctypes.data, dec.ctypes.data)
    return div, fast, dec.astype(bool)


# ---------------------------------------------------------------------------------------------
# the generator's own conditions
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GRID_NAMES)
def test_generator_cases_are_not_vacuous(name, hyp):
    """From the reference alone: lattice counts as the issue states them (1961 / 20 and
    13273 / 36, layers (2, 5) and (8, 13) on ulp5); edge windows with points on both sides of every
    edge; every r = d case with a point exactly at r that the lower neighbour of r drops; hits and
    misses among the candidate-cell points."""
    x, y, _ = E.window(name)
    assert len(x) <= 110_000
    if name in E.LATTICE:
        assert len(x) == 108_900
        for metric in (0, 1):
            E.assert_lattice_counts(name, metric, hyp)
    else:
        assert len(x) <= 61_000
        E.assert_edges_straddled(name)
        assert np.isnan(x).any() and np.isinf(y).any() and (x == 0).any() and (np.abs(x) == 1e300).any()
    assert E.on_edge_count(name) > 0
    for q in E.queries(name):
        for metric in (0, 1):
            for r, d in E.realized_radii(name, q, metric, hyp):
                if r == d:
                    assert E.assert_realized_case(name, q, d, metric, hyp) >= 1


def test_oracle_hypot_within_one_ulp_of_rational(oracle_mod, hyp):
    """The hypot metric's reference values: the oracle's fdlibm hypot against exact rational
    arithmetic on coordinate differences sampled from every catalogue window (a few thousand pairs)
    and on random magnitudes."""
    rng = np.random.default_rng(5)
    n = 0
    for name in GRID_NAMES:
        x, y, _ = E.window(name)
        ok = np.flatnonzero(E.in_grid(name))
        q = E.queries(name)[0]
        for i in rng.choice(ok, 500, replace=False):
            a, b = q[0] - x[i], q[1] - y[i]
            assert E.exact_hypot_ulps(float(a), float(b), oracle_mod.hypot(a, b)), (name, a, b)
            n += 1
    for _ in range(1500):
        a = math.ldexp(rng.uniform(-1, 1), int(rng.integers(-300, 300)))
        b = a * rng.uniform(-4, 4) if rng.random() < 0.7 else math.ldexp(rng.uniform(-1, 1), int(rng.integers(-300, 300)))
        assert E.exact_hypot_ulps(a, b, oracle_mod.hypot(a, b)), (a, b)
        n += 1
    assert n >= 5000


# ---------------------------------------------------------------------------------------------
# the oracle == the independent reference, on every catalogue case
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GRID_NAMES)
def test_oracle_cells_and_layers_equal_reference(name, oracle_mod, hyp):
    og = oracle_mod.grid(*E.GRIDS[name])
    G = E.RefGrid(name)
    assert og.cellLength == G.cl
    for x, y, _ in (E.window(name), E.second_window(name)):
        cx, cy = oracle_mod.assign_cells(og, x, y)
        rx, ry = G.cells(x, y)
        np.testing.assert_array_equal(cx, rx)
        np.testing.assert_array_equal(cy, ry)
    radii = E.layer_radii(name) + [c[3] for c in E.range_cases(name, hyp)] + [np.inf, np.nan, 1e300, 5e-324]
    for r in radii:
        assert oracle_mod.layers(og, r) == E.ref_layers(G.cl, r), (name, r)


@pytest.mark.parametrize("name", GRID_NAMES)
def test_oracle_range_pp_equals_reference(name, oracle_mod, hyp):
    og = oracle_mod.grid(*E.GRIDS[name])
    x, y, _ = E.window(name)
    hits = 0
    for tag, qx, qy, r, metric in E.range_cases(name, hyp):
        exp = E.ref_range_pp(name, x, y, qx, qy, r, False, metric, hyp)
        np.testing.assert_array_equal(oracle_mod.range_pp(og, x, y, qx, qy, r, False, metric), exp,
                                      err_msg=f"{name} {tag} r={r!r} metric {metric}")
        hits += len(exp)
        if metric == 0:  # the approximate mode takes no distance
            np.testing.assert_array_equal(oracle_mod.range_pp(og, x, y, qx, qy, r, True, 0),
                                          E.ref_range_pp(name, x, y, qx, qy, r, True), err_msg=f"{name} {tag} r={r!r} approx")
    assert hits > 0


@pytest.mark.parametrize("name", GRID_NAMES)
def test_oracle_knn_equals_reference(name, oracle_mod, hyp):
    og = oracle_mod.grid(*E.GRIDS[name])
    for x, y, obj in (E.window(name), E.second_window(name)):
        for qx, qy, r, metric, k in E.knn_cases(name, hyp):
            st, oo, od, oi = oracle_mod.knn(og, x, y, obj, qx, qy, r, k, metric)
            eo, ed, ei = E.ref_knn(name, x, y, obj, qx, qy, r, k, metric, hyp)
            assert st == 0
            np.testing.assert_array_equal(oo, eo, err_msg=f"{name} r={r!r} k={k} metric {metric}")
            np.testing.assert_array_equal(od.view(np.uint64), ed.view(np.uint64))
            np.testing.assert_array_equal(oi, ei)
    if name in E.LATTICE:  # k = 20 ends inside a pair of equal distances: the smaller objID is kept
        q = E.queries(name)[0]
        x, y, obj = E.window(name)
        eo, ed, _ = E.ref_knn(name, x, y, obj, q[0], q[1], 25 * E.U, 21)
        assert ed[19] == ed[20] and eo[19] < eo[20]


@pytest.mark.parametrize("name", GRID_NAMES)
def test_oracle_join_pp_equals_reference(name, oracle_mod, hyp):
    og = oracle_mod.grid(*E.GRIDS[name])
    x, y, _ = E.window(name)
    qi = E.join_query_side(name)
    qx, qy = x[qi], y[qi]
    for r, metric in E.join_cases(name, hyp):
        info = {}
        exp = E.ref_join_pp(name, x, y, qx, qy, r, False, metric, hyp, info)
        st, pairs = oracle_mod.join_pp(og, og, x, y, qx, qy, r, False, metric)
        assert st == 0
        np.testing.assert_array_equal(E.sorted_pairs(pairs), exp, err_msg=f"{name} r={r!r} metric {metric}")
        assert info["cand_hit"] >= 1 and info["cand_miss"] >= 1, (name, r, info)
    r = E.join_cases(name, hyp)[0][0]
    st, pairs = oracle_mod.join_pp(og, og, x, y, qx, qy, r, True, 0)
    np.testing.assert_array_equal(E.sorted_pairs(pairs), E.ref_join_pp(name, x, y, qx, qy, r, True))


# ---------------------------------------------------------------------------------------------
# the host build of gf_numerics.hpp
# ---------------------------------------------------------------------------------------------
def _hypot_branch_inputs():
    """(a, b) reaching every branch of fdlibm's e_hypot: b == 0, exponent gap above 60, w > b and
    w <= b, the +-600 scalings (a > 2^500, b < 2^-500), subnormal b, inf / NaN."""
    rng = np.random.default_rng(11)
    sub = 5e-324
    a = [3.0, 0.0, -0.0, 1.0, 1e-300, 1.0, 2.0 ** 61, 1.0, 3.0, 1.0, 1.0, 1.5]
    b = [0.0, 0.0, 0.0, 2.0 ** -61, 1e300, 2.0 ** -60, 1.0, 0.4, 4.0, 1.0, 0.999, 1.0]
    a += [2.0 ** 501, 1e300, 1.7e308, 2.0 ** 600, 2.0 ** -501, 1e-300, 2.0 ** -1000, 2.0 ** 520]
    b += [2.0 ** 500, 1e300, 1.7e308, 2.0 ** 560, 2.0 ** -502, 3e-301, 2.0 ** -1010, 2.0 ** -520]
    a += [sub, 4 * sub, 2.0 ** -1022, 1e-310, 2.2e-308, 2.0 ** -1030, 1e-320]
    b += [sub, 3 * sub, 2.0 ** -1023, 3e-311, 1e-308, 2.0 ** -1074, 0.0]
    a += [np.inf, -np.inf, np.inf, np.nan, np.nan, np.nan, np.inf, 1.0]
    b += [1.0, np.nan, np.inf, 1.0, np.inf, np.nan, 0.0, -np.inf]
    a, b = np.array(a), np.array(b)
    for lo, hi in ((-1074, -960), (-560, -440), (-70, 70), (440, 560), (960, 1023)):
        e = rng.integers(lo, hi, 4000)
        m = np.ldexp(rng.uniform(0.5, 1.0, 4000), e)
        ratio = np.where(rng.random(4000) < 0.5, rng.uniform(0.3, 3.0, 4000), np.ldexp(1.0, rng.integers(-64, 64, 4000)))
        with np.errstate(all="ignore"):
            a, b = np.concatenate([a, m]), np.concatenate([b, m * ratio * rng.choice([-1.0, 1.0], 4000)])
    return np.concatenate([a, b]), np.concatenate([b, a])


def test_core_hypot_bit_identical_to_oracle_and_one_ulp(core, hyp):
    a, b = _hypot_branch_inputs()
    got = core_hypot(core, a, b)
    exp = hyp(a, b)
    np.testing.assert_array_equal(got.view(np.uint64)[~np.isnan(exp)], exp.view(np.uint64)[~np.isnan(exp)])
    np.testing.assert_array_equal(np.isnan(got), np.isnan(exp))
    assert np.isinf(got[np.isinf(a) | np.isinf(b)]).all()   # inf wins over NaN
    # every branch was reached: equal magnitudes (w <= b), w > b, big and tiny scalings, subnormals
    aa, bb = np.abs(a), np.abs(b)
    fin = np.isfinite(a) & np.isfinite(b)
    big, small = np.where(fin, np.maximum(aa, bb), 1.0), np.where(fin, np.minimum(aa, bb), 1.0)
    with np.errstate(over="ignore"):
        assert ((small == 0) & fin).any() and (fin & (small > 0) & (big / np.where(small > 0, small, 1) > 2.0 ** 61)).any()
    assert (fin & (big - small > small)).any() and (fin & (small > 0) & (big - small <= small)).any()
    assert (fin & (big > 2.0 ** 501)).any() and (fin & (small < 2.0 ** -501) & (small > 0)).any()
    assert (fin & (small > 0) & (small < 2.0 ** -1022)).any()
    rng = np.random.default_rng(12)
    ok = np.flatnonzero(fin & np.isfinite(got))
    for i in rng.choice(ok, 4000, replace=False):
        assert E.exact_hypot_ulps(float(a[i]), float(b[i]), float(got[i])), (a[i], b[i], got[i])
    # and on the catalogue's own coordinate differences
    for name in GRID_NAMES:
        x, y, _ = E.window(name)
        q = E.queries(name)[1]
        with np.errstate(all="ignore"):
            dx, dy = q[0] - x, q[1] - y
        np.testing.assert_array_equal(core_hypot(core, dx, dy).view(np.uint64), hyp(dx, dy).view(np.uint64))


def test_core_smax_for_is_the_exact_inverse_of_sqrt(core):
    """smax_for(T) = the largest s with fl(sqrt(s)) <= T: sqrt(s) <= T < sqrt(nextup(s))."""
    rng = np.random.default_rng(13)
    T = np.concatenate([
        np.ldexp(rng.uniform(0.5, 1.0, 3000), rng.integers(-540, 512, 3000)),
        np.ldexp(1.0, np.arange(-1074, 1024, 7)), np.ldexp(1.0, np.arange(-40, 45)),
        [5e-324, 1e-320, 2.2250738585072014e-308, 1e-310, 0.0, 1.7976931348623157e308, 1.3407807929942596e154,
         1.3407807929942597e154, 1.0, 25 * E.U, 65 * E.U],
        [r for n in GRID_NAMES for r in E.layer_radii(n)]])
    with np.errstate(over="ignore"):
        T = np.concatenate([T, np.nextafter(T, 0.0), np.nextafter(T, np.inf)])
    T = _f64(T[np.isfinite(T)])
    s = np.empty(len(T))
    core.core_smax_many(T.ctypes.data, len(T), s.ctypes.data)
    assert (s >= 0).all()
    assert (np.sqrt(s) <= T).all()
    with np.errstate(all="ignore"):
        up = np.nextafter(s, np.inf)
        assert ((np.sqrt(up) > T) | np.isinf(up)).all()
    # metric 0 prefilter is smax; the hypot prefilter is never below it (survivors are re-tested)
    p0, p1 = np.empty(len(T)), np.empty(len(T))
    core.core_s_prefilter_many(T.ctypes.data, len(T), 0, p0.ctypes.data)
    core.core_s_prefilter_many(T.ctypes.data, len(T), 1, p1.ctypes.data)
    np.testing.assert_array_equal(p0, s)
    big = T > 1e-150   # T*T is normal: the (1 + 2^-30) margin is real
    assert (p1[big] >= s[big]).all()
    sp = _f64([np.inf, np.nan, -1.0, -0.0, -np.inf])
    o = np.empty(len(sp))
    core.core_smax_many(sp.ctypes.data, len(sp), o.ctypes.data)
    assert o[0] == np.inf and o[1] == -1.0 and o[2] == -1.0 and o[3] == 0.0 and o[4] == -1.0


def test_core_jint_and_layers_equal_reference(core, hyp):
    v = _f64([np.nan, np.inf, -np.inf, 0.0, -0.0, 0.9, -0.9, 2147483646.5, 2147483647.0, 2147483648.0, -2147483648.0,
              -2147483649.0, 1e300, -1e300, 5e-324])
    out = np.empty(len(v), np.int32)
    core.core_jint_many(v.ctypes.data, len(v), out.ctypes.data)
    np.testing.assert_array_equal(out, E.ref_jint(v))
    for name in GRID_NAMES:
        cl = E.cell_length(name)
        for r in E.layer_radii(name) + [25 * E.U, 65 * E.U, np.inf, np.nan]:
            g, c = C.c_int32(), C.c_int32()
            core.core_layers(cl, r, C.byref(g), C.byref(c))
            assert (g.value, c.value) == E.ref_layers(cl, r), (name, r)


@pytest.mark.parametrize("name", GRID_NAMES)
def test_thresholds_agree_with_cell_index(name, core):
    """first_at_least(c) of the product library (the thresholds the scans compare against instead
    of dividing) for every c of the grid: cell(T) >= c and cell(prev(T)) < c, under the reference
    division and under the host build's cell_index; axis_iv(a, b) is [T[a], T[b + 1])."""
    from spatialflink_amd import _lib

    L = _lib.lib()
    fal = getattr(L, "_ZN2gf14first_at_leastEldd")   # gf::first_at_least(long, double, double)
    fal.argtypes = [C.c_int64, C.c_double, C.c_double]
    fal.restype = C.c_double

    class Iv(C.Structure):
        _fields_ = [("lo", C.c_double), ("hi_excl", C.c_double)]

    aiv = getattr(L, "_ZN2gf7axis_ivElldd")          # gf::axis_iv(long, long, double, double)
    aiv.argtypes = [C.c_int64, C.c_int64, C.c_double, C.c_double]
    aiv.restype = Iv
    n, x0, _, y0, _ = E.GRIDS[name]
    cl = E.cell_length(name)
    for mn in (x0, y0):
        cs = np.arange(-2, n + 3)
        T = np.array([fal(int(c), mn, cl) for c in cs])
        assert np.isfinite(T).all() and (np.diff(T) >= 0).all()
        below = np.nextafter(T, -np.inf)
        for cells in (lambda v: E.ref_cells(v, mn, cl), lambda v: core_cells(core, v, mn, cl)[0]):
            assert (cells(T) >= cs).all(), name
            assert (cells(below) < cs).all(), name
        if name == "subulp":   # two cells per double: a threshold serves two cells
            assert (np.diff(T[2:n + 2]) == 0).sum() >= n // 2 - 1
        for a, b in ((0, n - 1), (3, 3), (n // 2, n // 2 + 2), (-1, 0), (5, 4)):
            iv = aiv(a, b, mn, cl)
            if a > b:
                assert math.isnan(iv.lo) and math.isnan(iv.hi_excl)
            else:
                assert iv.lo == fal(a, mn, cl) and iv.hi_excl == fal(b + 1, mn, cl)


def _near_edge_triples(rng, m):
    """(v, mn, cl) with v within 0..4 ulps of a cell edge mn + c*cl: origins and cell lengths of every
    magnitude the catalogue has (and random ones), c inside and just outside the grid."""
    kind = rng.integers(0, 4, m)
    mn = np.select([kind == 0, kind == 1, kind == 2],
                   [rng.uniform(-180.0, 180.0, m), np.ldexp(rng.uniform(-1, 1, m), rng.integers(-10, 42, m)),
                    rng.choice([115.5, 39.6, -180.0, -90.0, -1.0, 1.2e7, 4.8e6, E.P40, 0.0], m)],
                   rng.uniform(-1e7, 1e7, m))
    cl = np.select([kind == 0, kind == 1, kind == 2],
                   [np.ldexp(rng.uniform(0.5, 1.0, m), rng.integers(-20, 8, m)),
                    np.ldexp(1.0, rng.integers(-14, 6, m)).astype(np.float64),
                    rng.choice([2.1 / 100, 1.0, 2.0 / 7, 41234.5 / 2048, 2.1 / 2049, 5 * E.U, E.U / 2, 2.1 / 1000], m)],
                   rng.uniform(1e-4, 50.0, m))
    c = np.where(rng.random(m) < 0.9, rng.integers(-3, 2052, m), rng.integers(-(1 << 31), 1 << 31, m)).astype(np.float64)
    v = mn + c * cl
    k = rng.integers(-4, 5, m)
    step = np.maximum(np.spacing(np.abs(v)), np.where(rng.random(m) < 0.5, np.spacing(np.abs(mn)), 0.0))
    return v + k * step, mn, cl


def test_cell_index_fast_equals_division_when_decided(core):
    """The device branch of cell_index on the host: whenever the multiply-by-reciprocal's guard band
    decides, its cell is the division's -- on every catalogue window and on 10^7 triples within 0..4
    ulps of a cell edge; the division itself equals the numpy reference."""
    decided = total = 0
    for name in GRID_NAMES:
        n, x0, _, y0, _ = E.GRIDS[name]
        cl = E.cell_length(name)
        for x, y, _ in (E.window(name),):
            for v, mn in ((x, x0), (y, y0)):
                div, fast, dec = core_cells(core, v, mn, cl)
                np.testing.assert_array_equal(div, E.ref_cells(v, mn, cl))
                np.testing.assert_array_equal(fast[dec], div[dec], err_msg=name)
                assert not dec[~np.isfinite(v)].any()   # NaN / inf: the division decides
                decided += int(dec.sum())
                total += len(v)
    assert 0 < decided < total   # both outcomes occur on the windows
    rng = np.random.default_rng(17)
    und = 0
    for _ in range(10):
        v, mn, cl = _near_edge_triples(rng, 1_000_000)
        div, fast, dec = core_cells(core, v, mn, cl)
        np.testing.assert_array_equal(div, E.ref_cells(v, mn, cl))
        bad = np.flatnonzero(dec & (fast != div))
        assert len(bad) == 0, (v[bad[:5]], mn[bad[:5]], cl[bad[:5]], fast[bad[:5]], div[bad[:5]])
        und += int((~dec).sum())
    assert 100_000 < und < 9_900_000   # the triples sit where the guard band is exercised both ways
