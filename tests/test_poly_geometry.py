"""CPU: the C oracle's point-polygon geometry and polygon operators against the independent numpy /
rational reference of tests/poly_cases.py, on a catalogue of degenerate and many-vertex polygons
(comb, star, staircase, near-rectangles, holes, spike and duplicated vertex, sliver, 1000-gons, the
near-collinear lattice family), so that the GPU tests (tests/test_gpu_poly_geometry.py) hold the
device code to a proven checker.  Where the two disagree, the arbiter is the JTS 1.16.1 algorithm
as restated in the header comments of gf_geom.hpp and tests/golden/pyref.py: exact orientation
sign, otherwise plain IEEE double.

Probes per shape: every vertex and its 8 ulp neighbours; on every edge the points at t = 0.25,
0.5, 0.75 and on its extension at t = -0.5, 1.5, each also +-1 and +-2 ulps in x and in y; for
every distinct vertex ordinate a row of 11 abscissae from left of the envelope to right of it, at
the ordinate and +-1 ulp; the envelope's sides and corners and 1 ulp outside; random points of
every ring's envelope (shell interior, holes) and every ring's centroid; NaN in x, in y, in both;
a point outside the grid.  Vertices, edges and ordinates are subsampled on the 1000-gons.

The catalogue's own conditions (enough probes inside / on / outside every shell and hole, the
plain-double orientation sign changing answers on the near-collinear family, every realized radius
flipping a probe, the near-rectangles differing from their boxes) are asserted here, so that no
comparison passes vacuously."""
import numpy as np
import pytest

import edge_cases as E
import poly_cases as PC

METRICS = (0, 1)


@pytest.fixture(scope="module")
def hyp(oracle_mod):
    """The oracle's hypot as an array function (tests/test_numeric_edges.py ties it to rational
    arithmetic and to the device's fdlibm_hypot)."""
    f = np.frompyfunc(oracle_mod.lib().orc_hypot, 2, 1)

    def hypot(a, b):
        with np.errstate(all="ignore"):
            return f(a, b).astype(np.float64)
    return hypot


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def probe_points(name):
    x, y, _, pi = PC.window(name)
    return x[pi], y[pi]


def counts(loc):
    return [int((loc == v).sum()) for v in (PC.LOC_I, PC.LOC_B, PC.LOC_E)]


# ---------------------------------------------------------------------------------------------
# the catalogue's own conditions
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PC.SHAPES)
def test_probes_cover_interior_boundary_exterior(name):
    """>= 20 probes located I, >= 20 B and >= 20 E for every shell (the zero-width ring and the
    three-corner ring, which runs out and back along two sides, enclose nothing: B and E only); the
    holed shapes: >= 10 probes I of a hole and >= 5 B of a hole."""
    px, py = probe_points(name)
    for q, rings in enumerate(PC.polygons(name)):
        i, b, e = counts(PC.ring_locate(px, py, rings[0]))
        degenerate = name == "near_rects" and PC.NEAR_RECTS[q] in ("zero_width", "three_corners")
        assert (degenerate or i >= 20) and b >= 20 and e >= 20, (name, q, i, b, e)
        if degenerate:
            assert i == 0
    if name.startswith("holed"):
        rings = PC.polygons(name)[0]
        hole = [counts(PC.ring_locate(px, py, h)) for h in rings[1:]]
        assert len(hole) == 3
        assert sum(h[0] for h in hole) >= 10 and sum(h[1] for h in hole) >= 5, hole
        assert all(h[0] >= 1 for h in hole)   # a probe inside each hole
        # a hole's envelope is pruned for some probe: farther than the distance found so far
        d, _ = PC.polygon_distance(px, py, rings[:-1])
        assert (PC.env_distance(rings[-1], px, py) > d).sum() >= 20
    if name == "ngon":
        assert [len(r) for rings in PC.polygons(name) for r in rings] == [1001, 1001, 301]


def test_shapes_lie_in_the_grid_and_lattice_range():
    for name in PC.NAMES:
        x1, x2, y1, y2 = PC.extent(name)
        assert PC.BEIJING[0] <= x1 and x2 <= PC.BEIJING[1] and PC.BEIJING[2] <= y1 and y2 <= PC.BEIJING[3], name
    for name in ("collinear_tiled", "collinear_stacked"):   # multiples of 2^-46 in [64,128) x [32,64)
        for rings in PC.polygons(name):
            for vx, vy in rings[0][:2]:
                assert 64 <= vx < 128 and 32 <= vy < 64 and (vx / PC.U).is_integer() and (vy / PC.U).is_integer()
    x, _, _, _ = PC.window("comb")
    assert len(x) % 2 == 1 and len(x) % 64 != 0


def test_holed_rings_reordered_by_area():
    """The hole-first listing is the same polygon once the rings are ordered (Polygon.java: the
    largest ring is the shell), for the reference and for the package's Polygon."""
    assert PC.polygons("holed_rev") == PC.polygons("holed")
    assert PC.raw_polygons("holed_rev")[0][0] != PC.polygons("holed")[0][0]
    from spatialflink_amd.spatialObjects import Polygon

    for name in ("holed", "holed_rev"):
        assert Polygon(PC.raw_polygons(name)[0]).rings == PC.polygons(name)[0]


def test_collinear_family_needs_the_exact_sign():
    """Tiled layout: >= 100 cases whose location under the plain-double orientation sign differs
    from the exact one, >= 40 whose d <= 0 answer changes; the lattice determinant is j exactly."""
    P, polys = PC.collinear_tiled()
    assert len(polys) >= 1000
    loc_diff = ans_diff = 0
    for p, rings in zip(P, polys):
        px, py = np.array([p[0]]), np.array([p[1]])
        d, loc = PC.polygon_distance(px, py, rings)
        dn, locn = PC.polygon_distance(px, py, rings, exact=False)
        assert loc[0][0] != PC.LOC_B           # j != 0: never on the edge
        loc_diff += int(loc[0][0] != locn[0][0])
        ans_diff += int((d[0] <= 0) != (dn[0] <= 0))
    assert loc_diff >= 100 and ans_diff >= 40, (loc_diff, ans_diff)
    assert len(PC.collinear_stacked()) >= 64


def test_collinear_stack_overflows_the_join_worklist(hyp):
    """Stacked layout, from the reference: the shared probe pairs with more than kJoinKeep polygons
    at d <= 0, and fewer than 256 - 17 window points lie outside some triangle's envelope, so that
    every full round of 256 queued points holds at least 17 points with all 64 triangles on their
    worklist: 17 * 64 > 1024 entries."""
    x, y, _, pi = PC.window("collinear_stacked")
    polys = PC.polygons("collinear_stacked")
    D = PC.window_distances("collinear_stacked", 0, hyp)
    assert x[pi[0]] == PC.STACK_P[0] and y[pi[0]] == PC.STACK_P[1]
    assert int((D[:, pi[0]] <= PC.TINY).sum()) > PC.JOIN_KEEP
    inside_all = np.ones(len(x), bool)
    for rings in polys:
        x1, y1, x2, y2 = PC.shell_bbox(rings)
        inside_all &= (x >= x1) & (x <= x2) & (y >= y1) & (y <= y2)
    need = -(-(PC.JOIN_WORK + 1) // len(polys))
    assert (~inside_all).sum() <= PC.JOIN_ROUND - need and inside_all.sum() >= 2 * PC.JOIN_ROUND
    pairs = PC.ref_join_ppoly(PC.Grid(), x, y, polys, PC.TINY, D)
    assert np.bincount(pairs[:, 0]).max() > PC.JOIN_KEEP


@pytest.mark.parametrize("name", PC.NAMES)
def test_tiny_radius_means_distance_zero(name, hyp):
    """No distance of the catalogue lies in (0, TINY]: d <= TINY is d <= 0."""
    for metric in METRICS:
        D = PC.window_distances(name, metric, hyp)
        assert not ((D > 0) & (D <= PC.TINY)).any()
        assert (D == 0).any()


@pytest.mark.parametrize("name", PC.NAMES)
def test_realized_radii_flip_a_point(name, hyp):
    """Every realized radius d: the range result at r = d holds a point that the result at
    nextafter(d, 0) lacks, and those points are exactly the ones at distance d."""
    x, y, _, _ = PC.window(name)
    G = PC.Grid()
    polys = PC.polygons(name)
    for metric in METRICS:
        D = PC.window_distances(name, metric, hyp)
        dmin = D.min(axis=0)
        for d in PC.realized_radii(name, metric, hyp):
            a = PC.ref_range_ppoly(G, x, y, polys, d, D)
            b = PC.ref_range_ppoly(G, x, y, polys, E.toward0(d), D)
            flipped = np.setdiff1d(a, b)
            assert len(flipped) >= 1 and len(np.setdiff1d(b, a)) == 0, (name, metric, d)
            assert (dmin[flipped] == d).all()
            assert len(a) < len(x)   # misses remain


def test_near_rectangles(hyp):
    """The true rectangles (a collinear mid-edge vertex, a duplicated corner, clockwise from every
    corner) have the distances of the plain 5-vertex rectangle of the same box, bit for bit; the
    three non-rectangles differ from their bounding box's rectangle on at least one probe."""
    px, py = probe_points("near_rects")
    polys = dict(zip(PC.NEAR_RECTS, PC.polygons("near_rects")))
    for metric in METRICS:
        plain = PC.polygon_distance(px, py, polys["plain"], metric, hyp)[0]
        for k in PC.TRUE_RECTS:
            assert PC.shell_bbox(polys[k]) == PC.RECT_BOX
            d = PC.polygon_distance(px, py, polys[k], metric, hyp)[0]
            np.testing.assert_array_equal(bits(d), bits(plain), err_msg=k)
        for k in PC.NON_RECTS:
            x1, y1, x2, y2 = PC.shell_bbox(polys[k])
            box = [PC._rect(x1, y1, x2, y2)]
            d = PC.polygon_distance(px, py, polys[k], metric, hyp)[0]
            if x1 < x2:
                differ = (d <= 0) != (PC.polygon_distance(px, py, box, metric, hyp)[0] <= 0)
            else:   # zero width: its box is no polygon; points beside the line are off it
                differ = (d > 0) & (py >= y1) & (py <= y2)
            assert differ.sum() >= 1, k


def test_degenerate_segment_branch_is_observable_or_dead(hyp):
    """Distance.pointToSegment's A == B branch on the rings with a duplicated vertex.  Both
    neighbours of a zero-length segment end at its vertex, and each answers distance(p, vertex)
    itself whenever its projection parameter leaves [0, 1] -- so dropping the branch can only show
    where both neighbours take their interior formula; this records whether any catalogue probe
    does (the GPU tests' mutation table cites the outcome)."""
    changed = 0
    for name, q in (("spike_dup", 0), ("near_rects", PC.NEAR_RECTS.index("dup_corner")),
                    ("near_rects", PC.NEAR_RECTS.index("zero_width"))):
        x, y, _, _ = PC.window(name)
        rings = PC.polygons(name)[q]
        assert any(a == b for a, b in zip(rings[0][:-1], rings[0][1:]))
        for metric in METRICS:
            d = PC.polygon_distance(x, y, rings, metric, hyp)[0]
            PC.DEGENERATE_BRANCH = False
            try:
                dn = PC.polygon_distance(x, y, rings, metric, hyp)[0]
            finally:
                PC.DEGENERATE_BRANCH = True
            changed += int((bits(d) != bits(dn)).sum())
    assert changed == DEGENERATE_CHANGED


# the outcome of the check above on this catalogue: 0 = the branch is observationally dead
DEGENERATE_CHANGED = 0


def test_horizontal_edge_boundary_test_changes_locations_not_distances(hyp):
    """RayCrossingCounter's horizontal-edge branch without its boundary test: probes on horizontal
    edges are then located I or E by the crossing parity (>= 20 locations change per shape, so the
    probes do reach the branch) -- yet no distance changes, on any window.  A point on a horizontal
    segment A B has ay == by == py, so pointToSegment's s is (0 * (bx - ax) - (ax - px) * 0) / len2
    == 0 exactly (and at an endpoint dx == dy == 0): the facet distance, which visits every ring,
    is 0 whatever the locator said; DistanceOp answers 0 for I and B alike.  The branch's boundary
    test is dead for every operator here (they see distances only), which is why no GPU test can
    fail on its removal."""
    for name in ("comb", "staircase", "near_rects", "holed", "spike_dup"):
        x, y, _, pi = PC.window(name)
        for rings in PC.polygons(name):
            if not any(a[1] == b[1] and a != b for rg in rings for a, b in zip(rg[:-1], rg[1:])):
                continue
            d, loc = PC.polygon_distance(x, y, rings, 0, hyp)
            d1 = PC.polygon_distance(x, y, rings, 1, hyp)[0]
            PC.HORIZONTAL_BRANCH = False
            try:
                dn, locn = PC.polygon_distance(x, y, rings, 0, hyp)
                dn1 = PC.polygon_distance(x, y, rings, 1, hyp)[0]
            finally:
                PC.HORIZONTAL_BRANCH = True
            changed = sum(int((a != b).sum()) for a, b in zip(loc, locn))
            assert changed >= (20 if name != "spike_dup" else 5), (name, changed)
            np.testing.assert_array_equal(bits(dn), bits(d))
            np.testing.assert_array_equal(bits(dn1), bits(d1))


# ---------------------------------------------------------------------------------------------
# the oracle against the reference
# ---------------------------------------------------------------------------------------------
def _probe_subset(name, q, n):
    """Probes compared against polygon q: all of them; on the tiled family the polygon's own probe
    and every 32nd other one."""
    if name != "collinear_tiled":
        return np.arange(n)
    return np.unique(np.concatenate([[q], np.arange(q % 32, n, 32)]))


@pytest.mark.parametrize("name", PC.NAMES)
def test_oracle_point_distances_equal_reference(name, oracle_mod, hyp):
    """orc_point_polygon_distance (both metrics) and orc_point_bbox_distance equal the reference bit
    for bit on every probe."""
    px, py = probe_points(name)
    polys = PC.polygons(name)
    OP = oracle_mod.Polygons(polys)
    for q, rings in enumerate(polys):
        sel = _probe_subset(name, q, len(px))
        x, y = px[sel], py[sel]
        for metric in METRICS:
            ref = PC.polygon_distance(x, y, rings, metric, hyp)[0]
            got = np.array([oracle_mod.point_polygon_distance(a, b, OP, q, metric) for a, b in zip(x, y)])
            np.testing.assert_array_equal(bits(got), bits(ref), err_msg=f"{name} polygon {q} metric {metric}")
        bb = PC.shell_bbox(rings)
        got = np.array([oracle_mod.point_bbox_distance(a, b, *bb) for a, b in zip(x, y)])
        np.testing.assert_array_equal(bits(got), bits(PC.bbox_distance(x, y, bb)), err_msg=f"{name} polygon {q} bbox")


@pytest.mark.parametrize("name", PC.NAMES)
def test_oracle_operators_equal_reference(name, oracle_mod, hyp):
    """orc_range_ppoly, orc_join_ppoly and orc_knn_ppoly_contract equal the reference's operator
    results on the entry's window: both metrics, exact and approximate, every radius of the entry;
    the kNN (one polygon per query: the entry's first 8) at r = 2 cell lengths with k = 7 and with k
    above the number of candidates."""
    x, y, obj, _ = PC.window(name)
    G = PC.Grid()
    og = oracle_mod.grid(PC.GRID_N, *PC.BEIJING)
    polys = PC.polygons(name)
    OP = oracle_mod.Polygons(polys)
    for metric in METRICS:
        for approximate in (False, True):
            if approximate and metric:
                continue   # the bbox distance has one metric
            D = PC.window_distances(name, metric, hyp, approximate=approximate)
            radii = PC.radii(name, metric, hyp)
            if approximate and name == "collinear_tiled":
                radii = radii[:2]   # the bbox distance of 1536 overlapping triangles: r = 0 and TINY
            for r in radii:
                msg = f"{name} metric {metric} approximate {approximate} r {r!r}"
                exp = PC.ref_range_ppoly(G, x, y, polys, r, D)
                assert (len(exp) == 0) == (r == 0.0), msg
                np.testing.assert_array_equal(oracle_mod.range_ppoly(og, x, y, OP, r, approximate, metric), exp, err_msg=msg)
                got = E.sorted_pairs(oracle_mod.join_ppoly(og, og, x, y, OP, r, approximate, metric))
                np.testing.assert_array_equal(got, PC.ref_join_ppoly(G, x, y, polys, r, D, approximate), err_msg=msg)
            for q, rings in enumerate(polys[:8]):
                O1 = oracle_mod.Polygons([rings])
                for k in (7, len(x)):
                    eo, ed, ei = PC.ref_knn_ppoly(G, x, y, obj, rings, PC.KNN_R, k, D[q])
                    m, oo, od, oi = oracle_mod.knn_ppoly(og, x, y, obj, O1, PC.KNN_R, k, approximate, metric)
                    assert m == len(eo) and (k == 7 or 7 < m < k), (name, q, k, m)
                    np.testing.assert_array_equal(oo, eo)
                    np.testing.assert_array_equal(bits(od), bits(ed))
                    np.testing.assert_array_equal(oi, ei)
