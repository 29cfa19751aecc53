"""Shared case generator of the numeric-edge tests (tests/test_numeric_edges.py on the CPU,
tests/test_gpu_numeric_edges.py on the GPU): a catalogue of grids chosen for what their arithmetic
reaches, a window per grid that sits on and around every cell edge, queries, radii taken from
realized distances -- and an INDEPENDENT reference of the operators in plain numpy float64
(element-wise IEEE arithmetic, unfused: what Java computes).  The reference never calls the C
oracle, except for the hypot metric's distance values, which the CPU tests first tie to exact
rational arithmetic (within 1 ulp).  No GPU, no torch."""
from __future__ import annotations

import functools
import math
from fractions import Fraction

import numpy as np

BEIJING = (115.5, 117.6, 39.6, 41.1)
U = 2.0 ** -12          # spacing of doubles in [2^40, 2^41)
P40 = 2.0 ** 40

# name -> (n, minX, maxX, minY, maxY)
GRIDS = {
    "beijing100": (100, *BEIJING),                                        # control
    "world360": (360, -180.0, 180.0, -90.0, 90.0),                        # cl == 1.0; negative coordinates
    "unit7": (7, -1.0, 1.0, -1.0, 1.0),                                   # straddles 0; cl = 2/7; one-pass radix
    "metres2048": (2048, 1.2e7, 1.2e7 + 41234.5, 4.8e6, 4.8e6 + 41234.5),  # largest division-free grid
    "beijing2049": (2049, *BEIJING),                                      # first grid on the division path
    "ulp5": (64, P40, P40 + 320 * U, P40, P40 + 320 * U),                 # every cell holds exactly 5 doubles
    "subulp": (2048, P40, P40 + 0.25, P40, P40 + 0.25),                   # two cells per double
}
LATTICE = ("ulp5", "subulp")
EDGE = tuple(k for k in GRIDS if k not in LATTICE)
LATTICE_QUERY_J = (162, 158)
# lattice radii (in units of U) -> (points within r, points exactly at r): integer points of the disc
LATTICE_COUNTS = {25: (1961, 20), 65: (13273, 36)}


def cell_length(name):
    n, x0, x1, _, _ = GRIDS[name]
    return (x1 - x0) / n


def prev(v):
    return float(np.nextafter(v, -np.inf))


def nxt(v):
    return float(np.nextafter(v, np.inf))


def toward0(v):
    return float(np.nextafter(v, 0.0))


# ---------------------------------------------------------------------------------------------
# the independent reference
# ---------------------------------------------------------------------------------------------
def ref_jint(q):
    """Java (int) of a double: NaN -> 0, saturate, else truncate."""
    q = np.atleast_1d(np.asarray(q, np.float64))
    out = np.zeros(q.shape, np.int64)
    ok = ~np.isnan(q)
    out[ok] = np.trunc(np.clip(q[ok], -2147483648.0, 2147483647.0)).astype(np.int64)
    return out.astype(np.int32)


def ref_cells(v, mn, cl):
    """jint(floor((v - mn) / cl)), element-wise."""
    with np.errstate(all="ignore"):
        return ref_jint(np.floor((np.asarray(v, np.float64) - mn) / cl))


def ref_layers(cl, r):
    """(guaranteed, candidate) layers: jint(floor(r / (cl * sqrt(2)) - 1)), jint(ceil(r / cl))."""
    with np.errstate(all="ignore"):
        cl, r = np.float64(cl), np.float64(r)
        g = ref_jint(np.floor(r / (cl * np.sqrt(np.float64(2.0))) - np.float64(1.0)))[0]
        c = ref_jint(np.ceil(r / cl))[0]
    return int(g), int(c)


def ref_dist(x, y, qx, qy, metric, hyp=None, bound=None):
    """Distances of the points to (qx, qy).  metric 0: sqrt(dx*dx + dy*dy).  metric 1: `hyp`
    (an array function of (dx, dy): the hypot the CPU tests tie to rational arithmetic).  With
    `bound`, hyp is only evaluated where it can matter: the sqrt form is within 3 ulps and hyp
    within 1 ulp of the true distance, so a point whose sqrt form exceeds bound * (1 + 1e-9) has
    hyp > bound; it is reported as +inf."""
    with np.errstate(all="ignore"):
        dx = np.float64(qx) - np.asarray(x, np.float64)
        dy = np.float64(qy) - np.asarray(y, np.float64)
        d0 = np.sqrt(dx * dx + dy * dy)
    if metric == 0:
        return d0
    need = ~np.isnan(d0) if bound is None else d0 <= bound * (1 + 1e-9)
    d = np.full(d0.shape, np.inf)
    d[np.isnan(d0)] = np.nan
    d[need] = hyp(dx[need], dy[need])
    return d


class RefGrid:
    def __init__(self, name):
        self.name = name
        self.n, self.minX, self.maxX, self.minY, self.maxY = GRIDS[name]
        self.cl = (self.maxX - self.minX) / self.n

    def cells(self, x, y):
        return ref_cells(x, self.minX, self.cl).astype(np.int64), ref_cells(y, self.minY, self.cl).astype(np.int64)

    def valid(self, cx, cy):
        return (cx >= 0) & (cy >= 0) & (cx < self.n) & (cy < self.n)


def _cell_sets(G: RefGrid, cx, cy, qcells, r):
    """(inG, inC): the window's points in a guaranteed cell / within the candidate layers of some
    query (valid cells only; guaranteed layers == 0 is the query cell itself)."""
    gl, cL = ref_layers(G.cl, r)
    valid = G.valid(cx, cy)
    inG = np.zeros(len(cx), bool)
    inC = np.zeros(len(cx), bool)
    for qcx, qcy in qcells:
        ax, ay = np.abs(cx - qcx), np.abs(cy - qcy)
        if gl == 0:
            inG |= (ax == 0) & (ay == 0)
        elif gl > 0:
            inG |= valid & (ax <= gl) & (ay <= gl)
        if cL > 0:
            inC |= valid & (ax <= cL) & (ay <= cL)
    return inG, inC


def _query_cells(G: RefGrid, qx, qy):
    qcx, qcy = G.cells(np.atleast_1d(qx), np.atleast_1d(qy))
    assert G.valid(qcx, qcy).all(), "the catalogue's queries lie inside their grid"
    return list(zip(qcx.tolist(), qcy.tolist()))


def ref_range_pp(name, x, y, qx, qy, r, approximate=False, metric=0, hyp=None, info=None):
    """The window-based point-point range query -> the emitted multiset of indices, ascending
    (a candidate-cell point of an approximate query once per query point).  info (a dict) receives
    the candidate-cell points' hit / miss counts."""
    G = RefGrid(name)
    qx, qy = np.atleast_1d(np.asarray(qx, np.float64)), np.atleast_1d(np.asarray(qy, np.float64))
    cx, cy = G.cells(x, y)
    inG, inC = _cell_sets(G, cx, cy, _query_cells(G, qx, qy), r)
    cand = inC & ~inG
    if approximate:
        out = np.concatenate([np.flatnonzero(inG)] + [np.flatnonzero(cand)] * len(qx))
        return np.sort(out, kind="stable")
    hit = np.zeros(len(cx), bool)
    for a, b in zip(qx, qy):
        hit |= ref_dist(x, y, a, b, metric, hyp, r) <= r
    if info is not None:
        info["cand_hit"] = int((cand & hit).sum())
        info["cand_miss"] = int((cand & ~hit).sum())
    return np.flatnonzero(inG | (cand & hit))


def ref_knn(name, x, y, obj, qx, qy, r, k, metric=0, hyp=None):
    """kNN contract: points of the candidate / guaranteed cells with d <= r, one entry per objID
    (its smallest (d, idx)), ordered by (d, objID), the first k -> (objID, d, idx)."""
    G = RefGrid(name)
    cx, cy = G.cells(x, y)
    inG, inC = _cell_sets(G, cx, cy, _query_cells(G, qx, qy), r)
    d = ref_dist(x, y, qx, qy, metric, hyp, r)
    idx = np.flatnonzero((inG | inC) & (d <= r))
    o, dd = np.asarray(obj, np.int64)[idx], d[idx]
    order = np.lexsort((idx, dd, o))
    o, dd, idx = o[order], dd[order], idx[order]
    first = np.ones(len(o), bool)
    first[1:] = o[1:] != o[:-1]
    o, dd, idx = o[first], dd[first], idx[first]
    order = np.lexsort((o, dd))[:k]
    return o[order], dd[order], idx[order]


def ref_join_pp(name, ox, oy, qx, qy, r, approximate=False, metric=0, hyp=None, info=None):
    """Point-point window join on one grid -> sorted pairs [m, 2] (ordinary index, query index):
    query q is replicated to the valid cells within the candidate layers of its cell (r == 0: to
    every cell), a pair is kept if approximate or d <= r."""
    G = RefGrid(name)
    cx, cy = G.cells(ox, oy)
    valid = G.valid(cx, cy)
    qcx, qcy = G.cells(qx, qy)
    cL = ref_layers(G.cl, r)[1]
    assert r == 0 or cL > 0
    pairs, nh, nm = [], 0, 0
    for q in range(len(qx)):
        m = valid.copy()
        if r != 0:
            m &= (np.abs(cx - qcx[q]) <= cL) & (np.abs(cy - qcy[q]) <= cL)
        p = np.flatnonzero(m)
        if not approximate:
            h = ref_dist(ox[p], oy[p], qx[q], qy[q], metric, hyp, r) <= r
            nh += int(h.sum())
            nm += int((~h).sum())
            p = p[h]
        pairs.append(np.stack([p, np.full(len(p), q, np.int64)], axis=1))
    if info is not None:
        info["cand_hit"], info["cand_miss"] = nh, nm
    out = np.concatenate(pairs) if pairs else np.zeros((0, 2), np.int64)
    return out[np.lexsort((out[:, 1], out[:, 0]))].astype(np.int64)


def exact_hypot_ulps(a, b, h):
    """|h - sqrt(a^2 + b^2)| in ulps of h, decided in exact rational arithmetic: returns True when
    h is within 1 ulp of the true value (finite inputs, h finite and > 0 or the true value 0)."""
    t2 = Fraction(a) ** 2 + Fraction(b) ** 2
    if t2 == 0:
        return h == 0.0
    ulp = Fraction(math.ulp(h))
    lo, hi = Fraction(h) - ulp, Fraction(h) + ulp
    return (lo <= 0 or lo * lo <= t2) and t2 <= hi * hi


# ---------------------------------------------------------------------------------------------
# windows
# ---------------------------------------------------------------------------------------------
def _ulps(v, k):
    v = np.asarray(v, np.float64).copy()
    for _ in range(abs(k)):
        v = np.nextafter(v, np.inf if k > 0 else -np.inf)
    return v


def _edge_family(mn, cl, n):
    """(values, c): min + c*cl for c = -2..n+2 with its +-1, +-2, +-3 ulp neighbours.  Where the
    edge is smaller in magnitude than the origin (an edge at or near 0.0 of a grid with a negative
    origin), v - mn absorbs those ulps, so the neighbours at +-1..3 ulps of the ORIGIN's size are
    added: they are the doubles that fall on the two sides of the edge."""
    c = np.arange(-2, n + 3)
    e = mn + c.astype(np.float64) * cl
    vals = [_ulps(e, k) for k in (-3, -2, -1, 0, 1, 2, 3)]
    tags = [c] * 7
    step = np.spacing(np.abs(np.float64(mn)))
    coarse = np.spacing(np.abs(e)) < step
    for k in (-3, -2, -1, 1, 2, 3):
        vals.append(e[coarse] + k * step)
        tags.append(c[coarse])
    return np.concatenate(vals), np.concatenate(tags)


@functools.lru_cache(maxsize=None)
def window(name):
    """(x, y, objID) of the grid's window -- read-only arrays, shared by every test."""
    n, x0, x1, y0, y1 = GRIDS[name]
    cl = cell_length(name)
    if name in LATTICE:
        j = np.arange(-5, 325)
        jx, jy = np.repeat(j, len(j)), np.tile(j, len(j))
        x, y = x0 + jx * U, y0 + jy * U
        obj = (jx % 97).astype(np.int64)
    else:
        rng = np.random.default_rng(sum(map(ord, name)))
        ex, ey = _edge_family(x0, cl, n)[0], _edge_family(y0, cl, n)[0]
        ix, iy = np.arange(len(ex)), np.arange(len(ey))
        # partners on the other axis: uniform inside the grid / an edge value of that axis
        py = np.where(ix % 2 == 0, rng.uniform(y0, y0 + n * cl, len(ex)), ey[(ix * 13 + 3) % len(ey)])
        px = np.where(iy % 2 == 0, rng.uniform(x0, x0 + n * cl, len(ey)), ex[(iy * 11 + 5) % len(ex)])
        sp = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1e300, -1e300])
        mx, my = x0 + (n / 2 + 0.25) * cl, y0 + (n / 2 + 0.25) * cl
        sx = np.concatenate([sp, np.full(len(sp), mx), sp])
        sy = np.concatenate([np.full(len(sp), my), sp, sp[::-1]])
        w, h = n * cl, n * cl
        ux = rng.uniform(x0 - 0.05 * w, x0 + 1.05 * w, 20_000)
        uy = rng.uniform(y0 - 0.05 * h, y0 + 1.05 * h, 20_000)
        # around every query: the point itself and 60 points within 7 cells, so that small radii
        # have realized distances too
        qs = queries(name)
        rad, ang = rng.uniform(0.0, 7.0 * cl, (len(qs), 60)), rng.uniform(0.0, 2 * np.pi, (len(qs), 60))
        nx = np.concatenate([[q[0] for q in qs]] + [q[0] + rad[i] * np.cos(ang[i]) for i, q in enumerate(qs)])
        ny = np.concatenate([[q[1] for q in qs]] + [q[1] + rad[i] * np.sin(ang[i]) for i, q in enumerate(qs)])
        x = np.concatenate([ex, px, sx, ux, nx])
        y = np.concatenate([py, ey, sy, uy, ny])
        obj = (np.arange(len(x)) % 4099).astype(np.int64)   # duplicates: a few points per objID
    for a in (x, y, obj):
        a.setflags(write=False)
    assert len(x) <= 110_000
    return x, y, obj


def second_window(name):
    """A second window on the same grid (kNN across consecutive windows): the first one reversed."""
    x, y, obj = window(name)
    return x[::-1].copy(), y[::-1].copy(), obj[::-1].copy()


def queries(name):
    """[(qx, qy)]: on a cell corner, at a cell centre, in the grid's last cell."""
    n, x0, _, y0, _ = GRIDS[name]
    cl = cell_length(name)
    if name in LATTICE:   # lattice points: the issue's query, a cell centre of ulp5, its last cell
        js = [LATTICE_QUERY_J, (102, 207), (317, 317) if name == "ulp5" else (250, 290)]
        return [(x0 + jx * U, y0 + jy * U) for jx, jy in js]
    a, b = n // 2, n // 3
    return [(x0 + a * cl, y0 + b * cl), (x0 + (b + 0.5) * cl, y0 + (a + 0.5) * cl),
            (x0 + (n - 0.5) * cl, y0 + (n - 0.5) * cl)]


def in_grid(name):
    G = RefGrid(name)
    x, y, _ = window(name)
    return G.valid(*G.cells(x, y)) & np.isfinite(x) & np.isfinite(y)


def on_edge_count(name):
    """In-grid points of the window that sit exactly on a cell edge as the reference computes it:
    a coordinate that is the first double of its cell (the double just below lies in the cell
    before)."""
    G = RefGrid(name)
    x, y, _ = window(name)
    ok = in_grid(name)
    on = np.zeros(int(ok.sum()), bool)
    for v, mn in ((x[ok], G.minX), (y[ok], G.minY)):
        on |= ref_cells(v, mn, G.cl) != ref_cells(np.nextafter(v, -np.inf), mn, G.cl)
    return int(on.sum())


def realized_radii(name, q, metric, hyp=None):
    """[(r, d)]: for three realized distances d of in-grid points to q under `metric` (small,
    about 1.5 cells, about 6 cells -- at most half the grid, so that candidate cells keep misses;
    the lattice: 25 U and 65 U), r = d and r = nextafter(d, 0)."""
    x, y, _ = window(name)
    cl = cell_length(name)
    if name in LATTICE:
        ds = [25 * U, 65 * U]
    else:
        ok = in_grid(name)
        d = ref_dist(x[ok], y[ok], q[0], q[1], metric, hyp)
        d = d[np.isfinite(d) & (d > 0)]
        ds = [float(d[np.argmin(np.abs(d - t * cl))]) for t in (0.3, 1.5, min(6.0, GRIDS[name][0] / 2))]
    out = []
    for v in ds:
        out += [(v, v), (toward0(v), v)]
    return out


def layer_radii(name):
    """r = cl, cl * sqrt(2) and the two neighbours of each (where the layer counts change), r = 0."""
    cl = cell_length(name)
    out = []
    for v in (cl, cl * math.sqrt(2.0)):
        out += [prev(v), v, nxt(v)]
    return out + [0.0]


def assert_realized_case(name, q, r_at, metric, hyp=None):
    """The non-vacuity conditions of an (r = d, r = nextafter(d, 0)) pair of range cases, from the
    reference alone: some point exactly at r; the two results differ by exactly the points at r;
    hits and misses among the candidate-cell points.  Returns the number of points exactly at r."""
    x, y, _ = window(name)
    i1, i0 = {}, {}
    a = ref_range_pp(name, x, y, q[0], q[1], r_at, False, metric, hyp, i1)
    b = ref_range_pp(name, x, y, q[0], q[1], toward0(r_at), False, metric, hyp, i0)
    G = RefGrid(name)
    cx, cy = G.cells(x, y)
    inG, inC = _cell_sets(G, cx, cy, _query_cells(G, q[0], q[1]), r_at)
    d = ref_dist(x, y, q[0], q[1], metric, hyp, r_at)
    at = np.flatnonzero((inG | inC) & (d == r_at))
    assert len(at) >= 1, (name, q, r_at, metric)
    # a guaranteed cell accepts its points untested: those stay in both results
    inG0, _ = _cell_sets(G, cx, cy, _query_cells(G, q[0], q[1]), toward0(r_at))
    np.testing.assert_array_equal(np.setdiff1d(a, b), at[~inG0[at]], err_msg=f"{name} {q} r={r_at!r} metric {metric}")
    assert len(np.setdiff1d(b, a)) == 0
    assert i1["cand_hit"] >= 1 and i1["cand_miss"] >= 1, (name, q, r_at, i1)
    return len(at)


def assert_lattice_counts(name, metric, hyp=None):
    """The issue's lattice figures, from the reference: points within r and exactly at r of the
    query (162 U, 158 U), both metrics the same sets, and nextafter(r, 0) drops exactly the latter."""
    x, y, _ = window(name)
    q = queries(name)[0]
    for ru, (within, at) in LATTICE_COUNTS.items():
        r = ru * U
        a = ref_range_pp(name, x, y, q[0], q[1], r, False, metric, hyp)
        b = ref_range_pp(name, x, y, q[0], q[1], toward0(r), False, metric, hyp)
        d = ref_dist(x, y, q[0], q[1], metric, hyp)
        assert len(a) == within == int((d <= r).sum()), (name, ru, len(a))
        assert int((d == r).sum()) == at
        np.testing.assert_array_equal(np.setdiff1d(a, b), np.flatnonzero(d == r))
        if name == "ulp5":
            assert ref_layers(cell_length(name), r) == {25: (2, 5), 65: (8, 13)}[ru]


def assert_edges_straddled(name):
    """Every tested edge c = 0..n of both axes has window points in cell c - 1 and in cell c among
    its +-3 ulp family (reference cells)."""
    n, x0, _, y0, _ = GRIDS[name]
    cl = cell_length(name)
    for mn in (x0, y0):
        v, tag = _edge_family(mn, cl, n)
        c = ref_cells(v, mn, cl)
        below = np.bincount(tag[(c == tag - 1) & (tag >= 0)], minlength=n + 3)[:n + 1]
        above = np.bincount(tag[(c == tag) & (tag >= 0)], minlength=n + 3)[:n + 1]
        assert (below > 0).all() and (above > 0).all(), (name, np.flatnonzero((below == 0) | (above == 0)))


def bucket_expected(name, x, y):
    """keyBy(gridID) restated on the reference cells: bucket = valid cell cy*n + cx (out-of-grid
    last), a bucket's points in arrival order -> (perm, cell_start)."""
    G = RefGrid(name)
    cx, cy = G.cells(x, y)
    key = np.where(G.valid(cx, cy), cy * G.n + cx, G.n * G.n)
    perm = np.argsort(key, kind="stable")
    start = np.searchsorted(key[perm], np.arange(G.n * G.n + 2), side="left")
    return perm, start


def sorted_pairs(p):
    p = np.asarray(p, np.int64).reshape(-1, 2)
    return p[np.lexsort((p[:, 1], p[:, 0]))]


# ---------------------------------------------------------------------------------------------
# the cases both test files run (the CPU file ties the oracle to the reference on exactly these)
# ---------------------------------------------------------------------------------------------
def query_sets(name):
    """[(tag, [(qx, qy)])]: each catalogue query alone (the arithmetic path) and the three together
    (the table path)."""
    qs = queries(name)
    return [("corner", qs[:1]), ("centre", qs[1:2]), ("last", qs[2:]), ("three", qs)]


def _dedupe(v):
    return list(dict.fromkeys(v))


def range_cases(name, hyp):
    """[(tag, qx, qy, r, metric)]: every query set at its realized radii and their lower
    neighbours (realized for the set's first query), the corner and the three-query set also at the
    radii where the layer counts change and at r = 0."""
    out = []
    for tag, qs in query_sets(name):
        for metric in (0, 1):
            rs = [r for r, _ in realized_radii(name, qs[0], metric, hyp)]
            if tag in ("corner", "three"):
                rs += layer_radii(name)
            for r in _dedupe(rs):
                out.append((tag, [q[0] for q in qs], [q[1] for q in qs], r, metric))
    return out


def knn_ks(name):
    """k of the kNN cases; on the lattice also a k that cuts through a group of exactly tied
    distances (objIDs j_x % 97: an objID's nearest point is its column's, so the distances tie in
    pairs, columns j_q - m and j_q + m, and an even k cuts a pair)."""
    return (1, 7, 50) + ((20,) if name in LATTICE else ())


def knn_cases(name, hyp):
    """[(qx, qy, r, metric, k)]: the corner and the last-cell query at the realized radii and the
    lower neighbours of the two larger ones with k = 50, every other k at the middle radius."""
    out = []
    qs = queries(name)
    for q in (qs[0], qs[2]):
        for metric in (0, 1):
            rr = realized_radii(name, q, metric, hyp)
            rs = _dedupe([r for r, _ in rr] if name in LATTICE else [rr[0][0]] + [r for r, _ in rr[2:]])
            out += [(q[0], q[1], r, metric, 50) for r in rs]
            mid = rr[0][0] if name in LATTICE else rr[2][0]
            out += [(q[0], q[1], mid, metric, k) for k in knn_ks(name) if k != 50]
    return out


def join_query_side(name):
    """Indices of the 200 window points that form the join's query side: the catalogue queries
    (they are window points), the special values, and an even sample of the rest."""
    x, y, _ = window(name)
    idx = []
    for q in queries(name):
        idx.append(int(np.flatnonzero((x == q[0]) & (y == q[1]))[0]))
    idx += np.flatnonzero(~(np.isfinite(x) & np.isfinite(y)) | (np.abs(x) >= 1e300) | (np.abs(y) >= 1e300)).tolist()
    idx += np.arange(7, len(x), max(1, len(x) // 230)).tolist()
    return np.array(_dedupe(idx)[:200], np.int64)


def join_cases(name, hyp):
    """[(r, metric)]: realized distances between window points and the first query-side point (small,
    about 1.5 cells and its lower neighbour; the lattice: 5 U = a 3-4-5 triangle, and on ulp5 25 U),
    the radii around r = cl where the candidate layer count changes, and r = 0 on the grids small
    enough for the reference's replication of every query point to every cell."""
    cl = cell_length(name)
    out = []
    for metric in (0, 1):
        if name in LATTICE:
            rs = [5 * U, toward0(5 * U)] + ([25 * U, toward0(25 * U)] if name == "ulp5" else [])
        else:
            rr = realized_radii(name, queries(name)[0], metric, hyp)
            rs = [rr[0][0], rr[2][0], rr[3][0], cl, nxt(cl)]
        if GRIDS[name][0] <= 100:
            rs.append(0.0)
        out += [(r, metric) for r in _dedupe(rs)]
    return out
