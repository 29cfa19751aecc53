"""Shared cases of the linestring-query tests (tests/test_linestring_ref.py on the CPU,
tests/test_gpu_linestring.py on the GPU): a numpy restatement of the reference's point-linestring
geometry and of the three operators built on it, a catalogue of the smallest linestrings that can
still go wrong, and a probe window per shape.

  Point.distance(LineString)  DistanceFunctions.java:38-42: a JTS DistanceOp with no containment
                              step -- the minimum of Distance.pointToSegment over the OPEN chain
                              (poly_cases.ring_min_distance on the chain); DBL_MAX where no segment
                              distance compares below it (a NaN coordinate)
  the approximate distance    getPointLineStringBBoxMinEuclideanDistance, :203-255 = the polygon
                              bbox function (poly_cases.bbox_distance) on the vertex envelope
  the cell sets               UniformGrid.java:208-222, 413-426: per-bbox-cell unions, as for polygons
                              (poly_cases.Grid.poly_cells on the vertex envelope)
  range / kNN / join          PointLineString{Range,KNN,Join}Query.java: the polygon window paths

The C oracle knows no linestrings; tests/test_linestring_ref.py pins this restatement to it where
the two must agree.  No GPU, no torch."""
from __future__ import annotations

import functools

import numpy as np

import edge_cases as E
import poly_cases as PC

BEIJING = PC.BEIJING
GRID_N = PC.GRID_N
CL = PC.CL
DBL_MAX = PC.DBL_MAX
BIG_R = PC.BIG_R                 # guaranteed layers 0 (the bbox cells), candidate layers 3
SMALL_R = 0.5 * CL               # below cl * sqrt(2): guaranteed layers -1, no cell is guaranteed
KNN_R = PC.KNN_R
CHAIN_RUN = 32                   # kChainRun of gf_internal.hpp
CHAIN_PLAIN_RUNS = 2             # kChainPlainRuns: lines of at most this many runs take the plain loop (range, join)
CHAIN_PLAIN_RUNS_KNN = 4         # kChainPlainRunsValue: the same for kNN
JOIN_KEEP = PC.JOIN_KEEP
WINDOW_N = 64 * 37 + 5           # several blocks and a partial last wave
LARGE_N = 20_005                 # the windows of zigzag_4097 and many


# ---------------------------------------------------------------------------------------------
# the restatement: geometry
# ---------------------------------------------------------------------------------------------
def chain_distance(px, py, chain, metric=0, hyp=None):
    """Point.distance(LineString) per point: min over the open chain's segments, DBL_MAX where none
    is taken."""
    px, py = np.asarray(px, np.float64), np.asarray(py, np.float64)
    m = PC.ring_min_distance(px, py, [(float(a), float(b)) for a, b in chain], metric, hyp)
    return np.where(m < DBL_MAX, m, DBL_MAX)


def bbox(chain):
    """(x1, y1, x2, y2): the vertex envelope."""
    minx, maxx, miny, maxy = PC.envelope(chain)
    return minx, miny, maxx, maxy


def bbox_distance(px, py, chain):
    return PC.bbox_distance(px, py, bbox(chain))


def distance_matrix(G, x, y, lines, metric=0, hyp=None, approximate=False):
    """[nline, n]: the (approximate: bbox) distance of every point to every line; +inf where the point
    is more than 4 cells from the line's bbox cells (poly_cases.near_mask: no operator at r <= 3 cell
    lengths asks for those with an answer <= r)."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    D = np.full((len(lines), len(x)), np.inf)
    for q, chain in enumerate(lines):
        m = np.flatnonzero(PC.near_mask(G, x, y, bbox(chain)))
        D[q, m] = bbox_distance(x[m], y[m], chain) if approximate else chain_distance(x[m], y[m], chain, metric, hyp)
    return D


# ---------------------------------------------------------------------------------------------
# the restatement: operators (built like poly_cases.ref_*_ppoly from the G / C cell sets + D)
# ---------------------------------------------------------------------------------------------
def ref_range_pls(G, x, y, lines, r, D):
    """PointLineStringRangeQuery.java:100-172 -> ascending indices: a point of a guaranteed cell, or of
    a candidate cell with some line within r."""
    cx, cy = G.cells(x, y)
    inG = np.zeros(len(cx), bool)
    inC = np.zeros(len(cx), bool)
    for chain in lines:
        g, c = G.poly_cells(cx, cy, bbox(chain), r)
        inG |= g
        inC |= c
    near = (D <= r).any(axis=0) if len(lines) else np.zeros(len(cx), bool)
    return np.flatnonzero(inG | (inC & near))


def ref_join_pls(G, x, y, lines, r, D, approximate=False):
    """PointLineStringJoinQuery.java windowBased -> sorted pairs [m, 2] (point, line): line q is
    replicated to its own guaranteed and candidate cells, a co-located pair is kept if approximate or
    d <= r."""
    cx, cy = G.cells(x, y)
    out = []
    for q, chain in enumerate(lines):
        g, c = G.poly_cells(cx, cy, bbox(chain), r)
        key = g | c
        p = np.flatnonzero(key if approximate else key & (D[q] <= r))
        out.append(np.stack([p, np.full(len(p), q, np.int64)], axis=1))
    out = np.concatenate(out) if out else np.zeros((0, 2), np.int64)
    return out[np.lexsort((out[:, 1], out[:, 0]))].astype(np.int64)


def ref_knn_pls(G, x, y, obj, chain, r, k, d):
    """PointLineStringKNNQuery.java windowBased + KNNQuery.kNNWinAllEvaluationPointStream: points of the
    line's candidate / guaranteed cells with d <= r, one entry per objID (its smallest (d, idx)),
    ordered by (d, objID), the first k -> (objID, d, idx).  d = distance_matrix(...)[0]."""
    cx, cy = G.cells(x, y)
    g, c = G.poly_cells(cx, cy, bbox(chain), r)
    idx = np.flatnonzero((g | c) & (d <= r))
    o, dd = np.asarray(obj, np.int64)[idx], d[idx]
    order = np.lexsort((idx, dd, o))
    o, dd, idx = o[order], dd[order], idx[order]
    first = np.ones(len(o), bool)
    first[1:] = o[1:] != o[:-1]
    o, dd, idx = o[first], dd[first], idx[first]
    order = np.lexsort((o, dd))[:k]
    return o[order], dd[order], idx[order]


def there_and_back(chain):
    """The closed zero-area ring a user without linestring queries passes as a polygon: the chain, then
    the chain reversed (the turning vertex twice, so that a 2-vertex chain still gives 4 vertices)."""
    chain = [(float(a), float(b)) for a, b in chain]
    return chain + chain[::-1]


# ---------------------------------------------------------------------------------------------
# the catalogue
# ---------------------------------------------------------------------------------------------
def zigzag(n, x0, x1, y0=40.3125, amp=CL):
    """n segments from x0 to x1, the ordinate alternating between y0 and y0 + amp."""
    return [(x0 + (x1 - x0) * i / n, y0 + (amp if i % 2 else 0.0)) for i in range(n + 1)]


def _many():
    """300 lines of 2 to 4 vertices, each within one cell length, over a 10 x 10 cell area."""
    rng = np.random.default_rng(300)
    x0, y0 = 116.25, 40.0
    out = []
    for _ in range(300):
        ax, ay = x0 + rng.uniform(0, 10 * CL), y0 + rng.uniform(0, 10 * CL)
        nv = int(rng.integers(2, 5))
        out.append([(ax, ay)] + [(ax + rng.uniform(-CL, CL), ay + rng.uniform(-CL, CL)) for _ in range(nv - 1)])
    return out


# (CHAIN_PLAIN_RUNS * CHAIN_RUN = 64 segments is the longest line that takes the plain loop in the range and join
# kernels, 65 the shortest whose runs are skipped; 128 and 129 are the same pair for kNN)
ZIGZAG_N = (CHAIN_RUN - 1, CHAIN_RUN, CHAIN_RUN + 1, CHAIN_PLAIN_RUNS * CHAIN_RUN, 2 * CHAIN_RUN + 1,
            CHAIN_PLAIN_RUNS_KNN * CHAIN_RUN, CHAIN_PLAIN_RUNS_KNN * CHAIN_RUN + 1, 4097)
ZIGZAGS = tuple(f"zigzag_{n}" for n in ZIGZAG_N)
SQUARE = (116.0, 40.5, 0.09375)     # x, y, side: 4.46 cell lengths, whole cells lie inside it
SINGLE = ("two", "horizontal", "vertical", "point_line", "dup_vertex", "closed_square", "bowtie", "outside") + ZIGZAGS
NAMES = SINGLE + ("many",)
OPEN = tuple(n for n in NAMES if n != "closed_square")   # (the square's first == last makes it the one closed chain)
LARGE = ("zigzag_4097", "many")


@functools.lru_cache(maxsize=None)
def lines(name):
    """The entry's linestrings: a list of vertex lists (one line but for `many`)."""
    if name == "many":
        return _many()
    if name.startswith("zigzag_"):
        n = int(name[7:])
        return [zigzag(n, 115.52, 117.58) if n > 1000 else zigzag(n, 116.6, 116.6 + 14 * CL)]
    sx, sy, ss = SQUARE
    return [{
        "two": [(116.0, 40.0), (116.046875, 40.03125)],
        "horizontal": [(116.0, 40.25), (116.0 + 5.5 * CL, 40.25)],
        "vertical": [(116.25, 40.25), (116.25, 40.25 + 4.5 * CL)],
        "point_line": [(116.3125, 40.125), (116.3125, 40.125)],
        "dup_vertex": [(116.375, 40.25), (116.4375, 40.28125), (116.4375, 40.28125), (116.5, 40.25)],
        "closed_square": [(sx, sy), (sx + ss, sy), (sx + ss, sy + ss), (sx, sy + ss), (sx, sy)],
        "bowtie": [(116.25, 40.5), (116.3125, 40.5625), (116.3125, 40.5), (116.25, 40.5625)],
        "outside": [(117.5625, 40.0), (117.6875, 40.0625), (117.625, 40.125)],
    }[name]]


def extent(name):
    env = [PC.envelope(c) for c in lines(name)]
    return min(e[0] for e in env), max(e[1] for e in env), min(e[2] for e in env), max(e[3] for e in env)


# ---------------------------------------------------------------------------------------------
# probes and windows
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def probes(name):
    """(x, y): the probes poly_cases.shape_probes makes of each line (on vertices, on segment interiors
    and extensions, one and two ulps either side, the vertex ordinates' rays, the envelope's sides),
    the last vertex -- which shape_probes leaves to a ring's closing one -- with its 8 ulp neighbours,
    and for the square a lattice of interior points; for `many`, of every sixth line."""
    px, py = [], []
    cs = lines(name)
    for chain in (cs[::6] if name == "many" else cs):
        a, b = PC.shape_probes([chain])
        px += a
        py += b
        lx, ly = chain[-1]
        for i in (-1, 0, 1):
            for k in (-1, 0, 1):
                px.append(PC.ulps(lx, i))
                py.append(PC.ulps(ly, k))
    if name == "closed_square":
        sx, sy, ss = SQUARE
        for u in np.linspace(0.05, 0.95, 13):
            for v in np.linspace(0.05, 0.95, 13):
                px.append(sx + u * ss)
                py.append(sy + v * ss)
    x, y = np.array(px), np.array(py)
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y


@functools.lru_cache(maxsize=None)
def window(name):
    """(x, y, objID, probe_idx): the probes, two NaN-coordinate points and uniform filler around the
    shape up to WINDOW_N points (LARGE_N for the LARGE entries; the next 64 m + 5 where the probes alone
    exceed it), shuffled with a fixed seed; objIDs repeat.  probe_idx[i] is the window index of probe i."""
    px, py = probes(name)
    rng = np.random.default_rng(sum(map(ord, name)))
    minx, maxx, miny, maxy = extent(name)
    n = LARGE_N if name in LARGE else WINDOW_N
    while n < len(px) + 2 + 200:
        n += 64
    nf = n - len(px) - 2
    x = np.concatenate([px, [np.nan, (minx + maxx) / 2], rng.uniform(minx - 4 * CL, maxx + 4 * CL, nf)])
    y = np.concatenate([py, [(miny + maxy) / 2, np.nan], rng.uniform(miny - 4 * CL, maxy + 4 * CL, nf)])
    perm = rng.permutation(n)
    pidx = np.empty(n, np.int64)
    pidx[perm] = np.arange(n)
    x, y = x[perm], y[perm]
    obj = (np.arange(n) % max(1, n // 3)).astype(np.int64)
    probe_idx = pidx[:len(px)]
    for a in (x, y, obj, probe_idx):
        a.setflags(write=False)
    assert n % 64 != 0 and n >= WINDOW_N
    return x, y, obj, probe_idx


_DIST = {}


def window_distances(name, metric, hyp, approximate=False):
    """distance_matrix of the entry's window on the n = 100 grid, computed once and left unchanged."""
    key = (name, metric, approximate)
    if key not in _DIST:
        x, y, _, _ = window(name)
        D = distance_matrix(PC.Grid(), x, y, lines(name), metric, hyp, approximate)
        D.setflags(write=False)
        _DIST[key] = D
    return _DIST[key]


def realized_radii(name, metric, hyp):
    """[d]: realized distances of in-grid window points (the smallest nonzero one, about 0.3 and about
    1.2 cell lengths: below cl * sqrt(2), so that no cell is guaranteed and the point at d flips between
    r = d and its lower neighbour), as poly_cases.realized_radii takes them."""
    x, y, _, _ = window(name)
    d = window_distances(name, metric, hyp).min(axis=0)
    cx, cy = PC.Grid().cells(x, y)
    ok = np.isfinite(d) & (d > 0) & (d < 1.3 * CL) & PC.Grid().valid(cx, cy)
    cand = np.sort(d[ok])
    out = [float(cand[0])] + [float(cand[np.argmin(np.abs(cand - t * CL))]) for t in (0.3, 1.2)]
    return list(dict.fromkeys(out))


def radii(name, metric, hyp):
    """Every radius of the entry: 0 (no cells: empty results), each realized distance with its two
    neighbours, SMALL_R (no guaranteed cell) and BIG_R (guaranteed cells exist)."""
    out = [0.0]
    for d in realized_radii(name, metric, hyp):
        out += [E.toward0(d), d, E.nxt(d)]
    return list(dict.fromkeys(out + [SMALL_R, BIG_R]))
