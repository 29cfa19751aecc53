"""Windows of the tRange / tFilter tests (tests/test_trange_ref.py, tests/test_gpu_trange.py).  The polygon
catalogue, its probes and its windows are tests/poly_cases.py's, imported as they are; this module adds the
objID assignments, the hand vector with its rows written out, the grid-edge and inside-cell cases.  A
case is (x, y, objID, ts, polys): polys as poly_cases.polygons gives them (closed rings, shell first)."""
import functools

import numpy as np

import poly_cases as PC

BEIJING = PC.BEIJING
CL = PC.CL
MODES = ("each", "mod", "one")


def ts_of(n):
    return 1_600_000_000_000 + (np.arange(n, dtype=np.int64) * 7919) % 1000


def objids(n, mode):
    """each: one objID per point (every boundary and hole point decides a row alone); mod: i % (n // 3);
    one: a single objID for the whole window"""
    if mode == "each":
        return np.arange(n, dtype=np.int64) * 3 + 11
    if mode == "mod":
        return (np.arange(n) % max(1, n // 3)).astype(np.int64)
    return np.full(n, 42, np.int64)


@functools.lru_cache(maxsize=None)
def shape_case(name, mode):
    x, y, _, _ = PC.window(name)
    return x, y, objids(len(x), mode), ts_of(len(x)), PC.polygons(name)


def _rect(x1, y1, x2, y2):
    return [(x1, y1), (x2, y1), (x2, y2), (x1, y2), (x1, y1)]


# The hand vector: a square (0,0)-(8,8) with the hole (2,2)-(6,6), an 8 x 8 grid of unit cells over it.
# objID, x, y, ts
HAND_GRID = (8, (0.0, 8.0, 0.0, 8.0))
HAND_POLYS = [[_rect(0.0, 0.0, 8.0, 8.0), _rect(2.0, 2.0, 6.0, 6.0)]]
HAND_ROWS = [
    (7, 9.0, 9.0, 100),    # 0  objID 7: outside
    (5, 8.0, 4.0, 101),    # 1  objID 5: only ever on the shell edge
    (9, 2.0, 3.0, 102),    # 2  objID 9: only ever on the hole edge
    (7, 1.0, 1.0, 103),    # 3  objID 7: interior -> 7 is hit
    (3, 4.0, 4.0, 104),    # 4  objID 3: only ever in the hole
    (5, 0.0, 0.0, 105),    # 5  a shell vertex
    (9, 6.0, 6.0, 106),    # 6  a hole vertex
    (7, 4.0, 4.0, 107),    # 7  in the hole
    (3, 3.0, 5.0, 108),    # 8  in the hole
    (5, 4.0, 8.0, 109),    # 9  on the shell edge
    (9, 4.0, 2.0, 110),    # 10 on the hole edge
    (3, 9.5, 4.0, 111),    # 11 outside
]
HAND_EXPECT = {"keys": [7], "off": [0, 3], "idx": [0, 3, 7], "points": [3]}


def hand_case():
    a = np.array(HAND_ROWS, np.float64)
    return a[:, 1].copy(), a[:, 2].copy(), a[:, 0].astype(np.int64), a[:, 3].astype(np.int64), HAND_POLYS


@functools.lru_cache(maxsize=None)
def grid_edge_case():
    """A polygon straddling the grid's upper-right corner, one wholly outside the grid (left of it), one
    well inside; points inside each, in-grid and out-of-grid, and random points across the grid's border."""
    x1, y1 = BEIJING[1], BEIJING[3]
    corner = [[(x1 - 2.5 * CL, y1 - 1.5 * CL), (x1 + 3.25 * CL, y1 - 0.5 * CL), (x1 + 1.5 * CL, y1 + 2.75 * CL),
               (x1 - 1.25 * CL, y1 + 1.5 * CL), (x1 - 2.5 * CL, y1 - 1.5 * CL)]]
    outside = [_rect(BEIJING[0] - 9.5 * CL, 40.0, BEIJING[0] - 3.25 * CL, 40.0 + 4.5 * CL),
               _rect(BEIJING[0] - 8.0 * CL, 40.0 + CL, BEIJING[0] - 5.0 * CL, 40.0 + 3.0 * CL)]
    inner = [[(116.0, 40.0), (116.0 + 3.5 * CL, 40.0 + 0.5 * CL), (116.0 + 1.5 * CL, 40.0 + 2.5 * CL), (116.0, 40.0)]]
    polys = [corner, outside, inner]
    rng = np.random.default_rng(77)
    xs, ys = [], []
    for rings in polys:
        minx, maxx, miny, maxy = PC.envelope(rings[0])
        xs.append(rng.uniform(minx - CL, maxx + CL, 900))
        ys.append(rng.uniform(miny - CL, maxy + CL, 900))
    xs.append(rng.uniform(BEIJING[0] - 12 * CL, BEIJING[1] + 5 * CL, 1500))
    ys.append(rng.uniform(BEIJING[2] - 3 * CL, BEIJING[3] + 5 * CL, 1500))
    # a point outside the grid inside the straddling polygon, one inside the grid inside it, the corner itself
    xs.append(np.array([x1 + 1.0 * CL, x1 - 1.0 * CL, x1, np.inf, -np.inf, x1 + 0.5 * CL]))
    ys.append(np.array([y1 + 1.0 * CL, y1 - 0.25 * CL, y1, y1, y1, np.inf]))
    x, y = np.concatenate(xs), np.concatenate(ys)
    n = len(x)
    return x, y, (np.arange(n) % 601).astype(np.int64), ts_of(n), polys


@functools.lru_cache(maxsize=None)
def inside_case():
    """A rectangle covering several whole cells of the 100 x 100 grid (cells 20..26 x 30..34 hold its
    edges; 21..25 x 31..33 are inside), points exactly on its edges, on the cell thresholds inside it and one
    ulp either side of each; plus a rectangle over cell 0 from outside the grid (cell (0, 0) inside) and
    NaN points, which land in cell (0, 0)."""
    gx = lambda c: BEIJING[0] + c * CL
    gy = lambda c: BEIJING[2] + c * CL
    R = (gx(20.5), gy(30.25), gx(26.5), gy(34.75))
    Z = (gx(-1.5), gy(-1.5), gx(1.5), gy(1.5))
    polys = [[_rect(R[0], R[1], R[2], R[3])], [_rect(Z[0], Z[1], Z[2], Z[3])]]
    xs, ys = [], []
    edge_x = [R[0], R[2]] + [gx(c) for c in range(20, 28)]
    edge_y = [R[1], R[3]] + [gy(c) for c in range(30, 36)]
    for ex in edge_x:
        for k in (-1, 0, 1):
            for ey in edge_y:
                for m in (-1, 0, 1):
                    xs.append(PC.ulps(ex, k))
                    ys.append(PC.ulps(ey, m))
    rng = np.random.default_rng(5)
    rx = rng.uniform(gx(19), gx(28), 3000)
    ry = rng.uniform(gy(29), gy(36), 3000)
    zx = rng.uniform(gx(-2.5), gx(2.5), 600)
    zy = rng.uniform(gy(-2.5), gy(2.5), 600)
    nanx = [np.nan, gx(0.5), np.nan]
    nany = [gy(0.5), np.nan, np.nan]
    x = np.concatenate([xs, rx, zx, nanx])
    y = np.concatenate([ys, ry, zy, nany])
    n = len(x)
    return x, y, np.arange(n, dtype=np.int64), ts_of(n), polys


def extra_cases():
    return {"hand": hand_case(), "grid_edge": grid_edge_case(), "inside": inside_case()}


def grid_of(case_name):
    """(n, box) of a case's grid"""
    return HAND_GRID if case_name == "hand" else (PC.GRID_N, BEIJING)
