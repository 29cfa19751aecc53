"""Case builders of the geometry-window tests (tests/test_geomwin_ref.py on the CPU,
tests/test_gpu_geomwin.py on the GPU): small windows of polygons and linestrings on a 10 x 10 unit grid
(cell length exactly 1) and on the 100 x 100 Beijing grid, with the query point sets that go with them.
A case is a dict: kind, grid = (n, box), objs (polygons: lists of rings; linestrings: chains), keys (objID
keys) and queries = {name: (qx, qy)}.  No GPU, no torch."""
from __future__ import annotations

import functools
import math
import random

import numpy as np

import poly_cases as PC

POLYGON, LINESTRING = 1, 2
UNIT = (10, (0.0, 10.0, 0.0, 10.0))            # cell length 1.0
BEIJING = (PC.GRID_N, PC.BEIJING)
INT32_MAX = 2 ** 31 - 1
THRESHOLDS = (1, 64, INT32_MAX)                 # wide_vertices: every object by waves, the middle, lanes only
R_G1 = 3.0     # unit grid: guaranteed layers 1, candidate layers 3
R_G0 = 1.6     # guaranteed layers 0 (the query cell), candidate layers 2
R_GM1 = 0.75   # guaranteed layers -1 (no G), candidate layers 1


def square(x, y, s):
    return [(x, y), (x + s, y), (x + s, y + s), (x, y + s), (x, y)]


def triangle(x, y, s):
    """a 4-vertex closed ring"""
    return [(x, y), (x + s, y), (x, y + s), (x, y)]


def ngon(cx, cy, rad, nv):
    """a closed ring of nv vertices (nv - 1 distinct)"""
    m = nv - 1
    pts = [(cx + rad * math.cos(2 * math.pi * i / m), cy + rad * math.sin(2 * math.pi * i / m)) for i in range(m)]
    return pts + [pts[0]]


def zigzag(x0, y0, dx, amp, nv):
    return [(x0 + dx * i, y0 + (amp if i & 1 else 0.0)) for i in range(nv)]


def _case(kind, grid, objs, queries, keys=None):
    keys = np.arange(len(objs), dtype=np.int64) if keys is None else np.asarray(keys, np.int64)
    return dict(kind=kind, grid=grid, objs=objs, keys=keys,
                queries={k: (np.array(v[0], np.float64), np.array(v[1], np.float64)) for k, v in queries.items()})


QUERIES_UNIT = {
    "one": ([5.5], [5.5]),
    "two_overlapping": ([5.5, 6.2], [5.5, 5.5]),
    "borders": ([0.5, 9.5, 5.5, 5.5], [5.5, 5.5, 0.5, 9.5]),          # four disjoint squares, each cut by the grid
    "five": ([1.5, 2.2, 8.5, 5.5, 5.6], [1.5, 1.7, 8.5, 5.5, 5.4]),   # overlapping pairs and a disjoint one
    "outside": ([-0.4], [5.5]),                                       # a query point outside the grid
}

HOLED = [square(3.0, 3.0, 1.9), square(3.5, 3.5, 1.0)]  # the hole (3.5, 3.5) - (4.5, 4.5)


@functools.lru_cache(maxsize=None)
def rules():
    """the rectangle rules and the invalid objects, with a background of one triangle per cell"""
    objs = [
        [square(5.2, 5.2, 0.3)],                        # 0 inside the query's own cell: all-G at every r with G
        [[(6.9, 8.9), (8.9, 8.9), (8.9, 6.9), (6.9, 8.9)]],  # 1 spans G and non-G cells at R_G1, geometry 3.39 away
        [square(-0.5, 5.2, 0.8)],                       # 2 .. 5 leave the grid on each side, within r of "borders"
        [square(9.7, 5.2, 0.8)],
        [square(5.2, -0.5, 0.8)],
        [square(5.2, 9.7, 0.8)],
        [square(-0.9, 5.2, 0.5)],                       # 6 wholly outside the grid, 0.9 from (0.5, 5.5)
        HOLED,                                          # 7 a hole
        [square(6.0, 3.0, 1.0)],                        # 8, 9 share the edge x = 7
        [square(7.0, 3.0, 1.0)],
        [[(5.1, 5.1), (5.3, 5.1), (5.1, 5.1)]],         # 10 a 3-vertex ring
        [[(5.1, 5.1), (5.3, 5.1), (5.3, 5.3), (5.1, 5.3)]],  # 11 an unclosed ring
        [triangle(5.6, 5.6, 0.2)],                      # 12 a neighbour of the invalid ones, unaffected
        [square(4.2, 4.2, 2.6), square(5.0, 5.0, 0.2)],  # 13 valid shell, holed, over 9 cells
        [square(5.2, 5.2, 0.3), [(5.25, 5.25), (5.3, 5.25), (5.25, 5.25)]],  # 14 a valid shell with a 3-vertex hole
        [],                                             # 15 no ring at all
    ]
    for i in range(10):
        for j in range(10):
            objs.append([triangle(i + 0.3, j + 0.35, 0.25)])
    return _case(POLYGON, UNIT, objs, QUERIES_UNIT)


@functools.lru_cache(maxsize=None)
def holes():
    """query points inside the hole, on the hole edge, on the shell edge, on a vertex, inside the shell; nested
    polygons that all contain one of them (ties at d = 0)"""
    objs = [HOLED, [square(2.0, 2.0, 1.0)], [square(3.0, 2.0, 1.0)]]     # 1, 2 share an edge; 2 touches the shell
    objs += [[square(3.2 - 0.05 * i, 3.2 - 0.05 * i, 0.1 * i)] for i in range(1, 6)]  # nested around (3.2, 3.2)
    keys = [7, 3, 3, 9, 1, 5, 1, 2]  # duplicates at different distances and at d = 0
    q = {"in_hole": ([4.0], [4.0]), "hole_edge": ([3.5], [4.0]), "shell_edge": ([3.0], [4.0]), "vertex": ([3.0], [3.0]),
         "in_shell": ([3.2], [3.2]), "shared_edge": ([3.0], [2.5])}
    return _case(POLYGON, UNIT, objs, q, keys)


RING_SIZES = (5, 63, 64, 65, 127, 128, 129)


@functools.lru_cache(maxsize=None)
def rings():
    """rings of every length around the wave path's thresholds, one 5,000-vertex ring (wide at the default
    threshold), and the degenerate shapes of tests/poly_cases.py as window objects -- on the Beijing grid"""
    cl = PC.CL
    objs = [[ngon(116.0 + 3 * cl * i, 40.0, 0.9 * cl, nv)] for i, nv in enumerate(RING_SIZES)]
    objs.append([ngon(116.2, 40.2, 1.7 * cl, 5000), ngon(116.2, 40.2, 0.4 * cl, 66)])  # holed
    px, py = [116.0 + 0.2 * cl, 116.2 + 0.1 * cl, 116.2 + 1.0 * cl], [40.0 + 1.5 * cl, 40.2, 40.2 + 1.1 * cl]
    for name in PC.SHAPES:
        polys = PC.polygons(name)
        objs += polys
        x, y = PC.probes(name)
        step = max(1, len(x) // 2)
        px += [float(v) for v in x[::step][:2]]
        py += [float(v) for v in y[::step][:2]]
    q = {f"p{i}": ([px[i]], [py[i]]) for i in range(len(px))}
    q["set3"] = (px[:3], py[:3])
    return _case(POLYGON, BEIJING, objs, q)


@functools.lru_cache(maxsize=None)
def lines():
    objs = [
        [(4.0, 5.0), (7.0, 5.0)],                                   # 0 horizontal: zero-height envelope
        [(5.0, 4.0), (5.0, 7.0)],                                   # 1 vertical: zero-width envelope
        [(5.25, 5.75), (5.25, 5.75), (5.25, 5.75)],                 # 2 one point repeated
        square(5.0, 5.0, 1.0),                                      # 3 closed: an interior point is at its edge distance
        [(5.5, 5.5)],                                               # 4 a 1-vertex chain
        [(5.4, 5.4), (5.6, 5.7)],                                   # 5 its neighbour
        [(-0.5, 5.5), (0.4, 5.6)],                                  # 6 leaves the grid
        [(-0.9, 5.2), (-0.3, 5.3)],                                 # 7 wholly outside
    ]
    objs += [zigzag(1.0, 2.0 + 0.5 * i, 7.0 / nv, 0.3, nv) for i, nv in enumerate((2, 63, 64, 65, 129, 5000))]
    for i in range(10):
        for j in range(10):
            objs.append([(i + 0.2, j + 0.2), (i + 0.5, j + 0.4), (i + 0.3, j + 0.7)])
    return _case(LINESTRING, UNIT, objs, QUERIES_UNIT)


CORNER = (10, (0.0, 3.0, 0.0, 3.0))   # cell length fl(0.3)
CORNER_R = 0.9                         # fl(0.9 / 0.3) = 3.0: candidate layers 3
CORNER_Q = (float(np.nextafter(0.3, 0.0)), 1.0)   # the last double of cell 0: N = columns 0 .. 3


@functools.lru_cache(maxsize=None)
def corner(kind):
    """An object with no cell in N whose distance is nevertheless <= r, across a cell corner: its nearest
    vertex is at x = 1.2, column floor(1.2 / 0.3) = 4, and the computed distance 1.2 - q is 0.9 exactly.  The
    reference drops it in the cell filter.  Object 1 is its twin one column nearer (kept), object 2 a farther one."""
    def obj(x):
        if kind == POLYGON:
            return [[(x, 1.0), (x + 0.2, 1.0), (x, 1.1), (x, 1.0)]]
        return [(x, 1.0), (x + 0.2, 1.05)]
    return _case(kind, CORNER, [obj(1.2), obj(1.19), obj(1.25)], {"corner": ([CORNER_Q[0]], [CORNER_Q[1]])}, [5, 6, 7])


SIZES = (0, 1, 63, 64, 65, 257, 3001)


@functools.lru_cache(maxsize=None)
def sized(kind, n, seed=7):
    """n small objects scattered over (and a little beyond) the unit grid; objID keys with duplicates"""
    rnd = random.Random(seed * 1000 + n + kind)
    objs = []
    for i in range(n):
        x, y, s = rnd.uniform(-0.6, 10.2), rnd.uniform(-0.6, 10.2), rnd.uniform(0.05, 0.6)
        if kind == POLYGON:
            objs.append([triangle(x, y, s) if i % 3 else square(x, y, s)] if i % 11 else
                        [square(x, y, s), square(x + s / 4, y + s / 4, s / 2)])
        else:
            objs.append(zigzag(x, y, s / 4, s / 3, 2 + i % 7))
    keys = [i % 701 - 3 for i in range(n)]
    return _case(kind, UNIT, objs, QUERIES_UNIT, keys)


def csr(case):
    """(ring_off or None, vert_off, vx, vy) as numpy arrays: the window as the C ABI takes it"""
    ring_off, vert_off, vx, vy = [0], [0], [], []
    for obj in case["objs"]:
        for ring in (obj if case["kind"] == POLYGON else [obj]):
            vx += [float(v[0]) for v in ring]
            vy += [float(v[1]) for v in ring]
            vert_off.append(len(vx))
        ring_off.append(len(vert_off) - 1)
    ro = np.array(ring_off, np.int32) if case["kind"] == POLYGON else None
    return ro, np.array(vert_off, np.int32), np.array(vx, np.float64), np.array(vy, np.float64)


def numpy_index(case):
    """(env [nobj, 4] = x1, y1, x2, y2; valid [nobj]) restated with numpy min / max over the shell / the chain"""
    kind = case["kind"]
    env, ok = np.zeros((len(case["objs"]), 4)), np.zeros(len(case["objs"]), bool)
    for i, obj in enumerate(case["objs"]):
        ring = obj if kind == LINESTRING else (obj[0] if obj else [])
        if len(ring):
            a = np.array(ring, np.float64)
            env[i] = a[:, 0].min(), a[:, 1].min(), a[:, 0].max(), a[:, 1].max()
        if kind == LINESTRING:
            ok[i] = len(obj) >= 2
        else:
            ok[i] = len(obj) >= 1 and all(len(r) >= 4 and tuple(r[0]) == tuple(r[-1]) for r in obj)
    return env, ok
