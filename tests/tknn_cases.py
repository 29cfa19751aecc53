"""The windows of the tKnn tests (tests/test_tknn_ref.py on the CPU, tests/test_gpu_tknn.py on the GPU),
all on the 100 x 100 Beijing grid (cell length 0.021), each the smallest that reaches its path.  The
query point Q = (116.5, 40.0) lies in cell (47, 19); r = 0.03 gives L = 2, r = 0.02 gives L = 1."""
import functools

import numpy as np

import spatialflink_amd as sf
from spatialflink_amd import _lib
from conftest import BEIJING

import tknn_ref as R
from tagg_ref import cells_of
from traj_ref import group_ref

I64_MIN = -(1 << 63)
EMPTY_MARK = (1 << 63) - 2  # the grouping table's own empty marker: a legal key like any other
Q = (116.5, 40.0)
R2, R1 = 0.03, 0.02
CL = (BEIJING[1] - BEIJING[0]) / 100


def grid():
    return sf.UniformGrid(100, *BEIJING)


# hand12 -- objIDs A..F = 10..60, ranks 0..5.  Distances from Q are the offsets written here.
#   cell (47, 19): A .004, B min(.002, .0015), C .001 (a single point)      cell (47, 20): A .03
#   cell (48, 19): B .01, D .012, E min(.011, .02)                          outside N: A, D, F (NaN x)
HAND12 = [(10, 116.504, 40.0), (20, 116.5, 40.002), (10, 117.0, 40.5), (30, 116.5, 40.001), (20, 116.51, 40.0),
          (40, 116.512, 40.0), (40, 115.0, 39.0), (50, 116.511, 40.0), (50, 116.52, 40.0), (10, 116.5, 40.03),
          (60, float("nan"), 40.0), (20, 116.5, 40.0015)]
# k = 2: the lists are (C, B), (B, E), (A): A was cut from the query cell's list, so its D is its far
# cell's; C is a single point.  k = 3: the lists are (C, B, A), (B, E, D), (A).
HAND12_ROWS = {2: [(20, 11, 2, [1, 4, 11]), (50, 7, 1, [7, 8])],
               3: [(20, 11, 2, [1, 4, 11]), (10, 0, 2, [0, 2, 9]), (50, 7, 1, [7, 8])]}  # key, point of D, cells, idx


def _quant(rng, n, lo, hi, step):
    """n coordinates on a lattice of `step` (a power of two) inside [lo, hi): exact ties are the rule"""
    a, b = int(np.ceil(lo / step)), int(np.floor(hi / step))
    return rng.integers(a, b, n) * step


@functools.lru_cache(maxsize=None)
def window(name):
    """(x, y, obj, ts, cx, cy, groups) of the named window, read-only and shared"""
    w, h = BEIJING[1] - BEIJING[0], BEIJING[3] - BEIJING[2]
    # the inside of the query cell, on the lattice
    x0, x1, y0, y1 = 116.488, 116.507, 39.9995, 40.0195
    if name == "hand12":
        obj = np.array([p[0] for p in HAND12], np.int64)
        x, y = np.array([p[1] for p in HAND12]), np.array([p[2] for p in HAND12])
    elif name == "wave65":  # one cell, 65 trajectories of 2 points each
        rng = np.random.default_rng(31)
        obj = rng.permutation(np.repeat(np.arange(65, dtype=np.int64) * 13 - 300, 2))
        x, y = _quant(rng, 130, x0, x1, 2.0 ** -12), _quant(rng, 130, y0, y1, 2.0 ** -12)
    elif name == "truncate":  # k = 4: nine single points nearer than A and B in the query cell
        pts = [(100 + j, Q[0] + 1e-4 * (j + 1), Q[1]) for j in range(9)]
        pts += [(1, Q[0] + 0.002, Q[1]), (2, Q[0], Q[1] + 0.003), (2, Q[0], Q[1] + 0.0031),
                (1, Q[0] + 0.015, Q[1]),                                  # A again, in cell (48, 19)
                (3, Q[0] + 0.012, Q[1]), (3, Q[0] + 0.013, Q[1])]         # C, both in cell (48, 19)
        order = np.random.default_rng(32).permutation(len(pts))
        obj = np.array([pts[i][0] for i in order], np.int64)
        x, y = np.array([pts[i][1] for i in order]), np.array([pts[i][2] for i in order])
    elif name == "ties":
        # (Q +- a, Q +- b), exact: four bit-equal distances; three stationary objIDs on one of them; and
        # two stationary objIDs on each of (Q +- 2^-6, Q), bit-equal too, in cells (48, 19) and (46, 19)
        a, b, c = 2.0 ** -9, 2.0 ** -11, 2.0 ** -6
        pts = []
        for j, (sx, sy) in enumerate([(1, 1), (1, -1), (-1, 1), (-1, -1)]):
            pts += [(7000 - 11 * j, Q[0] + sx * a, Q[1] + sy * b), (7000 - 11 * j, 117.3, 40.9)]
        for j in range(3):
            pts += [(-50 + j, Q[0] + a, Q[1] + b)] * 2
        for j in range(2):
            pts += [(900 + j, Q[0] + c, Q[1])] * 2 + [(800 - j, Q[0] - c, Q[1])] * 2
        order = np.random.default_rng(33).permutation(len(pts))
        obj = np.array([pts[i][0] for i in order], np.int64)
        x, y = np.array([pts[i][1] for i in order]), np.array([pts[i][2] for i in order])
    elif name == "hotcell20k":  # one cell over ~5k objIDs, distances tie all over
        rng = np.random.default_rng(34)
        n = 20_000
        obj = (rng.integers(0, 5000, n) * 7919 - 9_000_000).astype(np.int64)
        x, y = _quant(rng, n, x0, x1, 2.0 ** -11), _quant(rng, n, y0, y1, 2.0 ** -11)
    elif name == "hotpair20k":  # one (cell, objID) pair holds ~95 %; many of its points hold its minimum
        rng = np.random.default_rng(35)
        n = 20_000
        hot = rng.random(n) < 0.95
        obj = np.where(hot, 7, rng.integers(0, 40, n)).astype(np.int64)
        x = np.where(hot, _quant(rng, n, x0, x1, 2.0 ** -8), rng.uniform(BEIJING[0], BEIJING[1], n))
        y = np.where(hot, _quant(rng, n, y0, y1, 2.0 ** -8), rng.uniform(BEIJING[2], BEIJING[3], n))
    elif name == "mix200k":  # the population of test_gpu_tagg's mix200k, plus planted NaN pairs in column 0
        rng = np.random.default_rng(25)
        n = 200_000
        pool = np.concatenate([rng.integers(-(1 << 40), 1 << 40, 12_000), rng.integers(0, 5000, 2_000),
                               I64_MIN + rng.integers(0, 20_000, 5_996),
                               [_lib.OBJID_NULL, EMPTY_MARK, I64_MIN, -1]]).astype(np.int64)
        pool = np.unique(pool)
        hx = BEIJING[0] + w * rng.uniform(0.3, 0.6, len(pool))
        hy = BEIJING[2] + h * rng.uniform(0.3, 0.6, len(pool))
        who = rng.integers(0, len(pool), n)
        who[:4000] = rng.integers(len(pool) - 4, len(pool), 4000)  # (unique sorted: NULL / the marker are last)
        who[4000:8000] = rng.integers(0, 2, 4000)                  # INT64_MIN and its neighbour
        rng.shuffle(who)
        obj = pool[who]
        x = hx[who] + rng.normal(0, CL * 0.6, n)
        y = hy[who] + rng.normal(0, CL * 0.6, n)
        out = rng.random(n) < 0.04  # out of grid on every side
        side = rng.integers(0, 4, n)
        x = np.where(out & (side == 0), BEIJING[0] - rng.uniform(0, 3 * CL, n), x)
        x = np.where(out & (side == 1), BEIJING[1] + rng.uniform(0, 3 * CL, n), x)
        y = np.where(out & (side == 2), BEIJING[2] - rng.uniform(0, 3 * CL, n), y)
        y = np.where(out & (side == 3), BEIJING[3] + rng.uniform(0, 3 * CL, n), y)
        bad = rng.choice(n, 40, replace=False)
        x[bad[:10]] = np.nan
        y[bad[10:20]] = np.nan
        x[bad[20:25]] = np.inf
        y[bad[25:30]] = -np.inf
        x[bad[30:35]] = -1e300
        y[bad[35:40]] = 1e300
        # column 0 (a NaN x has cell 0): pairs whose first point is a NaN and a later one is not, and the converse
        spots = np.sort(rng.choice(n, 24, replace=False)).reshape(12, 2)
        for j, (p, q) in enumerate(spots.tolist()):
            obj[p] = obj[q] = 555_000_000 + j
            y[p] = y[q] = 40.0 + 0.02 * j
            x[p], x[q] = (np.nan, BEIJING[0] + 0.004) if j % 2 else (BEIJING[0] + 0.004, np.nan)
    else:
        raise KeyError(name)
    obj = np.asarray(obj, np.int64)
    x, y = np.asarray(x, np.float64).copy(), np.asarray(y, np.float64).copy()
    ts = np.random.default_rng(len(obj)).integers(0, 1 << 20, len(obj)).astype(np.int64)
    cx, cy = cells_of(grid(), x, y)
    groups = group_ref(obj)
    for a in (x, y, obj, ts, cx, cy, *groups):
        a.setflags(write=False)
    return x, y, obj, ts, cx, cy, groups


@functools.lru_cache(maxsize=None)
def expected(name, qx, qy, r, k, naive):
    """tknn_ref of the named window (computed once per query, shared, read-only)"""
    x, y, obj, ts, cx, cy, groups = window(name)
    res = R.tknn_ref(grid(), x, y, obj, ts, qx, qy, r, k, naive, cells=(cx, cy), groups=groups)
    for v in res.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return res
