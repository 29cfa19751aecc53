"""Windows of the tJoin tests (tests/test_tjoin_ref.py, tests/test_gpu_tjoin.py): the hand vector with its
rows written out, and the generators of the larger windows.  A window is (x, y, objID, ts)."""
import numpy as np

import spatialflink_amd as sf

BEIJING = (115.5, 117.6, 39.6, 41.1)
NULL_KEY = (1 << 63) - 1          # _lib.OBJID_NULL
DICT_KEY0 = -(1 << 63)            # dictionary ids: below the numeric key range


def small_grid():
    """8 x 8 cells of side 1 over [0, 8]^2"""
    return sf.UniformGrid(8, 0.0, 8.0, 0.0, 8.0)


def beijing_grid(n=100):
    return sf.UniformGrid(n, *BEIJING)


def _window(rows):
    a = np.array(rows, np.float64).reshape(-1, 4)
    return a[:, 1].copy(), a[:, 2].copy(), a[:, 0].astype(np.int64), a[:, 3].astype(np.int64)


# The hand vector: small_grid(), r = 1 (L = 1).  objID, x, y, ts
HAND_O = _window([
    (10, 2.5, 2.5, 100),   # 0  matches Q0, Q1, Q10
    (20, 5.5, 4.4, 100),   # 1  1.1 from Q3: no match
    (10, 2.6, 2.5, 101),   # 2
    (30, 6.5, 1.5, 102),   # 3  a single-point trajectory: its rows have emit 0
    (20, 5.5, 5.6, 103),   # 4  matches Q3, Q4
    (10, 0.5, 7.5, 104),   # 5  matches Q9 only, the LAST element of objID 7's run in cell (1, 7)
    (20, 7.5, 7.5, 105),   # 6  no match
    (10, -0.5, 2.5, 106),  # 7  outside the grid: never matches, though Q11 is 0.1 away
])
HAND_Q = _window([
    (7, 2.5, 2.4, 50),     # 0  cell (2, 2): the first match found for (10, 7)
    (7, 3.1, 2.5, 60),     # 1  cell (3, 2): the latest match of (10, 7) lies in another cell
    (7, 2.5, 3.9, 70),     # 2  later still, but 1.4 from O0: no match
    (8, 5.5, 5.5, 80),     # 3  ts tie with Q4: the smaller index wins
    (8, 5.4, 5.5, 80),     # 4
    (9, 6.5, 1.6, 90),     # 5  a single-point trajectory
    (8, 6.4, 1.5, 10),     # 6  matches O3
    (7, 1.9, 7.5, 99),     # 7  cell (1, 7), 1.4 from O5
    (7, 1.8, 7.5, 98),     # 8  cell (1, 7), 1.3 from O5
    (7, 1.4, 7.5, 5),      # 9  cell (1, 7), 0.9 from O5: the run's only match is its last element
    (8, 2.5, 2.6, 81),     # 10 matches O0, O2
    (8, -0.4, 2.5, 82),    # 11 outside the grid, next to O7 (which is outside too)
])
HAND_R = 1.0
# (okey, qkey, p_first, q_latest, emit, oslot, qslot), ascending by (t_o, t_q)
HAND_ROWS = [
    (10, 7, 0, 1, 1, 0, 0),
    (10, 8, 0, 10, 1, 0, 1),
    (20, 8, 4, 3, 1, 1, 1),
    (30, 8, 3, 6, 0, -1, -1),
    (30, 9, 3, 5, 0, -1, -1),
]
HAND_ORDINARY = {"keys": [10, 20], "off": [0, 4, 7], "idx": [0, 2, 5, 7, 1, 4, 6]}
HAND_QUERY = {"keys": [7, 8], "off": [0, 6, 11], "idx": [0, 1, 2, 7, 8, 9, 3, 4, 6, 10, 11]}
HAND_FIRST_POINT = {10: 0, 20: 4, 30: 3}


def walks(seed, n, ntraj, bounds, step, keys="mixed"):
    """n points of about ntraj trajectories, interleaved: short random walks (a trajectory's points share
    cells), some trajectories of a single point, a margin outside `bounds`, a few NaN coordinates, ts with
    ties.  keys: "mixed" = numeric, dictionary and the null key."""
    rng = np.random.default_rng(seed)
    t = rng.integers(0, ntraj, n)
    t[: ntraj // 8] = ntraj + np.arange(ntraj // 8)  # single-point trajectories
    rng.shuffle(t)
    w, h = bounds[1] - bounds[0], bounds[3] - bounds[2]
    sx = rng.uniform(bounds[0] - 0.03 * w, bounds[1] + 0.03 * w, ntraj + ntraj // 8)
    sy = rng.uniform(bounds[2] - 0.03 * h, bounds[3] + 0.03 * h, ntraj + ntraj // 8)
    x = sx[t] + step * rng.standard_normal(n)
    y = sy[t] + step * rng.standard_normal(n)
    bad = rng.integers(0, n, max(n // 5000, 1))
    x[bad[::2]] = np.nan
    y[bad[1::2]] = np.nan
    if keys == "mixed":
        pool = rng.integers(-(1 << 40), 1 << 40, ntraj + ntraj // 8).astype(np.int64)
        pool[::3] = DICT_KEY0 + np.arange(len(pool[::3]))
        pool[1] = NULL_KEY
    else:
        pool = np.arange(ntraj + ntraj // 8, dtype=np.int64) * 7 + 1
    ts = 1_600_000_000_000 + rng.integers(0, max(n // 4, 2), n).astype(np.int64)
    return x, y, pool[t], ts


def one_cell(seed, n, ntraj, cell=(47, 19)):
    """n points of exactly ntraj trajectories inside ONE cell of beijing_grid(100)"""
    rng = np.random.default_rng(seed)
    cl = (BEIJING[1] - BEIJING[0]) / 100
    x = BEIJING[0] + (cell[0] + rng.uniform(0.02, 0.98, n)) * cl
    y = BEIJING[2] + (cell[1] + rng.uniform(0.02, 0.98, n)) * cl
    obj = (rng.integers(0, ntraj, n) * 3 + 5).astype(np.int64)
    obj[:ntraj] = np.arange(ntraj) * 3 + 5
    ts = 1_600_000_000_000 + rng.integers(0, n // 3, n).astype(np.int64)
    return x, y, obj, ts


def device_window(w):
    x, y, obj, ts = (np.ascontiguousarray(a).copy() for a in w)
    return sf.PointWindow.from_numpy(x, y, obj, ts, start=1_000, end=11_000)
