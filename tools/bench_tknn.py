"""tKnn: ms per window of gf_tknn_run, warm, on device-resident windows already grouped by objID
(default 10M points over ~100k objIDs on the 100 x 100 Beijing grid, uniform, k = 50, r = 0.03: L = 2).
--r0: r = 0, N = every valid cell (the heavy case); --naive: runNaive; --hot F: one cell holds a share
F of the points.

Several distinct windows, together larger than the 256 MB MALL, are visited round-robin through ONE
gf_traj_groups and ONE gf_tknn object (their workspaces reused), so no window is served from cache.
Every figure is a median over the timed calls: device events around the call and the host clock around
it (the call ends in a stream synchronise).  gf_traj_group is timed apart: it is shared with tStats and
the sub-trajectory extraction.  The per-kernel-id device times (gf_ctx_timing) come from a second loop:
tknn = this operator's own kernels, group_tables = the two groupings of the points in N, radix = the
sorts.  The scan reads 20 B per point (x, y, trajectory id); scan_GBs_at_least divides that traffic by
ALL of tknn's kernel time, so it is a lower bound on the scan's bandwidth, close when N is small.
Prints one JSON line (and appends it to --out, default profiles/tknn_bench.jsonl)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BEIJING = (115.5, 117.6, 39.6, 41.1)
Q = (116.5, 40.0)


def make_window(seed, n, nobj, hot):
    rng = np.random.default_rng(seed)
    pool = np.concatenate([rng.integers(0, 1 << 40, nobj // 2), -(1 << 63) + np.arange(nobj - nobj // 2)]).astype(np.int64)
    obj = pool[rng.integers(0, len(pool), n)]
    x = rng.uniform(BEIJING[0], BEIJING[1], n)
    y = rng.uniform(BEIJING[2], BEIJING[3], n)
    if hot > 0:  # the query's cell holds a share of the points (and with it nearly every objID)
        m = rng.random(n) < hot
        x[m] = Q[0] + rng.uniform(-0.005, 0.005, int(m.sum()))
        y[m] = Q[1] + rng.uniform(0.0, 0.01, int(m.sum()))
    ts = 1_600_000_000_000 + np.arange(n, dtype=np.int64) // 8
    return x, y, obj, ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--objs", type=int, default=100_000)
    ap.add_argument("--grid", type=int, default=100)
    ap.add_argument("--k", type=int, default=50)
    ap.add_argument("--r", type=float, default=0.03)
    ap.add_argument("--r0", action="store_true", help="r = 0: N = every valid cell")
    ap.add_argument("--naive", action="store_true")
    ap.add_argument("--hot", type=float, default=0.0)
    ap.add_argument("--windows", type=int, default=4)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--big-cell", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tknn_bench.jsonl"))
    a = ap.parse_args()
    line = json.dumps(run(a))
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


def run(a):
    import torch

    import spatialflink_amd as sf
    from spatialflink_amd import _lib

    assert torch.cuda.is_available(), "bench_tknn needs a HIP device"
    L = _lib.lib()
    assert L.gf_build_is_product() == 1, L.gf_build_info().decode()
    grid = sf.UniformGrid(a.grid, *BEIJING)
    r = 0.0 if a.r0 else a.r
    mode = _lib.TKNN_NAIVE if a.naive else _lib.TKNN_GRID
    wins = [sf.PointWindow.from_numpy(*make_window(100 + i, a.n, a.objs, a.hot)) for i in range(a.windows)]
    g = sf.TrajectoryGroups(wins[0])
    ctx = g.ctx
    h = C.c_void_p()

    def tknn(w):
        pts = w.c_struct()
        _lib.check(L.gf_tknn_run(g.handle, C.byref(grid.c_grid), C.byref(pts), Q[0], Q[1], r, a.k, mode, C.byref(h)),
                   ctx.handle, "gf_tknn_run")

    tknn(wins[0])  # warm-up: code objects, the workspace
    if a.big_cell:
        _lib.check(L.gf_tknn_set_thresholds(h, a.big_cell), None, "gf_tknn_set_thresholds")

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        t0 = time.perf_counter()
        fn()
        host = (time.perf_counter() - t0) * 1e3
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), host

    grp, knn, info = [], [], []
    c = [C.c_int64() for _ in range(5)]
    for _ in range(a.reps):
        for w in wins:
            grp.append(timed(lambda: g.regroup(w)))
            knn.append(timed(lambda: tknn(w)))
            L.gf_tknn_info(h, *(C.byref(v) for v in c))
            info.append([v.value for v in c])
    med = lambda v, j: statistics.median(t[j] for t in v)  # noqa: E731
    rows, npts, in_cells, pairs, records = (int(statistics.median(col)) for col in zip(*info))
    res = {"bench": "tknn", "n": a.n, "objs": a.objs, "grid": a.grid, "k": a.k, "r": r, "naive": a.naive, "hot": a.hot,
           "windows": a.windows, "calls": len(knn), "big_cell": a.big_cell, "trajectories": g.ntraj,
           "rows": rows, "row_points": npts, "in_cells": in_cells, "pairs": pairs, "records": records,
           "tknn_ms": round(med(knn, 0), 4), "tknn_host_ms": round(med(knn, 1), 4),
           "tknn_min_max_ms": [round(min(t[0] for t in knn), 4), round(max(t[0] for t in knn), 4)],
           "traj_group_ms": round(med(grp, 0), 4), "total_ms": round(med(knn, 0) + med(grp, 0), 4)}
    ids = {"tknn": _lib.K_TKNN, "group_tables": _lib.K_TRAJ_GROUP, "radix": _lib.K_BUCKET}
    for w in wins:  # the groups of each window first, untimed: the breakdown is gf_tknn_run's alone
        g.regroup(w)
        ctx.set_timing(sum(1 << k for k in ids.values()))
        for k in ids.values():
            ctx.timing(k)
        tknn(w)
        for nm, k in ids.items():
            res.setdefault("kernel_ms_per_window", {}).setdefault(nm, 0.0)
            res["kernel_ms_per_window"][nm] += ctx.timing(k)[0] / len(wins)
        ctx.set_timing(0)
    res["kernel_ms_per_window"] = {nm: round(v, 4) for nm, v in res["kernel_ms_per_window"].items()}
    res["scan_GBs_at_least"] = round(20.0 * a.n / (res["kernel_ms_per_window"]["tknn"] * 1e-3) / 1e9, 1)
    L.gf_tknn_destroy(h)
    g.close()
    return res


if __name__ == "__main__":
    main()
