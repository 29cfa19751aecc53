"""tAggregate: ms per window of gf_tagg_group + gf_tagg_run, warm, on device-resident windows (default
10M points over ~100k objIDs on a 500 x 500 Beijing grid, uniform; --hot F puts a share F of the
points into one cell, --hot-group F gives one objID standing in one cell a share F).

Several distinct windows, together larger than the 256 MB MALL, are visited round-robin through ONE
object (its workspace reused), so no window is served from cache.  Every figure is a median over the
timed calls: device events on the context's stream around the call, and the host clock around it (both
calls end in a stream synchronise).  The reads of the per-cell table and of the ALL rows are timed
apart (they are host copies).  --traj times gf_traj_group + gf_tstats_run on the same windows in the
same process: the nearest existing work.  With --timing the per-kernel-group device times
(gf_ctx_timing) are added from a second loop.  The algorithmic floor it is set against: 32 B per point
read (x, y, objID, ts) plus the rows written: 68 B per cell (cx, cy, seven int64, its offset) and 16 B
per (cell, objID) group (the ALL rows).
Prints one JSON line (and appends it to --out, default profiles/tagg_bench.jsonl)."""
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

HBM_PEAK = 8.0e12  # B/s, MI355X HBM3E specification
BEIJING = (115.5, 117.6, 39.6, 41.1)


def make_window(seed, n, nobj, hot, hot_group):
    rng = np.random.default_rng(seed)
    pool = np.concatenate([rng.integers(0, 1 << 40, nobj // 2), -(1 << 63) + np.arange(nobj - nobj // 2)]).astype(np.int64)
    obj = pool[rng.integers(0, len(pool), n)]
    x = rng.uniform(BEIJING[0], BEIJING[1], n)
    y = rng.uniform(BEIJING[2], BEIJING[3], n)
    if hot > 0:  # one cell holds a share of the points (and with it nearly every objID)
        m = rng.random(n) < hot
        x[m], y[m] = 116.4001, 39.9001
    if hot_group > 0:  # one objID standing in one cell
        m = rng.random(n) < hot_group
        x[m], y[m], obj[m] = 116.9001, 40.3001, 4242
    ts = 1_600_000_000_000 + np.arange(n, dtype=np.int64) // 8 + rng.integers(0, 3, n)  # arrival order, some ties / late points
    return x, y, obj, ts


def floor_bytes(n, cells, groups):
    return 32 * n + 68 * cells + 16 * groups


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--objs", type=int, default=100_000)
    ap.add_argument("--grid", type=int, default=500)
    ap.add_argument("--hot", type=float, default=0.0)
    ap.add_argument("--hot-group", type=float, default=0.0)
    ap.add_argument("--windows", type=int, default=4)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--long-group", type=int, default=0)
    ap.add_argument("--big-cell", type=int, default=0)
    ap.add_argument("--traj", action="store_true", help="also time gf_traj_group + gf_tstats_run on the same windows")
    ap.add_argument("--timing", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tagg_bench.jsonl"))
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

    assert torch.cuda.is_available(), "bench_tagg needs a HIP device"
    L = _lib.lib()
    assert L.gf_build_is_product() == 1, L.gf_build_info().decode()
    grid = sf.UniformGrid(a.grid, *BEIJING)
    wins = [sf.PointWindow.from_numpy(*make_window(100 + i, a.n, a.objs, a.hot, a.hot_group)) for i in range(a.windows)]
    g = sf.TAggregateGroups(wins[0], grid)  # warm-up: code objects, the workspace
    g.set_thresholds(a.long_group, a.big_cell)
    g.run()
    ctx = g.ctx

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        t0 = time.perf_counter()
        fn()
        host = (time.perf_counter() - t0) * 1e3
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), host

    grp, stat, rd_cells, rd_all, cells, groups = [], [], [], [], [], []
    for _ in range(a.reps):
        for w in wins:
            grp.append(timed(lambda: g.regroup(w, grid)))
            stat.append(timed(lambda: g.run()))
            rd_cells.append(timed(lambda: g.cells()))
            rd_all.append(timed(lambda: g.all_rows()))
            cells.append(g.ncells)
            groups.append(g.ngroups)
    med = lambda v, j: statistics.median(t[j] for t in v)  # noqa: E731
    nc, ng = int(statistics.median(cells)), int(statistics.median(groups))
    fl = floor_bytes(a.n, nc, ng)
    floor_ms = fl / HBM_PEAK * 1e3
    total = med(grp, 0) + med(stat, 0)
    res = {"bench": "tagg", "n": a.n, "objs": a.objs, "grid": a.grid, "hot": a.hot, "hot_group": a.hot_group,
           "windows": a.windows, "calls": len(grp), "long_group": a.long_group, "big_cell": a.big_cell,
           "cells": nc, "groups": ng,
           "group_ms": round(med(grp, 0), 4), "group_host_ms": round(med(grp, 1), 4),
           "run_ms": round(med(stat, 0), 4), "run_host_ms": round(med(stat, 1), 4),
           "window_ms": round(total, 4),
           "group_min_max_ms": [round(min(t[0] for t in grp), 4), round(max(t[0] for t in grp), 4)],
           "run_min_max_ms": [round(min(t[0] for t in stat), 4), round(max(t[0] for t in stat), 4)],
           "read_cells_host_ms": round(med(rd_cells, 1), 4), "read_all_host_ms": round(med(rd_all, 1), 4),
           "floor_bytes": fl, "floor_ms_at_8TBs": round(floor_ms, 4), "x_floor": round(total / floor_ms, 1)}
    if a.traj:
        t = sf.TrajectoryGroups(wins[0])
        t.tstats()
        cnt = C.c_int64()

        def tstats_count_only(w):
            pts = w.c_struct()
            _lib.check(L.gf_tstats_run(t.handle, C.byref(pts), None, 0, None, None, None, None, 0, C.byref(cnt)),
                       ctx.handle, "gf_tstats_run")

        tg, tt = [], []
        for _ in range(a.reps):
            for w in wins:
                tg.append(timed(lambda: t.regroup(w)))
                tt.append(timed(lambda: tstats_count_only(w)))
        res["traj_group_ms"] = round(med(tg, 0), 4)
        res["traj_tstats_ms"] = round(med(tt, 0), 4)
        res["traj_both_ms"] = round(med(tg, 0) + med(tt, 0), 4)
        res["x_traj_both"] = round(total / (med(tg, 0) + med(tt, 0)), 2)
        t.close()
    if a.timing:
        ids = {"tagg": _lib.K_TAGG, "group_tables": _lib.K_TRAJ_GROUP, "radix": _lib.K_BUCKET}
        ctx.set_timing(sum(1 << k for k in ids.values()))
        for k in ids.values():
            ctx.timing(k)
        for w in wins:
            g.regroup(w, grid).run()
        res["kernel_ms_per_window"] = {nm: round(ctx.timing(k)[0] / len(wins), 4) for nm, k in ids.items()}
        ctx.set_timing(0)
    g.close()
    return res


if __name__ == "__main__":
    main()
