"""tRange: ms per window of gf_trange_run, warm, on device-resident windows already grouped by objID
(default 10M points over ~100k objIDs as short random walks on the 100 x 100 Beijing grid), against
today's two-call route to the closest answer: the gf_range_ppoly plan + gf_range_run, then gf_traj_select.

Polygon sets (--set):
  squares  the 1000 generateQueryPolygons squares tools/bench_workloads.py uses for ppoly
  zones    tests/golden/high_risk_zones_rings.json on the world grid its caller uses; the walks are laid
           around it
  ngon     --ngon V: a few V-vertex circles -- where the wave path starts to pay, so what wide_ring
           should be (--wide-ring sets it; 0 = the default)
--hot F puts a share F of the points into one zone under one objID.

Several distinct windows are visited round-robin through ONE plan and ONE gf_traj_groups.  Every figure
is a median over the timed calls: device events around the call and the host clock around it (both calls
end in a stream synchronise; both go through ctypes on a plan and buffers made before the timed
region).  gf_traj_group is timed apart: both routes need it.

The two-call route runs at radius 2^-70, not 0: at r = 0 a range plan has no candidate cells at all and
returns nothing, so 2^-70 is the smallest radius at which it computes `distance <= 0` (no nonzero distance
of these sets is that small).  ratio = two_call_ms / trange_ms.  floor_ms = 20 B per point read once
(x, y, did) plus the emitted CSR (28 B per emitted point read and written), at --hbm-gbs.

The per-kernel-id device times (gf_ctx_timing) come from a second loop: trange = this operator's own
kernels, select = the emit shared with gf_traj_select, range = the range scan of the two-call route.
Prints one JSON line (and appends it to --out, default profiles/trange_bench.jsonl)."""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

BEIJING = (115.5, 117.6, 39.6, 41.1)
WORLD = (-180.0, 180.0, -90.0, 90.0)


def polygon_set(a):
    """(raw polygons, grid box, the box the walks start in, the hot zone's box)"""
    if a.set == "squares":
        sys.path.insert(0, os.path.join(ROOT, "oracle"))
        import oracle as O

        raw = O.generate_query_polygons(1000, BEIJING[0], BEIJING[2], BEIJING[1], BEIJING[3])
        box, area = BEIJING, BEIJING
    elif a.set == "zones":
        with open(os.path.join(ROOT, "tests", "golden", "high_risk_zones_rings.json")) as f:
            raw = json.load(f)["polygons"]
        xs = [v[0] for p in raw for r in p for v in r]
        ys = [v[1] for p in raw for r in p for v in r]
        box, area = WORLD, (min(xs) - 0.05, max(xs) + 0.05, min(ys) - 0.05, max(ys) + 0.05)
    else:
        v = max(a.ngon, 3)
        raw = []
        for k in range(6):
            cx, cy, rad = BEIJING[0] + 0.3 * (k + 1), BEIJING[2] + 0.2 * (k + 1), 0.08
            ring = [(cx + rad * math.cos(2 * math.pi * i / v), cy + rad * math.sin(2 * math.pi * i / v)) for i in range(v)]
            raw.append([ring + [ring[0]]])
        box, area = BEIJING, BEIJING
    r0 = raw[0][0]
    hx, hy = [p[0] for p in r0], [p[1] for p in r0]
    mx, my = (min(hx) + max(hx)) / 2, (min(hy) + max(hy)) / 2
    hot = (mx - (max(hx) - min(hx)) / 8, mx + (max(hx) - min(hx)) / 8, my - (max(hy) - min(hy)) / 8, my + (max(hy) - min(hy)) / 8)
    return raw, box, area, hot


def make_window(seed, n, nobj, area, step, hot, hot_box):
    from bench_tjoin import make_window as walks

    x, y, obj, ts = walks(seed, n, nobj, 100, step, 0.0, False)
    x = area[0] + (x - BEIJING[0]) * (area[1] - area[0]) / (BEIJING[1] - BEIJING[0])
    y = area[2] + (y - BEIJING[2]) * (area[3] - area[2]) / (BEIJING[3] - BEIJING[2])
    if hot > 0:
        rng = np.random.default_rng(seed + 7)
        m = rng.random(n) < hot
        x[m] = rng.uniform(hot_box[0], hot_box[1], int(m.sum()))
        y[m] = rng.uniform(hot_box[2], hot_box[3], int(m.sum()))
        obj[m] = (1 << 41) + 5
    return x, y, obj, ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--objs", type=int, default=100_000)
    ap.add_argument("--set", choices=("squares", "zones", "ngon"), default="squares")
    ap.add_argument("--ngon", type=int, default=0, help="vertices per circle (implies --set ngon)")
    ap.add_argument("--wide-ring", type=int, default=0)
    ap.add_argument("--step", type=float, default=0.002)
    ap.add_argument("--hot", type=float, default=0.0)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--hbm-gbs", type=float, default=4000.0, help="the bandwidth the floor is quoted at")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trange_bench.jsonl"))
    a = ap.parse_args()
    if a.ngon:
        a.set = "ngon"
    line = json.dumps(run(a))
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


def run(a):
    import torch

    import spatialflink_amd as sf
    from spatialflink_amd import _lib

    assert torch.cuda.is_available(), "bench_trange needs a HIP device"
    L = _lib.lib()
    assert L.gf_build_is_product() == 1, L.gf_build_info().decode()
    raw, box, area, hot_box = polygon_set(a)
    grid = sf.UniformGrid(100, *box)
    polys = [sf.Polygon(rings, grid) for rings in raw]
    wins = [sf.PointWindow.from_numpy(*make_window(300 + i, a.n, a.objs, area, a.step, a.hot, hot_box)) for i in range(a.windows)]
    tg = sf.TrajectoryGroups(wins[0])
    ctx = tg.ctx
    plan = sf.TRangePlan(ctx, grid, polys)
    plan.set_thresholds(a.wide_ring)
    # the two-call route's plan, bitmap and counts once, outside the timed region, as the fused side's
    rq = sf.PointPolygonRangeQuery(sf.QueryConfiguration(sf.QueryType.WindowBased), grid)
    _, rplan = rq.plan(wins[0].x.device.index, polys, 2.0 ** -70)
    bitmap = torch.empty((a.n + 63) // 64, dtype=torch.int64, device=wins[0].x.device)
    counts = torch.zeros(2, dtype=torch.int64, device=wins[0].x.device)
    n = a.n
    keys, off = np.empty(tg.ntraj + a.objs + 16, np.int64), np.zeros(tg.ntraj + a.objs + 17, np.int64)
    x, y, ts, idx = np.empty(n, np.float64), np.empty(n, np.float64), np.empty(n, np.int64), np.empty(n, np.uint32)
    m, npts = C.c_int64(), C.c_int64()
    outs = (keys.ctypes.data, off.ctypes.data, len(keys), x.ctypes.data, y.ctypes.data, ts.ctypes.data, idx.ctypes.data, n,
            C.byref(m), C.byref(npts))

    def trange(i):
        p = wins[i].c_struct()
        _lib.check(L.gf_trange_run(plan.handle, tg.handle, C.byref(p), *outs), ctx.handle, "gf_trange_run")

    def two_call(i):
        p = wins[i].c_struct()
        _lib.check(L.gf_range_run(rplan, C.byref(p), bitmap.data_ptr(), None, counts.data_ptr()), ctx.handle, "gf_range_run")
        _lib.check(L.gf_traj_select(tg.handle, C.byref(p), bitmap.data_ptr(), *outs), ctx.handle, "gf_traj_select")

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        t0 = time.perf_counter()
        fn()
        host = (time.perf_counter() - t0) * 1e3
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), host

    trange(0)
    two_call(0)  # warm-up: code objects, workspaces, the cached range plan
    grp, tr, tc, rows = [], [], [], []
    for _ in range(a.reps):
        for i in range(a.windows):
            grp.append(timed(lambda: tg.regroup(wins[i])))
            tr.append(timed(lambda: trange(i)))
            rows.append((m.value, npts.value))
            tc.append(timed(lambda: two_call(i)))
            rows[-1] += (m.value, npts.value)
    med = lambda v, j: statistics.median(t[j] for t in v)  # noqa: E731
    mt, mp, ct, cp = (int(statistics.median(c)) for c in zip(*rows))
    floor_ms = (20.0 * n + 2 * 28.0 * mp) / (a.hbm_gbs * 1e9) * 1e3
    st = plan.stats()
    info = plan.info()
    res = {"bench": "trange", "set": a.set, "ngon": a.ngon, "npoly": len(polys), "n": n, "objs": a.objs, "hot": a.hot,
           "step": a.step, "wide_ring": info["wide_ring"], "windows": a.windows, "calls": len(tr), "trajectories": tg.ntraj,
           "plan": st, "info": info, "rows": mt, "points": mp, "two_call_rows": ct, "two_call_points": cp,
           "trange_ms": round(med(tr, 0), 4), "trange_host_ms": round(med(tr, 1), 4),
           "trange_min_max_ms": [round(min(t[0] for t in tr), 4), round(max(t[0] for t in tr), 4)],
           "two_call_ms": round(med(tc, 0), 4), "two_call_host_ms": round(med(tc, 1), 4),
           "ratio": round(med(tc, 0) / med(tr, 0), 3), "traj_group_ms": round(med(grp, 0), 4),
           "floor_ms": round(floor_ms, 4), "trange_over_floor": round(med(tr, 0) / floor_ms, 2)}
    ids = {"trange": _lib.K_TRANGE, "select": _lib.K_TRAJ_SELECT, "range": _lib.K_RANGE_SCAN}
    for label, fn in (("kernel_ms_trange", trange), ("kernel_ms_two_call", two_call)):
        acc = {nm: 0.0 for nm in ids}
        for i in range(a.windows):
            tg.regroup(wins[i])
            ctx.set_timing(sum(1 << k for k in ids.values()))
            for k in ids.values():
                ctx.timing(k)
            fn(i)
            for nm, k in ids.items():
                acc[nm] += ctx.timing(k)[0] / a.windows
            ctx.set_timing(0)
        res[label] = {nm: round(v, 4) for nm, v in acc.items()}
    plan.close()
    tg.close()
    return res


if __name__ == "__main__":
    main()
