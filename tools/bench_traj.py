"""Trajectory operators: ms per window of gf_traj_group and gf_tstats_run, warm, on device-resident
windows (default 10M points over ~100k objIDs; --hot F gives one objID a share F of the points).

Several distinct windows, together larger than the 256 MB MALL, are visited round-robin through ONE
groups object (its workspace reused), so no window is served from cache.  Every figure is a median
over the timed calls: device events on the context's stream around the call, and the host clock
around it (both calls end in a stream synchronise).  tStats is timed without its row read-back
(cap 0) and with it.  With --timing the per-kernel-group device times (gf_ctx_timing) are added from
a second loop.  The algorithmic floor it is set against: 32 B per point read (x, y, objID, ts) plus
perm (4 B per point) and the per-trajectory rows written (keys 8 B + seg_off 4 B; tStats 24 B).

Bytes moved come from a separate counter run (never together with a trace):
  rocprofv3 --pmc FETCH_SIZE -d OUT/fetch -o fetch --output-format csv -- python tools/bench_traj.py --plain --windows 2 --reps 1
  rocprofv3 --pmc WRITE_SIZE -d OUT/write -o write --output-format csv -- python tools/bench_traj.py --plain --windows 2 --reps 1
  python tools/bench_traj.py --pmc-summary OUT --calls 3        (calls = the warm-up + the timed windows of that run)
Prints one JSON line (and appends it to --out)."""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12  # B/s, MI355X HBM3E specification


def make_window(seed, n, nobj, hot):
    rng = np.random.default_rng(seed)
    pool = np.concatenate([rng.integers(0, 1 << 40, nobj // 2), -(1 << 63) + np.arange(nobj - nobj // 2)]).astype(np.int64)
    obj = pool[rng.integers(0, len(pool), n)]
    if hot > 0:
        obj[rng.random(n) < hot] = 4242
    x = rng.uniform(115.5, 117.6, n)
    y = rng.uniform(39.6, 41.1, n)
    ts = 1_600_000_000_000 + np.arange(n, dtype=np.int64) // 8 + rng.integers(0, 3, n)  # arrival order, some ties / late points
    return x, y, obj, ts


def floor_bytes(n, ntraj):
    # "both": one read of the window (32 B per point), perm, and every row -- the issue's floor for
    # grouping + tStats together; the two calls on their own re-read what they need
    return {"group": 32 * n + 4 * n + 12 * ntraj, "tstats": 24 * n + 4 * n + 24 * ntraj,
            "both": 32 * n + 4 * n + 36 * ntraj}


def pmc_summary(d, calls):
    tot = {}
    for counter in ("FETCH_SIZE", "WRITE_SIZE"):
        kb, per = 0.0, {}
        for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
            with open(f) as fh:
                for row in csv.DictReader(fh):
                    if row["Counter_Name"] != counter:
                        continue
                    name = row["Kernel_Name"].split("(")[0]
                    if not any(s in name for s in ("traj_", "tstats_", "radix_", "scan_")):
                        continue
                    v = float(row["Counter_Value"])
                    kb += v
                    per[name] = per.get(name, 0.0) + v
        tot[counter] = {"KB_per_call": kb / calls, "by_kernel_KB_per_call": {k: v / calls for k, v in sorted(per.items())}}
    # gfx950 reports half of wide streaming reads (FETCH_SIZE); both readings are given
    res = {"bench": "traj_pmc", "calls": calls, "fetch_bytes_per_window_raw": 1024.0 * tot["FETCH_SIZE"]["KB_per_call"],
           "fetch_bytes_per_window_x2": 2048.0 * tot["FETCH_SIZE"]["KB_per_call"],
           "write_bytes_per_window": 1024.0 * tot["WRITE_SIZE"]["KB_per_call"], "detail": tot}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--objs", type=int, default=100_000)
    ap.add_argument("--hot", type=float, default=0.0)
    ap.add_argument("--windows", type=int, default=4)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--long-threshold", type=int, default=0)
    ap.add_argument("--timing", action="store_true")
    ap.add_argument("--plain", action="store_true", help="counter runs: one grouping + one tStats (no rows) per window")
    ap.add_argument("--out", default=None)
    ap.add_argument("--pmc-summary", default=None)
    ap.add_argument("--calls", type=int, default=1)
    a = ap.parse_args()
    if a.pmc_summary:
        res = pmc_summary(a.pmc_summary, a.calls)
    else:
        res = run(a)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


def run(a):
    import torch

    import spatialflink_amd as sf
    from spatialflink_amd import _lib

    assert torch.cuda.is_available(), "bench_traj needs a HIP device"
    L = _lib.lib()
    assert L.gf_build_is_product() == 1, L.gf_build_info().decode()
    wins = [sf.PointWindow.from_numpy(*make_window(100 + i, a.n, a.objs, a.hot)) for i in range(a.windows)]
    g = sf.TrajectoryGroups(wins[0])  # warm-up: code objects, the workspace
    g.set_long_threshold(a.long_threshold)
    g.tstats()
    ctx = g.ctx
    cnt = C.c_int64()

    def tstats_count_only(w):
        pts = w.c_struct()
        _lib.check(L.gf_tstats_run(g.handle, C.byref(pts), None, 0, None, None, None, None, 0, C.byref(cnt)), ctx.handle,
                   "gf_tstats_run")

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        t0 = time.perf_counter()
        fn()
        host = (time.perf_counter() - t0) * 1e3
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), host

    grp, tst, rows, ntraj = [], [], [], []
    for _ in range(a.reps):
        for w in wins:
            grp.append(timed(lambda: g.regroup(w)))
            tst.append(timed(lambda: tstats_count_only(w)))
            rows.append(timed(lambda: g.tstats()) if not a.plain else tst[-1])
            ntraj.append(g.ntraj)
    med = lambda v, j: statistics.median(t[j] for t in v)  # noqa: E731
    nt = int(statistics.median(ntraj))
    fl = floor_bytes(a.n, nt)
    res = {"bench": "traj", "n": a.n, "objs": a.objs, "hot": a.hot, "windows": a.windows, "calls": len(grp),
           "long_threshold": a.long_threshold, "ntraj": nt,
           "group_ms": round(med(grp, 0), 4), "group_host_ms": round(med(grp, 1), 4),
           "tstats_ms": round(med(tst, 0), 4), "tstats_host_ms": round(med(tst, 1), 4),
           "tstats_with_rows_ms": round(med(rows, 0), 4), "tstats_with_rows_host_ms": round(med(rows, 1), 4),
           "group_min_max_ms": [round(min(t[0] for t in grp), 4), round(max(t[0] for t in grp), 4)],
           "tstats_min_max_ms": [round(min(t[0] for t in tst), 4), round(max(t[0] for t in tst), 4)],
           "floor_bytes": fl,
           "floor_ms_at_8TBs": {k: round(v / HBM_PEAK * 1e3, 4) for k, v in fl.items()},
           "x_floor": {"group": round(med(grp, 0) / (fl["group"] / HBM_PEAK * 1e3), 1),
                       "tstats": round(med(tst, 0) / (fl["tstats"] / HBM_PEAK * 1e3), 1),
                       "both": round((med(grp, 0) + med(tst, 0)) / (fl["both"] / HBM_PEAK * 1e3), 1)}}
    if a.timing:
        ids = {"traj_group": _lib.K_TRAJ_GROUP, "radix": _lib.K_BUCKET, "tstats": _lib.K_TSTATS}
        ctx.set_timing(sum(1 << k for k in ids.values()))
        for k in ids.values():
            ctx.timing(k)
        for w in wins:
            g.regroup(w)
            tstats_count_only(w)
        res["kernel_ms_per_window"] = {nm: round(ctx.timing(k)[0] / len(wins), 4) for nm, k in ids.items()}
        ctx.set_timing(0)
    return res


if __name__ == "__main__":
    main()
