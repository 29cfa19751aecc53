"""tJoin: ms per window pair of gf_tjoin_run, warm, on device-resident windows already grouped by objID
(default 10M ordinary and 1M query points over ~100k objIDs each on the 100 x 100 Beijing grid, r = one
cell length: L = 1).  Trajectories are short random walks, so one trajectory's points share cells -- what
the probe's run skip is for; --uniform scatters the points instead (the skip gains nothing); --hot F puts a
share F of BOTH sides into one cell.

Several distinct window pairs are visited round-robin through ONE pair of gf_traj_groups and ONE gf_tjoin
object (their workspaces and the row table reused).  Every figure is a median over the timed calls: device
events around the call and the host clock around it (the call ends in a stream synchronise).  gf_traj_group
of the two sides is timed apart: it is shared with tStats, tKnn and the sub-trajectory extraction.

On the same windows the tool also times gf_join_pp, today's route to the same answer up to the point where
the host would start reducing its pairs: first counting only (no pair buffer), then, when 8 B per pair fit
--max-pair-gb, materialising them.  join_pp_ms is the materialising call where it ran, else the counting
one (join_pp_materialised says which); ratio = join_pp_ms / tjoin_ms.

The per-kernel-id device times (gf_ctx_timing) come from a second loop: tjoin = this operator's own kernels
(the probe among them), radix = the sorts' passes, words = the sorts' key extraction.
Prints one JSON line (and appends it to --out, default profiles/tjoin_bench.jsonl)."""
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
HOT_CELL = (47, 19)


def make_window(seed, n, nobj, grid_n, step, hot, uniform):
    rng = np.random.default_rng(seed)
    pool = np.concatenate([rng.integers(0, 1 << 40, nobj // 2), -(1 << 63) + np.arange(nobj - nobj // 2)]).astype(np.int64)
    t = rng.integers(0, len(pool), n)
    if uniform:
        x = rng.uniform(BEIJING[0], BEIJING[1], n)
        y = rng.uniform(BEIJING[2], BEIJING[3], n)
    else:  # the k-th point of a trajectory = its start + the sum of k steps
        order = np.argsort(t, kind="stable")
        ts_sorted = t[order]
        first = np.ones(n, bool)
        first[1:] = ts_sorted[1:] != ts_sorted[:-1]
        x, y = np.empty(n), np.empty(n)
        for out, lo, hi in ((x, BEIJING[0], BEIJING[1]), (y, BEIJING[2], BEIJING[3])):
            walk = np.cumsum(step * rng.standard_normal(n))
            base = np.maximum.accumulate(np.where(first, np.arange(n), 0))
            out[order] = rng.uniform(lo, hi, len(pool))[ts_sorted] + (walk - walk[base])
    if hot > 0:
        cl = (BEIJING[1] - BEIJING[0]) / grid_n
        m = rng.random(n) < hot
        x[m] = BEIJING[0] + (HOT_CELL[0] + rng.uniform(0.01, 0.99, int(m.sum()))) * cl
        y[m] = BEIJING[2] + (HOT_CELL[1] + rng.uniform(0.01, 0.99, int(m.sum()))) * cl
    ts = 1_600_000_000_000 + np.arange(n, dtype=np.int64) // 8
    return x, y, pool[t], ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-o", type=int, default=10_000_000)
    ap.add_argument("--n-q", type=int, default=1_000_000)
    ap.add_argument("--objs", type=int, default=100_000)
    ap.add_argument("--grid", type=int, default=100)
    ap.add_argument("--r", type=float, default=0.0, help="0: one cell length")
    ap.add_argument("--step", type=float, default=0.002)
    ap.add_argument("--hot", type=float, default=0.0)
    ap.add_argument("--uniform", action="store_true")
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--max-pair-gb", type=float, default=48.0)
    ap.add_argument("--no-join", action="store_true", help="skip gf_join_pp")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tjoin_bench.jsonl"))
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

    assert torch.cuda.is_available(), "bench_tjoin needs a HIP device"
    L = _lib.lib()
    assert L.gf_build_is_product() == 1, L.gf_build_info().decode()
    grid = sf.UniformGrid(a.grid, *BEIJING)
    r = a.r if a.r > 0 else grid.getCellLength()
    wo = [sf.PointWindow.from_numpy(*make_window(100 + i, a.n_o, a.objs, a.grid, a.step, a.hot, a.uniform)) for i in range(a.windows)]
    wq = [sf.PointWindow.from_numpy(*make_window(200 + i, a.n_q, a.objs, a.grid, a.step, a.hot, a.uniform)) for i in range(a.windows)]
    go, gq = sf.TrajectoryGroups(wo[0]), sf.TrajectoryGroups(wq[0])
    ctx = go.ctx
    h = C.c_void_p()

    def tjoin(i):
        po, pq = wo[i].c_struct(), wq[i].c_struct()
        _lib.check(L.gf_tjoin_run(go.handle, C.byref(po), gq.handle, C.byref(pq), C.byref(grid.c_grid), r, _lib.TJOIN_PAIR,
                                  C.byref(h)), ctx.handle, "gf_tjoin_run")

    def regroup(i):
        go.regroup(wo[i])
        gq.regroup(wq[i])

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        t0 = time.perf_counter()
        fn()
        host = (time.perf_counter() - t0) * 1e3
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), host

    tjoin(0)  # warm-up: code objects, the workspace, the table's growth
    c = [C.c_int64() for _ in range(7)]
    L.gf_tjoin_info(h, *(C.byref(v) for v in c))
    first_passes = c[6].value
    grp, tj, info = [], [], []
    for _ in range(a.reps):
        for i in range(a.windows):
            grp.append(timed(lambda: regroup(i)))
            tj.append(timed(lambda: tjoin(i)))
            L.gf_tjoin_info(h, *(C.byref(v) for v in c))
            info.append([v.value for v in c])
    med = lambda v, j: statistics.median(t[j] for t in v)  # noqa: E731
    rows, emitted, otraj, opoints, qtraj, qpoints, passes = (int(statistics.median(col)) for col in zip(*info))
    res = {"bench": "tjoin", "n_o": a.n_o, "n_q": a.n_q, "objs": a.objs, "grid": a.grid, "r": r, "step": a.step, "hot": a.hot,
           "uniform": a.uniform, "windows": a.windows, "calls": len(tj), "trajectories": [go.ntraj, gq.ntraj],
           "rows": rows, "emitted": emitted, "otraj": otraj, "opoints": opoints, "qtraj": qtraj, "qpoints": qpoints,
           "probe_passes_first_call": first_passes, "probe_passes": passes,
           "tjoin_ms": round(med(tj, 0), 4), "tjoin_host_ms": round(med(tj, 1), 4),
           "tjoin_min_max_ms": [round(min(t[0] for t in tj), 4), round(max(t[0] for t in tj), 4)],
           "traj_group_ms": round(med(grp, 0), 4), "total_ms": round(med(tj, 0) + med(grp, 0), 4)}
    ids = {"tjoin": _lib.K_TJOIN, "radix": _lib.K_BUCKET, "words": _lib.K_TKNN}
    for i in range(a.windows):  # the groups of each pair first, untimed: the breakdown is gf_tjoin_run's alone
        regroup(i)
        ctx.set_timing(sum(1 << k for k in ids.values()))
        for k in ids.values():
            ctx.timing(k)
        tjoin(i)
        for nm, k in ids.items():
            res.setdefault("kernel_ms_per_window", {}).setdefault(nm, 0.0)
            res["kernel_ms_per_window"][nm] += ctx.timing(k)[0] / a.windows
        ctx.set_timing(0)
    res["kernel_ms_per_window"] = {nm: round(v, 4) for nm, v in res["kernel_ms_per_window"].items()}
    L.gf_tjoin_destroy(h)
    if not a.no_join:
        try:
            res.update(join_pp(a, L, _lib, torch, ctx, grid, r, wo, wq, timed, med))
            res["ratio_join_pp_over_tjoin"] = round(res["join_pp_ms"] / res["tjoin_ms"], 3)
        except (_lib.GeoFlinkError, ValueError, RuntimeError) as e:  # the tJoin figures stand on their own
            res["join_pp_error"] = str(e)
    go.close()
    gq.close()
    return res


def join_pp(a, L, _lib, torch, ctx, grid, r, wo, wq, timed, med):
    npairs = C.c_int64()

    def call(i, buf, cap):
        po, pq = wo[i].c_struct(), wq[i].c_struct()
        st = L.gf_join_pp(ctx.handle, C.byref(grid.c_grid), C.byref(grid.c_grid), C.byref(po), C.byref(pq), r, 0, _lib.METRIC_SQRT,
                          buf, cap, C.byref(npairs))
        if st != _lib.GF_ERR_CAPACITY:
            _lib.check(st, ctx.handle, "gf_join_pp")
        return st

    call(0, None, 0)  # warm-up
    cnt, counts = [], []
    for _ in range(a.reps):
        for i in range(a.windows):
            cnt.append(timed(lambda: call(i, None, 0)))
            counts.append(npairs.value)
    out = {"join_pp_pairs": int(statistics.median(counts)), "join_pp_pair_bytes": 8 * int(statistics.median(counts)),
           "join_pp_count_only_ms": round(med(cnt, 0), 4), "join_pp_materialised": False, "join_pp_ms": round(med(cnt, 0), 4)}
    cap = int(max(counts) * 1.02) + 1024
    free_b = torch.cuda.mem_get_info()[0]
    if 8 * cap <= min(a.max_pair_gb * 1e9, 0.4 * free_b):  # (the join's own spill scratch takes as much again)
        buf = torch.empty(2 * cap, dtype=torch.int32, device=wo[0].x.device)
        if call(0, buf.data_ptr(), cap) == _lib.GF_OK:
            mat = []
            for _ in range(a.reps):
                for i in range(a.windows):
                    mat.append(timed(lambda: call(i, buf.data_ptr(), cap)))
            out.update({"join_pp_materialised": True, "join_pp_ms": round(med(mat, 0), 4), "join_pp_host_ms": round(med(mat, 1), 4)})
    return out


if __name__ == "__main__":
    main()
