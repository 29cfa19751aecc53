"""Linestring queries: ms per window of the point-linestring range query and kNN (k = 50), warm, on
device-resident windows (default 10M uniform points on the 100 x 100 Beijing grid, one zigzag line of
4,096 segments crossing the grid corner to corner, r = one cell length), by three routes timed in one
process, interleaved window by window:

  a  the linestring plan (gf_range_pls_plan_create / gf_knn_pls_plan_create), sub-chain envelopes on
  b  the same plan in chain mode 1 (the plain segment loop)
  c  the route a user has without linestring queries: gf_range_ppoly_plan_create /
     gf_knn_ppoly_plan_create on the there-and-back closed ring of the same vertices

--segments N sets the line's length, --lines L cuts it into L consecutive shorter lines (the range query
takes the set; kNN, which takes one line, keeps the whole chain), --plain makes route a itself run in
mode 1.  Several distinct windows are visited round-robin; every figure is the median over >= 20 timed
windows after a warm-up pass of every route over every window, from device events around the call (the
range call is asynchronous, the kNN call ends in a synchronise), with the quartiles and the extremes
as the spread.  Before anything is printed the three routes must select the same points: equal bitmaps
per window, equal kNN objIDs and indices (a and b: equal distance bits too; c walks every segment in
both directions, whose minimum may differ from a's in the last bits -- tests/test_linestring_ref.py).
Prints one JSON line (and appends it to --out, default profiles/linestring_bench.jsonl)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BEIJING = (115.5, 117.6, 39.6, 41.1)
GRID_N = 100
CL = (BEIJING[1] - BEIJING[0]) / GRID_N


def zigzag(segments):
    """`segments` segments from the grid's lower left to its upper right, every other vertex one cell
    length above the diagonal: the line's envelope is the whole grid."""
    x0, x1, y0, y1 = BEIJING[0] + CL / 2, BEIJING[1] - CL / 2, BEIJING[2] + CL / 2, BEIJING[3] - 3 * CL / 2
    return [(x0 + (x1 - x0) * i / segments, y0 + (y1 - y0) * i / segments + (CL if i % 2 else 0.0))
            for i in range(segments + 1)]


def cut(chain, lines):
    """`lines` consecutive pieces of the chain (neighbours share a vertex), each of >= 1 segment."""
    nseg = len(chain) - 1
    lines = max(1, min(lines, nseg))
    cuts = [round(nseg * j / lines) for j in range(lines + 1)]
    return [chain[a:b + 1] for a, b in zip(cuts[:-1], cuts[1:])]


def there_and_back(chain):
    return [list(chain) + list(chain[::-1])]


def spread(v):
    v = sorted(v)
    q = statistics.quantiles(v, n=4)
    return {"median": round(statistics.median(v), 4), "q1": round(q[0], 4), "q3": round(q[2], 4),
            "min": round(v[0], 4), "max": round(v[-1], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--segments", type=int, default=4096)
    ap.add_argument("--lines", type=int, default=1)
    ap.add_argument("--plain", action="store_true", help="route a runs in chain mode 1 too")
    ap.add_argument("--k", type=int, default=50)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=8, help="timed passes over the windows (windows x rounds >= 20)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "linestring_bench.jsonl"))
    a = ap.parse_args()
    assert a.windows * a.rounds >= 20, "the median wants >= 20 timed windows"
    line = json.dumps(run(a))
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


def run(a):
    import torch

    import spatialflink_amd as sf
    from spatialflink_amd import _lib

    assert torch.cuda.is_available(), "bench_linestring needs a HIP device"
    L = _lib.lib()
    assert L.gf_build_is_product() == 1, L.gf_build_info().decode()
    grid = sf.UniformGrid(GRID_N, *BEIJING)
    chain = zigzag(a.segments)
    pieces = cut(chain, a.lines)
    r = CL
    conf = sf.QueryConfiguration(sf.QueryType.WindowBased)
    wins = []
    for i in range(a.windows):
        x, y = sf.synthetic_uniform(500 + i, a.n, *BEIJING)
        wins.append(sf.PointWindow.from_numpy(x, y, np.arange(a.n, dtype=np.int64)))
    dev = wins[0].x.device
    ctx = _lib.context(dev.index)

    # ---- plans, once, outside the timed region ----
    def range_op(mode):
        op = sf.PointLineStringRangeQuery(conf, grid)
        op.chain_mode = mode
        return op, op.plan(dev.index, [sf.LineString(c, grid) for c in pieces], r)[1]

    def knn_op(mode):
        op = sf.PointLineStringKNNQuery(conf, grid)
        op.chain_mode = mode
        return op, op.plan(dev.index, sf.LineString(chain, grid), r, a.k)[1]

    mode_a = 1 if a.plain else 0
    pop = sf.PointPolygonRangeQuery(conf, grid)
    pkn = sf.PointPolygonKNNQuery(conf, grid)
    keep = [range_op(mode_a), range_op(1), knn_op(mode_a), knn_op(1), pop, pkn]
    rplans = {"a": keep[0][1], "b": keep[1][1],
              "c": pop.plan(dev.index, [sf.Polygon(there_and_back(c), grid) for c in pieces], r)[1]}
    kplans = {"a": keep[2][1], "b": keep[3][1],
              "c": pkn.plan(dev.index, sf.Polygon(there_and_back(chain), grid), r, a.k)[1]}
    words = (a.n + 63) // 64
    bitmaps = {k: torch.zeros(words, dtype=torch.int64, device=dev) for k in rplans}
    counts = {k: torch.zeros(2, dtype=torch.int64, device=dev) for k in rplans}
    kout = {k: (np.empty(a.k, np.int64), np.empty(a.k, np.float64), np.empty(a.k, np.int64), C.c_int32()) for k in kplans}

    def do_range(route, i):
        p = wins[i].c_struct()
        _lib.check(L.gf_range_run(rplans[route], C.byref(p), bitmaps[route].data_ptr(), None, counts[route].data_ptr()),
                   ctx.handle, "gf_range_run")

    def do_knn(route, i):
        p = wins[i].c_struct()
        oo, od, oi, m = kout[route]
        _lib.check(L.gf_knn_run(kplans[route], C.byref(p), oo.ctypes.data, od.ctypes.data, oi.ctypes.data, C.byref(m)),
                   ctx.handle, "gf_knn_run")

    def timed(fn, route, i):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(route, i)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    # ---- warm-up + the same-points check, every route over every window ----
    hits = []
    for i in range(a.windows):
        for route in "abc":
            do_range(route, i)
            do_knn(route, i)
        torch.cuda.synchronize()
        assert torch.equal(bitmaps["a"], bitmaps["b"]) and torch.equal(bitmaps["a"], bitmaps["c"]), f"range: window {i}"
        assert int(counts["a"][0]) == int(counts["b"][0]) == int(counts["c"][0]) > 0
        hits.append(int(counts["a"][0]))
        ma = kout["a"][3].value
        assert ma == kout["b"][3].value == kout["c"][3].value == a.k, f"kNN: window {i}"
        for other in "bc":
            assert np.array_equal(kout["a"][0][:ma], kout[other][0][:ma]), f"kNN objIDs: window {i} route {other}"
            assert np.array_equal(kout["a"][2][:ma], kout[other][2][:ma]), f"kNN indices: window {i} route {other}"
        assert np.array_equal(kout["a"][1][:ma].view(np.int64), kout["b"][1][:ma].view(np.int64)), f"kNN distances: window {i}"

    # ---- timed: the three routes interleaved window by window ----
    tr = {k: [] for k in "abc"}
    tk = {k: [] for k in "abc"}
    for _ in range(a.rounds):
        for i in range(a.windows):
            for route in "abc":
                tr[route].append(timed(do_range, route, i))
            for route in "abc":
                tk[route].append(timed(do_knn, route, i))
    cells = [C.c_int64() for _ in range(4)]
    L.gf_range_plan_stats(rplans["a"], *[C.byref(c) for c in cells])
    res = {"bench": "linestring", "n": a.n, "segments": a.segments, "lines": len(pieces), "r_cells": 1.0, "k": a.k,
           "plain": bool(a.plain), "windows": a.windows, "timed_windows": len(tr["a"]),
           "hits_median": int(statistics.median(hits)),
           "plan_cells": {"none": cells[0].value, "candidate": cells[1].value, "guaranteed": cells[2].value,
                          "inside": cells[3].value},
           "range_ms": {"a_linestring": spread(tr["a"]), "b_plain_loop": spread(tr["b"]), "c_polygon_ring": spread(tr["c"])},
           "knn_ms": {"a_linestring": spread(tk["a"]), "b_plain_loop": spread(tk["b"]), "c_polygon_ring": spread(tk["c"])},
           "range_c_over_a": round(statistics.median(tr["c"]) / statistics.median(tr["a"]), 3),
           "range_b_over_a": round(statistics.median(tr["b"]) / statistics.median(tr["a"]), 3),
           "knn_c_over_a": round(statistics.median(tk["c"]) / statistics.median(tk["a"]), 3),
           "knn_b_over_a": round(statistics.median(tk["b"]) / statistics.median(tk["a"]), 3)}
    del keep
    return res


if __name__ == "__main__":
    main()
