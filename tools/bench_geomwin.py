"""Geometry windows: ms per window of the polygon / linestring window operators against query points
(gf_geom_prepare, gf_geom_range_run, gf_geom_knn_enqueue), warm, on device-resident windows (default 1M
regular 16-gons about a third of a cell across on the 100 x 100 Beijing grid).

  --vertices V   vertices per object (polygons: V distinct + the closing one; --lines: a V-vertex arc)
  --skew F       a share F of the objects has 4,096 vertices instead
  --lines        linestring windows
  --nq 1|16      query points of the range query (kNN always takes the first)
  --wide LIST    the wide_vertices values compared, interleaved in ONE process (0 = the library's default;
                 2147483647 = lanes only)

The library has no other route that evaluates a geometry window on the GPU, so there is no "before": the
comparison is lanes only against the wave path.  Before anything is printed the tool checks that every
variant selects the same objects (bitmaps equal, kNN records byte-equal).  Timing: device events around
each call on the context stream, after a warm-up of every variant; per (radius, variant) the median with
[min, max] over --windows x --reps timed windows, the variants alternating inside every window visit.
  prepare_ms     gf_geom_prepare of the window on the ONE index every window goes through (the per-window
                 path of a continuous query: the index's arrays are reused, nothing is allocated and nothing
                 waits); the variant is applied to the index before the timed call
  prepare_cold_ms  a NEW index for the window and its destruction, by the host clock with the stream
                 synchronised: the allocations and waits a first window pays (median over the windows)
  range_ms       classify + the exact passes + the count (gf_geom_range_run)
  knn_ms         classify + the exact passes + the select (gf_geom_knn_enqueue, k = --k)
  *_vertex_gbs   16 B x the window's vertices / that time: the prepare reads every vertex once, so its
                 figure is an effective bandwidth to hold against --hbm-gbs; the range / kNN figures
                 divide the same bytes by a pass that reads only the tested objects' vertices
Appends one JSON line per (radius, variant) to --out (default profiles/geomwin_bench.jsonl)."""
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
LONG_VERTICES = 4096
INT32_MAX = 2 ** 31 - 1


def make_window(seed, n, vertices, skew, lines):
    """(ring_off or None, vert_off, vx, vy): n objects, centres uniform over the grid's box"""
    rng = np.random.default_rng(seed)
    cx = rng.uniform(BEIJING[0], BEIJING[1], n)
    cy = rng.uniform(BEIJING[2], BEIJING[3], n)
    m = np.full(n, max(vertices, 3 if not lines else 2), np.int64)   # distinct vertices per object
    m[rng.random(n) < skew] = LONG_VERTICES
    nv = m if lines else m + 1                                         # polygons repeat the first vertex
    vert_off = np.zeros(n + 1, np.int64)
    np.cumsum(nv, out=vert_off[1:])
    obj = np.repeat(np.arange(n), nv)
    j = np.arange(vert_off[-1]) - vert_off[obj]
    mm = m[obj]
    ang = 2.0 * np.pi * (j % mm) / mm * (0.75 if lines else 1.0)       # a line: three quarters of the circle
    rad = CL / 6.0
    vx, vy = cx[obj] + rad * np.cos(ang), cy[obj] + rad * np.sin(ang)
    if not lines:  # closed bit for bit
        last = vert_off[1:] - 1
        vx[last], vy[last] = vx[vert_off[:-1]], vy[vert_off[:-1]]
    ring_off = None if lines else np.arange(n + 1, dtype=np.int32)
    return ring_off, vert_off.astype(np.int32), vx, vy


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--vertices", type=int, default=16)
    ap.add_argument("--skew", type=float, default=0.0)
    ap.add_argument("--lines", action="store_true")
    ap.add_argument("--nq", type=int, choices=(1, 16), default=1)
    ap.add_argument("--k", type=int, default=50)
    ap.add_argument("--radii", default="1,3", help="query radii in cell lengths")
    ap.add_argument("--wide", default="64,128,256,384,1024,2147483647")
    ap.add_argument("--windows", type=int, default=3, help="distinct windows visited round-robin")
    ap.add_argument("--reps", type=int, default=8, help="timed visits of every window: windows x reps >= 24")
    ap.add_argument("--hbm-gbs", type=float, default=4000.0, help="the bandwidth the project's roofline notes quote")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "geomwin_bench.jsonl"))
    a = ap.parse_args()
    rows = run(a)
    for row in rows:
        print(json.dumps(row))
    if a.out:
        with open(a.out, "a") as f:
            for row in rows:
                f.write(json.dumps(row) + "\n")


def run(a):
    import torch

    import spatialflink_amd as sf
    from spatialflink_amd import _lib
    from spatialflink_amd.spatialOperators import knn_record_bytes

    assert torch.cuda.is_available(), "bench_geomwin needs a HIP device"
    L = _lib.lib()
    assert L.gf_build_is_product() == 1, L.gf_build_info().decode()
    assert a.windows * a.reps >= 24, "at least 24 timed windows"
    variants = [int(v) for v in a.wide.split(",")]
    radii = [float(v) for v in a.radii.split(",")]
    kind = _lib.GEOM_LINESTRING if a.lines else _lib.GEOM_POLYGON
    grid = sf.UniformGrid(GRID_N, *BEIJING)
    import time

    wins, nvert, cold = [], [], []
    for i in range(a.windows):
        ro, vo, vx, vy = make_window(500 + i, a.n, a.vertices, a.skew, a.lines)
        wins.append(sf.GeometryWindow.from_csr(kind, ro, vo, vx, vy))
        nvert.append(len(vx))
    index = sf.GeometryIndex(wins[0], grid)  # the one index of the continuous query
    ctx = index.ctx
    dev = wins[0].vert_off.device
    geoms = [w.c_struct() for w in wins]
    for w in wins * 2:  # a new index per window: what the first window of a query pays
        ctx.synchronize()
        t0 = time.perf_counter()
        ix = sf.GeometryIndex(w, grid)
        ix.close()  # (waits for the stream)
        cold.append((time.perf_counter() - t0) * 1e3)
    # the query points: a 4 x 4 lattice 1.5 cells apart around the grid's middle (the first alone for nq = 1)
    qx = np.array([BEIJING[0] + (50.3 + 1.5 * (i % 4)) * CL for i in range(a.nq)], np.float64)
    qy = np.array([BEIJING[2] + (30.4 + 1.5 * (i // 4)) * CL for i in range(a.nq)], np.float64)
    words = (a.n + 63) // 64
    bitmap = torch.zeros(words, dtype=torch.int64, device=dev)
    counts = torch.zeros(2, dtype=torch.int64, device=dev)
    rec = torch.zeros(knn_record_bytes(a.k), dtype=torch.uint8, device=dev)

    def query(nq, r):
        h = C.c_void_p()
        _lib.check(L.gf_geom_query_create(ctx.handle, C.byref(grid.c_grid), qx.ctypes.data, qy.ctypes.data, nq, r, 0, 0,
                                          C.byref(h)), ctx.handle, "gf_geom_query_create")
        return h

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def info_of(q):
        v = [C.c_int64() for _ in range(4)]
        _lib.check(L.gf_geom_info(q, *(C.byref(c) for c in v)), ctx.handle, "gf_geom_info")
        return dict(zip(("filtered", "all_guaranteed", "tested", "wave_path"), (c.value for c in v)))

    out = []
    for rc in radii:
        r = rc * CL
        rq, kq = query(a.nq, r), query(1, r)
        vary = lambda t: _lib.check(L.gf_geom_index_set_thresholds(index.handle, t), ctx.handle, "set_thresholds")  # noqa: E731
        prep = lambda i: _lib.check(L.gf_geom_prepare(ctx.handle, C.byref(grid.c_grid), C.byref(geoms[i]), C.byref(index.handle)),  # noqa: E731
                                    ctx.handle, "gf_geom_prepare")
        rng_ = lambda i: _lib.check(L.gf_geom_range_run(rq, index.handle, bitmap.data_ptr(), counts.data_ptr()), ctx.handle, "range")  # noqa: E731
        knn = lambda i: _lib.check(L.gf_geom_knn_enqueue(kq, index.handle, a.k, C.c_void_p(rec.data_ptr())), ctx.handle, "knn")  # noqa: E731
        # check first (this is the warm-up too): every variant selects the same objects
        infos = {}
        for i in range(a.windows):
            ref = None
            for t in variants:
                vary(t)
                prep(i)
                rng_(i)
                knn(i)
                got = (bitmap.cpu().numpy().copy(), counts.cpu().numpy().copy(), rec.cpu().numpy().tobytes())
                head = _lib.GfKnnHeader.from_buffer_copy(got[2][: C.sizeof(_lib.GfKnnHeader)])
                assert head.status == 0 and 0 <= head.n <= a.k and head.k == a.k, f"kNN record not final: {head.status}, n = {head.n}"
                assert int(got[1][0]) == int(np.unpackbits(got[0].view(np.uint8)).sum()), "counts[0] is not the bitmap's count"
                if i == 0:
                    infos[t] = dict(range=info_of(rq), knn=info_of(kq), wide_objects=index.info()["wide"])
                if ref is None:
                    ref = got
                assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]) and got[2] == ref[2], \
                    f"wide_vertices = {t} selects other objects than {variants[0]} (window {i}, r = {rc} cells)"
        tp, tr, tk = ({t: [] for t in variants} for _ in range(3))
        for _ in range(a.reps):
            for i in range(a.windows):
                for t in variants:  # interleaved: every variant sees the same window at the same moment
                    vary(t)  # (not timed: it prepares the previous window again)
                    tp[t].append(timed(lambda: prep(i)))
                    tr[t].append(timed(lambda: rng_(i)))
                    tk[t].append(timed(lambda: knn(i)))
        gbs = lambda ms: round(16.0 * statistics.mean(nvert) / (ms * 1e-3) / 1e9, 1)  # noqa: E731
        for t in variants:
            mp, mr, mk = (statistics.median(v[t]) for v in (tp, tr, tk))
            out.append({"bench": "geomwin", "kind": "linestring" if a.lines else "polygon", "n": a.n, "vertices": a.vertices,
                        "skew": a.skew, "window_vertices": int(statistics.mean(nvert)), "nq": a.nq, "k": a.k, "r_cells": rc,
                        "wide_vertices": t, "timed_windows": len(tp[t]),
                        "prepare_cold_ms": round(statistics.median(cold), 3),
                        "prepare_ms": round(mp, 4), "prepare_min_max_ms": [round(min(tp[t]), 4), round(max(tp[t]), 4)],
                        "range_ms": round(mr, 4), "range_min_max_ms": [round(min(tr[t]), 4), round(max(tr[t]), 4)],
                        "knn_ms": round(mk, 4), "knn_min_max_ms": [round(min(tk[t]), 4), round(max(tk[t]), 4)],
                        "range_total_ms": round(mp + mr, 4), "knn_total_ms": round(mp + mk, 4),
                        "prepare_vertex_gbs": gbs(mp), "range_total_vertex_gbs": gbs(mp + mr), "knn_total_vertex_gbs": gbs(mp + mk),
                        "hbm_gbs": a.hbm_gbs, "info": infos[t]})
        L.gf_geom_query_destroy(rq)
        L.gf_geom_query_destroy(kq)
    index.close()
    return out


if __name__ == "__main__":
    main()
