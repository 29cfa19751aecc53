"""Geometry windows against a query GEOMETRY: ms per window of the geometry-pair operators
(gf_geom_query_create_polygons / _linestrings through gf_geom_range_run and gf_geom_knn_enqueue), warm, on
device-resident windows prepared once (default 1M regular 16-gons about a third of a cell across on the
100 x 100 Beijing grid), against ONE query polygon (a regular --segments-gon six cells across) or ONE long
query linestring (a zigzag of --segments segments across a fifth of the grid).

  --lines          linestring windows (arcs of --vertices vertices)
  --query-lines    the query is the linestring (default: the polygon)
  --segments N     segments of the query geometry
  --skew F         a share F of the objects has 4,096 vertices instead
  --wide LIST      the wide_vertices values compared (0 = the library's default; 2147483647 = lanes only)
  --plain          also time every variant with chain mode 1 (no run envelope consulted): pruned against plain

The library has no other route that evaluates a geometry pair on the GPU and the parent commit has none
either, so there is no "before": the comparisons are the default against lanes only, and pruned against
plain.  Before anything is printed the tool checks that all variants select the same objects (bitmaps equal,
kNN records byte-equal).  Timing: device events around each call on the context stream, after a warm-up of
every variant; per (radius, variant) the median with [min, max] over --reps timed runs, the variants
alternating inside every visit.  The prepare is bench_geomwin.py's and is not timed here.
Appends one JSON line per (radius, variant) to --out (default profiles/geompair_bench.jsonl)."""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_geomwin import BEIJING, CL, GRID_N, make_window  # noqa: E402


def make_query(lines, segments):
    """the query geometry around the grid's middle"""
    cx, cy = BEIJING[0] + 50.3 * CL, BEIJING[2] + 30.4 * CL
    if lines:
        return [(cx - 10 * CL + 20 * CL * i / segments, cy + (0.8 * CL if i & 1 else 0.0) + 2 * CL * math.sin(i / 211.0))
                for i in range(segments + 1)]
    m = max(segments, 3)
    pts = [(cx + 3 * CL * math.cos(2 * math.pi * i / m), cy + 3 * CL * math.sin(2 * math.pi * i / m)) for i in range(m)]
    return [pts + [pts[0]]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--vertices", type=int, default=16)
    ap.add_argument("--skew", type=float, default=0.0)
    ap.add_argument("--lines", action="store_true")
    ap.add_argument("--query-lines", action="store_true")
    ap.add_argument("--segments", type=int, default=2048)
    ap.add_argument("--k", type=int, default=50)
    ap.add_argument("--radii", default="1,3", help="query radii in cell lengths")
    ap.add_argument("--wide", default="0,2147483647")
    ap.add_argument("--plain", action="store_true")
    ap.add_argument("--reps", type=int, default=24)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "geompair_bench.jsonl"))
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

    assert torch.cuda.is_available(), "bench_geompair needs a HIP device"
    L = _lib.lib()
    assert L.gf_build_is_product() == 1, L.gf_build_info().decode()
    assert a.reps >= 24, "at least 24 timed runs"
    kind = _lib.GEOM_LINESTRING if a.lines else _lib.GEOM_POLYGON
    grid = sf.UniformGrid(GRID_N, *BEIJING)
    ro, vo, vx, vy = make_window(500, a.n, a.vertices, a.skew, a.lines)
    win = sf.GeometryWindow.from_csr(kind, ro, vo, vx, vy)
    index = sf.GeometryIndex(win, grid)
    ctx = index.ctx
    dev = win.vert_off.device
    qgeom = make_query(a.query_lines, a.segments)
    qset = sf.LineStringSet([sf.LineString(qgeom)]) if a.query_lines else sf.PolygonSet([sf.Polygon(qgeom)])
    create = L.gf_geom_query_create_linestrings if a.query_lines else L.gf_geom_query_create_polygons
    bitmap = torch.zeros((a.n + 63) // 64, dtype=torch.int64, device=dev)
    counts = torch.zeros(2, dtype=torch.int64, device=dev)
    rec = torch.zeros(knn_record_bytes(a.k), dtype=torch.uint8, device=dev)
    variants = [(int(t), mode) for t in a.wide.split(",") for mode in ((0, 1) if a.plain else (0,))]

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
    for rc in [float(v) for v in a.radii.split(",")]:
        r = rc * CL
        cs = qset.c_struct()
        q = C.c_void_p()
        _lib.check(create(ctx.handle, C.byref(grid.c_grid), C.byref(cs), r, 0, 0, C.byref(q)), ctx.handle, "create")

        def vary(v):
            _lib.check(L.gf_geom_index_set_thresholds(index.handle, v[0]), ctx.handle, "set_thresholds")
            _lib.check(L.gf_geom_query_set_chain_mode(q, v[1]), ctx.handle, "set_chain_mode")
        rng_ = lambda: _lib.check(L.gf_geom_range_run(q, index.handle, bitmap.data_ptr(), counts.data_ptr()), ctx.handle, "range")  # noqa: E731
        knn = lambda: _lib.check(L.gf_geom_knn_enqueue(q, index.handle, a.k, C.c_void_p(rec.data_ptr())), ctx.handle, "knn")  # noqa: E731
        ref, infos = None, {}
        for v in variants:  # the check, and the warm-up
            vary(v)
            rng_()
            infos[v] = dict(range=info_of(q))
            knn()
            infos[v]["knn"] = info_of(q)
            got = (bitmap.cpu().numpy().copy(), counts.cpu().numpy().copy(), rec.cpu().numpy().tobytes())
            assert int(got[1][0]) == int(np.unpackbits(got[0].view(np.uint8)).sum()), "counts[0] is not the bitmap's count"
            ref = ref or got
            assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]) and got[2] == ref[2], \
                f"variant {v} selects other objects than {variants[0]} (r = {rc} cells)"
        tr, tk = ({v: [] for v in variants} for _ in range(2))
        for _ in range(a.reps):
            for v in variants:
                vary(v)  # (not timed: it takes the envelopes again)
                tr[v].append(timed(rng_))
                tk[v].append(timed(knn))
        for v in variants:
            out.append({"bench": "geompair", "window": "linestring" if a.lines else "polygon",
                        "query": "linestring" if a.query_lines else "polygon", "n": a.n, "vertices": a.vertices, "skew": a.skew,
                        "query_segments": a.segments, "k": a.k, "r_cells": rc, "wide_vertices": v[0], "plain": v[1],
                        "timed_runs": len(tr[v]), "selected": int(ref[1][0]),
                        "range_ms": round(statistics.median(tr[v]), 4), "range_min_max_ms": [round(min(tr[v]), 4), round(max(tr[v]), 4)],
                        "knn_ms": round(statistics.median(tk[v]), 4), "knn_min_max_ms": [round(min(tk[v]), 4), round(max(tk[v]), 4)],
                        "info": infos[v]})
        L.gf_geom_query_destroy(q)
    index.close()
    return out


if __name__ == "__main__":
    main()
