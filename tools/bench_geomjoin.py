"""The geometry-stream joins: ms per window of gf_geom_join_run / gf_geom_join_run_points, warm, on
device-resident windows prepared once.  Default shape: 1M regular 16-gons (a third of a cell across) joined
with 100k such 16-gons on the 500 x 500 Beijing grid at r = one cell, exact, sqrt metric.

  --lines          both geometry sides are linestrings (arcs of --vertices vertices)
  --query-points   the query side is a point window
  --skew F         a share F of the ordinary objects has 4,096 vertices instead
  --brute          also time brute mode (every pair through the rectangle pass) on the first --brute-nq queries,
                   beside the default on the same smaller query side
  --tile T         tile side (0 = the library's default); --long-tiles N likewise

The library has no other route that joins two geometry windows and the parent commit has none either, so there
is no "before": the comparison is the tile probe against brute.  Before anything is timed the tool checks that
the variants of one query side report the same pair count and replication count, and that a run with a buffer
returns the same triples as its twin (sorted).  A run is synchronous (it reads its counters on the way), so the
time is the host's wall clock around the call; per variant the median with [min, max] over --reps timed
runs after a warm-up, the variants alternating inside every visit.  A second, untimed visit with the library's
kernel timers on gives the split into binning / probe / exact kernels (events add overhead: the split is
not the wall clock).  Reads nothing outside the repository.  Appends one JSON line per variant to --out
(default profiles/geomjoin_bench.jsonl)."""
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
GRID_N = 500
CL = (BEIJING[1] - BEIJING[0]) / GRID_N
LONG_VERTICES = 4096
K_JOIN_PROBE, K_JOIN_BUCKET, K_GEOM = 5, 7, 19


def make_side(seed, n, vertices, skew, lines):
    """(ring_off or None, vert_off, vx, vy): n objects a third of a cell across, centres uniform over the box"""
    rng = np.random.default_rng(seed)
    cx = rng.uniform(BEIJING[0], BEIJING[1], n)
    cy = rng.uniform(BEIJING[2], BEIJING[3], n)
    m = np.full(n, max(vertices, 2 if lines else 3), np.int64)
    m[rng.random(n) < skew] = LONG_VERTICES
    nv = m if lines else m + 1                      # polygons repeat the first vertex
    vert_off = np.zeros(n + 1, np.int64)
    np.cumsum(nv, out=vert_off[1:])
    obj = np.repeat(np.arange(n), nv)
    j = np.arange(vert_off[-1]) - vert_off[obj]
    mm = m[obj]
    ang = 2.0 * np.pi * (j % mm) / mm * (0.75 if lines else 1.0)
    vx, vy = cx[obj] + CL / 6.0 * np.cos(ang), cy[obj] + CL / 6.0 * np.sin(ang)
    if not lines:                                   # closed bit for bit
        last = vert_off[1:] - 1
        vx[last], vy[last] = vx[vert_off[:-1]], vy[vert_off[:-1]]
    return (None if lines else np.arange(n + 1, dtype=np.int32)), vert_off.astype(np.int32), vx, vy


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--nq", type=int, default=100_000)
    ap.add_argument("--vertices", type=int, default=16)
    ap.add_argument("--lines", action="store_true")
    ap.add_argument("--query-points", action="store_true")
    ap.add_argument("--skew", type=float, default=0.0)
    ap.add_argument("--brute", action="store_true")
    ap.add_argument("--brute-nq", type=int, default=1000)
    ap.add_argument("--tile", type=int, default=0)
    ap.add_argument("--long-tiles", type=int, default=0)
    ap.add_argument("--r-cells", type=float, default=1.0)
    ap.add_argument("--approximate", action="store_true")
    ap.add_argument("--reps", type=int, default=24)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "geomjoin_bench.jsonl"))
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

    assert torch.cuda.is_available(), "bench_geomjoin needs a HIP device"
    L = _lib.lib()
    assert L.gf_build_is_product() == 1, L.gf_build_info().decode()
    assert a.reps >= 24, "at least 24 timed runs"
    kind = _lib.GEOM_LINESTRING if a.lines else _lib.GEOM_POLYGON
    grid = sf.UniformGrid(GRID_N, *BEIJING)
    win = sf.GeometryWindow.from_csr(kind, *make_side(500, a.n, a.vertices, a.skew, a.lines))
    index = sf.GeometryIndex(win, grid)
    ctx = index.ctx
    dev = win.vert_off.device
    r = a.r_cells * CL
    joiner = C.c_void_p()
    _lib.check(L.gf_geom_join_create(ctx.handle, C.byref(joiner)), ctx.handle, "gf_geom_join_create")

    def query_side(nq):
        if a.query_points:
            rng = np.random.default_rng(501)
            w = sf.PointWindow.from_numpy(rng.uniform(BEIJING[0], BEIJING[1], nq), rng.uniform(BEIJING[2], BEIJING[3], nq))
            return w, None
        w = sf.GeometryWindow.from_csr(kind, *make_side(501, nq, a.vertices, 0.0, a.lines))
        return w, sf.GeometryIndex(w, grid)

    def call(qw, qix, pairs, cap):
        n, m = C.c_int64(), C.c_int64()
        if qix is None:
            ps = qw.c_struct()
            st = L.gf_geom_join_run_points(joiner, index.handle, C.byref(grid.c_grid), C.byref(ps), r, int(a.approximate), 0,
                                           pairs, cap, C.byref(n), C.byref(m))
        else:
            st = L.gf_geom_join_run(joiner, index.handle, qix.handle, r, int(a.approximate), 0, 0, pairs, cap, C.byref(n), C.byref(m))
        if not (st == _lib.GF_ERR_CAPACITY and cap == 0):
            _lib.check(st, ctx.handle, "gf_geom_join_run")
        return n.value, m.value

    def info():
        v = [C.c_int64() for _ in range(6)]
        _lib.check(L.gf_geom_join_info(joiner, *(C.byref(c) for c in v)), ctx.handle, "gf_geom_join_info")
        return dict(zip(("candidates", "box_dropped", "tested", "wave_path", "long_objects", "long_queries"), (c.value for c in v)))

    out = []
    sides = [("default", a.nq, [("probe", 0)])]
    if a.brute:
        sides.append(("brute", a.brute_nq, [("probe", 0), ("brute", 1)]))
    for side, nq, variants in sides:
        qw, qix = query_side(nq)
        tune = lambda b: _lib.check(L.gf_geom_join_set_tuning(joiner, a.tile, a.long_tiles, b), ctx.handle, "set_tuning")  # noqa: E731
        ref, bufs, infos = None, {}, {}
        for name, b in variants:   # the check, and the warm-up
            tune(b)
            counts = call(qw, qix, None, 0)
            buf = torch.empty(3 * max(counts[0], 1), dtype=torch.int32, device=dev)
            assert call(qw, qix, buf.data_ptr(), counts[0]) == counts
            infos[name] = info()
            t = buf[: 3 * counts[0]].cpu().numpy().view(np.uint32).reshape(-1, 3)
            t = t[np.lexsort((t[:, 1], t[:, 0]))]
            ref = ref if ref is not None else (counts, t)
            assert counts == ref[0] and np.array_equal(t, ref[1]), f"variant {name} joins other pairs than {variants[0][0]}"
            bufs[name] = buf
        times = {name: [] for name, _ in variants}
        for _ in range(a.reps):
            for name, b in variants:
                tune(b)
                ctx.synchronize()
                t0 = time.perf_counter()
                call(qw, qix, bufs[name].data_ptr(), ref[0][0])
                times[name].append((time.perf_counter() - t0) * 1e3)
        split = {}
        ctx.set_timing((1 << K_JOIN_PROBE) | (1 << K_JOIN_BUCKET) | (1 << K_GEOM))
        for name, b in variants:
            tune(b)
            for k in (K_JOIN_BUCKET, K_JOIN_PROBE, K_GEOM):
                ctx.timing(k)   # (reads reset)
            for _ in range(3):
                call(qw, qix, bufs[name].data_ptr(), ref[0][0])
            split[name] = {lab: round(ctx.timing(k)[0] / 3, 4) for lab, k in (("bin_ms", K_JOIN_BUCKET), ("probe_ms", K_JOIN_PROBE),
                                                                              ("exact_ms", K_GEOM))}
        ctx.set_timing(0)
        for name, _ in variants:
            ts = times[name]
            out.append({"bench": "geomjoin", "sides": "linestring" if a.lines else "polygon",
                        "query": "point" if a.query_points else ("linestring" if a.lines else "polygon"), "n": a.n, "nq": nq,
                        "vertices": a.vertices, "skew": a.skew, "r_cells": a.r_cells, "approximate": bool(a.approximate),
                        "tile": a.tile, "long_tiles": a.long_tiles, "query_side": side, "variant": name, "timed_runs": len(ts),
                        "pairs": ref[0][0], "replicated": ref[0][1], "ms": round(statistics.median(ts), 3),
                        "min_max_ms": [round(min(ts), 3), round(max(ts), 3)], "kernels": split[name], "info": infos[name]})
        if qix is not None:
            qix.close()
    L.gf_geom_join_destroy(joiner)
    index.close()
    return out


if __name__ == "__main__":
    main()
