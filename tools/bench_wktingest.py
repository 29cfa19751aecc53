"""WKT ingest of point / polygon / linestring streams (gf_wkt_parse_geoms, gf_wkt_parse_points): ms per
call, warm, on device-resident text (default 1M generated lines "objID;POLYGON ((..));date" of 16-gons
on the Beijing box -- the geometries of tools/bench_geomingest.py, vertex for vertex).

  --n N          lines (default 1,000,000; --distinct of them are generated, the text repeats them)
  --vertices V   distinct vertices per object (polygons: + the closing one)
  --skew F       a share F of the objects has 4,096 vertices instead
  --lines        linestring streams
  --multi        MULTI* geometries of two members (the second is validated and dropped)
  --points       the point stream (gf_wkt_parse_points): "objID;POINT (x y);date"
  --host-n M     size of the host-route comparison (a Python WKT split + Polygon(...) + from_polygons)

Before timing, the window of a 10,000-line prefix is checked against tests/wktingest_ref.py bit for bit.
Timing, as tools/bench_geomingest.py: the exact-size call (capacities from one sizing call), --reps times
after --warmup; per call the device time between two events on torch's current stream around the call (the call is
synchronous: it waits for the context stream before it returns, so the pair brackets all its device work) and
the host clock around the whole call; median with [min, max]; the sizing call (zero capacities: index +
pass A + scans) is timed interleaved with it.  The split between the index, pass A, the scans and pass B
comes from a kernel trace run of its own: `rocprofv3 --kernel-trace --stats -- python
tools/bench_wktingest.py --n 200000 --reps 3`.
Appends one JSON line per configuration to --out (default profiles/wktingest_bench.jsonl)."""
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
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]

BEIJING = (115.5, 117.6, 39.6, 41.1)
LONG_VERTICES = 4096
POINT, POLYGON, LINESTRING = 0, 1, 2


def make_lines(seed, n, vertices, skew, lines, multi, points):
    """n lines "veh-k;<WKT>;yyyy-MM-dd HH:mm:ss" (the random draws of tools/bench_geomingest.py make_lines)"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        m = LONG_VERTICES if rng.random() < skew else vertices
        cx, cy = rng.uniform(BEIJING[0], BEIJING[1]), rng.uniform(BEIJING[2], BEIJING[3])
        date = f"2023-{1 + i % 12:02d}-{1 + i % 28:02d} {i % 24:02d}:{i % 60:02d}:{i % 59:02d}"
        if points:
            out.append(f"veh-{i % 5000};POINT ({cx!r} {cy!r});{date}".encode())
            continue
        ang = 2.0 * math.pi * np.arange(m) / m * (0.75 if lines else 1.0)
        rad = 0.007 * (0.8 + 0.2 * rng.random(m))
        xs, ys = cx + rad * np.cos(ang), cy + rad * np.sin(ang)
        pos = [f"{x!r} {y!r}" for x, y in zip(xs.tolist(), ys.tolist())]
        if not lines:
            pos.append(pos[0])
        chain = "(" + ", ".join(pos) + ")"
        if lines:
            g = "MULTILINESTRING (" + chain + ", " + chain + ")" if multi else "LINESTRING " + chain
        else:
            g = "MULTIPOLYGON ((" + chain + "), (" + chain + "))" if multi else "POLYGON (" + chain + ")"
        out.append(f"veh-{i % 5000};{g};{date}".encode())
    return out


def host_object(line):
    """the host route's per-line parse: the first member's positions"""
    body = line.split(b";")[1].decode()
    body = body[body.index("("):]
    first = body.lstrip("(").split(")")[0]
    pts = [tuple(float(v) for v in p.split()) for p in first.split(",")]
    return pts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--distinct", type=int, default=20_000)
    ap.add_argument("--vertices", type=int, default=16)
    ap.add_argument("--skew", type=float, default=0.0)
    ap.add_argument("--lines", action="store_true")
    ap.add_argument("--multi", action="store_true")
    ap.add_argument("--points", action="store_true")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-n", type=int, default=20_000)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wktingest_bench.jsonl"))
    args = ap.parse_args()

    import torch

    import spatialflink_amd as sf
    from spatialflink_amd import _lib
    from spatialflink_amd.spatialStreams import Deserialization as D, GfWktSchema, device_text
    import geomingest_ref as GR
    import wktingest_ref as R

    DATE = "yyyy-MM-dd HH:mm:ss"
    kind = POINT if args.points else LINESTRING if args.lines else POLYGON
    distinct = make_lines(5, min(args.distinct, args.n), args.vertices, args.skew, args.lines, args.multi, args.points)
    reps_of = (args.n + len(distinct) - 1) // len(distinct)
    all_lines = (distinct * reps_of)[:args.n]
    text = b"\n".join(all_lines) + b"\n"
    des = {POINT: D.WKTToTSpatial, POLYGON: D.WKTToTSpatialPolygon, LINESTRING: D.WKTToTSpatialLineString}[kind](None, DATE, ";")

    # the check before any timing: a 10,000-line prefix against the restatement, bit for bit
    k = min(10_000, args.n)
    pre = b"\n".join(all_lines[:k]) + b"\n"
    objs, ids, ts, bl, _ = R.parse(pre, kind, delimiter=b";", date_fmt=1)
    assert bl == -1
    w = des.parse(pre, device=args.device)
    u = lambda a: np.ascontiguousarray(a, np.float64).view(np.uint64)  # noqa: E731
    assert w.timeStampMillisec.cpu().tolist() == ts
    assert w.objid_strings() == [None if o is None else o.decode() for o in ids]
    if args.points:
        assert np.array_equal(u(w.x.cpu().numpy()), u([p[0] for p in objs]))
        assert np.array_equal(u(w.y.cpu().numpy()), u([p[1] for p in objs]))
    else:
        ro, vo, vx, vy = GR.csr(kind, objs)
        assert np.array_equal(w.vert_off.cpu().numpy(), vo) and np.array_equal(u(w.vx.cpu().numpy()), u(vx))
        assert np.array_equal(u(w.vy.cpu().numpy()), u(vy))
        assert kind == LINESTRING or np.array_equal(w.ring_off.cpu().numpy(), ro)

    dev = torch.device("cuda", args.device)
    t = device_text(text, args.device)
    ctx = _lib.context(args.device)
    sc = GfWktSchema(b";", b"\0\0\0", 1, 0)
    cnt = [C.c_int64() for _ in range(4)]
    bk = C.c_int32()
    E = lambda m, dt: torch.empty(m, dtype=dt, device=dev)  # noqa: E731

    if args.points:
        cap = args.n
        px, py, po, pt = E(cap, torch.float64), E(cap, torch.float64), E(cap, torch.int64), E(cap, torch.int64)

        def call(out):
            return _lib.lib().gf_wkt_parse_points(ctx.handle, C.c_void_p(t.data_ptr()), len(text), None, px.data_ptr(),
                                                  py.data_ptr(), po.data_ptr(), pt.data_ptr(), None, None,
                                                  cap if out else 0, C.byref(cnt[0]), C.byref(cnt[3]), C.byref(bk))

        zero, sizing_status = False, _lib.GF_ERR_CAPACITY
    else:
        def call(out):
            return _lib.lib().gf_wkt_parse_geoms(ctx.handle, None, C.c_void_p(t.data_ptr()), len(text), C.byref(sc),
                                                 C.byref(out), C.byref(cnt[0]), C.byref(cnt[1]), C.byref(cnt[2]),
                                                 C.byref(cnt[3]), C.byref(bk))

        zero, sizing_status = _lib.GfGeomsOut(kind, 0, 0, 0, None, None, None, None, None, None), _lib.GF_ERR_CAPACITY

    t0 = time.perf_counter()
    st = call(zero)
    sizing_ms = (time.perf_counter() - t0) * 1e3
    assert st == sizing_status, st
    n, r, v = (c.value for c in cnt[:3])
    if args.points:
        out, r, v = True, 0, n
    else:
        ro_t = E(n + 1, torch.int32) if kind == POLYGON else None
        vo_t = E((r if kind == POLYGON else n) + 1, torch.int32)
        vx_t, vy_t, o_t, ts_t = E(v, torch.float64), E(v, torch.float64), E(n, torch.int64), E(n, torch.int64)
        out = _lib.GfGeomsOut(kind, n, r, v, ro_t.data_ptr() if ro_t is not None else None, vo_t.data_ptr(),
                              vx_t.data_ptr(), vy_t.data_ptr(), o_t.data_ptr(), ts_t.data_ptr())
    dev_ms, host_ms, size_ms = [], [], []
    for i in range(args.warmup + args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        t0 = time.perf_counter()
        _lib.check(call(out), ctx.handle, "gf_wkt_parse")
        h = (time.perf_counter() - t0) * 1e3
        b.record()
        b.synchronize()
        t0 = time.perf_counter()
        call(zero)  # interleaved: the sizing call
        s = (time.perf_counter() - t0) * 1e3
        if i >= args.warmup:
            dev_ms.append(a.elapsed_time(b))
            host_ms.append(h)
            size_ms.append(s)

    # the route this replaces, at a size that finishes in seconds: a Python split + Polygon(...) + from_polygons
    m = min(args.host_n, args.n)
    t0 = time.perf_counter()
    if args.points:
        pts = [host_object(ln)[0] for ln in all_lines[:m]]
        sf.PointWindow.from_numpy(np.array([p[0] for p in pts]), np.array([p[1] for p in pts]), device=args.device)
    else:
        objs = []
        for ln in all_lines[:m]:
            c = host_object(ln)
            objs.append(sf.LineString(c).coordinates if args.lines else sf.Polygon([c]).rings)
        (sf.LineStringWindow.from_lines if args.lines else sf.PolygonWindow.from_polygons)(objs, device=args.device)
    torch.cuda.synchronize()
    host_route_ms = (time.perf_counter() - t0) * 1e3

    med = statistics.median
    row = {"tool": "bench_wktingest", "kind": ["point", "polygon", "linestring"][kind], "lines": n, "rings": r,
           "vertices": v, "text_bytes": len(text), "mean_line": len(text) / n, "vertices_per_object": args.vertices,
           "skew": args.skew, "multi": args.multi, "distinct_lines": len(distinct), "reps": args.reps,
           "call_ms": [med(host_ms), min(host_ms), max(host_ms)], "device_ms": [med(dev_ms), min(dev_ms), max(dev_ms)],
           "sizing_call_ms": [med(size_ms), min(size_ms), max(size_ms)], "first_sizing_call_ms": sizing_ms,
           "text_gbs": len(text) / med(host_ms) / 1e6, "vertices_per_s": v / med(host_ms) * 1e3,
           "lines_per_s": n / med(host_ms) * 1e3,
           "host_route": {"lines": m, "ms": host_route_ms, "lines_per_s": m / host_route_ms * 1e3}}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(row) + "\n")
    print(json.dumps(row))


if __name__ == "__main__":
    main()
