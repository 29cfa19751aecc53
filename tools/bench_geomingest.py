"""GeoJSON ingest of polygon / linestring streams (gf_geojson_parse_geoms): ms per call, warm, on
device-resident text (default 1M generated Feature records of 16-gons on the Beijing box).

  --n N          lines (default 1,000,000; --distinct of them are generated, the text repeats them)
  --vertices V   distinct vertices per object (polygons: + the closing one)
  --skew F       a share F of the objects has 4,096 vertices instead
  --lines        linestring streams
  --multi        Multi* geometries of two members (the second is validated and dropped)
  --host-n M     size of the host-route comparison (json.loads + Polygon(...) + from_polygons)

Before timing, the window of a 10,000-line prefix is checked against tests/geomingest_ref.py bit for
bit.  Timing: the exact-size call (capacities from one sizing call), --reps times after --warmup;
per call the device time between two events on the context stream and the host clock around the whole
synchronous call; median with [min, max]; the sizing call (zero capacities: index + pass A + scans)
is timed interleaved with it.  The split between the index, pass A, the scans and pass B comes from
a kernel trace run of its own: `rocprofv3 --kernel-trace --stats -- python tools/bench_geomingest.py
--n 200000 --reps 3`.
Appends one JSON line per configuration to --out (default profiles/geomingest_bench.jsonl)."""
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
POLYGON, LINESTRING = 1, 2


def make_lines(seed, n, vertices, skew, lines, multi):
    """n Feature records: {"key":i,"value":{"type":"Feature","geometry":{..},"properties":{"oid":..,"t":..}}}"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        m = LONG_VERTICES if rng.random() < skew else vertices
        cx, cy = rng.uniform(BEIJING[0], BEIJING[1]), rng.uniform(BEIJING[2], BEIJING[3])
        ang = 2.0 * math.pi * np.arange(m) / m * (0.75 if lines else 1.0)
        rad = 0.007 * (0.8 + 0.2 * rng.random(m))
        xs, ys = cx + rad * np.cos(ang), cy + rad * np.sin(ang)
        pos = [f"[{x!r},{y!r}]" for x, y in zip(xs.tolist(), ys.tolist())]
        if not lines:
            pos.append(pos[0])
        chain = "[" + ",".join(pos) + "]"
        if lines:
            t, c = ("MultiLineString", "[" + chain + "," + chain + "]") if multi else ("LineString", chain)
        else:
            t, c = ("MultiPolygon", "[[" + chain + "],[" + chain + "]]") if multi else ("Polygon", "[" + chain + "]")
        out.append(f'{{"key":{i},"value":{{"type":"Feature","geometry":{{"type":"{t}","coordinates":{c}}},'
                   f'"properties":{{"oid":"veh-{i % 5000}","t":{1600000000000 + i}}}}}}}'.encode())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--distinct", type=int, default=20_000)
    ap.add_argument("--vertices", type=int, default=16)
    ap.add_argument("--skew", type=float, default=0.0)
    ap.add_argument("--lines", action="store_true")
    ap.add_argument("--multi", action="store_true")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-n", type=int, default=20_000)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "geomingest_bench.jsonl"))
    args = ap.parse_args()

    import torch

    import spatialflink_amd as sf
    from spatialflink_amd import _lib
    from spatialflink_amd.spatialStreams import Deserialization as D, GfGeojsonSchema, device_text
    import geomingest_ref as R

    kind = LINESTRING if args.lines else POLYGON
    distinct = make_lines(5, min(args.distinct, args.n), args.vertices, args.skew, args.lines, args.multi)
    reps_of = (args.n + len(distinct) - 1) // len(distinct)
    all_lines = (distinct * reps_of)[:args.n]
    text = b"\n".join(all_lines) + b"\n"
    des = (D.GeoJSONToTSpatialLineString if args.lines else D.GeoJSONToTSpatialPolygon)(None, None, "t", "oid")

    # the check before any timing: a 10,000-line prefix against the restatement, bit for bit
    k = min(10_000, args.n)
    pre = b"\n".join(all_lines[:k]) + b"\n"
    objs, ids, ts, bl, _ = R.parse(pre, kind, prop_obj="oid", prop_ts="t")
    assert bl == -1
    w = des.parse(pre, device=args.device)
    ro, vo, vx, vy = R.csr(kind, objs)
    u = lambda a: np.ascontiguousarray(a, np.float64).view(np.uint64)  # noqa: E731
    assert np.array_equal(w.vert_off.cpu().numpy(), vo) and np.array_equal(u(w.vx.cpu().numpy()), u(vx))
    assert np.array_equal(u(w.vy.cpu().numpy()), u(vy)) and w.timeStampMillisec.cpu().tolist() == ts
    assert kind == LINESTRING or np.array_equal(w.ring_off.cpu().numpy(), ro)
    assert w.objid_strings() == [o.decode() for o in ids]

    dev = torch.device("cuda", args.device)
    t = device_text(text, args.device)
    ctx = _lib.context(args.device)
    sc = GfGeojsonSchema(b"oid", b"t", 0, 0, 0)
    cnt = [C.c_int64() for _ in range(4)]
    bk = C.c_int32()

    def call(out):
        return _lib.lib().gf_geojson_parse_geoms(ctx.handle, None, C.c_void_p(t.data_ptr()), len(text), C.byref(sc),
                                                 C.byref(out), C.byref(cnt[0]), C.byref(cnt[1]), C.byref(cnt[2]),
                                                 C.byref(cnt[3]), C.byref(bk))

    t0 = time.perf_counter()
    st = call(_lib.GfGeomsOut(kind, 0, 0, 0, None, None, None, None, None, None))
    sizing_ms = (time.perf_counter() - t0) * 1e3
    assert st == _lib.GF_ERR_CAPACITY, st
    n, r, v = (c.value for c in cnt[:3])
    ro_t = torch.empty(n + 1, dtype=torch.int32, device=dev) if kind == POLYGON else None
    vo_t = torch.empty((r if kind == POLYGON else n) + 1, dtype=torch.int32, device=dev)
    vx_t, vy_t = torch.empty(v, dtype=torch.float64, device=dev), torch.empty(v, dtype=torch.float64, device=dev)
    o_t, ts_t = torch.empty(n, dtype=torch.int64, device=dev), torch.empty(n, dtype=torch.int64, device=dev)
    out = _lib.GfGeomsOut(kind, n, r, v, ro_t.data_ptr() if ro_t is not None else None, vo_t.data_ptr(), vx_t.data_ptr(),
                          vy_t.data_ptr(), o_t.data_ptr(), ts_t.data_ptr())
    dev_ms, host_ms, size_ms = [], [], []
    for i in range(args.warmup + args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        t0 = time.perf_counter()
        _lib.check(call(out), ctx.handle, "gf_geojson_parse_geoms")
        h = (time.perf_counter() - t0) * 1e3
        b.record()
        b.synchronize()
        t0 = time.perf_counter()
        call(_lib.GfGeomsOut(kind, 0, 0, 0, None, None, None, None, None, None))  # interleaved: the sizing call
        s = (time.perf_counter() - t0) * 1e3
        if i >= args.warmup:
            dev_ms.append(a.elapsed_time(b))
            host_ms.append(h)
            size_ms.append(s)

    # the route this replaces, at a size that finishes in seconds: json.loads + Polygon(...) + from_polygons
    m = min(args.host_n, args.n)
    t0 = time.perf_counter()
    objs = []
    for ln in all_lines[:m]:
        g = json.loads(ln)["value"]["geometry"]
        c = g["coordinates"][0] if args.multi else g["coordinates"]
        objs.append(sf.LineString(c).coordinates if args.lines else sf.Polygon(c).rings)
    (sf.LineStringWindow.from_lines if args.lines else sf.PolygonWindow.from_polygons)(objs, device=args.device)
    torch.cuda.synchronize()
    host_route_ms = (time.perf_counter() - t0) * 1e3

    med = statistics.median
    row = {"tool": "bench_geomingest", "kind": "linestring" if args.lines else "polygon", "lines": n, "rings": r,
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
