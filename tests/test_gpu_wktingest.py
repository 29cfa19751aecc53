"""GPU: the WKT ingest of point, polygon and linestring streams (gf_wkt_parse_geoms, gf_wkt_parse_points,
k_wktingest.hip) against the restatement of tests/wktingest_ref.py, bit for bit: ring_off, vert_off,
vx / vy as uint64, ts and objID Strings -- at the parse blocks' edges, across scan and index segments, on a
line longer than a block's LDS staging, for ring order and Multi*, for the objID and time rules, for every
bad and unsupported line, for the capacity protocol, against the GeoJSON ingest of the same geometries, and
end to end through gf_geom_prepare, one range query and one kNN."""
import ctypes as C
import random

import numpy as np
import pytest

import spatialflink_amd as sf
from spatialflink_amd import _lib
from spatialflink_amd.spatialStreams import CSV_KINDS, Deserialization as D, GfWktSchema, device_text

import geomingest_ref as GR
import wktingest_gen as W
import wktingest_ref as R

T_LINES = W.T_LINES

pytestmark = pytest.mark.gpu

GEOMS = (W.POLYGON, W.LINESTRING)
KINDS = (W.POINT,) + GEOMS
DATE = "yyyy-MM-dd HH:mm:ss"
GRID = dict(uniformGridRows=100, minX=115.5, maxX=117.6, minY=39.6, maxY=41.1)


def _deser(kind, delim=None, df=0, grid=None, tz=0):
    if kind == W.POINT:
        return D.WKTToSpatial(grid) if delim is None else D.WKTToTSpatial(grid, DATE if df else None, delim)
    if delim is None:
        return (D.WKTToSpatialPolygon if kind == W.POLYGON else D.WKTToSpatialLineString)(grid)
    cls = D.WKTToTSpatialPolygon if kind == W.POLYGON else D.WKTToTSpatialLineString
    return cls(grid, DATE if df else None, delim, tz)


def _ref(text, kind, delim=None, df=0, tz=0):
    return R.parse(text, kind, delimiter=delim.encode() if delim else None, date_fmt=df, tz_off_min=tz)


def _u64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _assert_window(w, kind, objs, ids, ts, what="", grid=None):
    want = [None if o is None else o.decode("utf-8", "surrogateescape") for o in ids]
    assert w.objid_strings() == want, what
    assert w.timeStampMillisec.cpu().tolist() == list(ts), what
    if kind == W.POINT:
        assert w.n == len(objs), what
        assert np.array_equal(_u64(w.x.cpu().numpy()), _u64([p[0] for p in objs])), what
        assert np.array_equal(_u64(w.y.cpu().numpy()), _u64([p[1] for p in objs])), what
        if grid is not None:
            cells = [grid.cellOf(*p) for p in objs]
            assert w.extra["cx"].cpu().tolist() == [c[0] for c in cells] and w.extra["cy"].cpu().tolist() == [c[1] for c in cells]
        return
    ro, vo, vx, vy = GR.csr(kind, objs)
    assert w.nobj == len(objs) and w.kind == kind, what
    if kind == W.POLYGON:
        assert np.array_equal(w.ring_off.cpu().numpy(), ro), what
    else:
        assert w.ring_off is None
    assert np.array_equal(w.vert_off.cpu().numpy(), vo), what
    assert np.array_equal(_u64(w.vx.cpu().numpy()), _u64(vx)), what
    assert np.array_equal(_u64(w.vy.cpu().numpy()), _u64(vy)), what


def _parity(text, kind, gpu, delim=None, df=0, what="", grid=None, tz=0):
    objs, ids, ts, bl, bk = _ref(text, kind, delim, df, tz)
    assert bl == -1, (bl, bk)  # the generator stays inside the contract
    w = _deser(kind, delim, df, grid, tz).parse(text, device=gpu.index)
    _assert_window(w, kind, objs, ids, ts, what, grid)
    return w


# 64: the geometry passes' block (one wave); 192: the point kernel's block
@pytest.mark.parametrize("n", [1, 63, 64, 65, 191, 192, 193, 385])
@pytest.mark.parametrize("kind", KINDS)
def test_parity_at_the_block_edges(kind, n, gpu):
    grid = sf.UniformGrid(**GRID) if kind == W.POINT else None
    _parity(W.text_of(W.corpus(kind, n, 100 + n, ",", True)), kind, gpu, ",", 1, grid=grid)


@pytest.mark.parametrize("delim,df", [(None, 0), (",", 1), (";", 0), ("\t", 1)])
@pytest.mark.parametrize("kind", KINDS)
def test_parity_maps_crlf_and_final_newline(kind, delim, df, gpu):
    lines = W.corpus(kind, 193, 7 + df + (delim is not None), delim, bool(df))
    _parity(W.text_of(lines), kind, gpu, delim, df, tz=540)
    _parity(W.text_of(lines, crlf=True), kind, gpu, delim, df, "crlf")
    _parity(W.text_of(lines, final_newline=False), kind, gpu, delim, df, "no final newline")
    _parity(W.text_of(lines, crlf=True, final_newline=False), kind, gpu, delim, df, "crlf, no final newline")


@pytest.mark.parametrize("kind", KINDS)
def test_parity_across_index_and_scan_segments(kind, gpu):
    """1,500 compact lines, the text past several 64 KB index segments (points: past one; their lines are
    ~45 bytes, more than one per 32 index bytes is forced below) and the per-line counts past one scan block"""
    lines = W.corpus(kind, 1500, 31, ";", True, ws=0.0, small=kind == W.POLYGON, compact=True)
    text = W.text_of(lines)
    assert len(text) > (4 if kind != W.POINT else 1) * 65536
    _parity(text, kind, gpu, ";", 1)
    short = [b"POINT(1 2)", b"LINESTRING(0 0,1 1)"][kind == W.LINESTRING]
    if kind != W.POLYGON:  # lines shorter than 32 bytes: the index is regrown and the stage re-run
        _parity(W.text_of([short] * 700), kind, gpu)


@pytest.mark.parametrize("kind", GEOMS)
def test_a_line_longer_than_the_lds_staging(kind, gpu):
    """a 4,097-position ring / chain (~100 KB of text): alone, and between short lines"""
    big = W.gen_line(random.Random(3), kind, 0, ",", True, big=True, multi=False, nrings=1)[0]
    assert len(big) > 65536
    w = _parity(W.text_of([big]), kind, gpu, ",", 1, what="alone")
    assert w.vx.numel() == 4097
    lines = W.corpus(kind, 150, 9, ",", True, big_every=50)
    assert sum(len(ln) > 65536 for ln in lines) == 3
    _parity(W.text_of(lines), kind, gpu, ",", 1, what="between short lines")


def test_ring_order_and_multi(gpu):
    sq, hole, hole2 = "(0 0, 4 0, 4 4, 0 4, 0 0)", "(1 1, 2 1, 2 2, 1 1)", "(2 2, 3 2, 3 3, 2 2)"
    far, tiny = "((9 9, 19 9, 19 19, 9 9))", "(1 1, 1.5 1, 1.5 1.5, 1 1)"
    lines = [
        f"POLYGON ({hole}, {sq})",                            # the hole first: shell first
        f"POLYGON ({sq}, {hole}, {hole2})",                   # equal areas keep input order
        f"POLYGON ({sq}, {hole}, {tiny}, {hole2})",           # ... an equal ring inserted in front
        f"MULTIPOLYGON (({sq}, {hole}), {far}, {far})",       # the first polygon only
        W.SAMPLE_POLYGON.decode(),                            # the reference's own sample record
    ]
    text = W.text_of([ln.encode() for ln in lines])
    w = _parity(text, W.POLYGON, gpu)
    f = lambda s: [tuple(float(v) for v in p.split()) for p in s.strip("()").split(",")]  # noqa: E731
    objs = R.parse(text, W.POLYGON)[0]
    assert objs[0] == [f(sq), f(hole)] and objs[1] == [f(sq), f(hole), f(hole2)]
    assert objs[2] == [f(sq), f(hole2), f(hole), f(tiny)] and objs[3] == [f(sq), f(hole)]
    assert w.ring_off.cpu().tolist() == [0, 2, 5, 9, 11, 12] and int(w.vx.numel()) == 9 + 13 + 17 + 9 + 9
    ls = [b"MULTILINESTRING ((0 0, 1 1, 2 0), (5 5, 6 6), (7 7, 8 8))", b"LINESTRING (3 3, 4 4)"]
    w = _parity(W.text_of(ls), W.LINESTRING, gpu)
    assert w.vert_off.cpu().tolist() == [0, 3, 5]


def test_objid_and_time_rules(gpu):
    """objID absent because field 0 is the tag; the POLYGON objID dropped at ts 0 but kept for MULTIPOLYGON
    and linestrings; the date from the last field that parses; date_format 0; dictionary and numeric objIDs"""
    for kind, ln, d, df in T_LINES:
        r, k = R.wkt_line(ln, kind, delimiter=d.encode(), date_fmt=df, tz_off_min=-300)
        if k:
            with pytest.raises(ValueError) as e:
                _deser(kind, d, df, tz=-300).parse(ln, device=gpu.index)
            assert str(e.value) == f"line 0: {CSV_KINDS[k]}"
        else:
            _parity(ln + b"\n", kind, gpu, d, df, what=ln, tz=-300)
    # all of them that share a schema in one text: several dictionary Strings, some repeated
    lines = [ln for kind, ln, d, df in T_LINES if (kind, d, df) == (W.POLYGON, ",", 1)] * 3
    w = _parity(W.text_of(lines), W.POLYGON, gpu, ",", 1)
    assert w.objid_strings()[0] == "7" and int(w.objID[0]) == 7  # a canonical decimal is its value


def _raises_at(kind, lines, at, want, gpu):
    with pytest.raises(ValueError) as e:
        _deser(kind).parse(W.text_of(lines), device=gpu.index)
    assert str(e.value) == f"line {at}: {CSV_KINDS[want]}", (str(e.value), at, want, lines[at][:200])


@pytest.mark.parametrize("kind", KINDS)
def test_bad_and_unsupported_lines_fail_at_their_line_with_their_kind(kind, gpu):
    good = W.corpus(kind, 130, 17, small=True)
    cases = [(ln, k) for sk, ln, k in W.BAD if sk == kind] + [(ln, R.UNSUPPORTED) for sk, ln in W.UNSUPPORTED if sk == kind]
    cases.append((b"", R.EMPTY))
    for ln, want in cases:
        assert R.wkt_line(ln, kind)[1] == want
        _raises_at(kind, [ln], 0, want, gpu)
        lines = list(good)
        lines[70] = ln
        _raises_at(kind, lines, 70, want, gpu)


def test_the_earlier_of_two_bad_lines_is_reported(gpu):
    good = W.corpus(W.POLYGON, 130, 19, small=True)
    unclosed = b"POLYGON ((0 0, 4 0, 4 4, 0 4, 0 1))"   # found by pass B
    short = b"POLYGON ((0 0, 4 0, 0 0))"                # found by pass A
    number = b"POLYGON ((1.2.3 0, 4 0, 4 4, 0 0))"
    for (i, a, ka), (j, b, kb) in (((50, unclosed, 3), (100, number, 1)), ((50, number, 1), (100, unclosed, 3)),
                                   ((63, unclosed, 3), (64, unclosed, 3)), ((10, short, 3), (129, number, 1)),
                                   ((0, unclosed, 3), (1, number, 1))):
        lines = list(good)
        lines[i], lines[j] = a, b
        _raises_at(W.POLYGON, lines, i, ka, gpu)


def _call(gpu, text, kind, caps, arrays=True, schema=None):
    """the C entry point with capacities (obj, ring, vert) -> (status, counts, tensors)"""
    import torch

    t = device_text(text, gpu.index) if text else None
    dev = torch.device("cuda", gpu.index)
    ctx = _lib.context(gpu.index)
    oc, rc, vc = caps
    poly = kind == W.POLYGON
    mk = lambda n, dt: torch.full((n,), -7, dtype=dt, device=dev) if arrays else None  # noqa: E731
    ro, vo = (mk(oc + 1, torch.int32) if poly else None), mk((rc if poly else oc) + 1, torch.int32)
    vx, vy, o, ts = mk(vc, torch.float64), mk(vc, torch.float64), mk(oc, torch.int64), mk(oc, torch.int64)
    p = lambda a: a.data_ptr() if a is not None and a.numel() else None  # noqa: E731
    out = _lib.GfGeomsOut(kind, oc, rc, vc, p(ro), p(vo), p(vx), p(vy), p(o), p(ts))
    sc = schema or GfWktSchema(b",", b"\0\0\0", 1, 0)
    n = [C.c_int64(-1) for _ in range(4)]
    bk = C.c_int32(-1)
    st = _lib.lib().gf_wkt_parse_geoms(ctx.handle, None, C.c_void_p(t.data_ptr()) if t is not None else None,
                                       len(text), C.byref(sc), C.byref(out), C.byref(n[0]), C.byref(n[1]),
                                       C.byref(n[2]), C.byref(n[3]), C.byref(bk))
    return st, tuple(v.value for v in n[:3]), (ro, vo, vx, vy, o, ts)


@pytest.mark.parametrize("kind", GEOMS)
def test_capacities(kind, gpu):
    text = W.text_of(W.corpus(kind, 130, 23, ",", True))
    objs, ids, ts, _, _ = _ref(text, kind, ",", 1)
    ro, vo, vx, vy = GR.csr(kind, objs)
    exact = (len(objs), len(vo) - 1 if kind == W.POLYGON else 0, len(vx))
    st, counts, _ = _call(gpu, text, kind, (0, 0, 0), arrays=False)  # the sizing call
    assert st == _lib.GF_ERR_CAPACITY and counts == exact
    for k in range(3):
        if kind == W.LINESTRING and k == 1:
            continue
        caps = tuple(c - (i == k) for i, c in enumerate(exact))
        st, counts, _ = _call(gpu, text, kind, caps)
        assert st == _lib.GF_ERR_CAPACITY and counts == exact, (k, st, counts)
    st, counts, (gro, gvo, gvx, gvy, go, gts) = _call(gpu, text, kind, exact)
    assert st == _lib.GF_OK and counts == exact
    if kind == W.POLYGON:
        assert np.array_equal(gro.cpu().numpy(), ro)
    assert np.array_equal(gvo.cpu().numpy(), vo) and np.array_equal(_u64(gvx.cpu().numpy()), _u64(vx))
    assert np.array_equal(_u64(gvy.cpu().numpy()), _u64(vy)) and gts.cpu().tolist() == list(ts)
    # larger capacities: nothing past the counts is written
    big = tuple(c + 5 for c in exact)
    st, counts, (gro, gvo, gvx, gvy, go, gts) = _call(gpu, text, kind, big)
    assert st == _lib.GF_OK and counts == exact
    assert gvx.cpu().tolist()[-5:] == [-7.0] * 5 and gts.cpu().tolist()[-5:] == [-7] * 5
    assert gvo.cpu().tolist()[len(vo):] == [-7] * 5
    # empty text: an empty, valid window
    st, counts, (gro, gvo, *_rest) = _call(gpu, b"", kind, (4, 4, 4))
    assert st == _lib.GF_OK and counts == (0, 0, 0) and gvo.cpu().tolist()[0] == 0
    assert kind == W.LINESTRING or gro.cpu().tolist()[0] == 0
    st, counts, _ = _call(gpu, b"", kind, (0, 0, 0), arrays=False)
    assert st == _lib.GF_OK and counts == (0, 0, 0)
    w = _deser(kind).parse(b"", device=gpu.index)
    assert w.nobj == 0 and w.vert_off.cpu().tolist() == [0]
    # argument errors
    st, _, _ = _call(gpu, text, kind, (5, 5, 5), arrays=False)
    assert st == _lib.GF_ERR_ARG
    st, _, _ = _call(gpu, text, 3, (0, 0, 0), arrays=False)
    assert st == _lib.GF_ERR_ARG
    st, _, _ = _call(gpu, text, kind, (0, 0, 0), arrays=False, schema=GfWktSchema(b",", b"\0\0\0", 2, 0))
    assert st == _lib.GF_ERR_ARG
    st, _, _ = _call(gpu, text, kind, (0, 0, 0), arrays=False, schema=GfWktSchema(b'"', b"\0\0\0", 1, 0))
    assert st == _lib.GF_ERR_ARG  # '"' is removed before the split: never a delimiter


def test_point_capacity(gpu):
    import torch

    lines = W.corpus(W.POINT, 200, 3)
    text = W.text_of(lines)
    objs = _ref(text, W.POINT)[0]
    t = device_text(text, gpu.index)
    dev = torch.device("cuda", gpu.index)
    ctx = _lib.context(gpu.index)
    for cap in (0, 199, 200, 205):
        a = [torch.full((max(cap, 1),), -7, dtype=dt, device=dev) for dt in (torch.float64, torch.float64, torch.int64, torch.int64)]
        n, bl, bk = C.c_int64(-1), C.c_int64(-1), C.c_int32(-1)
        st = _lib.lib().gf_wkt_parse_points(ctx.handle, C.c_void_p(t.data_ptr()), len(text), None, *(x.data_ptr() for x in a),
                                            None, None, cap, C.byref(n), C.byref(bl), C.byref(bk))
        assert n.value == 200 and st == (_lib.GF_OK if cap >= 200 else _lib.GF_ERR_CAPACITY)
        if cap < 200:
            assert a[0].cpu().tolist() == [-7.0] * max(cap, 1)  # nothing is written
        else:
            assert np.array_equal(_u64(a[0].cpu().numpy()[:200]), _u64([p[0] for p in objs]))
            assert a[2].cpu().tolist()[:200] == [_lib.OBJID_NULL] * 200 and a[3].cpu().tolist()[:200] == [0] * 200
            assert a[1].cpu().tolist()[200:] == [-7.0] * (cap - 200)
    assert D.WKTToSpatial(None).parse(b"", device=gpu.index).n == 0


@pytest.mark.parametrize("kind", GEOMS)
def test_same_device_window_as_the_geojson_ingest(kind, gpu):
    rows = W.corpus(kind, 300, 13, json_safe=True, with_geoms=True, big_every=150)
    w = _deser(kind).parse(W.text_of([ln for ln, _ in rows]), device=gpu.index)
    cls = D.GeoJSONToSpatialPolygon if kind == W.POLYGON else D.GeoJSONToSpatialLineString
    g = cls(None, value_lines=True).parse(W.text_of([W.geojson_twin(kind, m, multi) for _, (m, multi) in rows]), device=gpu.index)
    assert w.nobj == g.nobj == 300
    if kind == W.POLYGON:
        assert np.array_equal(w.ring_off.cpu().numpy(), g.ring_off.cpu().numpy())
    assert np.array_equal(w.vert_off.cpu().numpy(), g.vert_off.cpu().numpy())
    assert np.array_equal(_u64(w.vx.cpu().numpy()), _u64(g.vx.cpu().numpy()))
    assert np.array_equal(_u64(w.vy.cpu().numpy()), _u64(g.vy.cpu().numpy()))
    assert np.array_equal(w.objID.cpu().numpy(), g.objID.cpu().numpy()) and not w.timeStampMillisec.any()


@pytest.mark.parametrize("kind", GEOMS)
def test_end_to_end_prepare_range_and_knn(kind, gpu):
    """800 ingested objects -> gf_geom_prepare -> one range query and one kNN (k = 8) on the 100 x 100 Beijing
    grid: as the same queries on the window built from the restatement's rings on the host"""
    text = W.text_of(W.corpus(kind, 800, 41, ";", True))
    objs, ids, ts, bl, _ = _ref(text, kind, ";", 1)
    assert bl == -1
    w = _deser(kind, ";", 1).parse(text, device=gpu.index)
    keys = w.objID.cpu().numpy()
    if kind == W.POLYGON:
        h = sf.PolygonWindow.from_polygons(objs, keys, ts, device=gpu.index)
        rq, kq = sf.PolygonPointRangeQuery, sf.PolygonPointKNNQuery
    else:
        h = sf.LineStringWindow.from_lines(objs, keys, ts, device=gpu.index)
        rq, kq = sf.LineStringPointRangeQuery, sf.LineStringPointKNNQuery
    grid = sf.UniformGrid(**GRID)
    conf = sf.QueryConfiguration(sf.QueryType.WindowBased)
    qs = [sf.Point("q", 116.4, 40.2), sf.Point("q", 116.9, 39.9)]
    r = 10.0 * (GRID["maxX"] - GRID["minX"]) / 100
    got = []
    for win in (w, h):
        ix = sf.GeometryIndex(win, grid)
        assert ix.info()["invalid"] == 0 and ix.info()["nobj"] == 800
        res = rq(conf, grid).run(win, qs, r, index=ix)
        kn = kq(conf, grid).run(win, qs[0], r, 8, index=ix)
        got.append((res.indices().astype(np.int64), kn.objID, kn.idx, _u64(kn.dist)))
        ix.close()
    assert len(got[0][0]) > 0 and len(got[0][1]) == 8
    for a, b in zip(got[0], got[1]):
        assert np.array_equal(np.asarray(a), np.asarray(b))
