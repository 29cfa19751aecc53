"""GPU: the GeoJSON ingest of polygon and linestring streams (gf_geojson_parse_geoms, k_geomingest.hip)
against the restatement of tests/geomingest_ref.py, bit for bit: ring_off, vert_off, vx / vy as uint64,
ts and objID Strings -- at the parse block's edges, across scan and index segments, on a line longer than
a block's LDS staging, for ring order and Multi*, for every bad and unsupported line, for the capacity
protocol, and end to end through gf_geom_prepare, one range query and one kNN."""
import ctypes as C

import numpy as np
import pytest

import spatialflink_amd as sf
from spatialflink_amd import _lib
from spatialflink_amd.spatialStreams import Deserialization as D, GfGeojsonSchema, device_text

import geomingest_gen as G
import geomingest_ref as R

pytestmark = pytest.mark.gpu

KINDS = (G.POLYGON, G.LINESTRING)
DATE = "yyyy-MM-dd HH:mm:ss"


def _deser(kind, vl=False, df=0):
    cls = D.GeoJSONToTSpatialPolygon if kind == G.POLYGON else D.GeoJSONToTSpatialLineString
    return cls(None, DATE if df else None, G.PROP_TS, G.PROP_OBJ, 0, vl)


def _ref(text, kind, vl=False, df=0):
    return R.parse(text, kind, prop_obj=G.PROP_OBJ, prop_ts=G.PROP_TS, date_fmt=df, value_lines=vl)


def _u64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _assert_window(w, kind, objs, ids, ts, what=""):
    ro, vo, vx, vy = R.csr(kind, objs)
    assert w.nobj == len(objs) and w.kind == kind, what
    if kind == G.POLYGON:
        assert np.array_equal(w.ring_off.cpu().numpy(), ro), what
    else:
        assert w.ring_off is None
    assert np.array_equal(w.vert_off.cpu().numpy(), vo), what
    assert np.array_equal(_u64(w.vx.cpu().numpy()), _u64(vx)), what
    assert np.array_equal(_u64(w.vy.cpu().numpy()), _u64(vy)), what
    assert w.timeStampMillisec.cpu().tolist() == list(ts), what
    want = [None if o is None else o.decode("utf-8", "surrogateescape") for o in ids]
    assert w.objid_strings() == want, what


def _parity(text, kind, gpu, vl=False, df=0, what=""):
    objs, ids, ts, bl, bk = _ref(text, kind, vl, df)
    assert bl == -1, (bl, bk)  # the generator stays inside the contract
    w = _deser(kind, vl, df).parse(text, device=gpu.index)
    _assert_window(w, kind, objs, ids, ts, what)
    return w


# 64: the parse block (one wave); 192: the point ingest's block
@pytest.mark.parametrize("n", [1, 63, 64, 65, 191, 192, 193, 385])
@pytest.mark.parametrize("kind", KINDS)
def test_parity_at_the_block_edges(kind, n, gpu):
    _parity(G.text_of(G.corpus(kind, n, 100 + n)), kind, gpu)


@pytest.mark.parametrize("vl,df", [(False, 0), (False, 1), (True, 0), (True, 1)])
@pytest.mark.parametrize("kind", KINDS)
def test_parity_value_lines_and_date_formats(kind, vl, df, gpu):
    lines = G.corpus(kind, 193, 7 + 2 * vl + df, vl, df)
    _parity(G.text_of(lines), kind, gpu, vl, df)
    _parity(G.text_of(lines, crlf=True), kind, gpu, vl, df, "crlf")
    _parity(G.text_of(lines, final_newline=False), kind, gpu, vl, df, "no final newline")
    _parity(G.text_of(lines, crlf=True, final_newline=False), kind, gpu, vl, df, "crlf, no final newline")


@pytest.mark.parametrize("kind", KINDS)
def test_parity_across_index_and_scan_segments(kind, gpu):
    """compact lines of a few hundred bytes, the text past several 64 KB index segments and the
    per-line counts past one scan block"""
    lines = G.corpus(kind, 1500, 31, ws=0.0, small=True)
    text = G.text_of(lines)
    assert len(text) > 4 * 65536 and len(text) / len(lines) < 600
    _parity(text, kind, gpu)


def test_the_non_t_deserializers_read_no_property(gpu):
    for kind, cls in ((G.POLYGON, D.GeoJSONToSpatialPolygon), (G.LINESTRING, D.GeoJSONToSpatialLineString)):
        text = G.text_of(G.corpus(kind, 70, 5))
        objs, ids, ts, bl, _ = R.parse(text, kind)
        assert bl == -1 and all(o is None for o in ids) and not any(ts)
        _assert_window(cls(None).parse(text, device=gpu.index), kind, objs, ids, ts)


@pytest.mark.parametrize("kind", KINDS)
def test_a_line_longer_than_the_lds_staging(kind, gpu):
    """a 4,097-position ring / chain (~100 KB of text): alone, and between short lines"""
    import random

    big = G.gen_line(random.Random(3), kind, 0, big=True, multi=False, nrings=1)
    assert len(big) > 65536
    w = _parity(G.text_of([big]), kind, gpu, what="alone")
    assert w.vx.numel() == 4097
    lines = G.corpus(kind, 150, 9, big_every=50)
    assert sum(len(ln) > 65536 for ln in lines) == 3
    _parity(G.text_of(lines), kind, gpu, what="between short lines")


def _feat(t, coords):
    return G._feat(t, coords)


def test_ring_order_and_multi(gpu):
    sq, hole, hole2 = G._SQ, "[[1,1],[2,1],[2,2],[1,1]]", "[[2,2],[3,2],[3,3],[2,2]]"
    far, tiny = "[[[9,9],[19,9],[19,19],[9,9]]]", "[[1,1],[1.5,1],[1.5,1.5],[1,1]]"
    lines = [
        _feat("Polygon", "[" + hole + "," + sq + "]"),                   # the hole first: shell first
        _feat("Polygon", "[" + sq + "," + hole + "," + hole2 + "]"),     # equal areas keep input order
        _feat("Polygon", "[" + sq + "," + hole + "," + tiny + "," + hole2 + "]"),  # ... an equal ring inserted in front
        _feat("MultiPolygon", "[[" + sq + "," + hole + "]," + far + "," + far + "]"),  # the first polygon only
    ]
    text = G.text_of(lines)
    w = _parity(text, G.POLYGON, gpu)
    f = lambda s: [(float(x), float(y)) for x, y in eval(s)]  # noqa: E731
    objs = R.parse(text, G.POLYGON)[0]
    assert objs[0] == [f(sq), f(hole)] and objs[1] == [f(sq), f(hole), f(hole2)]
    assert objs[2] == [f(sq), f(hole2), f(hole), f(tiny)] and objs[3] == [f(sq), f(hole)]
    assert w.ring_off.cpu().tolist() == [0, 2, 5, 9, 11] and int(w.vx.numel()) == 9 + 13 + 17 + 9
    ls = [_feat("MultiLineString", "[[[0,0],[1,1],[2,0]],[[5,5],[6,6]],[[7,7],[8,8]]]"), _feat("LineString", "[[3,3],[4,4]]")]
    w = _parity(G.text_of(ls), G.LINESTRING, gpu)
    assert w.vert_off.cpu().tolist() == [0, 3, 5]


def _raises_at(kind, lines, at, want, gpu):
    with pytest.raises(ValueError) as e:
        _deser(kind).parse(G.text_of(lines), device=gpu.index)
    from spatialflink_amd.spatialStreams import CSV_KINDS

    assert str(e.value) == f"line {at}: {CSV_KINDS[want]}", (str(e.value), at, want, lines[at][:200])


@pytest.mark.parametrize("kind", KINDS)
def test_bad_and_unsupported_lines_fail_at_their_line_with_their_kind(kind, gpu):
    good = G.corpus(kind, 300, 17)
    cases = [(ln, k) for sk, ln, k in G.BAD_GEOM if sk == kind] + [(ln, R.UNSUPPORTED) for sk, ln, _ in G.UNSUP_GEOM if sk == kind]
    cases.append((b"", R.EMPTY))
    for ln, want in cases:
        assert R.geom_line(ln, kind, prop_obj=G.PROP_OBJ, prop_ts=G.PROP_TS)[1] == want
        lines = list(good)
        lines[137] = ln
        _raises_at(kind, lines, 137, want, gpu)


def test_the_earlier_of_two_bad_lines_is_reported(gpu):
    good = G.corpus(G.POLYGON, 300, 19)
    unclosed = _feat("Polygon", "[[[0,0],[4,0],[4,4],[0,4],[0,1]]]")   # found by pass B
    short = _feat("Polygon", "[[[0,0],[4,0],[0,0]]]")                  # found by pass A
    number = _feat("Polygon", '[[["a",0],[4,0],[4,4],[0,0]]]')
    for (i, a, ka), (j, b, kb) in (((100, unclosed, 3), (200, number, 1)), ((100, number, 1), (200, unclosed, 3)),
                                   ((63, unclosed, 3), (64, unclosed, 3)), ((10, short, 3), (299, number, 1)),
                                   ((0, unclosed, 3), (1, number, 1))):
        lines = list(good)
        lines[i], lines[j] = a, b
        _raises_at(G.POLYGON, lines, i, ka, gpu)


def _call(gpu, text, kind, caps, arrays=True):
    """the C entry point with capacities (obj, ring, vert) -> (status, counts, tensors)"""
    import torch

    t = device_text(text, gpu.index) if text else None
    dev = torch.device("cuda", gpu.index)
    ctx = _lib.context(gpu.index)
    oc, rc, vc = caps
    poly = kind == G.POLYGON
    mk = lambda n, dt: torch.full((n,), -7, dtype=dt, device=dev) if arrays else None  # noqa: E731
    ro, vo = (mk(oc + 1, torch.int32) if poly else None), mk((rc if poly else oc) + 1, torch.int32)
    vx, vy, o, ts = mk(vc, torch.float64), mk(vc, torch.float64), mk(oc, torch.int64), mk(oc, torch.int64)
    p = lambda a: a.data_ptr() if a is not None and a.numel() else None  # noqa: E731
    out = _lib.GfGeomsOut(kind, oc, rc, vc, p(ro), p(vo), p(vx), p(vy), p(o), p(ts))
    sc = GfGeojsonSchema(G.PROP_OBJ.encode(), G.PROP_TS.encode(), 0, 0, 0)
    n = [C.c_int64(-1) for _ in range(4)]
    bk = C.c_int32(-1)
    st = _lib.lib().gf_geojson_parse_geoms(ctx.handle, None, C.c_void_p(t.data_ptr()) if t is not None else None,
                                           len(text), C.byref(sc), C.byref(out), C.byref(n[0]), C.byref(n[1]),
                                           C.byref(n[2]), C.byref(n[3]), C.byref(bk))
    return st, tuple(v.value for v in n[:3]), (ro, vo, vx, vy, o, ts)


@pytest.mark.parametrize("kind", KINDS)
def test_capacities(kind, gpu):
    text = G.text_of(G.corpus(kind, 130, 23))
    objs, ids, ts, _, _ = _ref(text, kind)
    ro, vo, vx, vy = R.csr(kind, objs)
    exact = (len(objs), len(vo) - 1 if kind == G.POLYGON else 0, len(vx))
    st, counts, _ = _call(gpu, text, kind, (0, 0, 0), arrays=False)  # the sizing call
    assert st == _lib.GF_ERR_CAPACITY and counts == exact
    for k in range(3):
        if kind == G.LINESTRING and k == 1:
            continue
        caps = tuple(c - (i == k) for i, c in enumerate(exact))
        st, counts, _ = _call(gpu, text, kind, caps)
        assert st == _lib.GF_ERR_CAPACITY and counts == exact, (k, st, counts)
    st, counts, (gro, gvo, gvx, gvy, go, gts) = _call(gpu, text, kind, exact)
    assert st == _lib.GF_OK and counts == exact
    if kind == G.POLYGON:
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
    assert kind == G.LINESTRING or gro.cpu().tolist()[0] == 0
    st, counts, _ = _call(gpu, b"", kind, (0, 0, 0), arrays=False)
    assert st == _lib.GF_OK and counts == (0, 0, 0)
    w = _deser(kind).parse(b"", device=gpu.index)
    assert w.nobj == 0 and w.vert_off.cpu().tolist() == [0]
    # argument errors
    st, _, _ = _call(gpu, text, kind, (5, 5, 5), arrays=False)
    assert st == _lib.GF_ERR_ARG
    st, _, _ = _call(gpu, text, 3, (0, 0, 0), arrays=False)
    assert st == _lib.GF_ERR_ARG


@pytest.mark.parametrize("kind", KINDS)
def test_end_to_end_prepare_range_and_knn(kind, gpu):
    """2,000 ingested objects -> gf_geom_prepare -> one range query and one kNN (k = 8) on the 100 x 100
    Beijing grid: as the same queries on the window built from the restatement's rings on the host"""
    text = G.text_of(G.corpus(kind, 2000, 41))
    objs, ids, ts, bl, _ = _ref(text, kind)
    assert bl == -1
    w = _deser(kind).parse(text, device=gpu.index)
    keys = w.objID.cpu().numpy()
    if kind == G.POLYGON:
        h = sf.PolygonWindow.from_polygons(objs, keys, ts, device=gpu.index)
        rq, kq = sf.PolygonPointRangeQuery, sf.PolygonPointKNNQuery
    else:
        h = sf.LineStringWindow.from_lines(objs, keys, ts, device=gpu.index)
        rq, kq = sf.LineStringPointRangeQuery, sf.LineStringPointKNNQuery
    grid = sf.UniformGrid(100, *G.BEIJING)
    conf = sf.QueryConfiguration(sf.QueryType.WindowBased)
    qs = [sf.Point("q", 116.4, 40.2), sf.Point("q", 116.9, 39.9)]
    r = 10.0 * (G.BEIJING[1] - G.BEIJING[0]) / 100
    got = []
    for win in (w, h):
        ix = sf.GeometryIndex(win, grid)
        assert ix.info()["invalid"] == 0 and ix.info()["nobj"] == 2000
        res = rq(conf, grid).run(win, qs, r, index=ix)
        kn = kq(conf, grid).run(win, qs[0], r, 8, index=ix)
        got.append((res.indices().astype(np.int64), kn.objID, kn.idx, _u64(kn.dist)))
        ix.close()
    assert len(got[0][0]) > 0 and len(got[0][1]) == 8
    for a, b in zip(got[0], got[1]):
        assert np.array_equal(np.asarray(a), np.asarray(b))
