"""Python restatement of the GeoJSON geometry-stream ingest contract (include/geoflink_hip.h,
gf_geojson_parse_geoms) over the `json` module: per line either the window object -- a polygon's
rings in createPolygon order or a linestring's chain --, its objID String and ts, or the kind of
the failure.  The record's reading (strict JSON, depth, UTF-8, escapes, dates) is the point
oracle's, imported from oracle/oracle.py."""
import json
import json.decoder
import json.scanner
import math

import oracle as O

POLYGON, LINESTRING = 1, 2
OK, NUMBER_FORMAT, UNSUPPORTED, MISSING, EMPTY = 0, 1, 2, 3, 4
GEOMS = {"Point", "LineString", "Polygon", "MultiPoint", "MultiLineString", "MultiPolygon", "GeometryCollection"}
ALLOWED = {POLYGON: {"Polygon", "MultiPolygon"}, LINESTRING: {"LineString", "MultiLineString"}}


class JObj(dict):
    """A JSON object (last duplicate wins) that keeps its members in text order and remembers
    duplicate names and names written with an escape."""
    pairs = ()
    dup = False
    esc_keys = False


def _decoder(escapes, poison):
    def pint(t):
        v = int(t)
        if not -(1 << 63) <= v < (1 << 63):
            poison[0] = True
        return v

    def pfloat(t):
        v = float(t)
        if math.isinf(v):
            poison[0] = True
        return v

    def pconst(t):
        raise ValueError(t)

    def pairs(kv):
        d = JObj(kv)
        d.pairs = kv
        d.dup = len(d) != len(kv)
        d.esc_keys = any(getattr(k, "escaped", False) for k, _ in kv)
        return d

    dec = json.JSONDecoder(parse_int=pint, parse_float=pfloat, parse_constant=pconst, object_pairs_hook=pairs)
    if escapes:
        dec.parse_string = O._tagged_scanstring
        dec.scan_once = json.scanner.py_make_scanner(dec)
    return dec


def read_record(line: bytes):
    """The record as Jackson reads it -> (object, 0) or (None, kind), as oracle._geojson_line."""
    if line.endswith(b"\r"):
        line = line[:-1]
    if not line:
        return None, EMPTY
    if O._too_deep(line):
        return None, UNSUPPORTED
    if not O._utf8_structural(line):
        return None, MISSING
    poison = [False]
    try:
        text = line.decode("utf-8", "surrogateescape")
        if b"\\" in line:
            saved = json.decoder.scanstring
            json.decoder.scanstring = O._tagged_scanstring
            try:
                d = _decoder(True, poison).decode(text)
            finally:
                json.decoder.scanstring = saved
        else:
            d = _decoder(False, poison).decode(text)
    except ValueError:
        return None, MISSING
    if not isinstance(d, dict):
        return None, MISSING
    if poison[0]:
        return None, UNSUPPORTED
    return d, OK


def _brackets(v):
    """The value's text holds a '[' or ']' byte, or a backslash (an escape may spell one)."""
    if isinstance(v, str):
        return "[" in v or "]" in v or getattr(v, "escaped", False)
    if isinstance(v, list):
        return True
    if isinstance(v, dict):
        return any(_brackets(k) or _brackets(x) for k, x in v.pairs)
    return False


def _before(obj, name):
    """the members of obj in front of its member `name`"""
    out = []
    for k, v in obj.pairs:
        if k == name:
            break
        out.append((k, v))
    return out


def _position(p):
    if not isinstance(p, list):
        return MISSING
    for v in p[:2]:
        if not O._num(v):
            return NUMBER_FORMAT
    return OK if len(p) == 2 else UNSUPPORTED


def _chain(c, least):
    if not isinstance(c, list):
        return MISSING
    if not c:
        return UNSUPPORTED
    for p in c:
        k = _position(p)
        if k:
            return k
    return MISSING if len(c) < least else OK


def _poly(c):
    if not isinstance(c, list):
        return MISSING
    if not c:
        return UNSUPPORTED
    for ring in c:
        k = _chain(ring, 4)
        if k:
            return k
    return OK


def _xy(p):
    return (float(p[0]), float(p[1]))  # an int is Jackson's IntNode / LongNode: (double) of the long


def _closed(poly):
    return all(_xy(r[0]) == _xy(r[-1]) for r in poly)


def ring_area(ring):
    a = 0.0
    for (x1, y1), (x2, y2) in zip(ring[:-1], ring[1:]):
        a += x1 * y2 - x2 * y1
    return abs(a) / 2.0


def create_polygon(rings):
    """createPolygon order (Polygon.java:147-165, createPolygonArray :115-145)."""
    rings = [[_xy(p) for p in r] for r in rings]
    if len(rings) == 1:
        return rings
    ordered = []
    for r in rings:
        if not ordered or ring_area(ordered[-1]) >= ring_area(r):
            ordered.append(r)
        else:
            for i in range(len(ordered)):
                if ring_area(ordered[i]) <= ring_area(r):
                    ordered.insert(i, r)
                    break
    return ordered


def _build(t, c, before):
    """GeoJsonReader's geometry of type t from the coordinates c, then what the splitter needs of
    the text in front of them -> (object, 0) or (None, kind)"""
    if not isinstance(c, list):
        return None, MISSING
    if any(_brackets(k) or _brackets(v) for k, v in before):
        return None, UNSUPPORTED
    if t == "Polygon":
        k, members = _poly(c), [c]
    elif t == "LineString":
        k, members = _chain(c, 2), [c]
    else:
        k, members = (OK if c else UNSUPPORTED), c
        for m in c:
            if k:
                break
            k = _poly(m) if t == "MultiPolygon" else _chain(m, 2)
    if k:
        return None, k
    if t in ALLOWED[POLYGON]:
        if not all(_closed(m) for m in members):
            return None, MISSING
        return create_polygon(members[0]), OK
    return [_xy(p) for p in members[0]], OK


def _gtype(obj):
    t = obj.get("type")
    if not isinstance(t, str):
        return None
    if getattr(t, "escaped", False):
        raise O._Unsupported()
    return t


def _properties(V, prop_obj, prop_ts, date_fmt, tz_off_min):
    """(ts, objID bytes or None), 0 or (None, kind) -- the properties as oracle._geojson_line reads them"""
    ts, obj = 0, None
    props = V.get("properties")
    if not isinstance(props, dict) or (prop_ts is None and prop_obj is None):
        return (ts, obj), OK
    if props.esc_keys:
        return None, UNSUPPORTED
    if prop_ts is not None and prop_ts in props:
        v = props[prop_ts]
        if date_fmt == 0:
            if not (isinstance(v, int) and not isinstance(v, bool)) or not -(1 << 63) <= v < (1 << 63):
                return None, NUMBER_FORMAT
            ts = v
        else:
            if not isinstance(v, str):
                return None, NUMBER_FORMAT
            if getattr(v, "escaped", False):
                return None, UNSUPPORTED
            t, k = O._jdate(v, tz_off_min)
            if k:
                return None, k
            ts = t
    if prop_obj is not None and prop_obj in props:
        v = props[prop_obj]
        if isinstance(v, bool):
            obj = b"true" if v else b"false"
        elif v is None:
            obj = b"null"
        elif isinstance(v, int):
            obj = str(v).encode()
        elif isinstance(v, str):
            if getattr(v, "escaped", False):
                return None, UNSUPPORTED
            obj = v.encode("utf-8", "surrogateescape")
        else:
            return None, UNSUPPORTED
    return (ts, obj), OK


def value_of(line: bytes, value_lines=False):
    """(V, 0) or (None, kind): the object the maps call toString() on"""
    d, k = read_record(line)
    if k:
        return None, k
    if value_lines:
        return d, OK
    if d.esc_keys:
        return None, UNSUPPORTED
    V = d.get("value")
    return (V, OK) if isinstance(V, dict) else (None, MISSING)


def geom_line(line: bytes, kind, prop_obj=None, prop_ts=None, date_fmt=0, tz_off_min=0, value_lines=False):
    """One line -> ((object, objID bytes or None, ts), 0) or (None, kind)."""
    V, k = value_of(line, value_lines)
    if k:
        return None, k
    if not isinstance(V, dict):
        return None, MISSING
    if V.esc_keys or V.dup:
        return None, UNSUPPORTED
    try:
        tv = _gtype(V)
        if tv == "FeatureCollection":
            return None, UNSUPPORTED
        own = tv in GEOMS
        obj = None
        if own:
            if tv not in ALLOWED[kind]:
                return None, UNSUPPORTED
            obj, k = _build(tv, V.get("coordinates"), _before(V, "coordinates"))
            if k == UNSUPPORTED:
                return None, k
        if obj is None:
            G = V.get("geometry")
            if not isinstance(G, dict):
                return None, MISSING
            if G.esc_keys or G.dup:
                return None, UNSUPPORTED
            tg = _gtype(G)
            if tg is None or tg not in GEOMS | {"Feature", "FeatureCollection"}:
                return None, MISSING
            if tg not in ALLOWED[kind]:
                return None, UNSUPPORTED
            obj, k = _build(tg, G.get("coordinates"), _before(V, "geometry") + _before(G, "coordinates"))
            if k:
                return None, k
            if own:
                return None, UNSUPPORTED
    except O._Unsupported:
        return None, UNSUPPORTED
    pr, k = _properties(V, prop_obj, prop_ts, date_fmt, tz_off_min)
    if k:
        return None, k
    return (obj, pr[1], pr[0]), OK


def split_lines(text: bytes):
    lines = text.split(b"\n")
    if lines and lines[-1] == b"" and (text.endswith(b"\n") or not text):
        lines = lines[:-1]
    return lines


def parse(text: bytes, kind, **kw):
    """-> (objects, objIDs, ts, bad_line, bad_kind): the first bad line wins"""
    objs, ids, ts = [], [], []
    for i, ln in enumerate(split_lines(text)):
        r, k = geom_line(ln, kind, **kw)
        if k:
            return None, None, None, i, k
        objs.append(r[0])
        ids.append(r[1])
        ts.append(r[2])
    return objs, ids, ts, -1, 0


def csr(kind, objs):
    """(ring_off or None, vert_off, vx, vy) of the window"""
    import numpy as np

    ring_off, vert_off, vx, vy = [0], [0], [], []
    for o in objs:
        for chain in (o if kind == POLYGON else [o]):
            vx += [p[0] for p in chain]
            vy += [p[1] for p in chain]
            vert_off.append(len(vx))
        ring_off.append(len(vert_off) - 1)
    return (np.asarray(ring_off, np.int32) if kind == POLYGON else None, np.asarray(vert_off, np.int32),
            np.asarray(vx, np.float64), np.asarray(vy, np.float64))
