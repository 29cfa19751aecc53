"""Seeded generator of GeoJSON geometry-stream lines inside the restated contract
(gf_geojson_parse_geoms), and the hand-built lines outside it: BAD_GEOM (one line per failure rule,
with its kind) and UNSUP_GEOM (one line per canonical condition and per foreign type).

Generated lines cover: both stream kinds; Feature and bare-geometry values, both member orders;
Multi* with 1-3 members; 1-4 rings with the hole listed before the shell, and two identical rings
(the tie); ring sizes 4..40 plus a few of 4,097; integer, exponent and 17-digit ordinates, "-0";
whitespace in every legal place; properties after the geometry holding "],[" in strings and arrays."""
import math
import random

POLYGON, LINESTRING = 1, 2
BEIJING = (115.5, 117.6, 39.6, 41.1)
PROP_OBJ, PROP_TS = "oid", "t"


class Lit(str):
    """a number literal, written as is"""


def _num(rnd, v=None, box=None):
    """a literal and nothing else: the value is whatever the literal reads as"""
    form = rnd.choice([0, 0, 0, 4, 4, 6, 6, 6, 2, 2, 3, 5, 5, 1])
    if v is None:
        x0, x1 = box
        v = x0 + (x1 - x0) * rnd.random()
    if form == 0:
        return Lit(repr(v))                       # up to 17 significant digits
    if form == 1:
        return Lit(str(int(round(v))))            # an integer literal (IntNode)
    if form == 2:
        return Lit(f"{v:.6e}".replace("e+0", "e").replace("e+", "E+"))
    if form == 3:
        return Lit(f"{v * 1000:.3f}e-3")
    if form == 4:
        return Lit(f"{v:.17g}")
    if form == 5:
        return Lit(rnd.choice(["-0", "0", "-0.0", "0.0", "0e0"])) if rnd.random() < 0.3 else Lit(f"{v:.5f}")
    return Lit(f"{v:.7f}")


def _ring(rnd, cx, cy, rad, m):
    """a closed ring of m positions around (cx, cy): m - 1 literal pairs, the first one repeated"""
    pts = []
    for k in range(m - 1):
        a = 2.0 * math.pi * k / (m - 1)
        rr = rad * (0.7 + 0.3 * rnd.random())
        pts.append([_num(rnd, cx + rr * math.cos(a)), _num(rnd, cy + rr * math.sin(a))])
    first = list(pts[0])
    if rnd.random() < 0.2 and float(first[0]) == int(float(first[0])):
        first[0] = Lit(f"{int(float(first[0]))}.0")  # the same value by another literal
    return pts + [first]


def _chain(rnd, cx, cy, rad, m):
    return [[_num(rnd, cx + rad * (rnd.random() - 0.5)), _num(rnd, cy + rad * (rnd.random() - 0.5))] for _ in range(m)]


def _size(rnd, big, small=False):
    if big:
        return 4097
    if small:
        return rnd.choice([4, 5])
    return rnd.choice([4, 4, 5, 7, 16, 17, 33, 40, rnd.randint(4, 40)])


def _polygon(rnd, big=False, nrings=None, tie=False, small=False):
    cx = BEIJING[0] + (BEIJING[1] - BEIJING[0]) * rnd.random()
    cy = BEIJING[2] + (BEIJING[3] - BEIJING[2]) * rnd.random()
    rad = 0.002 + 0.03 * rnd.random()
    nr = nrings or rnd.choice([1, 1, 1, 2, 3, 4])
    rings = [_ring(rnd, cx, cy, rad, _size(rnd, big, small))]
    for _ in range(nr - 1):
        rings.append(_ring(rnd, cx, cy, rad * (0.1 + 0.4 * rnd.random()), _size(rnd, False, small)))
    if tie:
        rings.append([list(p) for p in rings[-1]])  # two identical rings: equal areas
    if len(rings) > 1:
        shell = rings[0]
        rnd.shuffle(rings)
        if rings[0] is shell and rnd.random() < 0.7:  # a hole listed before the shell
            rings.append(rings.pop(0))
    return rings


def _linestring(rnd, big=False, small=False):
    cx = BEIJING[0] + (BEIJING[1] - BEIJING[0]) * rnd.random()
    cy = BEIJING[2] + (BEIJING[3] - BEIJING[2]) * rnd.random()
    return _chain(rnd, cx, cy, 0.05, 4097 if big else rnd.choice([2, 3]) if small else rnd.choice([2, 2, 3, 5, 16, 40, rnd.randint(2, 40)]))


def ser(v, rnd, ws=0.0):
    """JSON text of v (dicts keep their order, Lit as is) with whitespace in every legal place"""
    def w():
        return rnd.choice([" ", "  ", "\t", " \t "]) if ws and rnd.random() < ws else ""

    def s(x):
        if isinstance(x, Lit):
            return str(x)
        if isinstance(x, dict):
            return "{" + w() + ",".join(w() + _jstr(k) + w() + ":" + w() + s(y) + w() for k, y in x.items()) + "}"
        if isinstance(x, list):
            return "[" + w() + ",".join(w() + s(y) + w() for y in x) + "]"
        if isinstance(x, str):
            return _jstr(x)
        if x is None:
            return "null"
        if isinstance(x, bool):
            return "true" if x else "false"
        return repr(x)

    return s(v)


def _jstr(x):
    return '"' + x + '"'  # (the corpora hold no character that needs an escape)


def _props(rnd, i, date_fmt, after_geometry):
    p = {}
    r = rnd.random()
    if r < 0.4:
        p[PROP_OBJ] = f"veh-{rnd.randrange(50)}"
    elif r < 0.6:
        p[PROP_OBJ] = str(rnd.randrange(10 ** 6))       # a canonical decimal
    elif r < 0.75:
        p[PROP_OBJ] = Lit(str(rnd.randrange(-5, 10 ** 9)))
    elif r < 0.85 and after_geometry:
        p[PROP_OBJ] = f"a],[{i}"
    if rnd.random() < 0.9:
        if date_fmt == 0:
            p[PROP_TS] = Lit(str(1600000000000 + 1000 * i + rnd.randrange(1000)))
        else:
            p[PROP_TS] = f"2023-{rnd.randint(1, 12):02d}-{rnd.randint(1, 28):02d} {rnd.randint(0, 23):02d}:{rnd.randint(0, 59):02d}:{rnd.randint(0, 59):02d}"
    p["speed"] = Lit(f"{rnd.random() * 30:.2f}")
    if after_geometry and rnd.random() < 0.5:
        p["tags"] = [[Lit("1"), Lit("2")], [Lit("3")], "x],[y"]
        p["note"] = "] , ["
    items = list(p.items())
    rnd.shuffle(items)
    return dict(items)


def gen_line(rnd, kind, i, value_lines=False, date_fmt=0, ws=0.0, big=False, multi=None, nrings=None, tie=False,
             small=False):
    """one supported line (bytes, no newline)"""
    multi = rnd.random() < 0.3 if multi is None else multi
    if kind == POLYGON:
        members = [_polygon(rnd, big and m == 0, nrings, tie, small) for m in range(rnd.randint(1, 3) if multi else 1)]
        t = "MultiPolygon" if multi else "Polygon"
    else:
        members = [_linestring(rnd, big and m == 0, small) for m in range(rnd.randint(1, 3) if multi else 1)]
        t = "MultiLineString" if multi else "LineString"
    coords = members if multi else members[0]
    geom = {"type": t, "coordinates": coords} if rnd.random() < 0.5 else {"coordinates": coords, "type": t}
    form = rnd.randrange(4)
    if form == 0:    # a Feature, geometry first
        V = {"type": "Feature", "geometry": geom, "properties": _props(rnd, i, date_fmt, True)}
    elif form == 1:  # a Feature, properties first (nothing with a bracket before the geometry)
        V = {"properties": _props(rnd, i, date_fmt, False), "geometry": geom, "type": "Feature"}
    elif form == 2:  # a bare geometry with properties of its own
        V = dict(geom)
        V["properties"] = _props(rnd, i, date_fmt, True)
    else:            # no "type" (or an unknown one): the catch branch
        V = {"geometry": geom, "properties": _props(rnd, i, date_fmt, True)}
        if rnd.random() < 0.5:
            V = {"type": "Thing", **V}
    if value_lines:
        rec = V
    elif rnd.random() < 0.5:
        rec = {"key": [Lit(str(i)), "[k]"], "value": V}
    else:
        rec = {"value": V, "key": Lit(str(i))}
    return ser(rec, rnd, ws).encode()


def corpus(kind, n, seed, value_lines=False, date_fmt=0, ws=0.3, big_every=0, small=False):
    """n supported lines: every variety above in turn (small: rings of 4-5, chains of 2-3 positions)"""
    rnd = random.Random(seed * 7919 + kind)
    out = []
    for i in range(n):
        big = bool(big_every) and i % big_every == big_every // 2
        tie = kind == POLYGON and i % 11 == 3
        nrings = (2 + i % 3) if kind == POLYGON and i % 5 == 1 else None
        out.append(gen_line(rnd, kind, i, value_lines, date_fmt, ws if i % 3 else 0.0, big, None, nrings, tie, small))
    return out


def text_of(lines, crlf=False, final_newline=True):
    sep = b"\r\n" if crlf else b"\n"
    t = sep.join(lines)
    return t + sep if final_newline and lines else t


# ---- outside the contract --------------------------------------------------------------------------
def _rec(v):
    return ('{"key":1,"value":' + v + "}").encode()


_SQ = "[[0,0],[4,0],[4,4],[0,4],[0,0]]"          # a closed ring, area 16
_HOLE = "[[1,1],[2,1],[2,2],[1,1]]"
_PROPS = '"properties":{"oid":"a","t":5}'
_LS = "[[0,0],[1,1],[2,0]]"


def _feat(t, coords, pre="", post=""):
    return _rec('{"type":"Feature",' + pre + '"geometry":{"type":"' + t + '","coordinates":' + coords + "}," + _PROPS +
                post + "}")


# (stream kind, line, failure kind): one per failure rule
BAD_GEOM = [
    (POLYGON, _feat("Polygon", '[[["a",0],[4,0],[4,4],[0,4],[0,0]]]'), 1),       # an ordinate is not a number
    (POLYGON, _feat("Polygon", "[[[0,null],[4,0],[4,4],[0,4],[0,0]]]"), 1),
    (POLYGON, _feat("Polygon", "[[[0,0],5,[4,4],[0,4],[0,0]]]"), 3),             # a non-array position
    (POLYGON, _feat("Polygon", "[5]"), 3),                                       # a non-array ring
    (POLYGON, _feat("Polygon", "5"), 3),                                         # non-array coordinates
    (POLYGON, _rec('{"type":"Feature","geometry":{"type":"Polygon"},' + _PROPS + "}"), 3),  # no coordinates
    (POLYGON, _feat("MultiPolygon", "[[" + _SQ + "],7]"), 3),                    # a non-array polygon
    (POLYGON, _feat("Polygon", "[[[0,0],[4,0],[0,0]]]"), 3),                     # a ring of 3 positions
    (POLYGON, _feat("Polygon", "[" + _SQ + ",[[1,1],[2,1],[1,1]]]"), 3),         # ... the second ring
    (POLYGON, _feat("Polygon", "[[[0,0],[4,0],[4,4],[0,4],[0,1]]]"), 3),         # an unclosed ring (pass B)
    (POLYGON, _feat("Polygon", "[" + _SQ + ",[[1,1],[2,1],[2,2],[1,1.5]]]"), 3),  # an unclosed hole
    (POLYGON, _feat("MultiPolygon", "[[" + _SQ + "],[[[9,9],[10,9],[10,10],[9,8]]]]"), 3),  # ... in a dropped polygon
    (POLYGON, _rec('{"type":"Feature",' + _PROPS + "}"), 3),                     # no geometry
    (POLYGON, _rec('{"type":"Feature","geometry":null,' + _PROPS + "}"), 3),
    (POLYGON, _rec('{"geometry":{"type":"Blob","coordinates":[' + _SQ + "]}}"), 3),  # an unknown geometry type
    (POLYGON, b'{"key":1,"value":7}', 3),                                        # V is not an object
    (POLYGON, b'{"key":1}', 3),
    (POLYGON, _rec('{"type":"Polygon","coordinates":[[[0,0],[4,0],[0,0]]]}'), 3),  # V's own fails, no geometry
    (POLYGON, _rec('{"type":"Polygon","coordinates":5,"geometry":{"type":"Polygon",'
                   '"coordinates":[[[0,"y"],[4,0],[4,4],[0,0]]]}}'), 1),          # ... and the geometry fails too
    (POLYGON, _rec('{"type":"Polygon","coordinates":null,"geometry":{"type":"Polygon",'
                   '"coordinates":[[[0,0],[4,0],[4,4],[0,2]]]}}'), 3),            # ... with an unclosed ring
    (POLYGON, _feat("Polygon", "[" + _SQ + "]") + b"]", 3),                      # malformed JSON
    (POLYGON, _rec('{"type":"Feature","geometry":{"type":"Polygon","coordinates":[' + _SQ +
                   ']},"properties":{"oid":"a","t":"x"}}'), 1),                   # the time property
    (LINESTRING, _feat("LineString", "[[0,0]]"), 3),                             # a linestring of 1 position
    (LINESTRING, _feat("MultiLineString", "[" + _LS + ",[[5,5]]]"), 3),          # ... a later member
    (LINESTRING, _feat("LineString", '[[0,0],["1",1]]'), 1),
    (LINESTRING, _feat("LineString", "[[0,0],true]"), 3),
    (LINESTRING, _feat("LineString", "{}"), 3),
    (LINESTRING, _feat("MultiLineString", "[" + _LS + ",3]"), 3),
]

# (stream kind, line, splitter): one per canonical condition and per foreign type; splitter: the
# reference's string splitter reads something else than the plain structure (or throws) -- the
# rest is refused because JTS, Jackson's re-serialisation or the map itself is not restated there
UNSUP_GEOM = [
    (POLYGON, _feat("Polygon", "[" + _SQ + "]", pre='"bbox":[0,0,4,4],'), True),
    (POLYGON, _rec('{"type":"Feature","properties":{"oid":"a","tags":[1,2]},"geometry":{"type":"Polygon",'
                   '"coordinates":[' + _SQ + "]}}"), True),
    (POLYGON, _rec('{"type":"Feature","properties":{"oid":"a[1]"},"geometry":{"type":"Polygon",'
                   '"coordinates":[' + _SQ + "]}}"), True),
    (POLYGON, _rec('{"type":"Feature","properties":{"oid":"a\\u005b"},"geometry":{"type":"Polygon",'
                   '"coordinates":[' + _SQ + "]}}"), True),
    (POLYGON, _rec('{"type":"Feature","properties":{"note":"a\\nb"},"geometry":{"type":"Polygon",'
                   '"coordinates":[' + _SQ + "]}}"), False),                      # an escape that hides nothing
    (POLYGON, _feat("Polygon", "[[[0,0,1],[4,0,1],[4,4,1],[0,4,1],[0,0,1]],[[1,1,1],[2,1,1],[2,2,1],[1,1,1]]]"), True),
    (POLYGON, _feat("Polygon", "[[[0,0],[4,0],[4,4],[0,4],[0]]]"), True),        # one ordinate
    (POLYGON, _feat("Polygon", "[]"), True),                                     # empty arrays, every level
    (POLYGON, _feat("Polygon", "[" + _SQ + ",[]]"), True),
    (POLYGON, _feat("Polygon", "[[[0,0],[4,0],[4,4],[],[0,0]]]"), True),
    (POLYGON, _feat("MultiPolygon", "[]"), True),
    (POLYGON, _feat("MultiPolygon", "[[" + _SQ + "],[]]"), True),
    (POLYGON, _rec('{"type":"Feature","geometry":{"type":"Point","coordinates":[0,0]},"geometry":{"type":"Polygon",'
                   '"coordinates":[' + _SQ + "]}}"), False),                      # a duplicate member name in V
    (POLYGON, _rec('{"type":"Feature","geometry":{"type":"Polygon","coordinates":[[[0,0],[1,0],[1,1],[0,0]]],'
                   '"coordinates":[' + _SQ + "]}}"), False),                      # ... in the geometry
    (POLYGON, _rec('{"type":"Polygon","coordinates":[[[0,0],[4,0],[0,0]]],"geometry":{"type":"Polygon",'
                   '"coordinates":[' + _SQ + "]}}"), True),                       # the catch branch succeeds
    (POLYGON, _rec('{"type":"Polygon","coordinates":[[[0,0],[4,0],[4,4],[0,1]]],"geometry":{"type":"Polygon",'
                   '"coordinates":[' + _SQ + "]}}"), True),                       # ... after an unclosed ring (pass B)
    (POLYGON, _rec('{"type":"Polygon","coordinates":5,"geometry":{"type":"Polygon",'
                   '"coordinates":[' + _SQ + "]}}"), False),                      # ... with no bracket of V's own
    (POLYGON, _feat("Point", "[1,2]"), False),                                   # foreign types
    (POLYGON, _feat("MultiPoint", "[[1,2],[3,4]]"), False),
    (POLYGON, _feat("LineString", _LS), False),
    (POLYGON, _feat("MultiLineString", "[" + _LS + "]"), False),
    (POLYGON, _rec('{"type":"Feature","geometry":{"type":"GeometryCollection","geometries":[]}}'), False),
    (POLYGON, _rec('{"type":"FeatureCollection","features":[]}'), False),
    (POLYGON, _rec('{"type":"Point","coordinates":[1,2]}'), False),
    (LINESTRING, _feat("Polygon", "[" + _SQ + "]"), False),
    (LINESTRING, _feat("MultiPolygon", "[[" + _SQ + "]]"), False),
    (LINESTRING, _feat("Point", "[1,2]"), False),
    (LINESTRING, _feat("LineString", _LS, pre='"bbox":[0,0,2,1],'), True),
    (LINESTRING, _feat("LineString", "[]"), True),
    (LINESTRING, _feat("MultiLineString", "[" + _LS + ",[]]"), True),
    (LINESTRING, _feat("LineString", "[[0,0],[1]]"), True),
    (LINESTRING, _feat("LineString", "[[0,0],[1,1]]", pre='"id":1e999,'), False),  # a number json-simple cannot read
]
