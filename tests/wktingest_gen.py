"""Seeded generator of WKT stream lines inside the restated contract (gf_wkt_parse_geoms,
gf_wkt_parse_points), and the hand-built lines outside it: BAD (one line per failure rule, with its
kind) and UNSUPPORTED (one line per rule).

Knobs of the generated lines: blanks in every legal place; exponent, signed-zero and 17+ digit
literals (and the forms only Double.parseDouble takes: a leading '+', ".5", "5."); holes in any
order and two identical rings; Multi* with 1-3 members; an objID field present or absent; a trailing
date; Kafka-record wrapping; a big line (a 4,097-position ring or chain).  The geometries come from
tests/geomingest_gen.py, so the same literals can be written as GeoJSON (geojson_twin)."""
import random

import geomingest_gen as G
from wktingest_ref import at_rounding_boundary

POINT, POLYGON, LINESTRING = 0, 1, 2
TAG = {POINT: "POINT", POLYGON: "POLYGON", LINESTRING: "LINESTRING"}
# the reference's own sample records (Deserialization.java:474, :761); the second is malformed:
# "-170.0, 45.0" is a position with one number
SAMPLE_POLYGON = (b'{"key":1,"value":"MULTIPOLYGON (((-74.15010482037168 40.62183511874645, -74.15016701565006 '
                  b'40.62177739783489, -74.1502116609276 40.62180593197037, -74.15015270982748 40.62185788893257, '
                  b'-74.15014748371995 40.62186259918266, -74.1501238625006 40.6218473986088, -74.150107093191 '
                  b'40.62186251414858, -74.15008804280825 40.621850243299434, -74.15010482037168 40.62183511874645)))"}')
SAMPLE_LINESTRING = b'{"key":1,"value":"MULTILINESTRING((170.0 45.0,180.0 45.0,-180.0 45.0,-170.0, 45.0))"}'


def _lit(rnd, lit, json_safe):
    """the literal itself, or the same kind of value in a form only WKT takes"""
    s = str(lit)
    if json_safe:
        return "-0.0" if s == "-0" else s  # (GeoJSON reads the integer literal -0 as +0.0)
    # 20+ digits: decided and extended by the literal alone, so that a ring's repeated first position stays equal
    own = random.Random(s)
    if own.random() < 0.1 and len(s) >= 15 and "." in s and "e" not in s.lower():
        ext = s + "".join(own.choice("0123456789") for _ in range(own.randint(4, 12)))
        return s if at_rounding_boundary(ext.encode()) else ext  # (1 in ~1000: outside the contract)
    r = rnd.random()
    if r < 0.06 and not s.startswith("-"):
        return "+" + s
    if r < 0.10 and s.startswith("0."):
        return s[1:]                                   # ".5"
    if r < 0.14 and s.isdigit():
        return s + "."                                 # "5."
    return s


def _b(rnd, ws, least=""):
    return rnd.choice([" ", "  ", "\t", " \t "]) if ws and rnd.random() < ws else least


def _chain_text(rnd, chain, ws, json_safe):
    pos = [_lit(rnd, x, json_safe) + _b(rnd, ws, " ") + _lit(rnd, y, json_safe) for x, y in chain]
    sep = rnd.choice([",", ", "]) if not ws else None
    body = "".join((p if k == 0 else (sep or _b(rnd, ws) + "," + _b(rnd, ws)) + p) for k, p in enumerate(pos))
    return "(" + _b(rnd, ws) + body + _b(rnd, ws) + ")"


def _list_text(rnd, members, ws):
    return "(" + _b(rnd, ws) + (_b(rnd, ws) + "," + _b(rnd, ws)).join(members) + _b(rnd, ws) + ")"


def wkt_text(rnd, kind, members, multi, ws=0.0, json_safe=False):
    """the WKT geometry of `members` (tests/geomingest_gen.py shapes: polygons = lists of rings)"""
    if kind == POLYGON:
        body = [_list_text(rnd, [_chain_text(rnd, r, ws, json_safe) for r in poly], ws) for poly in members]
    else:
        body = [_chain_text(rnd, c, ws, json_safe) for c in members]
    tag = ("MULTI" if multi else "") + TAG[kind]
    return tag + _b(rnd, ws, rnd.choice(["", " "])) + (_list_text(rnd, body, ws) if multi else body[0])


def geojson_twin(kind, members, multi):
    """the same literals as a GeoJSON value line (json_safe geometries only)"""
    fix = lambda v: "-0.0" if str(v) == "-0" else str(v)  # noqa: E731
    ch = lambda c: "[" + ",".join(f"[{fix(x)},{fix(y)}]" for x, y in c) + "]"  # noqa: E731
    if kind == POLYGON:
        body = ["[" + ",".join(ch(r) for r in poly) + "]" for poly in members]
        t = "MultiPolygon" if multi else "Polygon"
    else:
        body = [ch(c) for c in members]
        t = "MultiLineString" if multi else "LineString"
    coords = "[" + ",".join(body) + "]" if multi else body[0]
    return ('{"type":"Feature","geometry":{"type":"' + t + '","coordinates":' + coords + "}}").encode()


def gen_geom(rnd, kind, big=False, multi=None, nrings=None, tie=False, small=False):
    multi = rnd.random() < 0.3 if multi is None else multi
    n = rnd.randint(1, 3) if multi else 1
    if kind == POLYGON:
        return [G._polygon(rnd, big and m == 0, nrings, tie, small) for m in range(n)], multi
    return [G._linestring(rnd, big and m == 0, small) for m in range(n)], multi


def _date(rnd):
    return (f"20{rnd.randint(10, 30):02d}-{rnd.randint(1, 12):02d}-{rnd.randint(1, 28):02d} "
            f"{rnd.randint(0, 23):02d}:{rnd.randint(0, 59):02d}:{rnd.randint(0, 59):02d}")


def gen_line(rnd, kind, i, delim=None, date=False, ws=0.0, kafka=None, json_safe=False, compact=False, **geom):
    """one supported line (bytes, no newline), and its geometry (members, multi)"""
    if kind == POINT:
        x = G._num(rnd, box=G.BEIJING[:2])
        y = G._num(rnd, box=G.BEIJING[2:])
        text = "POINT" + _b(rnd, ws, rnd.choice(["", " "])) + "(" + _b(rnd, ws) + _lit(rnd, x, json_safe) + _b(rnd, ws, " ") + \
            _lit(rnd, y, json_safe) + _b(rnd, ws) + ")"
        members, multi = [[(x, y)]], False
    else:
        members, multi = gen_geom(rnd, kind, **geom)
        text = wkt_text(rnd, kind, members, multi, ws, json_safe)
    d = delim or ","
    if compact:  # objID, geometry, date: the benchmark's line
        return (f"{rnd.randrange(10 ** 6)}{d}{text}{d}{_date(rnd)}").encode(), (members, multi)
    sep = rnd.choice([d, d + " ", " " + d + " "]) if d != "\t" else d
    r = rnd.random()
    if delim is not None or rnd.random() < 0.3:
        if r < 0.35:
            text = rnd.choice([f"veh-{rnd.randrange(40)}", str(rnd.randrange(10 ** 6)), f"{rnd.randrange(99):03d}",
                               " padded id "]) + sep + text
        elif r < 0.45:
            text = sep.join(["a", str(i), text])          # the geometry in a later field
        if date or rnd.random() < 0.2:
            tail = [_date(rnd)]
            if rnd.random() < 0.3:
                tail = rnd.choice([[tail[0], "not a date"], ["1.5", tail[0] + " UTC"], ["x", "y"]])
            text = sep.join([text] + tail)
    kafka = rnd.random() < 0.3 if kafka is None else kafka
    if kafka:
        text = '{"key":' + str(i) + ',"value":"' + text + '"}'
    return text.encode(), (members, multi)


def corpus(kind, n, seed, delim=None, date=False, ws=0.3, big_every=0, small=False, json_safe=False, compact=False,
           with_geoms=False):
    """n supported lines: every variety above in turn (small: rings of 4-5, chains of 2-3 positions)"""
    rnd = random.Random(seed * 6151 + kind)
    out = []
    for i in range(n):
        geom = {}
        if kind != POINT:
            geom = dict(big=bool(big_every) and i % big_every == big_every // 2, tie=kind == POLYGON and i % 11 == 3,
                        nrings=(2 + i % 3) if kind == POLYGON and i % 5 == 1 else None, small=small)
        ln, g = gen_line(rnd, kind, i, delim, date, ws if i % 3 else 0.0, None, json_safe, compact, **geom)
        out.append((ln, g) if with_geoms else ln)
    return out


def text_of(lines, crlf=False, final_newline=True):
    return G.text_of(lines, crlf, final_newline)


# ---- outside the contract: (stream kind, line, failure kind), one line per rule -------------------------
_SQ = "(0 0, 4 0, 4 4, 0 4, 0 0)"
_HOLE = "(1 1, 2 1, 2 2, 1 1)"
BAD = [
    (POLYGON, b"polygon ((0 0, 4 0, 4 4, 0 0))", 3),                         # a lower-case tag: no tag
    (POLYGON, b"7, 2020-01-01 00:00:00", 3),                                 # no tag at all
    (LINESTRING, b"POLYGON ((0 0, 4 0, 4 4, 0 0))", 3),                      # another stream's tag
    (POINT, b"1,2", 3),
    (POLYGON, b"POLYGON ((0 0, 4 0, 1.2.3 4, 0 0))", 1),                     # parseDouble rejects the token
    (POLYGON, b"POLYGON ((0 0, 4 0, - 4, 0 0))", 1),
    (LINESTRING, b"LINESTRING (0 0, e5 1)", 1),
    (POINT, b"POINT (1e 2)", 1),
    (POINT, b"POINT (1 2-3)", 1),
    (POLYGON, b"POLYGON ((0 0, 4 0, 4, 0 0))", 3),                           # a position with one number
    (LINESTRING, b"LINESTRING (0 0, 1)", 3),
    (POINT, b"POINT (1)", 3),
    (LINESTRING, SAMPLE_LINESTRING, 3),                                      # the reference's own sample
    (POLYGON, b"POLYGON ((0 0, 4 0, 4 4, 0 0)", 3),                          # the line ends before the geometry closes
    (POLYGON, b"POLYGON ((0 0, 4 0, 4 4,", 3),
    (POLYGON, b"POLYGON", 3),
    (LINESTRING, b"MULTILINESTRING ((0 0, 1 1), (2 2, 3 3)", 3),
    (POINT, b"POINT (1 2", 3),
    (POLYGON, b"POLYGON (0 0, 4 0, 4 4, 0 0)", 3),                           # a wrong bracket
    (POLYGON, b"POLYGON ((0 0, 4 0, 4 4, 0 0]]", 3),
    (POLYGON, b"POLYGON ((0 0; 4 0; 4 4; 0 0))", 3),
    (POLYGON, b"MULTIPOLYGON ((0 0, 4 0, 4 4, 0 0))", 3),
    (LINESTRING, b"LINESTRING ((0 0, 1 1))", 3),
    (LINESTRING, b"MULTILINESTRING (0 0, 1 1)", 3),
    (POINT, b"POINT ((1 2))", 3),
    (POINT, b"POINT (1 2, 3 4)", 3),
    (POLYGON, b"POLYGON ()", 3),                                             # an empty member list
    (POLYGON, b"POLYGON (())", 3),
    (POLYGON, ("POLYGON (" + _SQ + ",)").encode(), 3),
    (LINESTRING, b"LINESTRING ()", 3),
    (LINESTRING, b"MULTILINESTRING ()", 3),
    (POLYGON, b"POLYGON ((0 0, 4 0, 0 0))", 3),                              # a ring of 3 positions
    (POLYGON, ("POLYGON (" + _SQ + ", (1 1, 2 1, 1 1))").encode(), 3),       # ... the second ring
    (POLYGON, b"POLYGON ((0 0, 4 0, 4 4, 0 4, 0 1))", 3),                    # an unclosed ring (pass B)
    (POLYGON, ("POLYGON (" + _SQ + ", (1 1, 2 1, 2 2, 1 1.5))").encode(), 3),  # an unclosed hole
    (POLYGON, ("MULTIPOLYGON ((" + _SQ + "), ((9 9, 10 9, 10 10, 9 8)))").encode(), 3),  # ... in a dropped polygon
    (LINESTRING, b"LINESTRING (0 0)", 3),                                    # a linestring of 1 position
    (LINESTRING, b"MULTILINESTRING ((0 0, 1 1), (5 5))", 3),                 # ... a later member
]
UNSUPPORTED = [
    (POLYGON, b"POLYGON Z ((0 0 1, 4 0 1, 4 4 1, 0 0 1))"),                  # between the tag and its '('
    (POLYGON, b"POLYGON M ((0 0 1, 4 0 1, 4 4 1, 0 0 1))"),
    (POLYGON, b"POLYGON ZM ((0 0 1 2, 4 0 1 2, 4 4 1 2, 0 0 1 2))"),
    (POLYGON, b"POLYGON EMPTY"),
    (POLYGON, b"POLYGONZ ((0 0 1, 4 0 1, 4 4 1, 0 0 1))"),
    (LINESTRING, b"LINESTRING EMPTY"),
    (LINESTRING, b"MULTILINESTRINGS ((0 0, 1 1))"),
    (POINT, b"POINT EMPTY"),
    (POINT, b"POINTS (1 2)"),
    (POLYGON, ("MULTIPOLYGON ((" + _SQ + "), EMPTY)").encode()),             # EMPTY anywhere
    (POLYGON, ("POLYGON (" + _SQ + ", EMPTY)").encode()),
    (LINESTRING, b"MULTILINESTRING ((0 0, 1 1), EMPTY)"),
    (POLYGON, b"POLYGON ((0 0 1, 4 0 1, 4 4 1, 0 0 1))"),                    # a third number
    (LINESTRING, b"LINESTRING (0 0, 1 1 1)"),
    (POINT, b"POINT (1 2 3)"),
    (POLYGON, b"POLYGON ((0 0, 4 0, NaN 4, 0 0))"),                          # a token holding another letter
    (POLYGON, b"POLYGON ((0 0, 4 0, Infinity 4, 0 0))"),
    (LINESTRING, b"LINESTRING (0 0, 1d 1)"),
    (LINESTRING, b"LINESTRING (0 0, 1.5f 1)"),
    (POINT, b"POINT (0x10 2)"),
    (POINT, b"POINT (1 0x1p3)"),
    (POLYGON, b"POLYGON ((0 0, 4 0, # 4 4, 0 0))"),                          # '#'
    (LINESTRING, b"LINESTRING (0 0,# 1 1)"),
    (POLYGON, b"POLYGON ((0 0, 4 0,\xc2\xa04 4, 0 0))"),                     # a byte >= 0x80
    (POINT, b"POINT (1\xff 2)"),
    (POLYGON, b"POLYGON ((0 0, 4 0,\x0b4 4, 0 0))"),                         # a control byte other than tab
    (LINESTRING, b"LINESTRING (0 0,\r1 1)"),
    (POINT, b"POINT\x01(1 2)"),
]

SQ = b"POLYGON ((0 0, 4 0, 4 4, 0 4, 0 0))"
T_LINES = [  # (kind, line, delimiter, date format) -> the objID and time rules
    (POLYGON, b"7, " + SQ + b", 2020-01-02 03:04:05", ",", 1),
    (POLYGON, b"7, " + SQ, ",", 1),                                   # POLYGON at ts 0: objID dropped
    (POLYGON, b"7, " + SQ + b", 1970-01-01 00:00:00", ",", 1),        # ... a date that parses to the epoch
    (POLYGON, b"7, MULTI" + SQ[:8] + b"(" + SQ[8:] + b")", ",", 1),   # MULTIPOLYGON keeps it
    (LINESTRING, b"veh-1; LINESTRING (0 0, 1 1)", ";", 1),            # linestrings keep it
    (LINESTRING, b"veh-1; LINESTRING (0 0, 1 1); 2020-01-02 03:04:05", ";", 0),  # date_format 0
    (POLYGON, SQ + b", 2020-01-02 03:04:05", ",", 1),                 # field 0 is the tag: objID null
    (POLYGON, b' "MULTI' + SQ[:8] + b"(" + SQ[8:] + b')" , 2020-01-02 03:04:05', ",", 1),
    (POLYGON, b"7;" + SQ + b";2020-01-02 03:04:05;x;2021-01-02 03:04:05 tail;nope", ";", 1),  # the last that parses
    (POLYGON, b'"0"07\t' + SQ + b"\t2020-01-02 03:04:05", "\t", 1),   # quotes are removed: "007", a dictionary String
    (POLYGON, b"\t" + SQ + b"\t2020-01-02 03:04:05", "\t", 1),        # a leading separator: objID ""
    (POLYGON, b"a b  \t  c " + SQ + b"\t 2020-01-02 03:04:05", "\t", 1),  # a whitespace run holding the tab
    (LINESTRING, b"-12,LINESTRING (0 0, 1 1),2020-13-40 25:61:61", ",", 1),  # lenient rollover
    (LINESTRING, b"5,LINESTRING (0 0, 1 1),1400-01-01 00:00:00", ",", 1),    # before 1583: unsupported
    (LINESTRING, b",,", ",", 1),                                      # no field at all
]
