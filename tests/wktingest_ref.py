"""An independent Python restatement of the WKT ingest contract (include/geoflink_hip.h,
gf_wkt_parse_geoms / gf_wkt_parse_points): a StreamTokenizer-style tokenizer set up as JTS's WKTReader
sets its own up (word characters: letters, digits, + - .; blanks skipped; '#', bytes >= 0x80 and
control bytes outside the subset), the reader's subset (POINT, LINESTRING, POLYGON, MULTILINESTRING,
MULTIPOLYGON), JTS's LinearRing / LineString checks, and the six maps of Deserialization.java
(:214-232, :261-288, :461-490, :524-586, :748-835).  Per line: ((object, objID bytes or None, ts), 0)
or (None, kind)."""
import calendar
import re

from geomingest_ref import create_polygon

OK, NUMBER_FORMAT, UNSUPPORTED, MISSING, EMPTY = 0, 1, 2, 3, 4
POINT, POLYGON, LINESTRING = 0, 1, 2
TAGS = {POINT: (None, b"POINT"), POLYGON: (b"MULTIPOLYGON", b"POLYGON"),
        LINESTRING: (b"MULTILINESTRING", b"LINESTRING")}

_WORD = frozenset(b"abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789+-.")
_NUMC = frozenset(b"0123456789+-.eE")
_JAVA_DOUBLE = re.compile(rb"[+-]?(\d+\.?\d*|\.\d+)([eE][+-]?\d+)?\Z")
_DATE = re.compile(rb"(\d+)-(\d+)-(\d+) (\d+):(\d+):(\d+)")
_TRIM = bytes(range(0x21))  # String.trim(): every char <= ' '


class Fail(Exception):
    def __init__(self, kind):
        super().__init__(kind)
        self.kind = kind


class Tokens:
    """the tokens of the geometry text, read lazily: document order decides which failure is first"""

    def __init__(self, text):
        self.t, self.i, self.held = text, 0, None

    def _read(self):
        t, n = self.t, len(self.t)
        while self.i < n and t[self.i] in b" \t":
            self.i += 1
        if self.i >= n:
            return ("end", None)
        c = t[self.i]
        if c in _WORD:
            j = self.i
            while j < n and t[j] in _WORD:
                j += 1
            w = t[self.i:j]
            self.i = j
            return ("num" if all(b in _NUMC for b in w) else "word", w)
        self.i += 1
        if c in b"(),":
            return (chr(c), None)
        if c == 0x23 or c >= 0x80 or c < 0x20:
            raise Fail(UNSUPPORTED)
        return ("other", None)

    def peek(self):
        if self.held is None:
            self.held = self._read()
        return self.held

    def next(self):
        tok = self.peek()
        self.held = None
        return tok


def _unexpected(tok):
    raise Fail(UNSUPPORTED if tok[0] == "word" else MISSING)


def _expect(tk, what):
    tok = tk.next()
    if tok[0] != what:
        _unexpected(tok)


def at_rounding_boundary(tok: bytes):
    """a literal of more than 19 significant digits whose first 19, and those plus one unit, round to
    different doubles: the device path does not take it (GF_CSV_UNSUPPORTED, as in gf_csv_parse)"""
    m = re.match(rb"[+-]?(\d*)\.?(\d*)(?:[eE]([+-]?\d+))?\Z", tok)
    digits = (m.group(1) + m.group(2)).lstrip(b"0")
    if len(digits) <= 19 or not digits[19:].strip(b"0"):
        return False
    q = len(digits) - 19 - len(m.group(2)) + int(m.group(3) or 0)
    w = int(digits[:19])
    return float(f"{w}e{q}") != float(f"{w + 1}e{q}")


def _number(tk):
    tok = tk.next()
    if tok[0] != "num":
        _unexpected(tok)
    if not _JAVA_DOUBLE.match(tok[1]):
        raise Fail(NUMBER_FORMAT)
    if at_rounding_boundary(tok[1]):
        raise Fail(UNSUPPORTED)
    return float(tok[1])  # Double.parseDouble: correctly rounded, as Python's float()


def _position(tk):
    x = _number(tk)
    y = _number(tk)
    if tk.peek()[0] == "num":
        raise Fail(UNSUPPORTED)  # a third ordinate
    return (x, y)


def _chain(tk, least):
    _expect(tk, "(")
    out = [_position(tk)]
    while tk.peek()[0] == ",":
        tk.next()
        out.append(_position(tk))
    _expect(tk, ")")
    if len(out) < least:
        raise Fail(MISSING)  # LinearRing / LineString: IllegalArgumentException
    return out


def _list(tk, member):
    _expect(tk, "(")
    out = [member(tk)]
    while tk.peek()[0] == ",":
        tk.next()
        out.append(member(tk))
    _expect(tk, ")")
    return out


def _polygon(tk):
    return _list(tk, lambda t: _chain(t, 4))


def read_geometry(text, multi, kind):
    """WKTReader.read of the text after the tag -> the geometry's members"""
    tk = Tokens(text)
    i = 0
    while i < len(text) and text[i] in b" \t":
        i += 1
    if i >= len(text):
        raise Fail(MISSING)
    if text[i] != 0x28:
        raise Fail(UNSUPPORTED)  # Z / M / EMPTY / a run-on tag
    if kind == POINT:
        _expect(tk, "(")
        p = _position(tk)
        _expect(tk, ")")
        return p
    if kind == POLYGON:
        polys = _list(tk, _polygon) if multi else [_polygon(tk)]
        for poly in polys:
            for ring in poly:
                if ring[0] != ring[-1]:  # equals2D: -0.0 closes 0.0
                    raise Fail(MISSING)
        return polys
    return _list(tk, lambda t: _chain(t, 2)) if multi else [_chain(tk, 2)]


def parse_date(field, tz_off_min):
    """SimpleDateFormat("yyyy-MM-dd HH:mm:ss").parse(field) (lenient, a prefix): ms, or None on a
    ParseException"""
    m = _DATE.match(field)
    if not m:
        return None
    if any(len(g) >= 10 for g in m.groups()):
        raise Fail(UNSUPPORTED)
    f = [int(g) for g in m.groups()]
    y, mo = f[0] + (f[1] - 1) // 12, (f[1] - 1) % 12 + 1
    if y < 1:
        raise Fail(UNSUPPORTED)
    secs = calendar.timegm((y, mo, 1, 0, 0, 0)) + (f[2] - 1) * 86400 + f[3] * 3600 + f[4] * 60 + f[5]
    if secs < -12219292800:  # Java's Julian calendar
        raise Fail(UNSUPPORTED)
    return secs * 1000 - tz_off_min * 60000


def fields_of(line, delimiter):
    """Arrays.asList(str.replace("\\"", "").split("\\\\s*" + delimiter + "\\\\s*"))"""
    parts = re.split(rb"\s*" + re.escape(delimiter) + rb"\s*", line.replace(b'"', b""))
    while parts and parts[-1] == b"":
        parts.pop()
    return parts


def wkt_line(line: bytes, kind, delimiter=None, date_fmt=0, tz_off_min=0):
    if line.endswith(b"\r"):
        line = line[:-1]
    if not line:
        return None, EMPTY
    multi_tag, tag = TAGS[kind]
    try:
        oid, ts = None, 0
        if delimiter is not None and kind != POINT:
            fields = fields_of(line, delimiter)
            if not fields:
                raise Fail(MISSING)  # get(0): IndexOutOfBoundsException
            f0 = fields[0].strip(_TRIM)
            if not f0.startswith(tag) and not f0.startswith(multi_tag):
                oid = f0
            if date_fmt:
                for f in reversed(fields):
                    t = parse_date(f.strip(_TRIM), tz_off_min)
                    if t is not None:
                        ts = t
                        break
        pos = line.find(multi_tag) if multi_tag else -1
        multi = pos >= 0
        if not multi:
            pos = line.find(tag)
            if pos < 0:
                raise Fail(MISSING)  # substring(-1)
        geom = read_geometry(line[pos + len(multi_tag if multi else tag):], multi, kind)
    except Fail as f:
        return None, f.kind
    if kind == POINT:
        return (geom, None, 0), OK
    if kind == POLYGON:
        if not multi and ts == 0:
            oid = None  # (:577-582) Polygon(list, uGrid)
        return (create_polygon(geom[0]), oid, ts), OK
    return (geom[0], oid, ts), OK


def split_lines(text: bytes):
    lines = text.split(b"\n")
    if lines and lines[-1] == b"" and (text.endswith(b"\n") or not text):
        lines = lines[:-1]
    return lines


def parse(text: bytes, kind, **kw):
    """-> (objects, objIDs, ts, bad_line, bad_kind): the first bad line wins"""
    objs, ids, ts = [], [], []
    for i, ln in enumerate(split_lines(text)):
        r, k = wkt_line(ln, kind, **kw)
        if k:
            return None, None, None, i, k
        objs.append(r[0])
        ids.append(r[1])
        ts.append(r[2])
    return objs, ids, ts, -1, 0
