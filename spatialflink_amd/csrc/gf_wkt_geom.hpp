// gf_wkt_geom.hpp -- the per-line evaluator of the WKT ingest: Deserialization.WKTToSpatial /
// WKTToTSpatial (Deserialization.java:214-232, :261-288), WKTToSpatialPolygon / WKTToTSpatialPolygon
// (:461-490, :524-586), WKTToSpatialLineString / WKTToTSpatialLineString (:748-835) and their
// WKTReader helpers (:1456-1528); contract: include/geoflink_hip.h, gf_wkt_parse_geoms.
// __host__ __device__ as gf_geojson_geom.hpp is: k_wktingest.hip runs it one lane per line, and
// tests/native/wktingest_main.cpp builds the very same code for the host.
//
// Two halves, as the device pipeline has two passes:
//   wkt_line_eval    pass A: the fields (objID, ts) of a T variant, the tag, the canonical grammar
//                    with every number token checked, the counts of the taken object, the byte
//                    position of the geometry's first '(' and its type.  With `values` it also
//                    applies ring closure, so it is the whole contract (the host test build, and
//                    the one lane that names the first bad line's kind).
//   wkt_closed /     pass B: ring closure (first == last), then the taken object's positions parsed
//   wkt_fill         into vx / vy, a polygon's rings in createPolygon order (ring_order).
#pragma once

#include "gf_geojson_geom.hpp"

namespace gf {

constexpr int kWktPoints = 0;  // the point stream, next to GF_GEOM_POLYGON / GF_GEOM_LINESTRING

// what the maps need of the schema (by value, as GeoProps is)
struct WktProps {
  int32_t kind;      // kWktPoints | GF_GEOM_POLYGON | GF_GEOM_LINESTRING
  char delim;        // 0: a non-T map (no field is read)
  int32_t date_fmt;  // 0: dateFormat == null
  int64_t tz_off_ms;
  const uint64_t* pow5;
};

// ---- tokens (JTS's StreamTokenizer set-up, restated for the canonical subset) ---------------------
enum { WK_END, WK_LP, WK_RP, WK_COMMA, WK_NUM, WK_WORD, WK_BADBYTE, WK_OTHER };
GF_DHD inline bool wkt_blank(char c) { return c == ' ' || c == '\t'; }
GF_DHD inline bool wkt_digit(char c) { return c >= '0' && c <= '9'; }
GF_DHD inline bool wkt_numc(char c) { return wkt_digit(c) || c == '+' || c == '-' || c == '.' || c == 'e' || c == 'E'; }
template <class Src>
GF_DHD inline int64_t wkt_skip(const Src& s, int64_t i, int64_t e) {
  while (i < e && wkt_blank(s(i))) ++i;
  return i;
}
// the next token at or after i: its kind, *tb its first byte, i past it.  A word is a maximal run
// of letters, digits and + - . (WK_NUM when all its bytes are 0-9 + - . e E); '#', a byte >= 0x80
// and a control byte other than tab are WK_BADBYTE.
template <class Src>
GF_DHD inline int wkt_tok(const Src& s, int64_t& i, int64_t e, int64_t* tb) {
  i = wkt_skip(s, i, e);
  *tb = i;
  if (i >= e) return WK_END;
  const char c = s(i);
  if (jtok_char(c)) {
    bool num = true;
    while (i < e && jtok_char(s(i))) {
      num &= wkt_numc(s(i));
      ++i;
    }
    return num ? WK_NUM : WK_WORD;
  }
  ++i;
  if (c == '(') return WK_LP;
  if (c == ')') return WK_RP;
  if (c == ',') return WK_COMMA;
  const uint8_t u = (uint8_t)c;
  return c == '#' || u >= 0x80 || u < 0x20 ? WK_BADBYTE : WK_OTHER;
}
// a token where the grammar wants another: outside the subset, or a failure of any WKT reader
GF_DHD inline int wkt_unexpected(int t) { return t == WK_WORD || t == WK_BADBYTE ? kCsvUnsupported : kCsvMissingField; }
// Double.parseDouble of the number token [b, q) accepts it (the value itself is pass B's): over
// these bytes that is [+-]? (digits [. digits*] | . digits) ([eE] [+-]? digits)?.  More than 19
// mantissa digits: parse_java_double decides (a literal at a rounding boundary is unsupported).
template <class Src>
GF_DHD inline int wkt_num_check(const Src& s, int64_t b, int64_t q, const uint64_t* T) {
  int64_t i = b;
  if (s(i) == '+' || s(i) == '-') ++i;
  int64_t nd = 0, d0 = i;
  while (i < q && wkt_digit(s(i))) ++i;
  nd = i - d0;
  if (i < q && s(i) == '.') {
    d0 = ++i;
    while (i < q && wkt_digit(s(i))) ++i;
    nd += i - d0;
  }
  if (nd == 0) return kCsvNumberFormat;
  if (i < q && (s(i) == 'e' || s(i) == 'E')) {
    ++i;
    if (i < q && (s(i) == '+' || s(i) == '-')) ++i;
    d0 = i;
    while (i < q && wkt_digit(s(i))) ++i;
    if (i == d0) return kCsvNumberFormat;
  }
  if (i != q) return kCsvNumberFormat;
  if (nd > 19) {
    double v;
    const int st = parse_java_double(s, Field{b, q}, T, &v);
    if (st) return st == kNumUnsupported ? kCsvUnsupported : kCsvNumberFormat;
  }
  return kCsvOk;
}

// ---- pass A: the grammar (no number values) -----------------------------------------------------
// A position: exactly two number tokens.  One: GF_CSV_MISSING_FIELD; a third: GF_CSV_UNSUPPORTED.
template <class Src>
GF_DHD inline int wkt_pos_check(const Src& s, int64_t& i, int64_t e, const uint64_t* T) {
  int64_t tb = 0;
  int t = wkt_tok(s, i, e, &tb);
  if (t != WK_NUM) return wkt_unexpected(t);
  int st = wkt_num_check(s, tb, i, T);
  if (st) return st;
  t = wkt_tok(s, i, e, &tb);
  if (t != WK_NUM) return wkt_unexpected(t);  // (',' or ')': a position with one number)
  if ((st = wkt_num_check(s, tb, i, T))) return st;
  int64_t j = i;
  return wkt_tok(s, j, e, &tb) == WK_NUM ? (int)kCsvUnsupported : (int)kCsvOk;
}
// '(' position (',' position)* ')' with at least `least` positions (a ring: 4; a linestring: 2)
template <class Src>
GF_DHD inline int wkt_chain_check(const Src& s, int64_t& i, int64_t e, int least, const uint64_t* T, int64_t* count) {
  int64_t tb = 0, n = 0;
  int t = wkt_tok(s, i, e, &tb);
  if (t != WK_LP) return wkt_unexpected(t);
  do {
    const int st = wkt_pos_check(s, i, e, T);
    if (st) return st;
    ++n;
    t = wkt_tok(s, i, e, &tb);
  } while (t == WK_COMMA);
  if (t != WK_RP) return wkt_unexpected(t);
  *count = n;
  return n < least ? kCsvMissingField : kCsvOk;
}
template <class Src>
GF_DHD inline int wkt_poly_check(const Src& s, int64_t& i, int64_t e, const uint64_t* T, int64_t* nrings, int64_t* nverts) {
  int64_t tb = 0, nr = 0, nv = 0;
  int t = wkt_tok(s, i, e, &tb);
  if (t != WK_LP) return wkt_unexpected(t);
  do {
    int64_t n = 0;
    const int st = wkt_chain_check(s, i, e, 4, T, &n);
    if (st) return st;
    ++nr;
    nv += n;
    t = wkt_tok(s, i, e, &tb);
  } while (t == WK_COMMA);
  if (t != WK_RP) return wkt_unexpected(t);
  *nrings = nr;
  *nverts = nv;
  return kCsvOk;
}
// the geometry whose first '(' is at g: every member in document order (JTS builds them all), the
// first one's counts kept
template <class Src>
GF_DHD inline int wkt_struct(const Src& s, int64_t g, int64_t e, int tcode, const uint64_t* T, int64_t* nrings,
                             int64_t* nverts) {
  int64_t i = g, tb = 0;
  *nrings = 0;
  if (tcode == kTyPolygon) return wkt_poly_check(s, i, e, T, nrings, nverts);
  if (tcode == kTyLineString) return wkt_chain_check(s, i, e, 2, T, nverts);
  if (tcode == kTyPoint) {  // '(' position ')'
    int t = wkt_tok(s, i, e, &tb);
    if (t != WK_LP) return wkt_unexpected(t);
    const int st = wkt_pos_check(s, i, e, T);
    if (st) return st;
    *nverts = 1;
    t = wkt_tok(s, i, e, &tb);
    return t == WK_RP ? (int)kCsvOk : wkt_unexpected(t);
  }
  const bool poly = tcode == kTyMultiPolygon;
  int t = wkt_tok(s, i, e, &tb);  // (the caller saw the '(')
  bool first = true;
  do {
    int64_t nr = 0, nv = 0;
    const int st = poly ? wkt_poly_check(s, i, e, T, &nr, &nv) : wkt_chain_check(s, i, e, 2, T, &nv);
    if (st) return st;
    if (first) {
      *nrings = nr;
      *nverts = nv;
      first = false;
    }
    t = wkt_tok(s, i, e, &tb);
  } while (t == WK_COMMA);
  return t == WK_RP ? (int)kCsvOk : wkt_unexpected(t);
}

// ---- values: positions of a geometry whose structure passed -----------------------------------------
// the position at i (its first number's first byte) -> x, y; returns the index past the second number
template <class Src>
GF_DHD inline int64_t wkt_pos_read(const Src& s, int64_t i, int64_t e, const uint64_t* T, double* x, double* y) {
  int64_t q = i;
  while (q < e && wkt_numc(s(q))) ++q;
  parse_java_double(s, Field{i, q}, T, x);
  i = wkt_skip(s, q, e);
  q = i;
  while (q < e && wkt_numc(s(q))) ++q;
  parse_java_double(s, Field{i, q}, T, y);
  return q;
}
// past the position at i, unread
template <class Src>
GF_DHD inline int64_t wkt_pos_skip(const Src& s, int64_t i, int64_t e) {
  while (i < e && wkt_numc(s(i))) ++i;
  i = wkt_skip(s, i, e);
  while (i < e && wkt_numc(s(i))) ++i;
  return i;
}
// the next member of a list after the one ending at ve: its first byte, or the list's ')'
template <class Src>
GF_DHD inline int64_t wkt_next(const Src& s, int64_t ve, int64_t e) {
  int64_t i = wkt_skip(s, ve, e);
  if (i < e && s(i) == ',') i = wkt_skip(s, i + 1, e);
  return i;
}
// the ring at p (its '('): first == last (Coordinate.equals2D on the parsed doubles).  *end = past it.
template <class Src>
GF_DHD inline bool wkt_ring_closed(const Src& s, int64_t p, int64_t e, const uint64_t* T, int64_t* end) {
  int64_t i = wkt_skip(s, p + 1, e), last = i;
  double x0, y0, x1, y1;
  wkt_pos_read(s, i, e, T, &x0, &y0);
  while (s(i) != ')') {
    last = i;
    i = wkt_next(s, wkt_pos_skip(s, i, e), e);
  }
  wkt_pos_read(s, last, e, T, &x1, &y1);
  *end = i + 1;
  return x0 == x1 && y0 == y1;
}
template <class Src>
GF_DHD inline bool wkt_poly_closed(const Src& s, int64_t p, int64_t e, const uint64_t* T, int64_t* end) {
  int64_t i = wkt_skip(s, p + 1, e);
  while (s(i) != ')') {
    int64_t re = 0;
    if (!wkt_ring_closed(s, i, e, T, &re)) return false;
    i = wkt_next(s, re, e);
  }
  *end = i + 1;
  return true;
}
// every ring of the geometry (of every polygon of a MULTIPOLYGON) is closed; the rest: true
template <class Src>
GF_DHD inline bool wkt_closed(const Src& s, int64_t g, int64_t e, int tcode, const uint64_t* T) {
  int64_t end = 0;
  if (tcode == kTyPolygon) return wkt_poly_closed(s, g, e, T, &end);
  if (tcode != kTyMultiPolygon) return true;
  int64_t i = wkt_skip(s, g + 1, e);
  while (s(i) != ')') {
    if (!wkt_poly_closed(s, i, e, T, &end)) return false;
    i = wkt_next(s, end, e);
  }
  return true;
}
// the chain at p into x[0..), y[0..) (null: counted only); returns its positions; *area2 = the
// shoelace sum of gchain_read (the same expression, the same order), *end = past the chain
template <class Src>
GF_DHD inline int32_t wkt_chain_read(const Src& s, int64_t p, int64_t e, const uint64_t* T, double* x, double* y,
                                     double* area2, int64_t* end) {
  int64_t i = wkt_skip(s, p + 1, e);
  int32_t n = 0;
  double a = 0.0, px = 0.0, py = 0.0;
  while (s(i) != ')') {
    double cx, cy;
    const int64_t pe = wkt_pos_read(s, i, e, T, &cx, &cy);
    if (x) {
      x[n] = cx;
      y[n] = cy;
    }
    if (n > 0) a += px * cy - cx * py;
    px = cx;
    py = cy;
    ++n;
    i = wkt_next(s, pe, e);
  }
  *area2 = a;
  *end = i + 1;
  return n;
}
// The taken object of a good line (closure checked) -> vx / vy at vbase; a polygon's rings in
// createPolygon order with their starts in voff[0 .. nrings) (geom_fill's twin over WKT text).
template <class Src>
GF_DHD inline void wkt_fill(const Src& s, int64_t e, const GeomNote& n, const uint64_t* T, int32_t vbase, int32_t* voff,
                            const RingTmp& t, double* vx, double* vy) {
  const bool multi = n.tcode == kTyMultiPolygon || n.tcode == kTyMultiLineString;
  const int64_t op = multi ? wkt_skip(s, n.cpos + 1, e) : n.cpos;
  double a2 = 0.0;
  int64_t end = 0;
  if (n.nrings == 0) {  // a linestring
    wkt_chain_read(s, op, e, T, vx + vbase, vy + vbase, &a2, &end);
    return;
  }
  if (n.nrings == 1) {  // one ring is taken as is
    voff[0] = vbase;
    wkt_chain_read(s, wkt_skip(s, op + 1, e), e, T, vx + vbase, vy + vbase, &a2, &end);
    return;
  }
  int64_t i = wkt_skip(s, op + 1, e);
  for (int32_t r = 0; r < n.nrings; ++r) {
    t.start[r] = i;
    t.count[r] = wkt_chain_read(s, i, e, T, (double*)nullptr, (double*)nullptr, &a2, &end);
    t.area[r] = (a2 < 0.0 ? -a2 : a2) / 2.0;
    i = wkt_next(s, end, e);
  }
  ring_order(t, n.nrings);
  int32_t off = vbase;
  for (int32_t k = 0; k < n.nrings; ++k) {
    const int32_t r = t.order[k];
    voff[k] = off;
    wkt_chain_read(s, t.start[r], e, T, vx + off, vy + off, &a2, &end);
    off += t.count[r];
  }
}

// ---- the tag ------------------------------------------------------------------------------------
// str.indexOf(MULTI<tag>) if it occurs, else str.indexOf(<tag>) (points: "POINT" only): the first
// occurrence of <tag> that "MULTI" precedes, else the first one.  -1: none (substring(-1) throws).
template <class Src>
GF_DHD inline int64_t wkt_find_tag(const Src& s, int64_t b, int64_t e, int kind, int* tcode, int64_t* after) {
  const char* w = kind == GF_GEOM_POLYGON ? "POLYGON" : kind == GF_GEOM_LINESTRING ? "LINESTRING" : "POINT";
  const int wl = kind == GF_GEOM_POLYGON ? 7 : kind == GF_GEOM_LINESTRING ? 10 : 5;
  const char* mu = "MULTI";
  int64_t first = -1;
  for (int64_t i = b; i + wl <= e; ++i) {
    if (s(i) != w[0]) continue;
    bool m = true;
    for (int k = 1; m && k < wl; ++k) m = s(i + k) == w[k];
    if (!m) continue;
    if (kind == kWktPoints) {
      first = i;
      break;
    }
    bool mm = i - 5 >= b;
    for (int k = 0; mm && k < 5; ++k) mm = s(i - 5 + k) == mu[k];
    if (mm) {
      *tcode = kind == GF_GEOM_POLYGON ? kTyMultiPolygon : kTyMultiLineString;
      *after = i + wl;
      return i - 5;
    }
    if (first < 0) first = i;
  }
  *tcode = kind == GF_GEOM_POLYGON ? kTyPolygon : kind == GF_GEOM_LINESTRING ? kTyLineString : kTyPoint;
  *after = first + wl;
  return first;
}

// ---- the fields of a T variant ----------------------------------------------------------------------
GF_DHD inline bool wkt_regex_s(char c) {  // regex \s: [ \t\n\x0B\f\r]
  return c == ' ' || c == '\t' || c == '\n' || c == '\x0B' || c == '\f' || c == '\r';
}
GF_DHD inline bool wkt_sepc(char c) { return wkt_regex_s(c) || c == '"'; }  // ('"' is removed before the split)
// the bytes [b, e) with every '"' removed, read front to back (indices never decrease); 0 past the end
template <class Src>
struct WktUnquoted {
  const Src& s;
  int64_t e;
  mutable int64_t li, pi;
  GF_DHD WktUnquoted(const Src& src, int64_t b, int64_t end) : s(src), e(end), li(0), pi(b) { settle(); }
  GF_DHD void settle() const {
    while (pi < e && s(pi) == '"') ++pi;
  }
  GF_DHD char operator()(int64_t i) const {
    while (li < i && pi < e) {
      ++li;
      ++pi;
      settle();
    }
    return pi < e ? s(pi) : '\0';
  }
};
// Java trim() of a field of the line without its '"'
template <class Src>
GF_DHD inline Field wkt_trim(const Src& s, int64_t b, int64_t e) {
  while (b < e && (s(b) == '"' || java_ws(s(b)))) ++b;
  while (e > b && (s(e - 1) == '"' || java_ws(s(e - 1)))) --e;
  return Field{b, e};
}
// end of field 0 of split("\\s*" + d + "\\s*") over [b, e): the first separator's first byte (e: none)
template <class Src>
GF_DHD inline int64_t wkt_field0_end(const Src& s, int64_t b, int64_t e, char d) {
  if (!wkt_regex_s(d)) {
    int64_t i = b;
    while (i < e && s(i) != d) ++i;
    return i;
  }
  for (int64_t i = b; i < e;) {  // a whitespace delimiter: a run of whitespace holding it is one separator
    if (!wkt_sepc(s(i))) {
      ++i;
      continue;
    }
    int64_t j = i;
    bool hd = false;
    while (j < e && wkt_sepc(s(j))) {
      hd |= s(j) == d;
      ++j;
    }
    if (hd) return i;
    i = j;
  }
  return e;
}
// the field that ends at fe, walking back: its first byte; *sep = the first byte of the separator
// before it (-1: it is field 0)
template <class Src>
GF_DHD inline int64_t wkt_field_back(const Src& s, int64_t b, int64_t fe, char d, int64_t* sep) {
  int64_t k = fe;
  *sep = -1;
  if (!wkt_regex_s(d)) {
    while (k > b && s(k - 1) != d) --k;
    if (k > b) *sep = k - 1;
    return k;
  }
  while (k > b) {
    if (!wkt_sepc(s(k - 1))) {
      --k;
      continue;
    }
    int64_t r = k;
    bool hd = false;
    while (r > b && wkt_sepc(s(r - 1))) {
      hd |= s(r - 1) == d;
      --r;
    }
    if (hd) {
      *sep = r;
      return k;
    }
    k = r;
  }
  return b;
}
// objID and ts of a T line (:545-563, :797-812): the line without '"' split by \s*d\s*; objID =
// field 0 trimmed unless it starts with one of the stream's tags; ts = the last field that parses.
template <class Src>
GF_DHD inline int wkt_fields(const WktProps& a, const Src& s, int64_t b, int64_t e, LineOut* o) {
  const Field f0 = wkt_trim(s, b, wkt_field0_end(s, b, e, a.delim));
  const char* w = a.kind == GF_GEOM_POLYGON ? "MULTIPOLYGON" : "MULTILINESTRING";
  const int wl = a.kind == GF_GEOM_POLYGON ? 12 : 15;
  bool tag = false;
  for (int off = 0; !tag && off <= 5; off += 5) {  // startsWith(MULTI<tag>) || startsWith(<tag>)
    const WktUnquoted<Src> u(s, f0.b, f0.e);
    bool m = true;
    for (int k = off; m && k < wl; ++k) m = u(k - off) == w[k];
    tag = m;
  }
  if (!tag) {
    o->dict = !canonical_objid_key(s, f0, &o->obj);
    o->f_obj = f0;
    if (o->dict && f0.e - f0.b > (int64_t)kDictLenMask) return kCsvUnsupported;
  }
  if (a.date_fmt == 0) return kCsvOk;
  for (int64_t fe = e;;) {  // Collections.reverse, the first field that parses
    int64_t sep = -1;
    const int64_t fb = wkt_field_back(s, b, fe, a.delim, &sep);
    const Field f = wkt_trim(s, fb, fe);
    int64_t ms = 0;
    const int st = jdate(WktUnquoted<Src>(s, f.b, f.e), 0, INT64_MAX, a.tz_off_ms, &ms);
    if (st == 2) return kCsvUnsupported;
    if (st == 0) {
      o->ts = ms;
      break;
    }
    if (sep < 0) break;
    fe = sep;
  }
  return kCsvOk;
}

// One line [b, e) (not empty, the trailing '\r' removed).  values: ring closure too (see the top).
// A point line leaves x, y in *o.
template <class Src>
GF_DHD GF_NOINLINE int wkt_line_eval(WktProps a, Src s, int64_t b, int64_t e, bool values, GeomNote* n, LineOut* o) {
  if (e - b >= (int64_t)INT32_MAX) return kCsvUnsupported;
  o->ts = 0;
  o->obj = GF_OBJID_NULL;
  o->dict = false;
  if (a.delim != 0 && a.kind != kWktPoints) {
    const int st = wkt_fields(a, s, b, e, o);
    if (st) return st;
  }
  int tcode = 0;
  int64_t after = 0;
  const int64_t tag = wkt_find_tag(s, b, e, a.kind, &tcode, &after);
  if (tag < 0) return kCsvMissingField;
  const int64_t g = wkt_skip(s, after, e);  // only blanks between the tag and its '('
  if (g >= e) return kCsvMissingField;
  if (s(g) != '(') return kCsvUnsupported;
  int64_t nr = 0, nv = 0;
  const int st = wkt_struct(s, g, e, tcode, a.pow5, &nr, &nv);
  if (st) return st;
  if (tcode == kTyPoint) wkt_pos_read(s, wkt_skip(s, g + 1, e), e, a.pow5, &o->x, &o->y);
  if (values && !wkt_closed(s, g, e, tcode, a.pow5)) return kCsvMissingField;
  // (:577-582) a POLYGON without a time is built by Polygon(list, uGrid): its objID is null
  if (tcode == kTyPolygon && o->ts == 0) {
    o->obj = GF_OBJID_NULL;
    o->dict = false;
  }
  n->tcode = tcode;
  n->nrings = (int32_t)nr;  // (a line is shorter than 2^31 bytes)
  n->nverts = (int32_t)nv;
  n->cpos = g;
  return kCsvOk;
}

}  // namespace gf
