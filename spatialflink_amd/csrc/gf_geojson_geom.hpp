// gf_geojson_geom.hpp -- the per-line evaluator of the GeoJSON geometry-stream ingest
// (Deserialization.GeoJSONToSpatialPolygon / GeoJSONToTSpatialPolygon, Deserialization.java:327-458,
// and the LineString twins, :623-745; contract: include/geoflink_hip.h, gf_geojson_parse_geoms).
// __host__ __device__ as gf_geojson.hpp is: k_geomingest.hip runs it one lane per line, and
// tests/native/geomingest_main.cpp builds the very same code for the host.
//
// Two halves, as the device pipeline has two passes:
//   geom_line_eval   pass A: Jackson's strict parse and the member lookup (jvalidate, geo_walk_find
//                    of gf_geojson.hpp), the choice of the geometry, every rule that needs no number
//                    value, the counts of the taken object, the properties (geo_props).  With
//                    `values` it also applies the one rule that does -- ring closure -- so it is the
//                    whole contract (the host test build, and the one lane that names the first bad
//                    line's kind).
//   geom_closed /    pass B: ring closure (first == last), then the taken object's positions parsed
//   geom_fill        into vx / vy, a polygon's rings in createPolygon order.
#pragma once

#include "gf_geojson.hpp"

namespace gf {

// what pass A keeps of a good line
struct GeomNote {
  int32_t tcode;    // kTyPolygon / kTyMultiPolygon / kTyLineString / kTyMultiLineString
  int32_t nrings;   // rings of the taken polygon (0 for a linestring)
  int32_t nverts;   // positions of the taken polygon / linestring
  int64_t cpos;     // the taken "coordinates" array's '['
};

GF_DHD inline bool jnum_start(char c) { return c == '-' || (c >= '0' && c <= '9'); }
// the next element of an array after the value ending at ve: its first byte, or the array's ']'
template <class Src>
GF_DHD inline int64_t jarr_next(const Src& s, int64_t ve, int64_t e) {
  int64_t i = jskip(s, ve, e);
  if (i < e && s(i) == ',') i = jskip(s, i + 1, e);
  return i;
}
// a number token's value: the correctly rounded double; an integral literal is (double) of its
// long, so "-0" is +0.0 (the line passed jvalidate: every number reads)
template <class Src>
GF_DHD inline double jnum_value(const Src& s, int64_t p, int64_t e, const uint64_t* T, int64_t* end) {
  const int64_t ve = jval_end(s, p, e);
  bool integral = false;
  jnumber(s, p, ve, &integral);
  double v = 0.0;
  parse_java_double(s, Field{p, ve}, T, &v);
  *end = ve;
  return integral && v == 0.0 ? 0.0 : v;
}

// ---- pass A: structure (no number values) -------------------------------------------------
// A position: an array whose ordinates 0 and 1 are numbers (else GF_CSV_NUMBER_FORMAT; not an
// array: GF_CSV_MISSING_FIELD) and that has exactly two of them (else GF_CSV_UNSUPPORTED: the
// reference's splitter merges rings after a third ordinate; JTS defaults a missing one).
template <class Src>
GF_DHD inline int gpos_check(const Src& s, int64_t p, int64_t e, int64_t* end) {
  if (s(p) != '[') return kCsvMissingField;
  int64_t i = jskip(s, p + 1, e);
  int n = 0;
  while (i < e && s(i) != ']') {
    if (n < 2 && !jnum_start(s(i))) return kCsvNumberFormat;
    n += n < 3;
    i = jarr_next(s, jval_end(s, i, e), e);
  }
  *end = i + 1;
  return n == 2 ? kCsvOk : kCsvUnsupported;
}
// A chain of positions (a ring: least 4; a linestring: least 2); an empty array is unsupported.
template <class Src>
GF_DHD inline int gchain_check(const Src& s, int64_t p, int64_t e, int least, int64_t* count, int64_t* end) {
  if (s(p) != '[') return kCsvMissingField;
  int64_t i = jskip(s, p + 1, e);
  if (i < e && s(i) == ']') return kCsvUnsupported;
  int64_t n = 0;
  while (i < e && s(i) != ']') {
    int64_t pe = 0;
    const int st = gpos_check(s, i, e, &pe);
    if (st) return st;
    ++n;
    i = jarr_next(s, pe, e);
  }
  *count = n;
  *end = i + 1;
  return n < least ? kCsvMissingField : kCsvOk;
}
template <class Src>
GF_DHD inline int gpoly_check(const Src& s, int64_t p, int64_t e, int64_t* nrings, int64_t* nverts, int64_t* end) {
  if (s(p) != '[') return kCsvMissingField;
  int64_t i = jskip(s, p + 1, e);
  if (i < e && s(i) == ']') return kCsvUnsupported;
  int64_t nr = 0, nv = 0;
  while (i < e && s(i) != ']') {
    int64_t n = 0, re = 0;
    const int st = gchain_check(s, i, e, 4, &n, &re);
    if (st) return st;
    ++nr;
    nv += n;
    i = jarr_next(s, re, e);
  }
  *nrings = nr;
  *nverts = nv;
  *end = i + 1;
  return kCsvOk;
}
// the taken object of a "coordinates" array: the array itself, or a Multi*'s first member
template <class Src>
GF_DHD inline int64_t geom_taken(const Src& s, int64_t cpos, int64_t e, int tcode) {
  return tcode == kTyMultiPolygon || tcode == kTyMultiLineString ? jskip(s, cpos + 1, e) : cpos;
}
// every member in document order (JTS builds them all), the first one's counts kept
template <class Src>
GF_DHD inline int geom_struct(const Src& s, int64_t cpos, int64_t e, int tcode, int64_t* nrings, int64_t* nverts) {
  const bool poly = tcode == kTyPolygon || tcode == kTyMultiPolygon;
  int64_t end = 0, nr = 0, nv = 0;
  if (tcode == kTyPolygon) return gpoly_check(s, cpos, e, nrings, nverts, &end);
  *nrings = 0;
  if (tcode == kTyLineString) return gchain_check(s, cpos, e, 2, nverts, &end);
  int64_t i = jskip(s, cpos + 1, e);
  if (i < e && s(i) == ']') return kCsvUnsupported;
  for (bool first = true; i < e && s(i) != ']'; first = false) {
    const int st = poly ? gpoly_check(s, i, e, &nr, &nv, &end) : gchain_check(s, i, e, 2, &nv, &end);
    if (st) return st;
    if (first) {
      *nrings = nr;
      *nverts = nv;
    }
    i = jarr_next(s, end, e);
  }
  return kCsvOk;
}

// ---- ring closure (values) -----------------------------------------------------------------
template <class Src>
GF_DHD inline int64_t gpos_read(const Src& s, int64_t p, int64_t e, const uint64_t* T, double* x, double* y) {
  int64_t i = jskip(s, p + 1, e), ve = 0;
  *x = jnum_value(s, i, e, T, &ve);
  i = jarr_next(s, ve, e);
  *y = jnum_value(s, i, e, T, &ve);
  return jskip(s, ve, e) + 1;  // past the position's ']'
}
// the ring at p (structure checked): first == last (Coordinate.equals2D: x == x and y == y, so -0.0
// closes 0.0).  *end = past the ring.
template <class Src>
GF_DHD inline bool gring_closed(const Src& s, int64_t p, int64_t e, const uint64_t* T, int64_t* end) {
  int64_t i = jskip(s, p + 1, e), last = i;
  double x0, y0, x1, y1;
  gpos_read(s, i, e, T, &x0, &y0);
  while (s(i) != ']') {
    last = i;
    i = jarr_next(s, jval_end(s, i, e), e);
  }
  gpos_read(s, last, e, T, &x1, &y1);
  *end = i + 1;
  return x0 == x1 && y0 == y1;
}
template <class Src>
GF_DHD inline bool gpoly_closed(const Src& s, int64_t p, int64_t e, const uint64_t* T, int64_t* end) {
  int64_t i = jskip(s, p + 1, e);
  while (s(i) != ']') {
    int64_t re = 0;
    if (!gring_closed(s, i, e, T, &re)) return false;
    i = jarr_next(s, re, e);
  }
  *end = i + 1;
  return true;
}
// every ring of the geometry (of every polygon of a MultiPolygon) is closed; linestrings: true
template <class Src>
GF_DHD inline bool geom_closed(const Src& s, int64_t cpos, int64_t e, int tcode, const uint64_t* T) {
  int64_t end = 0;
  if (tcode == kTyPolygon) return gpoly_closed(s, cpos, e, T, &end);
  if (tcode != kTyMultiPolygon) return true;
  int64_t i = jskip(s, cpos + 1, e);
  while (s(i) != ']') {
    if (!gpoly_closed(s, i, e, T, &end)) return false;
    i = jarr_next(s, end, e);
  }
  return true;
}

// ---- the choice of the geometry ----------------------------------------------------------------
// two members of the (valid) object at obj carry the same name (no name is written with an
// escape: jfind reported that): Jackson keeps the first one's place and the last one's value, so
// the re-serialised text the reference splits is not the text read here
template <class Src>
GF_DHD inline bool jdup_names(const Src& s, int64_t obj, int64_t e) {
  bool esc = false;
  auto after = [&](int64_t ke) {  // past the member whose name ends at ke
    return jskip(s, jval_end(s, jskip(s, jskip(s, ke, e) + 1, e), e), e);
  };
  int64_t p = jskip(s, obj + 1, e);
  while (p < e && s(p) == '"') {
    const int64_t ke = jstr_end(s, p, e, &esc);
    const int64_t nx = after(ke);
    int64_t q = nx;
    while (q < e && s(q) == ',') {
      q = jskip(s, q + 1, e);
      const int64_t qe = jstr_end(s, q, e, &esc);
      bool same = qe - q == ke - p;
      for (int64_t k = 0; same && k < ke - p; ++k) same = s(q + k) == s(p + k);
      if (same) return true;
      q = after(qe);
    }
    if (nx >= e || s(nx) != ',') break;
    p = jskip(s, nx + 1, e);
  }
  return false;
}
GF_DHD inline bool geom_type_allowed(int kind, int t) {
  return kind == GF_GEOM_POLYGON ? (t == kTyPolygon || t == kTyMultiPolygon)
                                 : (t == kTyLineString || t == kTyMultiLineString);
}
// GeoJsonReader.read of the geometry object whose "coordinates" value starts at c (-1: absent) --
// then what the reference's splitter needs of V's text [V, c) to read the same array
template <class Src>
GF_DHD inline int geom_build(const Src& s, int64_t V, int64_t c, int64_t e, int tcode, bool values, const uint64_t* T,
                             GeomNote* o) {
  if (c < 0 || s(c) != '[') return kCsvMissingField;
  for (int64_t i = V; i < c; ++i) {  // the splitter starts at V's first '[' (an escape may hide one)
    const char b = s(i);
    if (b == '[' || b == ']' || b == '\\') return kCsvUnsupported;
  }
  int64_t nr = 0, nv = 0;
  const int st = geom_struct(s, c, e, tcode, &nr, &nv);
  if (st) return st;
  if (values && !geom_closed(s, c, e, tcode, T)) return kCsvMissingField;
  o->tcode = tcode;
  o->nrings = (int32_t)nr;  // (a line is shorter than 2^31 bytes: geom_line_eval)
  o->nverts = (int32_t)nv;
  o->cpos = c;
  return kCsvOk;
}

// steps 2-3 of the maps over located members (gf_geojson.hpp GeoPos), in the maps' order
template <class Src>
GF_DHD inline int geom_eval_body(const GeoProps& a, const Src& s, int64_t e, const GeoPos& g, int kind, bool values,
                                 GeomNote* n, LineOut* o) {
  if (g.V < 0 || s(g.V) != '{') return kCsvMissingField;  // value.toString() / .get("geometry"): NPE
  if (g.escV) return kCsvUnsupported;
  if (jdup_names(s, g.V, e)) return kCsvUnsupported;
  o->ts = 0;
  o->obj = GF_OBJID_NULL;
  o->dict = false;
  const int tv = geo_type_full(s, g.tV, e);
  if (tv == kTyFeatureColl || tv == kTyEscaped) return kCsvUnsupported;
  const bool own = tv == kTyPoint || tv >= kTyLineString;  // V's own "type" names a geometry
  bool have = false;
  if (own) {  // readGeoJSON(value.toString())
    if (!geom_type_allowed(kind, tv)) return kCsvUnsupported;
    const int st = geom_build(s, g.V, g.cV, e, tv, values, a.pow5, n);
    if (st == kCsvUnsupported) return st;
    have = st == kCsvOk;
  }
  if (!have) {  // the catch branch: readGeoJSON(value.get("geometry").toString())
    if (g.gV < 0 || s(g.gV) != '{') return kCsvMissingField;
    if (g.escG) return kCsvUnsupported;
    if (jdup_names(s, g.gV, e)) return kCsvUnsupported;
    const int tg = geo_type_full(s, g.tG, e);
    if (tg == kTyNone) return kCsvMissingField;
    if (!geom_type_allowed(kind, tg)) return kCsvUnsupported;
    const int st = geom_build(s, g.V, g.cG, e, tg, values, a.pow5, n);
    if (st) return st;
    if (own) return kCsvUnsupported;  // the splitter still reads V's own first bracket
  }
  if (g.prV < 0 || s(g.prV) != '{') return kCsvOk;
  if (g.escP && (a.len_ts >= 0 || a.len_obj >= 0)) return kCsvUnsupported;
  return geo_props(a, s, e, g.tsP, g.qP, o);
}

// One line [p, e) (s(p) == '{', trailing '\r' removed).  values: ring closure too (see the top).
template <class Src>
GF_DHD GF_NOINLINE int geom_line_eval(GeoProps a, Src s, int64_t p, int64_t e, int vlines, int kind, bool values,
                                      GeomNote* n, LineOut* o) {
  if (e - p >= (int64_t)INT32_MAX) return kCsvUnsupported;
  const int vs = jvalidate(s, p, e, a.pow5);
  if (vs) return vs;
  GeoPos g;
  const int fs = geo_walk_find(a, s, p, e, vlines, &g);
  if (fs) return fs;
  return geom_eval_body(a, s, e, g, kind, values, n, o);
}

// ---- pass B: the positions ---------------------------------------------------------------------
// the chain at p into x[0..), y[0..) (null: counted only); returns its positions; *area2 = the
// shoelace sum of spatialObjects.Polygon's ring area (x1*y2 - x2*y1 in ring order, fp64, no
// contraction), *end = past the chain
template <class Src>
GF_DHD inline int32_t gchain_read(const Src& s, int64_t p, int64_t e, const uint64_t* T, double* x, double* y,
                                  double* area2, int64_t* end) {
  int64_t i = jskip(s, p + 1, e);
  int32_t n = 0;
  double a = 0.0, px = 0.0, py = 0.0;
  while (s(i) != ']') {
    double cx, cy;
    const int64_t pe = gpos_read(s, i, e, T, &cx, &cy);
    if (x) {
      x[n] = cx;
      y[n] = cy;
    }
    if (n > 0) a += px * cy - cx * py;
    px = cx;
    py = cy;
    ++n;
    i = jarr_next(s, pe, e);
  }
  *area2 = a;
  *end = i + 1;
  return n;
}
// per-ring working arrays of one polygon (device scratch / host vectors), nrings entries each
struct RingTmp {
  double* area;    // abs(shoelace) / 2
  int64_t* start;  // the ring's '['
  int32_t* count;
  int32_t* order;  // createPolygonArray's list: ring indices by descending area
};
// t.order = createPolygonArray's list over t.area[0 .. nrings) (shared with the WKT ingest, gf_wkt_geom.hpp)
GF_DHD inline void ring_order(const RingTmp& t, int32_t nrings) {
  int32_t m = 0;
  for (int32_t r = 0; r < nrings; ++r) {
    const double ar = t.area[r];
    if (m == 0 || t.area[t.order[m - 1]] >= ar) {
      t.order[m++] = r;
      continue;
    }
    int32_t at = 0;
    while (at < m && !(t.area[t.order[at]] <= ar)) ++at;  // (found: the last one is smaller; m: an area is NaN)
    for (int32_t k = m; k > at; --k) t.order[k] = t.order[k - 1];
    t.order[at] = r;
    ++m;
  }
}
// The taken object of a good line (closure checked) -> vx / vy at vbase; a polygon's rings in
// createPolygon order (Polygon.java:147-165; several rings: createPolygonArray's insertion rule,
// :115-145 -- a ring is appended while the last area >= its own, else inserted before the first
// ring whose area <= its own) with their starts in voff[0 .. nrings).
template <class Src>
GF_DHD inline void geom_fill(const Src& s, int64_t e, const GeomNote& n, const uint64_t* T, int32_t vbase, int32_t* voff,
                             const RingTmp& t, double* vx, double* vy) {
  const int64_t op = geom_taken(s, n.cpos, e, n.tcode);
  double a2 = 0.0;
  int64_t end = 0;
  if (n.nrings == 0) {  // a linestring
    gchain_read(s, op, e, T, vx + vbase, vy + vbase, &a2, &end);
    return;
  }
  if (n.nrings == 1) {  // one ring is taken as is
    voff[0] = vbase;
    gchain_read(s, jskip(s, op + 1, e), e, T, vx + vbase, vy + vbase, &a2, &end);
    return;
  }
  int64_t i = jskip(s, op + 1, e);
  for (int32_t r = 0; r < n.nrings; ++r) {
    t.start[r] = i;
    t.count[r] = gchain_read(s, i, e, T, (double*)nullptr, (double*)nullptr, &a2, &end);
    t.area[r] = (a2 < 0.0 ? -a2 : a2) / 2.0;
    i = jarr_next(s, end, e);
  }
  ring_order(t, n.nrings);
  int32_t off = vbase;
  for (int32_t k = 0; k < n.nrings; ++k) {
    const int32_t r = t.order[k];
    voff[k] = off;
    gchain_read(s, t.start[r], e, T, vx + off, vy + off, &a2, &end);
    off += t.count[r];
  }
}

}  // namespace gf
