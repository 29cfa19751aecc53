// wktingest.cpp -- host side of the WKT ingest of point, polygon and linestring streams
// (k_wktingest.hip; contract: include/geoflink_hip.h gf_wkt_parse_geoms, gf_wkt_parse_points).
//
// The geometry streams follow geomingest.cpp's protocol step by step:
//   newline index (csv_nlindex) -> pass A (one lane per line: fields, tag, grammar, the per-line
//   counts) -> the two exclusive scans -> the head (totals, first bad line and its kind) -> SYNC 1:
//   the host needs the three totals to check the caller's capacities before a vertex is written ->
//   pass B (ring closure, then the positions into vx / vy at the scanned offsets) -> the head again
//   -> SYNC 2 -> objID Strings that are not canonical decimals -> dictionary keys (objid.cpp).
// The point stream is one pass and one sync: index -> points (x, y, cell) -> head.  A text with
// more than one line per 32 bytes re-runs the first stage once with a larger index.
#define GF_TU_NAME wktingest_cpp
#include "gf_buildtag.hpp"  // first: records this unit's command-line defines

#include <string>

#include "gf_host.hpp"
#include "k_wktingest.hpp"

using namespace gf;

constexpr int64_t kWktMeanLineDefault = 640;  // a 16-gon with 17-digit ordinates, an objID and a date
constexpr int64_t kWktPointMeanLineDefault = 48;

static int32_t wkt_lds_cap(int64_t mean, int lines) {  // a block's mean-length lines plus a quarter, in 1-KB steps
  const int64_t cap = (mean * lines * 5 / 4 + 1023) & ~(int64_t)1023;
  return (int32_t)std::min<int64_t>(std::max<int64_t>(cap, 16 * 1024), kCsvLdsMax);
}

static int wkt_bad_line(gf_ctx* ctx, const char* fn, const CsvErr& he, int64_t* bad_line, int32_t* bad_kind) {
  if (bad_line) *bad_line = (int64_t)he.line;
  if (bad_kind) *bad_kind = he.kind;
  static const char* what[] = {"ok", "a number token Double.parseDouble rejects",
                               "outside the canonical WKT subset (see gf_wkt_parse_geoms)",
                               "no tag / malformed WKT / a ring or linestring JTS refuses", "empty line"};
  const int k = he.kind >= 0 && he.kind <= 4 ? he.kind : 1;
  return set_err(ctx, GF_ERR_ARG, std::string(fn) + "line " + std::to_string(he.line) + ": " + what[k]);
}

extern "C" int gf_wkt_parse_geoms(gf_ctx* ctx, gf_objid_dict* dict, const char* text, int64_t len, const gf_wkt_schema* sc,
                                  const gf_geoms_out* out, int64_t* nobj, int64_t* nrings, int64_t* nverts,
                                  int64_t* bad_line, int32_t* bad_kind) {
  if (!ctx) return GF_ERR_ARG;
  const char* fn = "gf_wkt_parse_geoms: ";
  // ('"' is removed from the line before the split, so it can never be the delimiter)
  if (!sc || (sc->date_format != 0 && sc->date_format != 1) || sc->delimiter == '"')
    return set_err(ctx, GF_ERR_ARG, std::string(fn) + "bad schema");
  if (!out || (out->kind != GF_GEOM_POLYGON && out->kind != GF_GEOM_LINESTRING))
    return set_err(ctx, GF_ERR_ARG, std::string(fn) + "kind must be GF_GEOM_POLYGON or GF_GEOM_LINESTRING");
  const bool poly = out->kind == GF_GEOM_POLYGON;
  const int64_t obj_cap = out->obj_cap, ring_cap = poly ? out->ring_cap : 0, vert_cap = out->vert_cap;
  const bool any_cap = obj_cap > 0 || ring_cap > 0 || vert_cap > 0;
  if (!nobj || !nrings || !nverts || len < 0 || (len > 0 && !text) || obj_cap < 0 || out->ring_cap < 0 || vert_cap < 0 ||
      (obj_cap > 0 && (!out->objID || !out->ts)) || (vert_cap > 0 && (!out->vx || !out->vy)) ||
      (any_cap && !out->vert_off) || (poly && any_cap && !out->ring_off))
    return set_err(ctx, GF_ERR_ARG, std::string(fn) + "bad argument");
  if ((uintptr_t)text & 15) return set_err(ctx, GF_ERR_ALIGN, std::string(fn) + "text must be 16-byte aligned");
  if (len >= ((int64_t)1 << 33)) return set_err(ctx, GF_ERR_ARG, std::string(fn) + "text of 8 GiB or more");
  if (dict && dict->ctx != ctx) return set_err(ctx, GF_ERR_ARG, std::string(fn) + "dictionary of another context");
  int st = bind(ctx);
  if (st) return st;
  if (!dict && (st = ctx_dict(ctx, &dict))) return st;
  *nobj = *nrings = *nverts = 0;
  if (bad_line) *bad_line = -1;
  if (bad_kind) *bad_kind = GF_CSV_OK;
  if (len == 0) {  // an empty, valid window
    if (out->vert_off) GF_HIP_CHECK(ctx, hipMemsetAsync(out->vert_off, 0, sizeof(int32_t), ctx->stream));
    if (poly && out->ring_off) GF_HIP_CHECK(ctx, hipMemsetAsync(out->ring_off, 0, sizeof(int32_t), ctx->stream));
    GF_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return GF_OK;
  }
  WktIngestArgs a{};
  a.text = text;
  a.len = len;
  a.kind = out->kind;
  a.delim = (int32_t)(unsigned char)sc->delimiter;
  a.date_fmt = sc->delimiter ? sc->date_format : 0;
  a.tz_off_ms = (int64_t)sc->tz_offset_minutes * 60000;
  a.lds_cap = wkt_lds_cap(ctx->wkt_mean_line[0] > 0 ? ctx->wkt_mean_line[0] : kWktMeanLineDefault, kGeomLines);
  const int64_t nseg = (len + kCsvSeg - 1) / kCsvSeg;
  int64_t nl_cap = len / 32 + 2;
  GeomHead h{};
  GeomHead* d_head = nullptr;
  for (int pass = 0; pass < 2; ++pass) {
    const int64_t G = nl_cap + 1;  // line slots
    Arena ar;
    uint32_t *tot = nullptr, *cnt_r = nullptr, *cnt_v = nullptr, *off_r = nullptr, *off_v = nullptr;
    CsvErr* err = nullptr;
    int64_t* nl = nullptr;
    ar.take(d_head, 1);
    ar.take(tot, 1);
    ar.take(err, 1);
    ar.take(nl, (size_t)nl_cap);
    ar.take(cnt_r, (size_t)G);
    ar.take(cnt_v, (size_t)G);
    ar.take(off_r, (size_t)G + 1);
    ar.take(off_v, (size_t)G + 1);
    ar.take(a.gpos, (size_t)G);
    ar.take(a.tcode, (size_t)G);
    ar.take(a.ts_s, (size_t)G);
    ar.take(a.obj_s, (size_t)G);
    const size_t tmp_n = (size_t)std::max<int64_t>(ring_cap, 1);
    ar.take(a.tmp.area, tmp_n);
    ar.take(a.tmp.start, tmp_n);
    ar.take(a.tmp.count, tmp_n);
    ar.take(a.tmp.order, tmp_n);
    if ((st = ar.alloc(ctx))) return st;
    if ((st = dict_reserve_batch(dict, (uint64_t)G, (uint64_t)G))) return st;  // at most one String per line
    // (the index's first block also resets the error slot and the dictionary counters)
    if ((st = lookback_launch(ctx, nseg, nseg, "launch_csv_nlindex", [&](const ExpandState& es) {
          return launch_csv_nlindex(ctx->stream, text, len, nseg, nl, nl_cap, tot, es, err, dict->counters + 2);
        })))
      return st;
    a.nl = nl;
    a.nl_total = tot;
    a.nl_cap = nl_cap;
    a.grid_lines = G;
    a.cnt_r = cnt_r;
    a.cnt_v = cnt_v;
    a.off_r = off_r;
    a.off_v = off_v;
    a.err = err;
    a.head = d_head;
    a.dict_work = (DictWork*)dict->work[0];
    a.dict_n = (uint32_t*)(dict->counters + 2);
    a.dict_bytes = dict->counters + 3;
    GF_HIP_CHECK(ctx, launch_wktingest_a(ctx, a));
    if ((st = scan1(ctx, cnt_r, G, off_r))) return st;
    if ((st = scan1(ctx, cnt_v, G, off_v))) return st;
    GF_HIP_CHECK(ctx, launch_wktingest_head(ctx, a));
    if ((st = read_scalar_sync(ctx, d_head, &h))) return st;  // sync 1
    if ((int64_t)h.newlines <= nl_cap) break;
    nl_cap = (int64_t)h.newlines + 1;  // short lines: a larger index, the stage again
  }
  const int64_t lines = (int64_t)h.lines;
  if (lines >= (int64_t)INT32_MAX) return set_err(ctx, GF_ERR_ARG, std::string(fn) + "2^31 - 1 lines or more");
  if (h.err.line != ~0ull) {
    // pass A's first bad line: an earlier line may still fail ring closure (pass B, nothing written)
    a.fill = 0;
    a.limit = (int64_t)h.err.line;
    if (a.limit > 0) {
      GF_HIP_CHECK(ctx, launch_wktingest_b(ctx, a));
      GF_HIP_CHECK(ctx, launch_wktingest_head(ctx, a));
      if ((st = read_scalar_sync(ctx, d_head, &h))) return st;
    }
    return wkt_bad_line(ctx, fn, h.err, bad_line, bad_kind);
  }
  if (h.nrings > (unsigned long long)INT32_MAX || h.nverts > (unsigned long long)INT32_MAX)
    return set_err(ctx, GF_ERR_ARG, std::string(fn) + "the window's rings or vertices do not fit int32 offsets");
  *nobj = lines;
  *nrings = (int64_t)h.nrings;
  *nverts = (int64_t)h.nverts;
  ctx->wkt_mean_line[0] = (len + lines - 1) / lines;
  if (lines > obj_cap || *nrings > ring_cap || *nverts > vert_cap)
    return set_err(ctx, GF_ERR_CAPACITY, std::string(fn) + "the window exceeds a capacity (counts returned)");
  a.fill = 1;
  a.limit = lines;
  a.lds_cap = wkt_lds_cap(ctx->wkt_mean_line[0], kGeomLines);
  a.ring_off = out->ring_off;
  a.vert_off = out->vert_off;
  a.vx = out->vx;
  a.vy = out->vy;
  a.objID = out->objID;
  a.ts = out->ts;
  GF_HIP_CHECK(ctx, launch_wktingest_b(ctx, a));
  GF_HIP_CHECK(ctx, launch_wktingest_head(ctx, a));
  if ((st = read_scalar_sync(ctx, d_head, &h))) return st;  // sync 2
  if (h.err.line != ~0ull) return wkt_bad_line(ctx, fn, h.err, bad_line, bad_kind);
  // objID Strings that are not canonical decimals: keys from the dictionary (ids in line order)
  const uint32_t nw = (uint32_t)h.dict_n;
  if (nw > 0) {
    if ((st = dict_reserve_table(dict, nw, h.dict_bytes))) return st;
    if ((st = dict_run(dict, text, 1, nw, (uint64_t)lines, out->objID))) return st;
  }
  return GF_OK;
}

extern "C" int gf_wkt_parse_points(gf_ctx* ctx, const char* text, int64_t len, const gf_grid* g, double* x, double* y,
                                   int64_t* objID, int64_t* ts, int32_t* cx, int32_t* cy, int64_t cap, int64_t* n_out,
                                   int64_t* bad_line, int32_t* bad_kind) {
  if (!ctx) return GF_ERR_ARG;
  const char* fn = "gf_wkt_parse_points: ";
  if (!n_out || len < 0 || (len > 0 && !text) || cap < 0 || !x || !y || !objID || !ts || (!cx) != (!cy) || (cx && !g))
    return set_err(ctx, GF_ERR_ARG, std::string(fn) + "bad argument");
  if (g && !(g->n > 0 && g->cellLength > 0)) return set_err(ctx, GF_ERR_ARG, std::string(fn) + "bad grid");
  if ((uintptr_t)text & 15) return set_err(ctx, GF_ERR_ALIGN, std::string(fn) + "text must be 16-byte aligned");
  if (len >= ((int64_t)1 << 33)) return set_err(ctx, GF_ERR_ARG, std::string(fn) + "text of 8 GiB or more");
  int st = bind(ctx);
  if (st) return st;
  *n_out = 0;
  if (bad_line) *bad_line = -1;
  if (bad_kind) *bad_kind = GF_CSV_OK;
  if (len == 0) return GF_OK;
  WktPointArgs a{};
  a.text = text;
  a.len = len;
  a.cap = cap;
  a.x = x;
  a.y = y;
  a.objID = objID;
  a.ts = ts;
  a.cx = cx;
  a.cy = cy;
  if (g) {
    a.minX = g->minX;
    a.minY = g->minY;
    a.cl = g->cellLength;
  }
  a.lds_cap = wkt_lds_cap(ctx->wkt_mean_line[1] > 0 ? ctx->wkt_mean_line[1] : kWktPointMeanLineDefault, kWktPointLines);
  const int64_t nseg = (len + kCsvSeg - 1) / kCsvSeg;
  int64_t nl_cap = len / 32 + 2;
  GeomHead h{};
  for (int pass = 0; pass < 2; ++pass) {
    Arena ar;
    uint32_t* tot = nullptr;
    unsigned long long* unused = nullptr;  // (the index resets two dictionary counters: none here)
    int64_t* nl = nullptr;
    ar.take(a.head, 1);
    ar.take(tot, 1);
    ar.take(a.err, 1);
    ar.take(unused, 2);
    ar.take(nl, (size_t)nl_cap);
    if ((st = ar.alloc(ctx))) return st;
    if ((st = lookback_launch(ctx, nseg, nseg, "launch_csv_nlindex", [&](const ExpandState& es) {
          return launch_csv_nlindex(ctx->stream, text, len, nseg, nl, nl_cap, tot, es, a.err, unused);
        })))
      return st;
    a.nl = nl;
    a.nl_total = tot;
    a.nl_cap = nl_cap;
    a.grid_lines = std::min<int64_t>(nl_cap + 1, cap);
    GF_HIP_CHECK(ctx, launch_wkt_points(ctx, a));
    if ((st = read_scalar_sync(ctx, a.head, &h))) return st;  // the call's one sync
    if ((int64_t)h.newlines <= nl_cap) break;
    nl_cap = (int64_t)h.newlines + 1;  // short lines: a larger index, the call again (nothing was written)
  }
  const int64_t lines = (int64_t)h.lines;
  *n_out = lines;
  if (lines > cap) return set_err(ctx, GF_ERR_CAPACITY, std::string(fn) + "more lines than capacity");
  if (lines > (int64_t)UINT32_MAX) return set_err(ctx, GF_ERR_ARG, std::string(fn) + "more than 2^32-1 lines");
  if (lines > 0) ctx->wkt_mean_line[1] = (len + lines - 1) / lines;
  if (h.err.line != ~0ull) return wkt_bad_line(ctx, fn, h.err, bad_line, bad_kind);
  return GF_OK;
}
