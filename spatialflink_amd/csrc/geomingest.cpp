// geomingest.cpp -- host side of the GeoJSON ingest of polygon and linestring streams
// (k_geomingest.hip; contract: include/geoflink_hip.h gf_geojson_parse_geoms).
//
//   newline index (csv_nlindex) -> pass A (one lane per line: everything but the number values, the
//   per-line counts) -> the two exclusive scans -> the head (totals, first bad line and its kind)
//   -> SYNC 1: the host needs the three totals to check the caller's capacities before a vertex is
//   written -> pass B (ring closure, then the positions into vx / vy at the scanned offsets) -> the
//   head again -> SYNC 2: the call is synchronous, and ring closure can still fail a line -> objID
//   Strings that are not canonical decimals -> dictionary keys (objid.cpp; its own syncs, only
//   when such objIDs exist).  A text with more than one line per 32 bytes re-runs the first stage
//   once with a larger index, as gf_csv_parse does.
#define GF_TU_NAME geomingest_cpp
#include "gf_buildtag.hpp"  // first: records this unit's command-line defines

#include <cstring>
#include <string>

#include "gf_host.hpp"
#include "k_geomingest.hpp"

using namespace gf;

constexpr int64_t kGeomMeanLineDefault = 768;  // a Feature record of a 16-gon with 17-digit ordinates

static int32_t geom_lds_cap(int64_t mean) {  // a block's mean-length lines plus a quarter, in 1-KB steps
  const int64_t cap = (mean * kGeomLines * 5 / 4 + 1023) & ~(int64_t)1023;
  return (int32_t)std::min<int64_t>(std::max<int64_t>(cap, 16 * 1024), kCsvLdsMax);
}

static int geom_bad_line(gf_ctx* ctx, const CsvErr& he, int64_t* bad_line, int32_t* bad_kind) {
  if (bad_line) *bad_line = (int64_t)he.line;
  if (bad_kind) *bad_kind = he.kind;
  static const char* what[] = {"ok", "a position's ordinate is not a number",
                               "outside the restated subset (see gf_geojson_parse_geoms)",
                               "malformed JSON / no geometry / a ring or linestring JTS refuses", "empty line"};
  const int k = he.kind >= 0 && he.kind <= 4 ? he.kind : 1;
  return set_err(ctx, GF_ERR_ARG, "gf_geojson_parse_geoms: line " + std::to_string(he.line) + ": " + what[k]);
}

extern "C" int gf_geojson_parse_geoms(gf_ctx* ctx, gf_objid_dict* dict, const char* text, int64_t len,
                                      const gf_geojson_schema* sc, const gf_geoms_out* out, int64_t* nobj,
                                      int64_t* nrings, int64_t* nverts, int64_t* bad_line, int32_t* bad_kind) {
  if (!ctx) return GF_ERR_ARG;
  const char* fn = "gf_geojson_parse_geoms: ";
  if (!sc || (sc->date_format != 0 && sc->date_format != 1) || (sc->value_lines != 0 && sc->value_lines != 1))
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
  GeomIngestArgs a{};
  a.len_obj = a.len_ts = -1;
  for (int k = 0; k < 2; ++k) {
    const char* name = k ? sc->time_property : sc->objid_property;
    if (!name) continue;
    const size_t n = std::strlen(name);
    if (n >= (size_t)kGeoPropMax) return set_err(ctx, GF_ERR_ARG, std::string(fn) + "property name longer than 63 bytes");
    std::memcpy(k ? a.prop_ts : a.prop_obj, name, n);
    (k ? a.len_ts : a.len_obj) = (int32_t)n;
  }
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
  a.text = text;
  a.len = len;
  a.kind = out->kind;
  a.value_lines = sc->value_lines;
  a.date_fmt = sc->date_format;
  a.tz_off_ms = (int64_t)sc->tz_offset_minutes * 60000;
  a.lds_cap = geom_lds_cap(ctx->geom_mean_line > 0 ? ctx->geom_mean_line : kGeomMeanLineDefault);
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
    ar.take(a.cpos, (size_t)G);
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
    GF_HIP_CHECK(ctx, launch_geomingest_a(ctx, a));
    if ((st = scan1(ctx, cnt_r, G, off_r))) return st;
    if ((st = scan1(ctx, cnt_v, G, off_v))) return st;
    GF_HIP_CHECK(ctx, launch_geomingest_head(ctx, a));
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
      GF_HIP_CHECK(ctx, launch_geomingest_b(ctx, a));
      GF_HIP_CHECK(ctx, launch_geomingest_head(ctx, a));
      if ((st = read_scalar_sync(ctx, d_head, &h))) return st;
    }
    return geom_bad_line(ctx, h.err, bad_line, bad_kind);
  }
  if (h.nrings > (unsigned long long)INT32_MAX || h.nverts > (unsigned long long)INT32_MAX)
    return set_err(ctx, GF_ERR_ARG, std::string(fn) + "the window's rings or vertices do not fit int32 offsets");
  *nobj = lines;
  *nrings = (int64_t)h.nrings;
  *nverts = (int64_t)h.nverts;
  ctx->geom_mean_line = (len + lines - 1) / lines;
  if (lines > obj_cap || *nrings > ring_cap || *nverts > vert_cap)
    return set_err(ctx, GF_ERR_CAPACITY, std::string(fn) + "the window exceeds a capacity (counts returned)");
  a.fill = 1;
  a.limit = lines;
  a.lds_cap = geom_lds_cap(ctx->geom_mean_line);
  a.ring_off = out->ring_off;
  a.vert_off = out->vert_off;
  a.vx = out->vx;
  a.vy = out->vy;
  a.objID = out->objID;
  a.ts = out->ts;
  GF_HIP_CHECK(ctx, launch_geomingest_b(ctx, a));
  GF_HIP_CHECK(ctx, launch_geomingest_head(ctx, a));
  if ((st = read_scalar_sync(ctx, d_head, &h))) return st;  // sync 2
  if (h.err.line != ~0ull) return geom_bad_line(ctx, h.err, bad_line, bad_kind);
  // objID Strings that are not canonical decimals: keys from the dictionary (ids in line order)
  const uint32_t nw = (uint32_t)h.dict_n;
  if (nw > 0) {
    if ((st = dict_reserve_table(dict, nw, h.dict_bytes))) return st;
    if ((st = dict_run(dict, text, 1, nw, (uint64_t)lines, out->objID))) return st;
  }
  return GF_OK;
}
