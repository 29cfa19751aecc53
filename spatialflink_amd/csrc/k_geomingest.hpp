// k_geomingest.hpp -- what geomingest.cpp and k_geomingest.hip share: the argument block of the
// GeoJSON geometry-stream ingest (gf_geojson_parse_geoms) and its launchers.
#pragma once

#include "gf_geojson_geom.hpp"
#include "gf_internal.hpp"

namespace gf {

constexpr int kGeomLines = 64;  // lines (= lanes) per block of both passes: one wave
// what the host reads back after pass A + scans, and again after pass B
struct GeomHead {
  unsigned long long newlines;  // found by csv_nlindex (more than nl_cap: the index was cut)
  unsigned long long lines;
  unsigned long long nrings, nverts;  // of the lines that passed
  unsigned long long dict_n, dict_bytes;
  CsvErr err;
};
struct GeomIngestArgs {
  const char* text;
  int64_t len;
  const int64_t* nl;         // newline positions (csv_nlindex)
  const uint32_t* nl_total;  // their count, on the device
  int64_t nl_cap;
  int64_t grid_lines;        // line slots of the per-line arrays below: nl_cap + 1
  int32_t kind;              // GF_GEOM_POLYGON | GF_GEOM_LINESTRING
  int32_t value_lines, len_obj, len_ts, date_fmt;
  int64_t tz_off_ms;
  char prop_obj[kGeoPropMax];
  char prop_ts[kGeoPropMax];
  int32_t lds_cap;           // dynamic LDS staging bytes of a block
  // pass A, per line slot (zero counts for bad lines and for slots past the text's lines)
  uint32_t* cnt_r;           // rings / positions of the taken object
  uint32_t* cnt_v;
  int64_t* cpos;             // the taken "coordinates" array
  int32_t* tcode;            // its geometry type (gf_geojson.hpp kTy*)
  int64_t* ts_s;             // ts and the objID key (dictionary Strings: filled by the dictionary pass)
  int64_t* obj_s;
  const uint32_t* off_r;     // [grid_lines + 1] the exclusive scans of cnt_r / cnt_v
  const uint32_t* off_v;
  CsvErr* err;
  GeomHead* head;            // device; the host copies it out
  DictWork* dict_work;
  uint32_t* dict_n;
  unsigned long long* dict_bytes;
  // pass B: lines [0, limit); fill 0 = closure only (an earlier pass found a bad line at `limit`)
  int32_t fill;
  int64_t limit;
  int32_t* ring_off;
  int32_t* vert_off;
  double* vx;
  double* vy;
  int64_t* objID;
  int64_t* ts;
  RingTmp tmp;               // [ring_cap] each: the rings of polygons with several
};

hipError_t launch_geomingest_a(gf_ctx* ctx, const GeomIngestArgs& a);     // pass A
hipError_t launch_geomingest_head(gf_ctx* ctx, const GeomIngestArgs& a);  // totals, first bad line and its kind
hipError_t launch_geomingest_b(gf_ctx* ctx, const GeomIngestArgs& a);     // pass B

}  // namespace gf
