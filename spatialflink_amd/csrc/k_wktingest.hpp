// k_wktingest.hpp -- what wktingest.cpp and k_wktingest.hip share: the argument blocks of the WKT
// ingest (gf_wkt_parse_geoms, gf_wkt_parse_points) and their launchers.
#pragma once

#include "gf_wkt_geom.hpp"
#include "k_geomingest.hpp"  // GeomHead, kGeomLines: the geometry passes keep k_geomingest.hip's shape

namespace gf {

constexpr int kWktPointLines = 192;  // lines (= lanes) per block of the point kernel: three waves

struct WktIngestArgs {
  const char* text;
  int64_t len;
  const int64_t* nl;         // newline positions (csv_nlindex)
  const uint32_t* nl_total;  // their count, on the device
  int64_t nl_cap;
  int64_t grid_lines;        // line slots of the per-line arrays below: nl_cap + 1
  int32_t kind;              // GF_GEOM_POLYGON | GF_GEOM_LINESTRING
  int32_t delim;             // gf_wkt_schema.delimiter (0: a non-T map)
  int32_t date_fmt;
  int32_t lds_cap;           // dynamic LDS staging bytes of a block
  int64_t tz_off_ms;
  // pass A, per line slot (zero counts for bad lines and for slots past the text's lines)
  uint32_t* cnt_r;           // rings / positions of the taken object
  uint32_t* cnt_v;
  int64_t* gpos;             // the geometry's first '('
  int32_t* tcode;            // its type (gf_geojson.hpp kTy*)
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

struct WktPointArgs {
  const char* text;
  int64_t len;
  const int64_t* nl;
  const uint32_t* nl_total;
  int64_t nl_cap;
  int64_t cap;               // the caller's output capacity in lines
  int64_t grid_lines;        // lines the grid covers: min(nl_cap + 1, cap)
  int32_t lds_cap;
  double* x;
  double* y;
  int64_t* objID;
  int64_t* ts;
  int32_t* cx;               // nullable: fused cell assignment
  int32_t* cy;
  double minX, minY, cl;
  CsvErr* err;
  GeomHead* head;
};

hipError_t launch_wktingest_a(gf_ctx* ctx, const WktIngestArgs& a);     // pass A
hipError_t launch_wktingest_head(gf_ctx* ctx, const WktIngestArgs& a);  // totals, first bad line and its kind
hipError_t launch_wktingest_b(gf_ctx* ctx, const WktIngestArgs& a);     // pass B
hipError_t launch_wkt_points(gf_ctx* ctx, const WktPointArgs& a);       // the point kernel, then its head

}  // namespace gf
