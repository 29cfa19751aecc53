// Test-only stand-alone host program over the per-line evaluator of the WKT ingest
// (spatialflink_amd/csrc/gf_wkt_geom.hpp): the very code k_wktingest.hip runs per lane, compiled for
// the CPU.  tests/test_wktingest_ref.py builds it with -fsanitize=address,undefined and compares every
// line with tests/wktingest_ref.py.  Not part of the product.
//
//   wktingest_main FILE KIND DELIM DATE_FMT TZ_MIN      (KIND 0 points, 1 polygons, 2 linestrings;
//                                                        DELIM: the delimiter's byte value, 0 = a non-T map)
// FILE holds '\n'-separated lines.  Output per line:
//   status statusA nrings nverts ts objID sizes... | xbits ybits ...
// status: the whole contract; statusA: pass A alone (no ring closure), which must pass whatever the
// whole contract passes, with the same counts; objID: "null", "k:<key>" or "s:<hex bytes>" ('"'
// skipped, as the dictionary stores it); sizes: a polygon's ring sizes in window order; the vertices
// as the hex bits of x and y.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../spatialflink_amd/csrc/gf_wkt_geom.hpp"

static const uint64_t kPow5Host[] = {GF_POW5_TABLE};

static uint64_t bits(double v) {
  uint64_t b;
  std::memcpy(&b, &v, sizeof b);
  return b;
}

int main(int argc, char** argv) {
  if (argc != 6) { fprintf(stderr, "usage: see the source\n"); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  std::vector<char> buf;
  char chunk[1 << 16];
  size_t got;
  while ((got = fread(chunk, 1, sizeof chunk, f)) > 0) buf.insert(buf.end(), chunk, chunk + got);
  fclose(f);
  const gf::WktProps wp{atoi(argv[2]), (char)atoi(argv[3]), atoi(argv[4]), (int64_t)atoi(argv[5]) * 60000, kPow5Host};
  // each line in a buffer of exactly its size, so that a read past it is a sanitizer finding
  const int64_t len = (int64_t)buf.size();
  for (int64_t b = 0; b < len;) {
    int64_t nl = b;
    while (nl < len && buf[(size_t)nl] != '\n') ++nl;
    std::vector<char> line(buf.begin() + b, buf.begin() + nl);
    b = nl + 1;
    const gf::GBytes s{line.data()};
    int64_t e = (int64_t)line.size();
    if (e > 0 && s(e - 1) == '\r') --e;
    gf::GeomNote n{0, 0, 0, 0}, na{0, 0, 0, 0};
    gf::LineOut o{0, 0, 0.0, 0.0, false, {0, 0}}, oa = o;
    int st, sta;
    if (e <= 0) {
      st = sta = gf::kCsvEmptyLine;
    } else {
      st = gf::wkt_line_eval(wp, s, 0, e, true, &n, &o);
      sta = gf::wkt_line_eval(wp, s, 0, e, false, &na, &oa);
    }
    if (st == gf::kCsvOk && (sta != gf::kCsvOk || na.nrings != n.nrings || na.nverts != n.nverts || na.cpos != n.cpos ||
                             na.tcode != n.tcode || oa.ts != o.ts || oa.obj != o.obj || oa.dict != o.dict)) {
      fprintf(stderr, "pass A disagrees with the whole contract on a good line\n");
      return 3;
    }
    if (st != gf::kCsvOk) {
      printf("%d %d\n", st, sta);
      continue;
    }
    if (!gf::wkt_closed(s, n.cpos, e, n.tcode, kPow5Host)) { fprintf(stderr, "wkt_closed disagrees\n"); return 3; }
    std::string oid = "null";
    if (o.dict) {
      oid = "s:";
      char h[3];
      for (int64_t i = o.f_obj.b; i < o.f_obj.e; ++i) {
        if (s(i) == '"') continue;
        snprintf(h, sizeof h, "%02x", (unsigned)(unsigned char)s(i));
        oid += h;
      }
    } else if (o.obj != GF_OBJID_NULL) {
      oid = "k:" + std::to_string(o.obj);
    }
    printf("%d %d %d %d %" PRId64 " %s", st, sta, n.nrings, n.nverts, o.ts, oid.c_str());
    if (wp.kind == gf::kWktPoints) {
      printf(" | %016" PRIx64 " %016" PRIx64 "\n", bits(o.x), bits(o.y));
      continue;
    }
    // exactly-sized outputs: pass B must write what pass A counted
    const size_t nr = (size_t)n.nrings;
    std::vector<double> vx((size_t)n.nverts), vy((size_t)n.nverts), area(nr);
    std::vector<int64_t> start(nr);
    std::vector<int32_t> count(nr), order(nr), voff(nr + 1);
    const gf::RingTmp t{area.data(), start.data(), count.data(), order.data()};
    gf::wkt_fill(s, e, n, kPow5Host, 0, voff.data(), t, vx.data(), vy.data());
    voff[nr] = n.nverts;
    for (size_t r = 0; r < nr; ++r) printf(" %d", voff[r + 1] - voff[r]);
    printf(" |");
    for (size_t i = 0; i < vx.size(); ++i) printf(" %016" PRIx64 " %016" PRIx64, bits(vx[i]), bits(vy[i]));
    printf("\n");
  }
  return 0;
}
