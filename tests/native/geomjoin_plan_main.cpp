// Test-only stand-alone host program over the cell arithmetic of the geometry-stream joins
// (spatialflink_amd/csrc/gf_geomjoin_plan.hpp).  It reads one check per line from standard input, each
// carrying the value tests/geomjoin_ref.py computed with Python's unbounded integers, and holds the header's
// functions to it:
//   M ro[4] rq[4] c n whole out  ->  eq[4] m        join_expand, join_multiplicity
//   T n c requested              ->  shift nt       join_tile_shift, join_tiles_side
//   R ro[4] eq[4] shift nt       ->  ref covered    join_ref_tile, join_tiles_covered(eq)
//   C ro[4] rq[4] c n whole out shift long_tiles brute  ->  class_o class_q
// tests/test_geomjoin_ref.py builds it with -fsanitize=address,undefined (signed overflow in an area or a
// sum would stop it) and feeds it rectangles up to the saturated indices.  Not part of the product.
// Prints "ok <checks>"; a mismatch ends it with status 3.
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "../../spatialflink_amd/csrc/gf_geomjoin_plan.hpp"

static bool read_rect(const char*& s, gf::JoinRect& r) {
  int n = 0;
  int64_t v[4];
  if (sscanf(s, " %" SCNd64 " %" SCNd64 " %" SCNd64 " %" SCNd64 "%n", &v[0], &v[1], &v[2], &v[3], &n) != 4) return false;
  s += n;
  r = gf::JoinRect{v[0], v[1], v[2], v[3]};
  return true;
}
static bool read_ints(const char*& s, int64_t* v, int count) {
  for (int i = 0; i < count; ++i) {
    int n = 0;
    if (sscanf(s, " %" SCNd64 "%n", &v[i], &n) != 1) return false;
    s += n;
  }
  return true;
}
static bool same(const gf::JoinRect& a, const gf::JoinRect& b) {
  if (gf::join_empty(a) && gf::join_empty(b)) return true;
  return a.x1 == b.x1 && a.y1 == b.y1 && a.x2 == b.x2 && a.y2 == b.y2;
}

int main() {
  char line[512];
  long checks = 0;
  while (fgets(line, sizeof line, stdin)) {
    const char* s = line + 1;
    gf::JoinRect ro, rq, eq, want;
    int64_t v[8];
    bool ok = false;
    switch (line[0]) {
      case 'M':
        if (!read_rect(s, ro) || !read_rect(s, rq) || !read_ints(s, v, 4) || !read_rect(s, want) || !read_ints(s, v + 4, 1)) break;
        eq = gf::join_expand(rq, v[0], (int32_t)v[1], v[2] != 0);
        ok = same(eq, want) && (int64_t)gf::join_multiplicity(ro, eq, rq, v[3] != 0, (int32_t)v[1]) == v[4];
        break;
      case 'T':
        if (!read_ints(s, v, 5)) break;
        ok = gf::join_tile_shift((int32_t)v[0], v[1], v[2]) == v[3] &&
             gf::join_tiles_side((int32_t)v[0], (int32_t)v[3]) == v[4];
        break;
      case 'R':
        if (!read_rect(s, ro) || !read_rect(s, eq) || !read_ints(s, v, 4)) break;
        ok = gf::join_ref_tile(ro, eq, (int32_t)v[0], v[1]) == v[2] && gf::join_tiles_covered(eq, (int32_t)v[0]) == v[3];
        break;
      case 'C':
        if (!read_rect(s, ro) || !read_rect(s, rq) || !read_ints(s, v, 7)) break;
        {
          int64_t w[2];
          if (!read_ints(s, w, 2)) break;
          eq = gf::join_expand(rq, v[0], (int32_t)v[1], v[2] != 0);
          ok = gf::join_class_object(ro, (int32_t)v[1], (int32_t)v[4], v[5], v[6] != 0) == w[0] &&
               gf::join_class_query(rq, eq, v[3] != 0, (int32_t)v[1], (int32_t)v[4], v[5], v[6] != 0) == w[1];
        }
        break;
      default:
        break;
    }
    if (!ok) {
      fprintf(stderr, "check failed: %s", line);
      return 3;
    }
    ++checks;
  }
  printf("ok %ld\n", checks);
  return 0;
}
