// Test-only stand-alone host program over the pure host part of a geometry-window query
// (spatialflink_amd/csrc/gf_geom_plan.hpp): reads grids, query cells and cell rectangles from the file
// named on the command line, builds the summed-area tables, checks them against a brute-force count of
// its own and prints the rectangle sums.  tests/test_geomwin_ref.py builds it with
// -fsanitize=address,undefined and compares the sums with its own.  Not part of the product.
//
// Input (whitespace separated integers): the number of sets, then per set
//   n nq g_layers c_layers whole_n, nq pairs qcx qcy, nrect, nrect quadruples x1 y1 x2 y2.
// Output per set: "status cellsN cellsG", then (status 0) per rectangle "countN countG area".
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../spatialflink_amd/csrc/gf_geom_plan.hpp"

static long read_long(FILE* f) {
  long v;
  if (fscanf(f, "%ld", &v) != 1) { fprintf(stderr, "short input\n"); exit(2); }
  return v;
}

#define REQUIRE(c)                                                      \
  do {                                                                  \
    if (!(c)) { fprintf(stderr, "invariant failed: %s\n", #c); return 3; } \
  } while (0)

// a cell's membership from the table alone: the sum over the one-cell rectangle
static bool member(const std::vector<int32_t>& sat, int32_t n, int32_t x, int32_t y) {
  return gf::geom_rect_count(sat.data(), n, x, y, x, y) == 1;
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "r");
  if (!f) return 2;
  const long nsets = read_long(f);
  for (long s = 0; s < nsets; ++s) {
    const int32_t n = (int32_t)read_long(f), nq = (int32_t)read_long(f);
    const int32_t gl = (int32_t)read_long(f), cl = (int32_t)read_long(f);
    const bool whole = read_long(f) != 0;
    std::vector<int32_t> qcx((size_t)nq), qcy((size_t)nq);
    for (int32_t q = 0; q < nq; ++q) { qcx[q] = (int32_t)read_long(f); qcy[q] = (int32_t)read_long(f); }
    gf::GeomTables T;
    const int st = gf::geom_build_tables(n, nq, qcx.data(), qcy.data(), gl, cl, whole, T);
    const long nrect = read_long(f);
    std::vector<int32_t> rect(4 * (size_t)nrect);
    for (auto& v : rect) v = (int32_t)read_long(f);
    if (st) {
      printf("%d 0 0\n", st);
      continue;
    }
    const size_t w = (size_t)n + 1;
    REQUIRE(T.satN.size() == w * w && T.satG.size() == w * w);
    REQUIRE(T.satN[w * w - 1] == T.cellsN && T.satG[w * w - 1] == T.cellsG);
    for (size_t i = 0; i < w; ++i) REQUIRE(T.satN[i] == 0 && T.satN[i * w] == 0 && T.satG[i] == 0 && T.satG[i * w] == 0);
    printf("0 %lld %lld\n", (long long)T.cellsN, (long long)T.cellsG);
    for (long k = 0; k < nrect; ++k) {
      const int32_t x1 = rect[4 * k], y1 = rect[4 * k + 1], x2 = rect[4 * k + 2], y2 = rect[4 * k + 3];
      const int64_t cn = gf::geom_rect_count(T.satN.data(), n, x1, y1, x2, y2);
      const int64_t cg = gf::geom_rect_count(T.satG.data(), n, x1, y1, x2, y2);
      int64_t bn = 0, bg = 0;  // brute force over the rectangle's in-grid cells
      for (int64_t y = y1 < 0 ? 0 : y1; y <= y2 && y < n; ++y)
        for (int64_t x = x1 < 0 ? 0 : x1; x <= x2 && x < n; ++x) {
          bn += member(T.satN, n, (int32_t)x, (int32_t)y);
          bg += member(T.satG, n, (int32_t)x, (int32_t)y);
        }
      REQUIRE(cn == bn && cg == bg);
      printf("%lld %lld %lld\n", (long long)cn, (long long)cg, (long long)gf::geom_rect_area(x1, y1, x2, y2));
    }
  }
  fclose(f);
  return 0;
}
