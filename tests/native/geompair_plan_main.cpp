// Test-only stand-alone host program over the pure host part of a geometry-pair query
// (spatialflink_amd/csrc/gf_geom_plan.hpp: geom_build_tables_rects, geom_rect_meets / geom_rect_within,
// geom_query_set_valid): for grids of n = 1, 2, 7 and 100 and sets of query rectangles inside, partly outside
// and wholly outside the grid, at guaranteed layers -1, 0, 1, 2 and candidate layers 0, 1, 3, it checks every
// cell of the rectangle-marked tables against a brute-force membership test written from the contract (a cell
// is within L layers of a rectangle's cell), the `leaves` flag, and the two rectangle predicates against cell
// loops.  tests/test_geompair_ref.py builds it with -fsanitize=address,undefined and runs it.  Not part of
// the product.  Prints "ok <checks>"; any failed invariant ends it with status 3.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../spatialflink_amd/csrc/gf_geom_plan.hpp"

#define REQUIRE(c)                                                                          \
  do {                                                                                      \
    if (!(c)) { fprintf(stderr, "invariant failed (line %d): %s\n", __LINE__, #c); return 3; } \
  } while (0)

static uint32_t lcg_state = 12345u;
static int32_t rnd(int32_t lo, int32_t hi) {  // inclusive
  lcg_state = lcg_state * 1664525u + 1013904223u;
  return lo + (int32_t)((lcg_state >> 8) % (uint32_t)(hi - lo + 1));
}

// within `layers` of a cell of rc (layers >= 0), by the definition
static bool near_rect(const int32_t* rc, int32_t layers, int64_t x, int64_t y) {
  return x >= (int64_t)rc[0] - layers && x <= (int64_t)rc[2] + layers && y >= (int64_t)rc[1] - layers &&
         y <= (int64_t)rc[3] + layers;
}

static long checks = 0;

static int check_set(int32_t n, const std::vector<int32_t>& rects, int32_t gl, int32_t cl) {
  const int32_t nq = (int32_t)(rects.size() / 4);
  gf::GeomTables T;
  bool leaves = false;
  REQUIRE(gf::geom_build_tables_rects(n, nq, rects.data(), gl, cl, T, &leaves) == 0);
  const size_t w = (size_t)n + 1;
  REQUIRE(T.satN.size() == w * w && T.satG.size() == w * w);
  int64_t cn = 0, cg = 0;
  bool want_leaves = false;
  for (int32_t q = 0; q < nq; ++q) {
    const int32_t* rc = &rects[4 * (size_t)q];
    if (gl == 0 && (rc[0] < 0 || rc[1] < 0 || rc[2] >= n || rc[3] >= n)) want_leaves = true;
  }
  REQUIRE(leaves == want_leaves);
  for (int32_t y = 0; y < n; ++y)
    for (int32_t x = 0; x < n; ++x) {
      bool inG = false, inC = false;
      for (int32_t q = 0; q < nq; ++q) {
        const int32_t* rc = &rects[4 * (size_t)q];
        if (gl >= 0 && near_rect(rc, gl, x, y)) inG = true;
        if (cl > 0 && near_rect(rc, cl, x, y)) inC = true;
      }
      const bool inN = inG || inC;
      REQUIRE((gf::geom_rect_count(T.satG.data(), n, x, y, x, y) == 1) == inG);
      REQUIRE((gf::geom_rect_count(T.satN.data(), n, x, y, x, y) == 1) == inN);
      cn += inN;
      cg += inG;
      checks += 2;
    }
  REQUIRE(cn == T.cellsN && cg == T.cellsG);
  // rectangle sums against cell loops, for rectangles in and out of the grid
  for (int k = 0; k < 40; ++k) {
    const int32_t x1 = rnd(-3, n + 1), y1 = rnd(-3, n + 1), x2 = x1 + rnd(0, 4), y2 = y1 + rnd(0, 4);
    int64_t bn = 0;
    for (int64_t y = y1; y <= y2; ++y)
      for (int64_t x = x1; x <= x2; ++x)
        if (x >= 0 && y >= 0 && x < n && y < n) bn += gf::geom_rect_count(T.satN.data(), n, (int32_t)x, (int32_t)y, (int32_t)x, (int32_t)y);
    REQUIRE(gf::geom_rect_count(T.satN.data(), n, x1, y1, x2, y2) == bn);
    // the corner predicates of one query rectangle
    const int32_t* rc = &rects[0];
    bool meets = false, within = true;
    for (int64_t y = y1; y <= y2; ++y)
      for (int64_t x = x1; x <= x2; ++x) {
        const bool in = near_rect(rc, 0, x, y);
        meets = meets || in;
        within = within && in;
      }
    REQUIRE(gf::geom_rect_meets(rc, x1, y1, x2, y2) == meets);
    REQUIRE(gf::geom_rect_within(rc, x1, y1, x2, y2) == within);
    checks += 3;
  }
  return 0;
}

int main() {
  const int32_t sizes[] = {1, 2, 7, 100};
  const int32_t gls[] = {-1, 0, 1, 2}, cls[] = {0, 1, 3};
  for (int32_t n : sizes)
    for (int32_t gl : gls)
      for (int32_t cl : cls) {
        // one rectangle inside, partly outside on each side, wholly outside, saturated; then sets of 2 and 5
        std::vector<std::vector<int32_t>> sets = {
            {0, 0, 0, 0},
            {n / 2, n / 2, n / 2 + 1, n / 2},
            {-2, n / 3, 0, n / 3 + 1},
            {n - 1, -1, n + 2, 0},
            {-3, -3, n + 2, n + 2},
            {-5, 1, -4, 2},
            {n + 3, n + 3, n + 4, n + 5},
            {INT32_MIN, 0, INT32_MIN + 1, 0},
            {INT32_MAX - 1, n - 1, INT32_MAX, n - 1},
            {0, 0, 0, 0, n - 1, n - 1, n, n},
        };
        std::vector<int32_t> five;
        for (int q = 0; q < 5; ++q) {
          const int32_t x = rnd(-2, n), y = rnd(-2, n);
          five.insert(five.end(), {x, y, x + rnd(0, 3), y + rnd(0, 3)});
        }
        sets.push_back(five);
        for (const auto& s : sets)
          if (int st = check_set(n, s, gl, cl)) return st;
      }
  {  // refusals and the validity of query sets
    gf::GeomTables T;
    const int32_t rc[4] = {0, 0, 0, 0};
    REQUIRE(gf::geom_build_tables_rects(0, 1, rc, 0, 1, T, nullptr) == 1);
    REQUIRE(gf::geom_build_tables_rects(gf::kGeomMaxGrid + 1, 1, rc, 0, 1, T, nullptr) == 1);
    const double x[] = {0, 1, 1, 0, 0, 2, 3}, y[] = {0, 0, 1, 1, 0, 2, 3};
    const int32_t ro[] = {0, 1}, vo5[] = {0, 5}, vo4[] = {0, 4}, vo3[] = {0, 3}, vol[] = {0, 5, 7}, vol1[] = {0, 5, 6};
    const int32_t ro_empty[] = {0, 0}, ro_bad[] = {1, 2}, vo_bad[] = {1, 5};
    REQUIRE(gf::geom_query_set_valid(1, ro, vo5, x, y));
    REQUIRE(!gf::geom_query_set_valid(1, ro, vo4, x, y));       // unclosed
    REQUIRE(!gf::geom_query_set_valid(1, ro, vo3, x, y));       // fewer than 4 vertices
    REQUIRE(!gf::geom_query_set_valid(1, ro_empty, vo5, x, y)); // no ring
    REQUIRE(!gf::geom_query_set_valid(1, ro_bad, vo5, x, y));
    REQUIRE(!gf::geom_query_set_valid(1, ro, vo_bad, x, y));
    REQUIRE(!gf::geom_query_set_valid(0, ro, vo5, x, y));
    REQUIRE(!gf::geom_query_set_valid(1, ro, vo5, nullptr, y));
    REQUIRE(gf::geom_query_set_valid(2, nullptr, vol, x, y));   // chains of 5 and 2 vertices
    REQUIRE(!gf::geom_query_set_valid(2, nullptr, vol1, x, y)); // a 1-vertex chain
    checks += 12;
  }
  printf("ok %ld\n", checks);
  return 0;
}
