// Test-only stand-alone host program over the pure host part of a tRange plan
// (spatialflink_amd/csrc/gf_trange_plan.hpp): reads a grid and polygon sets from the file named on the
// command line, builds the tables, checks their invariants and prints one line of counts per set.
// tests/test_trange_ref.py builds it with -fsanitize=address,undefined and compares the counts with its
// own.  Not part of the product.
//
// Input (whitespace separated; doubles as C hex floats): the number of sets, then per set
//   n minX maxX minY maxY npoly, per polygon nrings, per ring nv and nv pairs x y.
// Output per set: status none test inside entries extras maxlist
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../spatialflink_amd/csrc/gf_trange_plan.hpp"

static double read_double(FILE* f) {
  char buf[128];
  if (fscanf(f, "%127s", buf) != 1) { fprintf(stderr, "short input\n"); exit(2); }
  return strtod(buf, nullptr);
}
static long read_long(FILE* f) {
  long v;
  if (fscanf(f, "%ld", &v) != 1) { fprintf(stderr, "short input\n"); exit(2); }
  return v;
}

#define REQUIRE(c)                                                      \
  do {                                                                  \
    if (!(c)) { fprintf(stderr, "invariant failed: %s\n", #c); return 3; } \
  } while (0)

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "r");
  if (!f) return 2;
  const long nsets = read_long(f);
  for (long s = 0; s < nsets; ++s) {
    gf_grid g{};
    g.n = (int32_t)read_long(f);
    g.minX = read_double(f); g.maxX = read_double(f); g.minY = read_double(f); g.maxY = read_double(f);
    g.cellLength = (g.maxX - g.minX) / g.n;
    const long np = read_long(f);
    std::vector<int32_t> ring_off(1, 0), vert_off(1, 0);
    std::vector<double> vx, vy;
    for (long p = 0; p < np; ++p) {
      const long nr = read_long(f);
      for (long r = 0; r < nr; ++r) {
        const long nv = read_long(f);
        for (long v = 0; v < nv; ++v) {
          vx.push_back(read_double(f));
          vy.push_back(read_double(f));
        }
        vert_off.push_back((int32_t)vx.size());
      }
      ring_off.push_back((int32_t)vert_off.size() - 1);
    }
    gf_polygons polys{(int32_t)np, ring_off.data(), vert_off.data(), vx.data(), vy.data()};
    gf::TrangeTables T;
    const int st = gf::trange_build_tables(g, polys, T);
    if (st) {
      printf("%d 0 0 0 0 0 0\n", st);
      continue;
    }
    const int64_t cells = (int64_t)g.n * g.n;
    REQUIRE((int64_t)T.cls.size() == cells && (int64_t)T.cand_off.size() == cells + 1);
    REQUIRE(T.cells[0] + T.cells[1] + T.cells[2] == cells);
    REQUIRE(T.cand_off[0] == 0 && T.cand_off[cells] == (int32_t)T.cand_list.size());
    REQUIRE(T.extra.size() % 5 == 0 && (long)T.max_ring.size() >= np);
    int64_t maxlist = 0;
    for (int64_t c = 0; c < cells; ++c) {
      const int32_t a = T.cand_off[c], b = T.cand_off[c + 1];
      REQUIRE(a <= b);
      REQUIRE((T.cls[c] == gf::kTrTest) == (b > a));  // exactly the test cells have lists
      for (int32_t e = a; e < b; ++e) {
        REQUIRE(T.cand_list[e] >= 0 && T.cand_list[e] < np);
        REQUIRE(e == a || T.cand_list[e - 1] < T.cand_list[e]);  // ascending, each polygon once
      }
      maxlist = b - a > maxlist ? b - a : maxlist;
    }
    for (size_t e = 0; e < T.extra.size(); e += 5) {
      REQUIRE(T.extra[e] >= 0 && T.extra[e] < np);
      REQUIRE(T.extra[e + 1] < 0 || T.extra[e + 3] < 0 || T.extra[e + 2] >= g.n || T.extra[e + 4] >= g.n);
    }
    printf("0 %lld %lld %lld %lld %lld %lld\n", (long long)T.cells[0], (long long)T.cells[1], (long long)T.cells[2],
           (long long)T.cand_list.size(), (long long)(T.extra.size() / 5), (long long)maxlist);
  }
  fclose(f);
  return 0;
}
