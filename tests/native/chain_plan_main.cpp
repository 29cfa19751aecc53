// Test-only stand-alone host program over the pure host part of the linestring plans
// (spatialflink_amd/csrc/gf_chain_plan.hpp): reads linestring sets from the file named on the command
// line, validates each, builds its tables with the given run length, checks their invariants and prints
// one line per set.  tests/test_linestring_ref.py builds it with -fsanitize=address,undefined and
// compares the lines with its own.  Not part of the product.
//
// Input (whitespace separated; doubles as C hex floats): the number of sets, then per set
//   run nline, per line nv and nv pairs x y.
// Output per set: valid runs, then per line x1 y1 x2 y2 of its bbox as hex floats (valid 0: "0 0").
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../spatialflink_amd/csrc/gf_chain_plan.hpp"

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
    const int run = (int)read_long(f);
    const long nl = read_long(f);
    std::vector<int32_t> vert_off(1, 0);
    std::vector<double> vx, vy;
    for (long l = 0; l < nl; ++l) {
      const long nv = read_long(f);
      for (long v = 0; v < nv; ++v) {
        vx.push_back(read_double(f));
        vy.push_back(read_double(f));
      }
      vert_off.push_back((int32_t)vx.size());
    }
    gf_linestrings ls{(int32_t)nl, vert_off.data(), vx.data(), vy.data()};
    if (!gf::chain_valid(&ls)) {
      printf("0 0\n");
      continue;
    }
    gf::ChainTables T;
    gf::chain_build(ls, run, T);
    REQUIRE((long)T.run_off.size() == nl + 1 && T.run_off[0] == 0);
    REQUIRE(T.bbox.size() >= 4 * (size_t)nl && T.run_env.size() >= 4 * (size_t)T.run_off[nl] && !T.run_env.empty());
    for (long l = 0; l < nl; ++l) {
      const int32_t v0 = vert_off[l], nseg = vert_off[l + 1] - v0 - 1;
      REQUIRE(T.run_off[l + 1] - T.run_off[l] == (nseg + run - 1) / run);
      const double* bb = &T.bbox[4 * (size_t)l];
      for (int32_t i = 0; i < nseg; ++i) {  // both ends of segment i inside its run's envelope, that inside the bbox
        const double* e = &T.run_env[4 * (size_t)(T.run_off[l] + i / run)];
        for (int32_t v = v0 + i; v <= v0 + i + 1; ++v)
          REQUIRE(vx[v] >= e[0] && vx[v] <= e[2] && vy[v] >= e[1] && vy[v] <= e[3]);
        REQUIRE(e[0] >= bb[0] && e[1] >= bb[1] && e[2] <= bb[2] && e[3] <= bb[3]);
      }
    }
    printf("1 %d", (int)T.run_off[nl]);
    for (long l = 0; l < nl; ++l) printf(" %a %a %a %a", T.bbox[4 * l], T.bbox[4 * l + 1], T.bbox[4 * l + 2], T.bbox[4 * l + 3]);
    printf("\n");
  }
  fclose(f);
  return 0;
}
