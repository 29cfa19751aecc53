// gf_geom_plan.hpp -- the pure host part of a geometry-window query (geom.cpp uploads what it builds):
// the per-cell N / G sets of a query point set as summed-area tables, and the rectangle sums the
// classify kernel asks of them (k_geom.hip includes this for those).  No device call and no context
// here, so a stand-alone host program (tests/native/geom_plan_main.cpp, built with the host sanitizers)
// can drive it.
//
// N and G of ONE query point are squares clipped to the grid; of a point set, unions of squares.  With
// S[y][x] = the number of member cells in [0, x) x [0, y) (int32, (n + 1)^2 entries, largest entry n^2:
// n <= 46340 keeps it inside int32), the members of any cell rectangle are four reads:
//   some cell of the rectangle in N   <=>  count_N(rect n grid) > 0
//   every cell of the rectangle in G  <=>  count_G(rect n grid) == area(rect), the UNCLAMPED area --
// a rectangle that leaves the grid has cells in no set, so it is never all-G.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../include/geoflink_hip.h"
#include "gf_numerics.hpp"

namespace gf {

constexpr int32_t kGeomMaxGrid = 46340;       // floor(sqrt(2^31 - 1)): the tables' largest entry is n^2
constexpr int32_t kGeomWideVertices = 384;    // default wide_vertices: gf_trange's wide_ring (not measured here)

struct GeomTables {
  int32_t n = 0;
  std::vector<int32_t> satN, satG;  // [(n + 1)^2], row-major: S[y * (n + 1) + x]
  int64_t cellsN = 0, cellsG = 0;   // members of each set
};

// members of sat's set among the cells [x1..x2] x [y1..y2] (inclusive, any int32 values; an empty or
// wholly outside rectangle: 0)
GF_HD int64_t geom_rect_count(const int32_t* sat, int32_t n, int32_t x1, int32_t y1, int32_t x2, int32_t y2) {
  const int64_t a = x1 < 0 ? 0 : x1, b = y1 < 0 ? 0 : y1;
  const int64_t c = x2 >= n ? (int64_t)n - 1 : x2, d = y2 >= n ? (int64_t)n - 1 : y2;
  if (a > c || b > d) return 0;
  const int64_t w = (int64_t)n + 1;
  return (int64_t)sat[(d + 1) * w + (c + 1)] - (int64_t)sat[b * w + (c + 1)] - (int64_t)sat[(d + 1) * w + a] +
         (int64_t)sat[b * w + a];
}
// the cells of the rectangle, in or out of the grid (0 when it is empty)
GF_HD int64_t geom_rect_area(int32_t x1, int32_t y1, int32_t x2, int32_t y2) {
  if (x1 > x2 || y1 > y2) return 0;
  return ((int64_t)x2 - x1 + 1) * ((int64_t)y2 - y1 + 1);
}

// The sets of nq query points whose cells are (qcx[q], qcy[q]) (as computed, in or out of the grid):
//   N: whole_n ? every cell : the cells within c_layers of a query cell            (contract 2)
//   G: g_layers < 0 ? none : the cells within g_layers of a query cell (0: the cell itself)
// 0: built; 1: n outside [1, kGeomMaxGrid]
inline int geom_build_tables(int32_t n, int32_t nq, const int32_t* qcx, const int32_t* qcy, int32_t g_layers,
                             int32_t c_layers, bool whole_n, GeomTables& T) {
  if (n < 1 || n > kGeomMaxGrid) return 1;
  T.n = n;
  const size_t cells = (size_t)n * n, w = (size_t)n + 1;
  std::vector<uint8_t> inN(cells, whole_n ? 1 : 0), inG(cells, 0);
  auto mark = [&](std::vector<uint8_t>& m, int32_t cx, int32_t cy, int32_t layers) {
    const int64_t x0 = std::max<int64_t>((int64_t)cx - layers, 0), x1 = std::min<int64_t>((int64_t)cx + layers, n - 1);
    const int64_t y0 = std::max<int64_t>((int64_t)cy - layers, 0), y1 = std::min<int64_t>((int64_t)cy + layers, n - 1);
    for (int64_t y = y0; y <= y1; ++y)
      for (int64_t x = x0; x <= x1; ++x) m[(size_t)y * n + x] = 1;
  };
  for (int32_t q = 0; q < nq; ++q) {
    if (!whole_n && c_layers > 0) mark(inN, qcx[q], qcy[q], c_layers);
    if (g_layers >= 0) mark(inG, qcx[q], qcy[q], g_layers);
  }
  auto sum = [&](const std::vector<uint8_t>& m, std::vector<int32_t>& S) -> int64_t {
    S.assign(w * w, 0);
    for (size_t y = 0; y < (size_t)n; ++y) {
      int32_t row = 0;
      for (size_t x = 0; x < (size_t)n; ++x) {
        row += m[y * n + x];
        S[(y + 1) * w + (x + 1)] = S[y * w + (x + 1)] + row;
      }
    }
    return S[w * w - 1];
  };
  T.cellsN = sum(inN, T.satN);
  T.cellsG = sum(inG, T.satG);
  return 0;
}

}  // namespace gf
