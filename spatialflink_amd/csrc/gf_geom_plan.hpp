// gf_geom_plan.hpp -- the pure host part of a geometry-window query (geom.cpp uploads what it builds):
// the per-cell N / G sets of a query point set -- or of a set of query geometries' cell rectangles
// (geom_build_tables_rects) -- as summed-area tables, and the rectangle sums the classify kernels ask of
// them (k_geom.hip and k_geompair.hip include this for those).  No device call and no context here, so
// stand-alone host programs (tests/native/geom_plan_main.cpp, geompair_plan_main.cpp, built with the host
// sanitizers) can drive it.
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

// The sets of nq query GEOMETRIES (polygons or linestrings) whose cell rectangles are rects[4 q ..] =
// cx1, cy1, cx2, cy2 (as computed, in or out of the grid, possibly empty); the tables hold the in-grid
// members ("geometry windows against geometry queries", contract 2):
//   G: g_layers < 0 ? none : the cells within g_layers of a cell of a rectangle.  The union over a
//      rectangle's cells of the squares of g layers is the rectangle grown by g on every side; g > 0
//      keeps the valid cells only, g == 0 keeps every cell of the rectangle -- those outside the grid are
//      members too, which no table can hold: `leaves` reports that case.
//   N: G, and when c_layers > 0 the valid cells within c_layers of a cell of a rectangle.
// No whole-grid rule and no refusal here: c_layers <= 0 and g_layers < 0 give two empty sets.
// 0: built; 1: n outside [1, kGeomMaxGrid].  *leaves (nullable): g_layers == 0 and some non-empty
// rectangle has a cell outside the grid.
inline int geom_build_tables_rects(int32_t n, int32_t nq, const int32_t* rects, int32_t g_layers, int32_t c_layers,
                                   GeomTables& T, bool* leaves) {
  if (n < 1 || n > kGeomMaxGrid) return 1;
  T.n = n;
  const size_t cells = (size_t)n * n, w = (size_t)n + 1;
  std::vector<uint8_t> inN(cells, 0), inG(cells, 0);
  auto mark = [&](std::vector<uint8_t>& m, const int32_t* rc, int32_t layers) {
    if (rc[0] > rc[2] || rc[1] > rc[3]) return;  // no cell: nothing to grow
    const int64_t x0 = std::max<int64_t>((int64_t)rc[0] - layers, 0), x1 = std::min<int64_t>((int64_t)rc[2] + layers, n - 1);
    const int64_t y0 = std::max<int64_t>((int64_t)rc[1] - layers, 0), y1 = std::min<int64_t>((int64_t)rc[3] + layers, n - 1);
    for (int64_t y = y0; y <= y1; ++y)
      for (int64_t x = x0; x <= x1; ++x) m[(size_t)y * n + x] = 1;
  };
  bool out = false;
  for (int32_t q = 0; q < nq; ++q) {
    const int32_t* rc = rects + 4 * (size_t)q;
    if (c_layers > 0) mark(inN, rc, c_layers);
    if (g_layers >= 0) {
      mark(inG, rc, g_layers);
      mark(inN, rc, g_layers);
    }
    if (g_layers == 0 && rc[0] <= rc[2] && rc[1] <= rc[3] && (rc[0] < 0 || rc[1] < 0 || rc[2] >= n || rc[3] >= n)) out = true;
  }
  if (leaves) *leaves = out;
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

// A legal query set of nq >= 1 geometries: offsets from 0 and monotone; polygons (ring_off != null): at
// least one ring each, every ring closed with >= 4 vertices; linestrings: chains of >= 2 vertices.
inline bool geom_query_set_valid(int32_t nq, const int32_t* ring_off, const int32_t* vert_off, const double* vx,
                                 const double* vy) {
  if (nq < 1 || !vert_off || !vx || !vy) return false;
  int32_t nrings = nq;
  if (ring_off) {
    if (ring_off[0] != 0) return false;
    for (int32_t q = 0; q < nq; ++q)
      if (ring_off[q + 1] <= ring_off[q]) return false;
    nrings = ring_off[nq];
  }
  if (vert_off[0] != 0) return false;
  for (int32_t j = 0; j < nrings; ++j) {
    const int32_t v0 = vert_off[j], nv = vert_off[j + 1] - v0;
    if (nv < (ring_off ? 4 : 2)) return false;
    if (ring_off && (vx[v0] != vx[v0 + nv - 1] || vy[v0] != vy[v0 + nv - 1])) return false;
  }
  return true;
}

// The out-of-grid corner of ONE query rectangle q = (cx1, cy1, cx2, cy2) at g_layers == 0, where G = the
// rectangle itself and N's members outside the grid are the rectangle's (int32 cells, int64-free: plain
// comparisons).  An object rectangle o:
//   has a cell in N outside the tables  <=>  o and q share a cell (a shared cell inside the grid is in the
//                                            tables as well, so OR-ing the two answers is exact);
//   has every cell in G                 <=>  o is non-empty and lies within q.
GF_HD bool geom_rect_meets(const int32_t* q, int32_t x1, int32_t y1, int32_t x2, int32_t y2) {
  const int32_t a = x1 > q[0] ? x1 : q[0], b = y1 > q[1] ? y1 : q[1];
  const int32_t c = x2 < q[2] ? x2 : q[2], d = y2 < q[3] ? y2 : q[3];
  return a <= c && b <= d;
}
GF_HD bool geom_rect_within(const int32_t* q, int32_t x1, int32_t y1, int32_t x2, int32_t y2) {
  return x1 <= x2 && y1 <= y2 && x1 >= q[0] && y1 >= q[1] && x2 <= q[2] && y2 <= q[3];
}

}  // namespace gf
