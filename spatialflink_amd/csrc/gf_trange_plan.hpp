// gf_trange_plan.hpp -- the pure host part of a tRange plan (trange.cpp uploads what it builds):
// ring envelopes, the per-cell classes, the per-cell polygon lists and the polygons whose bbox
// cells leave the grid.  No device call and no context here, so a stand-alone host program
// (tests/native/trange_plan_main.cpp, built with the host sanitizers) can drive it.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../include/geoflink_hip.h"
#include "gf_numerics.hpp"

namespace gf {

constexpr uint8_t kTrNone = 0, kTrTest = 1, kTrInside = 2;
constexpr int32_t kTrangeWideRing = 384;          // default: rings of at least this many vertices take the wave path (measured)
constexpr int64_t kTrangeMaxEntries = (int64_t)1 << 28;  // cell-list entries a plan may hold

struct TrangeTables {
  int32_t n = 0;                   // grid partitions
  int32_t npoly = 0, nrings = 0;
  std::vector<double> ring_env;    // [nrings * 4] minx, maxx, miny, maxy
  std::vector<int32_t> max_ring;   // [npoly] vertices of the polygon's largest ring
  std::vector<uint8_t> cls;        // [n * n] kTrNone / kTrTest / kTrInside, cell = cy * n + cx
  std::vector<int32_t> cand_off;   // [n * n + 1] lists of the kTrTest cells (others empty)
  std::vector<int32_t> cand_list;  // polygon ids, ascending per cell
  std::vector<int32_t> extra;      // [n_extra * 5] polygon, x0, x1, y0, y1: bbox cell ranges leaving [0, n)
  int64_t cells[3] = {0, 0, 0};    // cells per class
};

// 0: built; 1: a polygon without a shell; 2: a ring not closed or of fewer than 4 vertices;
// 3: the grid is too large for a cell table; 4: the cell lists would exceed kTrangeMaxEntries
inline int trange_build_tables(const gf_grid& g, const gf_polygons& polys, TrangeTables& T) {
  const int32_t np = polys.npoly;
  const int32_t nrings = np > 0 ? polys.ring_off[np] : 0;
  const int64_t n = g.n;
  if (n * n > (int64_t)1 << 30 || n > 16384) return 3;
  for (int32_t p = 0; p < np; ++p)
    if (polys.ring_off[p + 1] <= polys.ring_off[p]) return 1;
  for (int32_t j = 0; j < nrings; ++j) {  // Polygon.createPolygon / JTS LinearRing, as range.cpp
    const int32_t v0 = polys.vert_off[j], v1 = polys.vert_off[j + 1];
    if (v1 - v0 < 4 || polys.vx[v0] != polys.vx[v1 - 1] || polys.vy[v0] != polys.vy[v1 - 1]) return 2;
  }
  T.n = g.n;
  T.npoly = np;
  T.nrings = nrings;
  T.ring_env.assign(4 * (size_t)std::max(nrings, 1), 0.0);
  for (int32_t j = 0; j < nrings; ++j) {
    const int32_t v0 = polys.vert_off[j], v1 = polys.vert_off[j + 1];
    double mnx = polys.vx[v0], mxx = mnx, mny = polys.vy[v0], mxy = mny;
    for (int32_t v = v0 + 1; v < v1; ++v) {
      mnx = std::min(mnx, polys.vx[v]); mxx = std::max(mxx, polys.vx[v]);
      mny = std::min(mny, polys.vy[v]); mxy = std::max(mxy, polys.vy[v]);
    }
    T.ring_env[4 * j] = mnx; T.ring_env[4 * j + 1] = mxx; T.ring_env[4 * j + 2] = mny; T.ring_env[4 * j + 3] = mxy;
  }
  T.max_ring.assign((size_t)std::max(np, 1), 0);
  struct Rect { int64_t x0, x1, y0, y1; };
  std::vector<Rect> base((size_t)np);
  std::vector<uint8_t> rectf((size_t)np, 0);
  T.cls.assign((size_t)(n * n), kTrNone);
  T.extra.clear();
  auto lo = [](int64_t v) { return std::max<int64_t>(v, 0); };
  auto hi = [n](int64_t v) { return std::min<int64_t>(v, n - 1); };
  for (int32_t p = 0; p < np; ++p) {
    for (int32_t j = polys.ring_off[p]; j < polys.ring_off[p + 1]; ++j)
      T.max_ring[p] = std::max(T.max_ring[p], polys.vert_off[j + 1] - polys.vert_off[j]);
    // the shell envelope's bbox cells: HelperClass.assignGridCellID(bBox, uGrid), HelperClass.java:123-143
    const double* e = &T.ring_env[4 * (size_t)polys.ring_off[p]];
    const double x1 = e[0], x2 = e[1], y1 = e[2], y2 = e[3];
    const Rect b = {cell_index(x1, g.minX, g.cellLength), cell_index(x2, g.minX, g.cellLength),
                    cell_index(y1, g.minY, g.cellLength), cell_index(y2, g.minY, g.cellLength)};
    base[p] = b;
    if (b.x0 < 0 || b.y0 < 0 || b.x1 >= n || b.y1 >= n) {
      T.extra.push_back(p);
      T.extra.push_back((int32_t)b.x0); T.extra.push_back((int32_t)b.x1);
      T.extra.push_back((int32_t)b.y0); T.extra.push_back((int32_t)b.y1);
    }
    for (int64_t y = lo(b.y0); y <= hi(b.y1); ++y)
      for (int64_t x = lo(b.x0); x <= hi(b.x1); ++x) T.cls[y * n + x] = kTrTest;
    // a one-ring axis-aligned rectangle: the test of the range plans
    if (!(x1 < x2 && y1 < y2) || polys.ring_off[p + 1] - polys.ring_off[p] != 1) continue;
    const int32_t v0 = polys.vert_off[polys.ring_off[p]], v1 = polys.vert_off[polys.ring_off[p] + 1];
    bool rect = (v1 - v0 == 5);
    int corners = 0;
    for (int32_t v = v0; rect && v < v1; ++v) {
      const double X = polys.vx[v], Y = polys.vy[v];
      rect = (X == x1 || X == x2) && (Y == y1 || Y == y2);
      if (rect && v > v0) rect = (X == polys.vx[v - 1]) != (Y == polys.vy[v - 1]);  // one axis moves
      if (rect && v < v1 - 1) corners |= 1 << ((X == x2) + 2 * (Y == y2));
    }
    rectf[p] = rect && corners == 15;
  }
  // inside: the cells strictly between the cells of a rectangle's edges.  cell_index is monotone, so
  // every coordinate of a cell above cell(x1) exceeds x1 and every coordinate of a cell below cell(x2)
  // is below x2: the cell's closed extent [X_c, prev(X_{c+1})] lies in the open box, and no cell
  // holding an edge coordinate qualifies.  A NaN lands in cell 0 whatever its value: the kernel
  // accepts only non-NaN points untested.
  for (int32_t p = 0; p < np; ++p) {
    if (!rectf[p]) continue;
    const Rect& b = base[p];
    for (int64_t y = lo(b.y0 + 1); y <= hi(b.y1 - 1); ++y)
      for (int64_t x = lo(b.x0 + 1); x <= hi(b.x1 - 1); ++x) T.cls[y * n + x] = kTrInside;
  }
  T.cells[0] = T.cells[1] = T.cells[2] = 0;
  for (uint8_t c : T.cls) T.cells[c]++;
  // the lists of the test cells, polygons ascending (the order the reference walks them in)
  T.cand_off.assign((size_t)(n * n) + 1, 0);
  T.cand_list.clear();
  for (int pass = 0; pass < 2; ++pass) {
    std::vector<int32_t> cur;
    if (pass == 1) {
      int64_t total = 0;
      for (int64_t i = 0; i < n * n; ++i) total += T.cand_off[i + 1];
      if (total > kTrangeMaxEntries) return 4;
      for (int64_t i = 0; i < n * n; ++i) T.cand_off[i + 1] += T.cand_off[i];
      cur.assign(T.cand_off.begin(), T.cand_off.end() - 1);
      T.cand_list.resize((size_t)total);
    }
    for (int32_t p = 0; p < np; ++p) {
      const Rect& b = base[p];
      for (int64_t y = lo(b.y0); y <= hi(b.y1); ++y)
        for (int64_t x = lo(b.x0); x <= hi(b.x1); ++x) {
          const int64_t cell = y * n + x;
          if (T.cls[cell] != kTrTest) continue;
          if (pass == 0) T.cand_off[cell + 1]++;
          else T.cand_list[cur[cell]++] = p;
        }
    }
  }
  return 0;
}

}  // namespace gf
