// gf_geomjoin_plan.hpp -- the cell arithmetic of the geometry-stream joins (include/geoflink_hip.h,
// "geometry-stream joins"), shared by the host (geomjoin.cpp), the kernels (k_geomjoin.hip) and a
// stand-alone host program (tests/native/geomjoin_plan_main.cpp, built with the host sanitizers);
// tests/geomjoin_ref.py restates every function here.  No device call and no context.
//
// A rectangle is four inclusive int64 bounds; x1 > x2 or y1 > y2 is the empty rectangle.  Cell indices
// are int32 and saturate (Java's (int)), so a side is at most 2^32 cells long and every sum of an index
// and a layer count fits int64.  Areas can reach 2^64: join_area saturates, and a multiplicity is
// reported as min(m, 2^32 - 1) -- min(a + b, M) = min(min(a, M) + min(b, M), M) keeps the sum small.
#pragma once

#include <cstdint>

#include "gf_numerics.hpp"

namespace gf {

constexpr int64_t kJoinLongTiles = 16;      // default long_tiles (a guess, not measured)
constexpr int64_t kJoinMaxTileSide = 1024;  // at most this many tiles per grid side: the CSR holds <= 2^20 tiles
constexpr uint64_t kJoinMaxM = 0xFFFFFFFFull;

struct JoinRect {
  int64_t x1, y1, x2, y2;
};
GF_HD bool join_empty(const JoinRect& a) { return a.x1 > a.x2 || a.y1 > a.y2; }
GF_HD JoinRect join_rect(int32_t cx1, int32_t cy1, int32_t cx2, int32_t cy2) { return JoinRect{cx1, cy1, cx2, cy2}; }
GF_HD JoinRect join_meet(const JoinRect& a, const JoinRect& b) {
  return JoinRect{a.x1 > b.x1 ? a.x1 : b.x1, a.y1 > b.y1 ? a.y1 : b.y1, a.x2 < b.x2 ? a.x2 : b.x2, a.y2 < b.y2 ? a.y2 : b.y2};
}
GF_HD JoinRect join_grid(int32_t n) { return JoinRect{0, 0, (int64_t)n - 1, (int64_t)n - 1}; }
GF_HD bool join_leaves(const JoinRect& a, int32_t n) {  // a non-empty rectangle with a cell outside the grid
  return !join_empty(a) && (a.x1 < 0 || a.y1 < 0 || a.x2 >= n || a.y2 >= n);
}

// E_q, the in-grid part of K(q): the valid cells within c layers of a cell of R_q (contract 2, the
// rectangle form).  `whole`: the point rule at r == 0, every valid cell.  c <= 0 or an empty R_q: nothing.
GF_HD JoinRect join_expand(const JoinRect& rq, int64_t c, int32_t n, bool whole) {
  if (whole) return join_grid(n);
  if (c <= 0 || join_empty(rq)) return JoinRect{0, 0, -1, -1};
  return join_meet(JoinRect{rq.x1 - c, rq.y1 - c, rq.x2 + c, rq.y2 + c}, join_grid(n));
}

// the cells of a rectangle, saturating at 2^64 - 1 (both sides 2^32 long is the only product that overflows)
GF_HD uint64_t join_area(const JoinRect& a) {
  if (join_empty(a)) return 0;
  const uint64_t w = (uint64_t)(a.x2 - a.x1) + 1, h = (uint64_t)(a.y2 - a.y1) + 1;
  if (w > kJoinMaxM && h > kJoinMaxM) return ~0ull;
  return w * h;
}

// m(o, q) = |R_o n E_q| + [out_members] (|R_o n R_q| - |R_o n R_q n grid|), reported as min(m, 2^32 - 1)
// (contract 3).  out_members: a geometry query at guaranteed layers 0, whose K holds every cell of R_q.
GF_HD uint32_t join_multiplicity(const JoinRect& ro, const JoinRect& eq, const JoinRect& rq, bool out_members, int32_t n) {
  uint64_t m = join_area(join_meet(ro, eq));  // inside the grid: <= 2^62
  if (m > kJoinMaxM) m = kJoinMaxM;
  if (out_members) {
    const JoinRect both = join_meet(ro, rq);
    uint64_t out = join_area(both) - join_area(join_meet(both, join_grid(n)));  // the subtrahend is a part of the minuend
    if (out > kJoinMaxM) out = kJoinMaxM;
    m += out;
    if (m > kJoinMaxM) m = kJoinMaxM;
  }
  return (uint32_t)m;
}

// Tiles are squares of 2^shift cells a side: the smallest power of two >= `requested`, or, for
// requested <= 0, >= min(2 c + 1, n); doubled until the grid has at most kJoinMaxTileSide tiles a side.
GF_HD int32_t join_tile_shift(int32_t n, int64_t c, int64_t requested) {
  int64_t want = requested;
  if (want <= 0) {
    want = c > 0 ? 2 * c + 1 : 1;
    if (want > n) want = n;
  }
  int32_t shift = 0;
  while (shift < 31 && ((int64_t)1 << shift) < want) ++shift;
  while (shift < 31 && (((int64_t)n - 1) >> shift) + 1 > kJoinMaxTileSide) ++shift;
  return shift;
}
GF_HD int64_t join_tiles_side(int32_t n, int32_t shift) { return (((int64_t)n - 1) >> shift) + 1; }
// the tile of a cell of the grid
GF_HD int64_t join_tile_of(int64_t cx, int64_t cy, int32_t shift, int64_t nt) { return (cy >> shift) * nt + (cx >> shift); }
// the tiles a rectangle INSIDE the grid touches (0 for the empty one)
GF_HD int64_t join_tiles_covered(const JoinRect& a, int32_t shift) {
  if (join_empty(a)) return 0;
  return ((a.x2 >> shift) - (a.x1 >> shift) + 1) * ((a.y2 >> shift) - (a.y1 >> shift) + 1);
}
// The reference tile of a pair: the tile holding the lower corner of R_o n E_q; -1 when they do not meet.
// A short object and a short query meet in the probe at every tile both touch and are taken at this one only.
GF_HD int64_t join_ref_tile(const JoinRect& ro, const JoinRect& eq, int32_t shift, int64_t nt) {
  const JoinRect b = join_meet(ro, eq);
  if (join_empty(b)) return -1;
  return join_tile_of(b.x1, b.y1, shift, nt);
}

// 0: never paired (no member of K at all); 1: short; 2: long.  A query is short when E_q touches at most
// long_tiles tiles and K(q) has no member outside the grid; an object when R_o n grid touches at most
// long_tiles tiles (none at all is short: it can only meet the out-of-grid members of long queries).
// brute: everything that can be paired is long, so every pair goes through the rectangle pass.
GF_HD int join_class_query(const JoinRect& rq, const JoinRect& eq, bool out_members, int32_t n, int32_t shift,
                           int64_t long_tiles, bool brute) {
  const bool outside = out_members && join_leaves(rq, n);
  if (join_empty(eq) && !outside) return 0;
  if (brute || outside) return 2;
  return join_tiles_covered(eq, shift) <= long_tiles ? 1 : 2;
}
GF_HD int join_class_object(const JoinRect& ro, int32_t n, int32_t shift, int64_t long_tiles, bool brute) {
  if (join_empty(ro)) return 0;
  if (brute) return 2;
  return join_tiles_covered(join_meet(ro, join_grid(n)), shift) <= long_tiles ? 1 : 2;
}

}  // namespace gf
