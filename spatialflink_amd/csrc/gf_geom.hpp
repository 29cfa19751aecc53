// gf_geom.hpp -- device restatements of the JTS 1.16.1 point-polygon geometry the reference
// calls through DistanceFunctions.getDistance(Point, Polygon) (DistanceFunctions.java:33-36:
// DistanceOp -> PointLocator / RayCrossingCounter / RobustDeterminant, Distance.pointToSegment)
// and of its own bbox distance (getPointPolygonBBoxMinEuclideanDistance, :150-200).  Shared by
// the range kernels (k_range.hip), the polygon-query kNN (k_knn.hip), tRange (k_trange.hip) and the geometry
// windows (k_geom.hip).
#pragma once

#include "gf_internal.hpp"

namespace gf {


__device__ __forceinline__ void two_sum(double a, double b, double& s, double& e) {
  const double x = a + b, bv = x - a, av = x - bv;
  s = x;
  e = (a - av) + (b - bv);
}
// exact sign of x1*y2 - y1*x2 (what JTS RobustDeterminant.signOfDet2x2 returns)
static __device__ __forceinline__ int sign_det2x2(double x1, double y1, double x2, double y2) {
  const double p1 = x1 * y2, e1 = fma(x1, y2, -p1);
  const double p2 = y1 * x2, e2 = fma(y1, x2, -p2);
  const double terms[4] = {e1, -e2, p1, -p2};
  double h[4];
  int m = 1;
  h[0] = terms[0];
  for (int t = 1; t < 4; ++t) {
    double q = terms[t];
    for (int i = 0; i < m; ++i) {
      double s, e;
      two_sum(q, h[i], s, e);
      h[i] = e;
      q = s;
    }
    h[m++] = q;
  }
  for (int i = m - 1; i >= 0; --i) {
    if (h[i] > 0) return 1;
    if (h[i] < 0) return -1;
  }
  return 0;
}

constexpr int kLocInterior = 0, kLocBoundary = 1, kLocExterior = 2;

// RayCrossingCounter.locatePointInRing (JTS 1.16) behind PointLocator's envelope test
static __device__ __forceinline__ int locate_in_ring(double px, double py, const double* vx, const double* vy, int nv,
                              const double* env) {
  if (px > env[1] || px < env[0] || py > env[3] || py < env[2]) return kLocExterior;
  int crossings = 0;
  for (int i = 1; i < nv; ++i) {
    const double p1x = vx[i], p1y = vy[i], p2x = vx[i - 1], p2y = vy[i - 1];
    if (p1x < px && p2x < px) continue;
    if (px == p2x && py == p2y) return kLocBoundary;
    if (p1y == py && p2y == py) {
      double mn = p1x, mx = p2x;
      if (mn > mx) { mn = p2x; mx = p1x; }
      if (px >= mn && px <= mx) return kLocBoundary;
      continue;
    }
    if (((p1y > py) && (p2y <= py)) || ((p2y > py) && (p1y <= py))) {
      const double x1 = p1x - px, y1 = p1y - py, x2 = p2x - px, y2 = p2y - py;
      int sgn = sign_det2x2(x1, y1, x2, y2);
      if (sgn == 0) return kLocBoundary;
      if (y2 < y1) sgn = -sgn;
      if (sgn > 0) ++crossings;
    }
  }
  return (crossings & 1) ? kLocInterior : kLocExterior;
}

// one edge (p2 -> p1) of locate_in_ring's loop: true = p is on it; else `crossings` counts it
static __device__ __forceinline__ bool ring_edge(double px, double py, double p1x, double p1y, double p2x, double p2y,
                                                 int& crossings) {
  if (p1x < px && p2x < px) return false;
  if (px == p2x && py == p2y) return true;
  if (p1y == py && p2y == py) {
    double mn = p1x, mx = p2x;
    if (mn > mx) { mn = p2x; mx = p1x; }
    return px >= mn && px <= mx;
  }
  if (((p1y > py) && (p2y <= py)) || ((p2y > py) && (p1y <= py))) {
    const double x1 = p1x - px, y1 = p1y - py, x2 = p2x - px, y2 = p2y - py;
    int sgn = sign_det2x2(x1, y1, x2, y2);
    if (sgn == 0) return true;
    if (y2 < y1) sgn = -sgn;
    if (sgn > 0) ++crossings;
  }
  return false;
}

// locate_in_ring by one whole wave (every lane calls it with the same arguments): the wave paths of
// k_trange.hip and k_geom.hip.  BOUNDARY is the OR over the edges, the rest the parity of a sum: both
// order-free, so the verdict is locate_in_ring's
static __device__ __forceinline__ int locate_in_ring_wave(double px, double py, const double* vx, const double* vy, int nv,
                                                          const double* env, int lane) {
  if (px > env[1] || px < env[0] || py > env[3] || py < env[2]) return kLocExterior;
  int crossings = 0;
  bool on = false;
  for (int i = 1 + lane; i < nv; i += 64) on |= ring_edge(px, py, vx[i], vy[i], vx[i - 1], vy[i - 1], crossings);
  if (__ballot(on)) return kLocBoundary;
  return (__popcll(__ballot(crossings & 1)) & 1) ? kLocInterior : kLocExterior;
}

static __device__ inline double point_to_segment(double px, double py, double ax, double ay, double bx, double by, int metric) {
  if (ax == bx && ay == by) return distance(px, py, ax, ay, metric);
  const double len2 = (bx - ax) * (bx - ax) + (by - ay) * (by - ay);
  const double r = ((px - ax) * (bx - ax) + (py - ay) * (by - ay)) / len2;
  if (r <= 0.0) return distance(px, py, ax, ay, metric);
  if (r >= 1.0) return distance(px, py, bx, by, metric);
  const double s = ((ay - py) * (bx - ax) - (ax - px) * (by - ay)) / len2;
  return fabs(s) * sqrt(len2);
}

// JTS Envelope.distance against a point envelope
static __device__ inline double env_point_distance(const double* e, double px, double py) {
  if (!(px > e[1] || px < e[0] || py > e[3] || py < e[2])) return 0.0;
  double dx = 0.0, dy = 0.0;
  if (e[1] < px) dx = px - e[1]; else if (e[0] > px) dx = e[0] - px;
  if (e[3] < py) dy = py - e[3]; else if (e[2] > py) dy = e[2] - py;
  if (dx == 0.0) return dy;
  if (dy == 0.0) return dx;
  return sqrt(dx * dx + dy * dy);
}

// DistanceOp(point, polygon): containment (shell, holes), then min facet distance.  Inlined
// like its helpers: as calls, the ABI's callee-saved registers and stack cost every kernel that
// tests polygons (the range scan with its deferred drain: 101 -> 87 VGPRs, 5 waves/SIMD).
static __device__ __forceinline__ double polygon_distance(double px, double py, const PolyView& a, int p) {
  const int r0 = a.ring_off[p], r1 = a.ring_off[p + 1];
  if (a.rect && a.rect[p]) {
    // one-ring axis-aligned rectangle: PointLocator's interior-or-boundary is exactly the
    // closed box (every orientation sign against an axis-aligned edge is a plain comparison);
    // outside it, the same facet loop as below (a NaN coordinate fails the box and lands there
    // too, as it does on the general path)
    const double* e = a.ring_env + 4 * r0;
    if (px >= e[0] && px <= e[1] && py >= e[2] && py <= e[3]) return 0.0;
  } else if (px == px) {  // NaN x: containment skipped (documented; matches the oracle)
    const int v0 = a.vert_off[r0], nv = a.vert_off[r0 + 1] - v0;
    const int loc = locate_in_ring(px, py, a.vx + v0, a.vy + v0, nv, a.ring_env + 4 * r0);
    if (loc == kLocBoundary) return 0.0;
    if (loc == kLocInterior) {
      bool inside = true;
      for (int h = r0 + 1; h < r1; ++h) {
        const int hv0 = a.vert_off[h], hnv = a.vert_off[h + 1] - hv0;
        const int hl = locate_in_ring(px, py, a.vx + hv0, a.vy + hv0, hnv, a.ring_env + 4 * h);
        if (hl == kLocInterior) { inside = false; break; }
        if (hl == kLocBoundary) return 0.0;
      }
      if (inside) return 0.0;
    }
  }
  double md = 1.7976931348623157e308;
  for (int rg = r0; rg < r1; ++rg) {
    const int v0 = a.vert_off[rg], nv = a.vert_off[rg + 1] - v0;
    if (env_point_distance(a.ring_env + 4 * rg, px, py) > md) continue;
    for (int i = 0; i < nv - 1; ++i) {
      const double d = point_to_segment(px, py, a.vx[v0 + i], a.vy[v0 + i], a.vx[v0 + i + 1], a.vy[v0 + i + 1],
                                        a.metric);
      if (d < md) md = d;
      if (md <= 0.0) return md;
    }
  }
  return md;
}

// DistanceFunctions.getPointPolygonBBoxMinEuclideanDistance -- DistanceFunctions.java:150-200
__device__ __forceinline__ double pp_euclid(double lon, double lat, double lon1, double lat1) {
  const double a = lat1 - lat, b = lon1 - lon;
  return sqrt(a * a + b * b);
}
__device__ __forceinline__ double bbox_border(double x, double y, double x1, double y1, double x2, double y2) {
  if (x1 == x2) return pp_euclid(x, y, x1, y);
  if (y1 == y2) return pp_euclid(x, y, x, y1);
  return 4.9e-324;
}
static __device__ inline double point_bbox_distance(double x, double y, const double* bb) {
  const double x1 = bb[0], y1 = bb[1], x2 = bb[2], y2 = bb[3];
  if (x <= x1) {
    if (y <= y1) return pp_euclid(x, y, x1, y1);
    if (y >= y2) return pp_euclid(x, y, x1, y2);
    return bbox_border(x, y, x1, y1, x1, y2);
  } else if (x >= x2) {
    if (y <= y1) return pp_euclid(x, y, x2, y1);
    if (y >= y2) return pp_euclid(x, y, x2, y2);
    return bbox_border(x, y, x2, y1, x2, y2);
  }
  if (y <= y1) return bbox_border(x, y, x1, y1, x2, y1);
  if (y >= y2) return bbox_border(x, y, x1, y2, x2, y2);
  return 0.0;
}

// Envelope prune for the exact point-polygon test.  The computed point-polygon distance of a
// point outside the (closed) shell envelope is a min of computed point-segment distances, each
// within ~16 eps x (coordinate scale) of a true distance >= the true envelope distance; the
// margin (1e-12 relative to the coordinates, 1e-9 relative to r) exceeds that by orders of
// magnitude, so a pruned polygon could never have tested <= r.
__device__ __forceinline__ bool env_far(const double* bb, double px, double py, double r) {
  const double dx = px < bb[0] ? bb[0] - px : (px > bb[2] ? px - bb[2] : 0.0);
  const double dy = py < bb[1] ? bb[1] - py : (py > bb[3] ? py - bb[3] : 0.0);
  const double scale = fabs(px) + fabs(py) + fabs(bb[0]) + fabs(bb[1]) + fabs(bb[2]) + fabs(bb[3]);
  const double rm = r + r * 1e-9 + scale * 1e-12;
  return dx > rm || dy > rm || dx * dx + dy * dy > rm * rm;
}
__device__ __forceinline__ bool env_holds(const double* bb, double px, double py) {
  return px >= bb[0] && px <= bb[2] && py >= bb[1] && py <= bb[3];
}

// Point.distance(LineString) -- DistanceFunctions.java:38-42: a JTS DistanceOp with no containment
// step, i.e. with md = Double.MAX_VALUE once per line: for each segment of the OPEN chain in order,
// d = Distance.pointToSegment; if (d < md) md = d; if (md <= 0) stop.  (DistanceOp's one envelope
// check per line compares against md = MAX and never skips.)  A NaN d never compares below md, so
// a point with a NaN coordinate is at DBL_MAX.  No locate_in_ring, no sign_det2x2: a point inside a
// closed chain is at its distance to the nearest segment.
//
// Sub-chain envelopes.  The host cuts every chain into runs of kChainRun consecutive segments and
// uploads one envelope per run (ChainView::run_env, in env_far's x1, y1, x2, y2 order); the loop
// visits the runs in order and skips a run when env_far(run envelope, p, bound) holds.  Every
// segment of a run lies inside the run's envelope, so the envelope-prune argument above holds per
// run: a segment's computed distance is within ~16 eps x (coordinate scale) of its true distance,
// which is >= the true envelope distance, and env_far's margin exceeds that by orders of
// magnitude -- a skipped run holds no segment whose COMPUTED distance is <= bound.
//   VALUE == false (range, join: only d <= r is asked), bound = r: the visited segments include
//     every one with computed d <= r, so (result <= r) equals the plain loop's (min <= r); the walk
//     ends after the first run that brought md to <= r (the returned value is then some segment's
//     distance <= r, not necessarily the minimum -- the callers only compare it with r).
//   VALUE == true (kNN: the value is stored), bound = min(md so far, T): a skipped segment has
//     computed d > md (it would not lower the minimum) or d > T.  So whenever the plain minimum is
//     <= T the result is that minimum bit for bit; otherwise both are > T and the caller drops the
//     point (every caller tests d <= T before using d).
// The early stop at md <= 0 returns the same 0 either way (a segment at 0 is never skipped for a
// bound >= 0; for a negative bound every result is > bound).  A null run_off (mode 1 of
// gf_*_plan_set_chain_mode), a line of at most kChainPlainRuns runs (kChainPlainRunsValue where the
// value is kept), or a NaN coordinate takes the plain loop.
//
// (kChainRun: gf_internal.hpp, with the reasoning for its value.)
template <bool VALUE>
static __device__ __forceinline__ double chain_distance(double px, double py, const ChainView& a, int l, double bound) {
  const int v0 = a.vert_off[l], nseg = a.vert_off[l + 1] - v0 - 1;
  double md = 1.7976931348623157e308;
  if (a.run_off && px == px && py == py) {
    const int r0 = a.run_off[l], nrun = a.run_off[l + 1] - r0;
    if (nrun > (VALUE ? kChainPlainRunsValue : kChainPlainRuns)) {
      for (int rn = 0; rn < nrun; ++rn) {
        const double b = VALUE ? (md < bound ? md : bound) : bound;
        if (env_far(a.run_env + 4 * (size_t)(r0 + rn), px, py, b)) continue;
        const int s0 = rn * kChainRun, s1 = s0 + kChainRun < nseg ? s0 + kChainRun : nseg;
        for (int i = s0; i < s1; ++i) {
          const double d = point_to_segment(px, py, a.vx[v0 + i], a.vy[v0 + i], a.vx[v0 + i + 1], a.vy[v0 + i + 1],
                                            a.metric);
          if (d < md) md = d;
          if (md <= 0.0) return md;
        }
        if (!VALUE && md <= bound) return md;  // the decision is made: some segment is within the bound
      }
      return md;
    }
  }
  for (int i = 0; i < nseg; ++i) {
    const double d = point_to_segment(px, py, a.vx[v0 + i], a.vy[v0 + i], a.vx[v0 + i + 1], a.vy[v0 + i + 1], a.metric);
    if (d < md) md = d;
    if (md <= 0.0) return md;
  }
  return md;
}

// ---- geometry-to-geometry distance (k_geompair.hip; include/geoflink_hip.h, "geometry windows against
// polygon and linestring queries", contract 5) -------------------------------------------------------

// JTS Distance.segmentToSegment(A, B, C, D) and nothing else: a degenerate segment is its point; segments
// whose envelopes are disjoint, whose denominator is 0 (parallel or collinear) or whose parameters r, s
// leave [0, 1] do not intersect and are at the minimum of the four point-to-segment distances (MathUtil.min,
// `v < min` in argument order); otherwise 0.0.
static __device__ __forceinline__ double segment_to_segment(double ax, double ay, double bx, double by, double cx, double cy,
                                                            double dx, double dy, int metric) {
  if (ax == bx && ay == by) return point_to_segment(ax, ay, cx, cy, dx, dy, metric);
  if (cx == dx && cy == dy) return point_to_segment(dx, dy, ax, ay, bx, by, metric);
  bool apart;
  {  // Envelope.intersects(A, B, C, D)
    const double minq = cx < dx ? cx : dx, maxq = cx > dx ? cx : dx, minp = ax < bx ? ax : bx, maxp = ax > bx ? ax : bx;
    const double minqy = cy < dy ? cy : dy, maxqy = cy > dy ? cy : dy, minpy = ay < by ? ay : by, maxpy = ay > by ? ay : by;
    apart = minp > maxq || maxp < minq || minpy > maxqy || maxpy < minqy;
  }
  if (!apart) {
    const double denom = (bx - ax) * (dy - cy) - (by - ay) * (dx - cx);
    if (denom == 0.0) {
      apart = true;
    } else {
      const double r_num = (ay - cy) * (dx - cx) - (ax - cx) * (dy - cy);
      const double s_num = (ay - cy) * (bx - ax) - (ax - cx) * (by - ay);
      const double s = s_num / denom, r = r_num / denom;
      apart = r < 0.0 || r > 1.0 || s < 0.0 || s > 1.0;
    }
  }
  if (!apart) return 0.0;
  double m = point_to_segment(ax, ay, cx, cy, dx, dy, metric);
  const double d2 = point_to_segment(bx, by, cx, cy, dx, dy, metric);
  if (d2 < m) m = d2;
  const double d3 = point_to_segment(cx, cy, ax, ay, bx, by, metric);
  if (d3 < m) m = d3;
  const double d4 = point_to_segment(dx, dy, ax, ay, bx, by, metric);
  if (d4 < m) m = d4;
  return m;
}

// DistanceFunctions.getBBoxBBoxMinEuclideanDistance(bBox1, bBox2) -- DistanceFunctions.java:298-361, its
// branches with their <= / >= as written; a, b = x1, y1, x2, y2.  The operators pass the QUERY's box first.
static __device__ inline double bbox_bbox_distance(const double* a, const double* b) {
  const double x1 = a[0], y1 = a[1], x2 = a[2], y2 = a[3];
  const double p1 = b[0], q1 = b[1], p2 = b[2], q2 = b[3];
  if (p2 <= x1) {
    if (q2 <= y1) return pp_euclid(x1, y1, p2, q2);       // a1, b3
    if (q1 >= y2) return pp_euclid(x1, y2, p2, q1);       // a4, b2
    return bbox_border(p2, q1, x1, y1, x1, y2);           // b2 against a1-a4
  } else if (p1 >= x2) {
    if (q2 <= y1) return pp_euclid(x2, y1, p1, q2);       // a2, b4
    if (q1 >= y2) return pp_euclid(x2, y2, p1, q1);       // a3, b1
    return bbox_border(p1, q1, x2, y1, x2, y2);           // b1 against a2-a3
  }
  if (q2 <= y1) return bbox_border(p1, q2, x1, y1, x2, y1);  // b4 against a1-a2
  if (q1 >= y2) return bbox_border(p1, q1, x2, y2, x1, y2);  // b1 against a3-a4
  return 0.0;
}

// env_far between two boxes: true only when every point of box a is provably farther than r from every
// point of box b.  The computed segment-to-segment distance of two segments inside the boxes is within a
// few tens of eps x (coordinate scale) of their true distance, which is >= the true box distance; the
// margin (1e-12 relative to the coordinates, 1e-9 relative to r) exceeds that by orders of magnitude, so a
// pair of segments from boxes that are `far` could never have tested <= r.  An infinite or NaN bound is
// never far.
__device__ __forceinline__ bool box_far(double ax1, double ay1, double ax2, double ay2, double bx1, double by1, double bx2,
                                        double by2, double r) {
  const double dx = ax2 < bx1 ? bx1 - ax2 : (bx2 < ax1 ? ax1 - bx2 : 0.0);
  const double dy = ay2 < by1 ? by1 - ay2 : (by2 < ay1 ? ay1 - by2 : 0.0);
  const double scale = fabs(ax1) + fabs(ay1) + fabs(ax2) + fabs(ay2) + fabs(bx1) + fabs(by1) + fabs(bx2) + fabs(by2);
  const double rm = r + r * 1e-9 + scale * 1e-12;
  return dx > rm || dy > rm || dx * dx + dy * dy > rm * rm;
}

// the rings / chains [r0, r1) of ONE geometry of a CSR set (ring r0 the shell when `polygon`)
struct GeomSide {
  const int32_t* vert_off;
  const double* vx;
  const double* vy;
  const double* ring_env;  // [rings * 4] minx, maxx, miny, maxy
  int r0, r1;
  bool polygon;
};

// PointLocator.locate(p, polygon) != EXTERIOR: the shell, then the holes in order (inside a hole is
// exterior, on a hole's ring is boundary).  WAVE: by one whole wave, every lane with the same arguments.
template <bool WAVE>
static __device__ __forceinline__ bool side_holds(double px, double py, const GeomSide& s, int lane) {
  for (int rg = s.r0; rg < s.r1; ++rg) {
    const int v0 = s.vert_off[rg], nv = s.vert_off[rg + 1] - v0;
    const int loc = WAVE ? locate_in_ring_wave(px, py, s.vx + v0, s.vy + v0, nv, s.ring_env + 4 * (size_t)rg, lane)
                         : locate_in_ring(px, py, s.vx + v0, s.vy + v0, nv, s.ring_env + 4 * (size_t)rg);
    if (loc == kLocBoundary) return true;
    if (rg == s.r0) {
      if (loc == kLocExterior) return false;
    } else if (loc == kLocInterior) {
      return false;
    }
  }
  return true;
}

// The facet distance of query geometry q against the segments of ONE object ring / chain that this caller
// owns: j = j0, j0 + jstep, ... < the ring's segments (the lane form owns them all: j0 = 0, jstep = 1; the
// wave form lane l owns l, l + 64, ...).  Lowers `l`, this caller's minimum so far, with `d < l`.
// Pruning, value-safe for every d <= r: bound = VALUE ? min(l, r) : r; an object segment whose
// box is box_far from a query ring's envelope skips that ring, and from a run's envelope that run -- a
// skipped pair has a computed distance > bound, so it could neither lower l nor test <= r.  q_run_off
// null, or a ring of at most kChainPlainRunsValue runs: no run is skipped.
template <bool VALUE>
static __device__ __forceinline__ void pair_ring_facets(const GeomSide& q, const int32_t* q_run_off, const double* q_run_env,
                                                        const double* ovx, const double* ovy, int onseg, int j0, int jstep,
                                                        double r, int metric, double& l) {
  for (int j = j0; j < onseg; j += jstep) {
    const double cx = ovx[j], cy = ovy[j], dx = ovx[j + 1], dy = ovy[j + 1];
    const double sx1 = cx < dx ? cx : dx, sx2 = cx < dx ? dx : cx, sy1 = cy < dy ? cy : dy, sy2 = cy < dy ? dy : cy;
    for (int ra = q.r0; ra < q.r1; ++ra) {
      const double* e = q.ring_env + 4 * (size_t)ra;
      double bound = VALUE ? (l < r ? l : r) : r;
      if (box_far(e[0], e[2], e[1], e[3], sx1, sy1, sx2, sy2, bound)) continue;
      const int v0 = q.vert_off[ra], nseg = q.vert_off[ra + 1] - v0 - 1;
      const double* qx = q.vx + v0;
      const double* qy = q.vy + v0;
      int nrun = 0, run0 = 0;
      if (q_run_off) { run0 = q_run_off[ra]; nrun = q_run_off[ra + 1] - run0; }
      if (nrun > kChainPlainRunsValue) {
        for (int rn = 0; rn < nrun; ++rn) {
          const double* re = q_run_env + 4 * (size_t)(run0 + rn);
          bound = VALUE ? (l < r ? l : r) : r;
          if (box_far(re[0], re[1], re[2], re[3], sx1, sy1, sx2, sy2, bound)) continue;
          const int s0 = rn * kChainRun, s1 = s0 + kChainRun < nseg ? s0 + kChainRun : nseg;
          for (int i = s0; i < s1; ++i) {
            const double d = segment_to_segment(qx[i], qy[i], qx[i + 1], qy[i + 1], cx, cy, dx, dy, metric);
            if (d < l) l = d;
          }
          if (l <= 0.0) return;
        }
      } else {
        for (int i = 0; i < nseg; ++i) {
          const double d = segment_to_segment(qx[i], qy[i], qx[i + 1], qy[i + 1], cx, cy, dx, dy, metric);
          if (d < l) l = d;
        }
        if (l <= 0.0) return;
      }
    }
    if (!VALUE && l <= r) return;  // the decision is made: some pair is within r
  }
}

// the wave's minimum by `t < l` (a NaN never wins), the same value in every lane
static __device__ __forceinline__ double wave_min(double l) {
  for (int o = 32; o > 0; o >>= 1) {
    const double t = __shfl_xor(l, o, 64);
    if (t < l) l = t;
  }
  return l;
}

// DistanceOp(query, object), terminate distance 0 (contract 5): containment both ways -- the object's first
// coordinate in a query polygon, then the query's first coordinate in an object polygon --, then the
// minimum over every pair of segments.  The minimum of non-NaN values by `d < md` does not depend on the
// order, so the lane form, the wave form (the lanes stride the object's segments, the query's are
// wave-uniform, wave_min between the object's rings) and JTS's own loop order give the same bits.
// VALUE == false (range): the result is compared with r only and may be any pair's distance <= r.
template <bool WAVE, bool VALUE>
static __device__ __forceinline__ double geom_distance(const GeomSide& q, const int32_t* q_run_off, const double* q_run_env,
                                                       const GeomSide& o, double r, int metric, int lane) {
  {
    const double ox = o.vx[o.vert_off[o.r0]], oy = o.vy[o.vert_off[o.r0]];
    if (q.polygon && ox == ox && side_holds<WAVE>(ox, oy, q, lane)) return 0.0;
    const double fx = q.vx[q.vert_off[q.r0]], fy = q.vy[q.vert_off[q.r0]];
    if (o.polygon && fx == fx && side_holds<WAVE>(fx, fy, o, lane)) return 0.0;
  }
  double md = 1.7976931348623157e308;
  for (int rb = o.r0; rb < o.r1; ++rb) {
    const int v0 = o.vert_off[rb], onseg = o.vert_off[rb + 1] - v0 - 1;
    double l = md;
    pair_ring_facets<VALUE>(q, q_run_off, q_run_env, o.vx + v0, o.vy + v0, onseg, WAVE ? lane : 0, WAVE ? 64 : 1, r, metric, l);
    md = WAVE ? wave_min(l) : l;
    if (md <= 0.0) return md;
    if (!VALUE && md <= r) return md;
  }
  return md;
}

}  // namespace gf
