// k_geompair.hip -- polygon and linestring WINDOWS against polygon and linestring QUERIES: range and kNN
// (include/geoflink_hip.h, "geometry windows against polygon and linestring queries"; range/ and knn/
// {Polygon,LineString}{Polygon,LineString}{Range,KNN}Query.java).  The prepare, the tables, the worklists,
// the bitmap and the kNN record path are k_geom.hip's and geom.cpp's, unchanged; new here is the distance
// between two geometries (gf_geom.hpp: segment_to_segment, geom_distance), O(object segments x query
// segments) per tested object where a query point costs O(object segments).
//   geompair_classify  geom_classify's body (gf_geom_win.hpp) with the out-of-grid corner of G: at
//                      guaranteed layers 0 the cells of the query's rectangle outside the grid are
//                      members of G and N, which the in-grid
//                      tables cannot hold; for ONE query they are a rectangle and two comparisons of
//                      rectangles (gf_geom_plan.hpp: geom_rect_meets / geom_rect_within) are exact.
//   geompair_short     one lane per short object: the query geometries looped inside with a break at the
//                      first d <= r; a query whose box is provably farther than r from the object's is not
//                      walked (box_far); geom_distance<lane>.
//   geompair_wide      one wave per wide object: geom_distance<wave> -- the lanes stride the object's
//                      segments, the query's segments are wave-uniform loads, the minimum is reduced with
//                      `d < md` between the object's rings; containment by locate_in_ring_wave.
// Range hits are OR-ed into the bitmap the classify wrote; kNN hits are appended as candidates.  Which lane
// or wave tests an object depends on scheduling and on wide_vertices; the bitmap and the record never do.
#define GF_TU_NAME k_geompair_hip
#include "gf_buildtag.hpp"  // first: records this unit's command-line defines

#include "gf_geom_plan.hpp"
#include "gf_geom_win.hpp"

namespace gf {

__global__ __launch_bounds__(kBlock) void geompair_classify_kernel(GeomPairArgs p) {
  geom_classify_body(p.g, [&](const int4& c) {
    if (!p.corner) return 0u;
    return (geom_rect_meets(p.q_rect, c.x, c.y, c.z, c.w) ? 1u : 0u) | (geom_rect_within(p.q_rect, c.x, c.y, c.z, c.w) ? 2u : 0u);
  });
}

static __device__ __forceinline__ GeomSide query_side(const GeomPairArgs& p, int32_t q) {
  GeomSide s;
  s.vert_off = p.q_vert_off; s.vx = p.qvx; s.vy = p.qvy; s.ring_env = p.q_ring_env;
  s.polygon = p.qkind == GF_GEOM_POLYGON;
  s.r0 = s.polygon ? p.q_ring_off[q] : q;
  s.r1 = s.polygon ? p.q_ring_off[q + 1] : q + 1;
  return s;
}
static __device__ __forceinline__ GeomSide object_side(const GeomArgs& a, uint32_t i) {
  GeomSide s;
  s.vert_off = a.vert_off; s.vx = a.vx; s.vy = a.vy; s.ring_env = a.ring_env;
  s.polygon = a.kind == GF_GEOM_POLYGON;
  s.r0 = s.polygon ? a.ring_off[i] : (int)i;
  s.r1 = s.polygon ? a.ring_off[i + 1] : (int)i + 1;
  return s;
}

// the first query within r of object i (wave-uniform arguments when WAVE); d = that query's distance
template <bool WAVE>
static __device__ __forceinline__ bool pair_test(const GeomPairArgs& p, uint32_t i, int lane, double& d) {
  const GeomArgs& a = p.g;
  const double* env = a.env + 4 * (size_t)i;
  const GeomSide o = object_side(a, i);
  for (int32_t q = 0; q < a.nq; ++q) {
    const double* qe = p.q_env + 4 * (size_t)q;
    if (a.approx) {
      d = bbox_bbox_distance(qe, env);
    } else {
      // (a polygon's holes are taken to lie inside its shell's envelope, as the point-query passes take them)
      if (box_far(qe[0], qe[1], qe[2], qe[3], env[0], env[1], env[2], env[3], a.r)) continue;
      const GeomSide qs = query_side(p, q);
      d = a.knn ? geom_distance<WAVE, true>(qs, p.q_run_off, p.q_run_env, o, a.r, a.metric, lane)
                : geom_distance<WAVE, false>(qs, p.q_run_off, p.q_run_env, o, a.r, a.metric, lane);
    }
    if (d <= a.r) return true;
  }
  return false;
}

__global__ __launch_bounds__(kBlock) void geompair_short_kernel(GeomPairArgs p) {
  const GeomArgs& a = p.g;
  const int64_t cnt = (int64_t)a.qctr[0];  // <= nobj
  for (int64_t e0 = (int64_t)blockIdx.x * kBlock; e0 < cnt; e0 += (int64_t)gridDim.x * kBlock) {  // wave-uniform
    const int64_t e = e0 + threadIdx.x;
    bool hit = false;
    uint32_t i = 0;
    double d = 0.0;
    if (e < cnt) {
      i = a.work_short[e];
      hit = pair_test<false>(p, i, 0, d);
    }
    geom_emit(a, hit, i, d);
  }
}

__global__ __launch_bounds__(kBlock) void geompair_wide_kernel(GeomPairArgs p) {
  const GeomArgs& a = p.g;
  const int lane = threadIdx.x & 63;
  const int64_t cnt = (int64_t)a.qctr[1];  // <= nobj
  const int64_t waves = (int64_t)gridDim.x * (kBlock / 64);
  for (int64_t e = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6); e < cnt; e += waves) {
    const uint32_t i = a.work_wide[e];  // wave-uniform, as everything pair_test decides
    double d = 0.0;
    const bool hit = pair_test<true>(p, i, lane, d);
    geom_emit(a, hit && lane == 0, i, d);
  }
}

static unsigned geompair_blocks(gf_ctx* ctx, int64_t items, int per_block) {
  const int64_t b = (items + per_block - 1) / per_block, cap = (int64_t)ctx->num_cus * 8;
  return (unsigned)(b < 1 ? 1 : (b > cap ? cap : b));
}

hipError_t launch_geompair(gf_ctx* ctx, int stage, const GeomPairArgs& p) {
  KTimer timer(ctx, GF_K_GEOM);
  hipStream_t s = ctx->stream;
  const dim3 blk(kBlock);
  const dim3 lanes(geompair_blocks(ctx, p.g.nobj, kBlock)), waves(geompair_blocks(ctx, p.g.nobj, kBlock / 64));
  switch (stage) {
    case kGeomPairClassify: hipLaunchKernelGGL(geompair_classify_kernel, lanes, blk, 0, s, p); break;
    case kGeomPairShort: hipLaunchKernelGGL(geompair_short_kernel, lanes, blk, 0, s, p); break;
    default: hipLaunchKernelGGL(geompair_wide_kernel, waves, blk, 0, s, p); break;
  }
  return hipGetLastError();
}

}  // namespace gf
