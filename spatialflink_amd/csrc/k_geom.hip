// k_geom.hip -- polygon and linestring WINDOWS against query points: range and kNN
// (include/geoflink_hip.h, "polygon and linestring windows"; range/PolygonPointRangeQuery.java,
// range/LineStringPointRangeQuery.java, knn/PolygonPointKNNQuery.java, knn/LineStringPointKNNQuery.java).
// Every window object is a different geometry of a different length tested against a few shared points
// -- the point-window kernels' work turned round.
//
// prepare (once per window)
//   geom_ring_env       one lane per ring: its envelope (exact min / max, `v < mn` / `v > mx` in vertex
//                       order) and whether it is a legal ring / chain.  A ring of at least wide_vertices
//                       vertices is only listed (slots by wave ballot + one atomic);
//   geom_ring_env_wide  one wave per listed ring: lane l takes vertices l, l + 64, ... (coalesced), the 64
//                       partial min / max are reduced by shuffles with the same comparisons.  min and max
//                       of finite doubles do not depend on the order, so the envelope is the serial one;
//   geom_objects        one lane per object: envelope (the shell's / the chain's), unclamped cell
//                       rectangle, validity, vertex count.
// per query run
//   geom_classify       one lane per object: "some cell in N" and "every cell in G" as rectangle sums over
//                       the query's summed-area tables (gf_geom_plan.hpp), one path for every nq.  Range:
//                       the all-G objects go straight into the bitmap (one ballot word per wave, every word
//                       written); the objects to test go to two worklists, short and wide.
//   geom_exact_short    one lane per short object, the query points looped inside with a break at the
//                       first d <= r; an object whose envelope is provably farther than r from a point
//                       (env_far, gf_geom.hpp) is not walked for that point.
//   geom_exact_wide     one wave per wide object: the lanes stride each ring's segments and edges.  The
//                       distance is per ring min-reduced with `d < md` (a NaN never wins; the minimum of
//                       non-NaN values is order-free, so it is the serial loop's bit for bit), and the
//                       serial loop's ring skip (ring envelope farther than md so far) is taken by the whole
//                       wave between rings, as the lane takes it.  Containment is locate_in_ring_wave: the
//                       orientation sign is exact per edge, the crossing count is a sum and the boundary
//                       verdict an OR, both order-free.
//   Range hits are OR-ed into whole bitmap words with atomics (the classify wrote every word before);
//   kNN hits are appended as (d, objID, idx) candidates for the library's select / sorted path.
// Which lane or wave tests an object, and the order of the worklists and the candidates, depend on
// scheduling; the bitmap and the record never do (the record's order (d, objID, idx) is total).
#define GF_TU_NAME k_geom_hip
#include "gf_buildtag.hpp"  // first: records this unit's command-line defines

#include "gf_geom_plan.hpp"
#include "gf_geom_win.hpp"  // geom_reserve, wave_sum, geom_emit: shared with k_geompair.hip

namespace gf {

static __device__ __forceinline__ bool ring_legal(const GeomArgs& a, int32_t v0, int32_t nv) {
  if (a.kind == GF_GEOM_LINESTRING) return nv >= 2;
  return nv >= 4 && a.vx[v0] == a.vx[v0 + nv - 1] && a.vy[v0] == a.vy[v0 + nv - 1];
}

static __device__ __forceinline__ void store_ring_env(const GeomArgs& a, int64_t j, double mnx, double mxx, double mny,
                                                      double mxy) {
  double* e = a.ring_env + 4 * j;
  e[0] = mnx; e[1] = mxx; e[2] = mny; e[3] = mxy;
}

__global__ __launch_bounds__(kBlock) void geom_ring_env_kernel(GeomArgs a) {
  for (int64_t j0 = (int64_t)blockIdx.x * kBlock; j0 < a.nrings; j0 += (int64_t)gridDim.x * kBlock) {  // wave-uniform
    const int64_t j = j0 + threadIdx.x;
    const bool in = j < a.nrings;
    int32_t v0 = 0, nv = 0;
    if (in) { v0 = a.vert_off[j]; nv = a.vert_off[j + 1] - v0; }
    const bool wide = in && nv >= a.wide_vertices;
    if (in) a.ring_ok[j] = nv > 0 && ring_legal(a, v0, nv);
    if (in && !wide) {
      double mnx = 0.0, mxx = 0.0, mny = 0.0, mxy = 0.0;
      if (nv > 0) {
        mnx = mxx = a.vx[v0];
        mny = mxy = a.vy[v0];
        for (int32_t v = v0 + 1; v < v0 + nv; ++v) {
          const double x = a.vx[v], y = a.vy[v];
          if (x < mnx) mnx = x;
          if (x > mxx) mxx = x;
          if (y < mny) mny = y;
          if (y > mxy) mxy = y;
        }
      }
      store_ring_env(a, j, mnx, mxx, mny, mxy);
    }
    geom_reserve(a.ictr, wide, [&](unsigned long long pos) { a.ring_wide[pos] = (uint32_t)j; });
  }
}

__global__ __launch_bounds__(kBlock) void geom_ring_env_wide_kernel(GeomArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t cnt = (int64_t)a.ictr[0];  // <= nrings: one slot per listed ring
  const int64_t waves = (int64_t)gridDim.x * (kBlock / 64);
  for (int64_t e = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6); e < cnt; e += waves) {
    const int64_t j = a.ring_wide[e];  // wave-uniform
    const int32_t v0 = a.vert_off[j], nv = a.vert_off[j + 1] - v0;  // nv >= wide_vertices >= 1
    double mnx = a.vx[v0], mxx = mnx, mny = a.vy[v0], mxy = mny;
    for (int32_t v = v0 + lane; v < v0 + nv; v += 64) {
      const double x = a.vx[v], y = a.vy[v];
      if (x < mnx) mnx = x;
      if (x > mxx) mxx = x;
      if (y < mny) mny = y;
      if (y > mxy) mxy = y;
    }
    for (int o = 32; o > 0; o >>= 1) {
      const double t0 = __shfl_xor(mnx, o, 64), t1 = __shfl_xor(mxx, o, 64);
      const double t2 = __shfl_xor(mny, o, 64), t3 = __shfl_xor(mxy, o, 64);
      if (t0 < mnx) mnx = t0;
      if (t1 > mxx) mxx = t1;
      if (t2 < mny) mny = t2;
      if (t3 > mxy) mxy = t3;
    }
    if (lane == 0) store_ring_env(a, j, mnx, mxx, mny, mxy);
  }
}

__global__ __launch_bounds__(kBlock) void geom_objects_kernel(GeomArgs a) {
  const int lane = threadIdx.x & 63;
  unsigned long long n_vert = 0, n_bad = 0, n_wide = 0;
  for (int64_t i0 = (int64_t)blockIdx.x * kBlock; i0 < a.nobj; i0 += (int64_t)gridDim.x * kBlock) {
    const int64_t i = i0 + threadIdx.x;
    if (i >= a.nobj) continue;
    int64_t r0 = i, r1 = i + 1;
    if (a.ring_off) { r0 = a.ring_off[i]; r1 = a.ring_off[i + 1]; }
    bool ok = r1 > r0;
    int64_t nv = 0;
    for (int64_t j = r0; j < r1; ++j) {
      ok = ok && a.ring_ok[j];
      nv += a.vert_off[j + 1] - a.vert_off[j];
    }
    double x1 = 0.0, y1 = 0.0, x2 = 0.0, y2 = 0.0;
    if (r1 > r0) {  // boundingBox: the shell's / the chain's envelope
      const double* e = a.ring_env + 4 * r0;
      x1 = e[0]; x2 = e[1]; y1 = e[2]; y2 = e[3];
    }
    double* env = a.env + 4 * i;
    env[0] = x1; env[1] = y1; env[2] = x2; env[3] = y2;
    int32_t* c = a.cells + 4 * i;  // HelperClass.assignGridCellID(bbox): not clamped
    c[0] = cell_index(x1, a.minX, a.cl);
    c[1] = cell_index(y1, a.minY, a.cl);
    c[2] = cell_index(x2, a.minX, a.cl);
    c[3] = cell_index(y2, a.minY, a.cl);
    const int32_t nvi = nv > INT32_MAX ? INT32_MAX : (int32_t)nv;
    a.valid[i] = ok;
    a.nvert[i] = nvi;
    n_vert += (unsigned long long)nv;
    n_bad += !ok;
    n_wide += nvi >= a.wide_vertices;
  }
  n_vert = wave_sum(n_vert);
  n_bad = wave_sum(n_bad);
  n_wide = wave_sum(n_wide);
  if (lane == 0) {
    if (n_vert) atomicAdd(a.ictr + 1, n_vert);
    if (n_bad) atomicAdd(a.ictr + 2, n_bad);
    if (n_wide) atomicAdd(a.ictr + 3, n_wide);
  }
}

__global__ __launch_bounds__(kBlock) void geom_classify_kernel(GeomArgs a) {
  geom_classify_body(a, [](const int4&) { return 0u; });  // point queries: the tables hold everything
}

static __device__ __forceinline__ PolyView poly_view(const GeomArgs& a) {
  PolyView p;
  p.ring_off = a.ring_off; p.vert_off = a.vert_off; p.vx = a.vx; p.vy = a.vy;
  p.ring_env = a.ring_env; p.metric = a.metric; p.rect = nullptr;
  return p;
}
static __device__ __forceinline__ ChainView chain_view(const GeomArgs& a) {
  ChainView c;
  c.run_off = nullptr; c.vert_off = a.vert_off; c.vx = a.vx; c.vy = a.vy;  // no runs: the plain segment loop
  c.run_env = nullptr; c.metric = a.metric;
  return c;
}

__global__ __launch_bounds__(kBlock) void geom_exact_short_kernel(GeomArgs a) {
  const int64_t cnt = (int64_t)a.qctr[0];  // <= nobj
  const PolyView pv = poly_view(a);
  const ChainView cv = chain_view(a);
  for (int64_t e0 = (int64_t)blockIdx.x * kBlock; e0 < cnt; e0 += (int64_t)gridDim.x * kBlock) {  // wave-uniform
    const int64_t e = e0 + threadIdx.x;
    bool hit = false;
    uint32_t i = 0;
    double d = 0.0;
    if (e < cnt) {
      i = a.work_short[e];
      const double* env = a.env + 4 * (size_t)i;
      for (int32_t q = 0; q < a.nq; ++q) {
        const double px = a.qx[q], py = a.qy[q];
        if (a.approx) {
          d = point_bbox_distance(px, py, env);
        } else {
          if (env_far(env, px, py, a.r)) continue;
          d = a.kind == GF_GEOM_POLYGON ? polygon_distance(px, py, pv, (int)i) : chain_distance<false>(px, py, cv, (int)i, a.r);
        }
        if (d <= a.r) { hit = true; break; }
      }
    }
    geom_emit(a, hit, i, d);
  }
}

// (polygon_distance_wave / chain_distance_wave: gf_geom_win.hpp, shared with k_geomjoin.hip)
__global__ __launch_bounds__(kBlock) void geom_exact_wide_kernel(GeomArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t cnt = (int64_t)a.qctr[1];  // <= nobj
  const PolyView pv = poly_view(a);
  const ChainView cv = chain_view(a);
  const int64_t waves = (int64_t)gridDim.x * (kBlock / 64);
  for (int64_t e = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6); e < cnt; e += waves) {
    const uint32_t i = a.work_wide[e];  // wave-uniform, as everything below
    const double* env = a.env + 4 * (size_t)i;
    bool hit = false;
    double d = 0.0;
    for (int32_t q = 0; q < a.nq; ++q) {
      const double px = a.qx[q], py = a.qy[q];
      if (env_far(env, px, py, a.r)) continue;
      d = a.kind == GF_GEOM_POLYGON ? polygon_distance_wave(px, py, pv, (int)i, lane) : chain_distance_wave(px, py, cv, (int)i, lane);
      if (d <= a.r) { hit = true; break; }
    }
    geom_emit(a, hit && lane == 0, i, d);
  }
}

__global__ __launch_bounds__(kBlock) void geom_count_kernel(GeomArgs a) {
  const int64_t words = (a.nobj + 63) >> 6;
  unsigned long long c = 0;
  for (int64_t w = (int64_t)blockIdx.x * kBlock + threadIdx.x; w < words; w += (int64_t)gridDim.x * kBlock)
    c += __popcll(a.bitmap[w]);
  c = wave_sum(c);
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(a.qctr + 4, c);
}
__global__ void geom_count_store_kernel(GeomArgs a) {
  a.counts[0] = (int64_t)a.qctr[4];
  a.counts[1] = (int64_t)a.qctr[3];
}

static unsigned geom_blocks(gf_ctx* ctx, int64_t items, int per_block) {
  const int64_t b = (items + per_block - 1) / per_block, cap = (int64_t)ctx->num_cus * 8;
  return (unsigned)(b < 1 ? 1 : (b > cap ? cap : b));
}

hipError_t launch_geom(gf_ctx* ctx, int stage, const GeomArgs& a) {
  KTimer timer(ctx, GF_K_GEOM);
  hipStream_t s = ctx->stream;
  const dim3 blk(kBlock);
  const dim3 lanes(geom_blocks(ctx, a.nobj, kBlock)), waves(geom_blocks(ctx, a.nobj, kBlock / 64));
  switch (stage) {
    case kGeomRingEnv: hipLaunchKernelGGL(geom_ring_env_kernel, dim3(geom_blocks(ctx, a.nrings, kBlock)), blk, 0, s, a); break;
    case kGeomRingEnvWide:
      hipLaunchKernelGGL(geom_ring_env_wide_kernel, dim3(geom_blocks(ctx, a.nrings, kBlock / 64)), blk, 0, s, a);
      break;
    case kGeomObjects: hipLaunchKernelGGL(geom_objects_kernel, lanes, blk, 0, s, a); break;
    case kGeomClassify: hipLaunchKernelGGL(geom_classify_kernel, lanes, blk, 0, s, a); break;
    case kGeomExactShort: hipLaunchKernelGGL(geom_exact_short_kernel, lanes, blk, 0, s, a); break;
    case kGeomExactWide: hipLaunchKernelGGL(geom_exact_wide_kernel, waves, blk, 0, s, a); break;
    default:
      hipLaunchKernelGGL(geom_count_kernel, dim3(geom_blocks(ctx, (a.nobj + 63) >> 6, kBlock)), blk, 0, s, a);
      hipLaunchKernelGGL(geom_count_store_kernel, dim3(1), dim3(1), 0, s, a);
      break;
  }
  return hipGetLastError();
}

}  // namespace gf
