// k_geomjoin.hip -- the geometry-stream joins (include/geoflink_hip.h, "geometry-stream joins";
// join/{Polygon,LineString}{Point,Polygon,LineString}JoinQuery.java): a window of polygons or linestrings
// joined with a window of points, polygons or linestrings.  Flink replicates the ordinary object to every
// cell of its rectangle R_o and the query to its cell set K(q), and joins on the cell key; here a pair's
// key matches are a closed form, m(o, q) = |R_o n K(q)| (gf_geomjoin_plan.hpp), and the work is finding the
// pairs with m > 0 without looking at all of them.
//   bin     geomjoin_point_cells   the cell of every query point (a geometry query's rectangles are its index's);
//           geomjoin_class         one lane per object and per query: E_q, the class (never paired, short,
//                                  long), the five lists by per-wave appends, and for a short query one
//                                  count per tile its E_q touches;
//           (exclusive scan of the counts: the library's own)
//           geomjoin_scatter       one lane per short query: its (tile, q) entries into the CSR.
//   probe   geomjoin_probe         one lane per short object: the tiles of R_o n grid, each tile's short
//                                  queries; a pair is taken at the tile holding the lower corner of
//                                  R_o n E_q only (join_ref_tile), so it appears once;
//           geomjoin_rect          grid-stride over (long object, any query) and (short object, long query):
//                                  the same m, no tiles.
//           Both run twice: a count pass, then -- the host sizes the candidate list in between -- a write
//           pass.  Exact mode drops a candidate whose boxes are provably farther apart than r (box_far /
//           env_far) and lists the rest for one lane or, when the SECOND geometry has at least
//           wide_vertices vertices, one wave; approximate mode decides the bbox distance here and writes pairs.
//   exact   geomjoin_exact_lane    one lane per listed candidate: geom_distance<lane>, or the point passes'
//                                  polygon_distance / chain_distance for a point query;
//           geomjoin_exact_wave    one wave per listed candidate: geom_distance<wave> (the lanes stride the
//                                  second geometry's segments) / polygon_distance_wave / chain_distance_wave.
//           Hits are appended to `pairs` as (o, q, m) up to cap and counted beyond it.
// Every append is geom_reserve's (one ballot and one atomic per wave).  The order of the lists, the
// candidates and the pairs depends on scheduling; the set of triples never does.
#define GF_TU_NAME k_geomjoin_hip
#include "gf_buildtag.hpp"  // first: records this unit's command-line defines

#include "gf_geom_win.hpp"
#include "gf_geomjoin_plan.hpp"

namespace gf {

static __device__ __forceinline__ JoinRect side_rect(const GeomJoinSide& s, int64_t i) {
  const int4 c = reinterpret_cast<const int4*>(s.cells)[i];
  return join_rect(c.x, c.y, c.z, c.w);
}

// the tiles of a rectangle inside the grid
template <class F>
static __device__ __forceinline__ void for_tiles(const GeomJoinArgs& a, const JoinRect& e, F&& f) {
  for (int64_t ty = e.y1 >> a.shift; ty <= e.y2 >> a.shift; ++ty)
    for (int64_t tx = e.x1 >> a.shift; tx <= e.x2 >> a.shift; ++tx) f(ty * a.nt + tx);
}

__global__ __launch_bounds__(kBlock) void geomjoin_point_cells_kernel(GeomJoinArgs a) {
  for (int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x; q < a.q.n; q += (int64_t)gridDim.x * kBlock) {
    const int32_t cx = cell_index(a.px[q], a.qminX, a.qcl), cy = cell_index(a.py[q], a.qminY, a.qcl);
    reinterpret_cast<int4*>(a.pcells)[q] = make_int4(cx, cy, cx, cy);  // may lie outside the grid: used as it is
  }
}

__global__ __launch_bounds__(kBlock) void geomjoin_class_kernel(GeomJoinArgs a) {
  const int64_t nmax = a.o.n > a.q.n ? a.o.n : a.q.n;
  unsigned long long entries = 0;
  for (int64_t i0 = (int64_t)blockIdx.x * kBlock; i0 < nmax; i0 += (int64_t)gridDim.x * kBlock) {  // wave-uniform
    const int64_t i = i0 + threadIdx.x;
    int oc = 0, qc = 0;
    if (i < a.o.n && a.o.valid[i]) oc = join_class_object(side_rect(a.o, i), a.n, a.shift, a.long_tiles, a.brute != 0);
    JoinRect eq{0, 0, -1, -1};
    if (i < a.q.n && (!a.q.valid || a.q.valid[i])) {
      const JoinRect rq = side_rect(a.q, i);
      eq = join_expand(rq, a.c, a.n, a.whole != 0);
      qc = join_class_query(rq, eq, a.out_members != 0, a.n, a.shift, a.long_tiles, a.brute != 0);
    }
    geom_reserve(a.ctr + kGeomJoinCtrShortO, oc == 1, [&](unsigned long long pos) { a.short_o[pos] = (uint32_t)i; });
    geom_reserve(a.ctr + kGeomJoinCtrLongO, oc == 2, [&](unsigned long long pos) { a.long_o[pos] = (uint32_t)i; });
    geom_reserve(a.ctr + kGeomJoinCtrShortQ, qc == 1, [&](unsigned long long pos) { a.short_q[pos] = (uint32_t)i; });
    geom_reserve(a.ctr + kGeomJoinCtrLongQ, qc == 2, [&](unsigned long long pos) { a.long_q[pos] = (uint32_t)i; });
    geom_reserve(a.ctr + kGeomJoinCtrActQ, qc != 0, [&](unsigned long long pos) { a.act_q[pos] = (uint32_t)i; });
    if (qc == 1)  // at most long_tiles tiles, every one inside [0, nt)^2: E_q lies in the grid
      for_tiles(a, eq, [&](int64_t t) {
        atomicAdd(a.tile_cnt + t, 1u);
        ++entries;
      });
  }
  entries = wave_sum(entries);
  if ((threadIdx.x & 63) == 0 && entries) atomicAdd(a.ctr + kGeomJoinCtrEntries, entries);
}

__global__ __launch_bounds__(kBlock) void geomjoin_scatter_kernel(GeomJoinArgs a) {
  const int64_t cnt = (int64_t)a.ctr[kGeomJoinCtrShortQ];  // <= q.n
  const unsigned long long entries = a.ctr[kGeomJoinCtrEntries];  // tile_q's length
  for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < cnt; e += (int64_t)gridDim.x * kBlock) {
    const uint32_t q = a.short_q[e];
    const JoinRect eq = join_expand(side_rect(a.q, q), a.c, a.n, a.whole != 0);
    for_tiles(a, eq, [&](int64_t t) {
      const unsigned long long pos = (unsigned long long)a.tile_off[t] + atomicAdd(a.tile_cur + t, 1u);
      if (pos < entries) a.tile_q[pos] = q;  // (always: the cursors repeat the class stage's counts)
    });
  }
}

struct JoinAcc {
  unsigned long long cand = 0, far = 0, lane = 0, wave = 0, hits = 0, rep = 0;
};

static __device__ __forceinline__ void store_triple(uint32_t* dst, unsigned long long pos, uint32_t o, uint32_t q, uint32_t m) {
  dst[3 * pos] = o;
  dst[3 * pos + 1] = q;
  dst[3 * pos + 2] = m;
}

// One candidate per lane with `have` (every lane of the wave calls it).  Count pass: the counters of the
// run.  Write pass: exact mode lists the candidate for its lane or wave, approximate mode emits the pair.
template <bool WRITE>
static __device__ __forceinline__ void join_take(const GeomJoinArgs& a, bool have, uint32_t o, uint32_t q, uint32_t m,
                                                 JoinAcc& acc) {
  bool keep = false, wide = false;
  if (have) {
    const double* eo = a.o.env + 4 * (size_t)o;
    if (a.q.kind == 0) {
      const double px = a.px[q], py = a.py[q];
      keep = a.approx ? point_bbox_distance(px, py, eo) <= a.r : !env_far(eo, px, py, a.r);
    } else {
      const double* eq = a.q.env + 4 * (size_t)q;
      if (a.approx) keep = (a.first_is_ordinary ? bbox_bbox_distance(eo, eq) : bbox_bbox_distance(eq, eo)) <= a.r;
      else keep = !box_far(eq[0], eq[1], eq[2], eq[3], eo[0], eo[1], eo[2], eo[3], a.r);
    }
    if (!a.approx && keep) {  // the geometry whose segments a wave's lanes would stride
      const bool second_is_query = a.q.kind != 0 && a.first_is_ordinary;
      wide = second_is_query ? a.q.nvert[q] >= a.q.wide_vertices : a.o.nvert[o] >= a.o.wide_vertices;
    }
    if (!WRITE) {
      ++acc.cand;
      if (a.approx) {
        if (keep) { ++acc.hits; acc.rep += m; }
      } else if (!keep) {
        ++acc.far;
      } else if (wide) {
        ++acc.wave;
      } else {
        ++acc.lane;
      }
    }
  }
  if (WRITE) {
    if (a.approx) {
      geom_reserve(a.ctr + kGeomJoinCtrOut, keep, [&](unsigned long long pos) {
        if ((int64_t)pos < a.cap) store_triple(a.pairs, pos, o, q, m);
      });
    } else {  // (the bounds always hold: the write pass repeats the count pass's decisions)
      geom_reserve(a.ctr + kGeomJoinCtrLaneCur, keep && !wide, [&](unsigned long long pos) {
        if (pos < a.n_lane) store_triple(a.cand, pos, o, q, m);
      });
      geom_reserve(a.ctr + kGeomJoinCtrWaveCur, keep && wide, [&](unsigned long long pos) {
        if (pos < a.n_wave) store_triple(a.cand, a.n_lane + pos, o, q, m);
      });
    }
  }
}

static __device__ __forceinline__ void flush_acc(const GeomJoinArgs& a, JoinAcc& acc) {
  acc.cand = wave_sum(acc.cand); acc.far = wave_sum(acc.far); acc.lane = wave_sum(acc.lane);
  acc.wave = wave_sum(acc.wave); acc.hits = wave_sum(acc.hits); acc.rep = wave_sum(acc.rep);
  if ((threadIdx.x & 63) != 0) return;
  if (acc.cand) atomicAdd(a.ctr + kGeomJoinCtrCand, acc.cand);
  if (acc.far) atomicAdd(a.ctr + kGeomJoinCtrFar, acc.far);
  if (acc.lane) atomicAdd(a.ctr + kGeomJoinCtrLane, acc.lane);
  if (acc.wave) atomicAdd(a.ctr + kGeomJoinCtrWave, acc.wave);
  if (acc.hits) atomicAdd(a.ctr + kGeomJoinCtrHits, acc.hits);
  if (acc.rep) atomicAdd(a.ctr + kGeomJoinCtrRep, acc.rep);
}

template <bool WRITE>
__global__ __launch_bounds__(kBlock) void geomjoin_probe_kernel(GeomJoinArgs a) {
  const int64_t cnt = (int64_t)a.ctr[kGeomJoinCtrShortO];  // <= o.n
  JoinAcc acc;
  for (int64_t e0 = (int64_t)blockIdx.x * kBlock; e0 < cnt; e0 += (int64_t)gridDim.x * kBlock) {  // wave-uniform
    const int64_t e = e0 + threadIdx.x;
    bool live = e < cnt;
    uint32_t o = 0, p = 0, pend = 0;
    JoinRect ro{0, 0, -1, -1};
    int64_t tx = 0, ty = 0, tx0 = 0, tx1 = -1, ty1 = -1;
    if (live) {
      o = a.short_o[e];
      ro = side_rect(a.o, o);
      const JoinRect rg = join_meet(ro, join_grid(a.n));
      live = !join_empty(rg);  // an object outside the grid meets long queries only
      if (live) {
        tx0 = tx = rg.x1 >> a.shift; tx1 = rg.x2 >> a.shift;
        ty = rg.y1 >> a.shift; ty1 = rg.y2 >> a.shift;
        p = a.tile_off[ty * a.nt + tx];
        pend = a.tile_off[ty * a.nt + tx + 1];
      }
    }
    for (;;) {  // every lane advances to its next candidate, then the wave takes them together
      bool have = false;
      uint32_t q = 0, m = 0;
      while (live && !have) {
        if (p < pend) {
          const uint32_t qq = a.tile_q[p++];
          const JoinRect rq = side_rect(a.q, qq);
          const JoinRect eq = join_expand(rq, a.c, a.n, a.whole != 0);
          if (join_ref_tile(ro, eq, a.shift, a.nt) == ty * a.nt + tx) {
            have = true;
            q = qq;
            m = join_multiplicity(ro, eq, rq, a.out_members != 0, a.n);
          }
        } else {
          if (++tx > tx1) { tx = tx0; ++ty; }
          if (ty > ty1) {
            live = false;
          } else {
            p = a.tile_off[ty * a.nt + tx];
            pend = a.tile_off[ty * a.nt + tx + 1];
          }
        }
      }
      if (__ballot(have) == 0) break;
      join_take<WRITE>(a, have, o, q, m, acc);
    }
  }
  if (!WRITE) flush_acc(a, acc);
}

template <bool WRITE>
__global__ __launch_bounds__(kBlock) void geomjoin_rect_kernel(GeomJoinArgs a) {
  const unsigned long long nlo = a.ctr[kGeomJoinCtrLongO], nso = a.ctr[kGeomJoinCtrShortO];
  const unsigned long long nact = a.ctr[kGeomJoinCtrActQ], nlq = a.ctr[kGeomJoinCtrLongQ];
  const unsigned long long first = nlo * nact, total = first + nso * nlq;  // <= o.n x q.n < 2^63
  JoinAcc acc;
  for (unsigned long long p0 = (unsigned long long)blockIdx.x * kBlock; p0 < total; p0 += (unsigned long long)gridDim.x * kBlock) {
    const unsigned long long p = p0 + threadIdx.x;
    bool have = false;
    uint32_t o = 0, q = 0, m = 0;
    if (p < total) {
      if (p < first) {
        o = a.long_o[p / nact];
        q = a.act_q[p % nact];
      } else {
        o = a.short_o[(p - first) / nlq];
        q = a.long_q[(p - first) % nlq];
      }
      const JoinRect rq = side_rect(a.q, q);
      m = join_multiplicity(side_rect(a.o, o), join_expand(rq, a.c, a.n, a.whole != 0), rq, a.out_members != 0, a.n);
      have = m > 0;
    }
    join_take<WRITE>(a, have, o, q, m, acc);
  }
  if (!WRITE) flush_acc(a, acc);
}

static __device__ __forceinline__ GeomSide join_side(const GeomJoinSide& s, uint32_t i) {
  GeomSide g;
  g.vert_off = s.vert_off; g.vx = s.vx; g.vy = s.vy; g.ring_env = s.ring_env;
  g.polygon = s.kind == GF_GEOM_POLYGON;
  g.r0 = g.polygon ? s.ring_off[i] : (int)i;
  g.r1 = g.polygon ? s.ring_off[i + 1] : (int)i + 1;
  return g;
}

// the operator's exact distance of candidate (o, q), compared with r only (WAVE: wave-uniform arguments)
template <bool WAVE>
static __device__ __forceinline__ double join_distance(const GeomJoinArgs& a, uint32_t o, uint32_t q, int lane) {
  if (a.q.kind == 0) {
    const double px = a.px[q], py = a.py[q];
    if (a.o.kind == GF_GEOM_POLYGON) {
      PolyView pv;
      pv.ring_off = a.o.ring_off; pv.vert_off = a.o.vert_off; pv.vx = a.o.vx; pv.vy = a.o.vy;
      pv.ring_env = a.o.ring_env; pv.metric = a.metric; pv.rect = nullptr;
      return WAVE ? polygon_distance_wave(px, py, pv, (int)o, lane) : polygon_distance(px, py, pv, (int)o);
    }
    ChainView cv;
    cv.run_off = nullptr; cv.vert_off = a.o.vert_off; cv.vx = a.o.vx; cv.vy = a.o.vy;  // no runs: the plain segment loop
    cv.run_env = nullptr; cv.metric = a.metric;
    return WAVE ? chain_distance_wave(px, py, cv, (int)o, lane) : chain_distance<false>(px, py, cv, (int)o, a.r);
  }
  const GeomSide so = join_side(a.o, o), sq = join_side(a.q, q);
  return a.first_is_ordinary ? geom_distance<WAVE, false>(so, nullptr, nullptr, sq, a.r, a.metric, lane)
                             : geom_distance<WAVE, false>(sq, nullptr, nullptr, so, a.r, a.metric, lane);
}

static __device__ __forceinline__ void emit_hit(const GeomJoinArgs& a, bool hit, uint32_t o, uint32_t q, uint32_t m) {
  geom_reserve(a.ctr + kGeomJoinCtrOut, hit, [&](unsigned long long pos) {
    if ((int64_t)pos < a.cap) store_triple(a.pairs, pos, o, q, m);
  });
}

__global__ __launch_bounds__(kBlock) void geomjoin_exact_lane_kernel(GeomJoinArgs a) {
  const int64_t cnt = (int64_t)a.n_lane;
  JoinAcc acc;
  for (int64_t e0 = (int64_t)blockIdx.x * kBlock; e0 < cnt; e0 += (int64_t)gridDim.x * kBlock) {  // wave-uniform
    const int64_t e = e0 + threadIdx.x;
    bool hit = false;
    uint32_t o = 0, q = 0, m = 0;
    if (e < cnt) {
      o = a.cand[3 * e]; q = a.cand[3 * e + 1]; m = a.cand[3 * e + 2];
      hit = join_distance<false>(a, o, q, 0) <= a.r;
    }
    if (hit) { ++acc.hits; acc.rep += m; }
    emit_hit(a, hit, o, q, m);
  }
  flush_acc(a, acc);
}

__global__ __launch_bounds__(kBlock) void geomjoin_exact_wave_kernel(GeomJoinArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t cnt = (int64_t)a.n_wave;
  const int64_t waves = (int64_t)gridDim.x * (kBlock / 64);
  JoinAcc acc;
  for (int64_t e = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6); e < cnt; e += waves) {
    const uint32_t* c = a.cand + 3 * ((int64_t)a.n_lane + e);  // wave-uniform, as everything join_distance decides
    const uint32_t o = c[0], q = c[1], m = c[2];
    const bool hit = join_distance<true>(a, o, q, lane) <= a.r;
    if (hit && lane == 0) { ++acc.hits; acc.rep += m; }
    emit_hit(a, hit && lane == 0, o, q, m);
  }
  flush_acc(a, acc);
}

static unsigned geomjoin_blocks(gf_ctx* ctx, unsigned long long items, int per_block) {
  const unsigned long long b = (items + per_block - 1) / per_block, cap = (unsigned long long)ctx->num_cus * 8;
  return (unsigned)(b < 1 ? 1 : (b > cap ? cap : b));
}

hipError_t launch_geomjoin(gf_ctx* ctx, int stage, const GeomJoinArgs& a) {
  KTimer timer(ctx, stage <= kGeomJoinScatter ? GF_K_JOIN_BUCKET : (stage == kGeomJoinExact ? GF_K_GEOM : GF_K_JOIN_PROBE));
  hipStream_t s = ctx->stream;
  const dim3 blk(kBlock);
  const dim3 per_o(geomjoin_blocks(ctx, (unsigned long long)a.o.n, kBlock)), per_q(geomjoin_blocks(ctx, (unsigned long long)a.q.n, kBlock));
  const dim3 per_pair(geomjoin_blocks(ctx, a.rect_pairs, kBlock));
  switch (stage) {
    case kGeomJoinPointCells: hipLaunchKernelGGL(geomjoin_point_cells_kernel, per_q, blk, 0, s, a); break;
    case kGeomJoinClass: hipLaunchKernelGGL(geomjoin_class_kernel, a.o.n > a.q.n ? per_o : per_q, blk, 0, s, a); break;
    case kGeomJoinScatter: hipLaunchKernelGGL(geomjoin_scatter_kernel, per_q, blk, 0, s, a); break;
    case kGeomJoinProbeCount:
      hipLaunchKernelGGL(geomjoin_probe_kernel<false>, per_o, blk, 0, s, a);
      if (a.rect_pairs) hipLaunchKernelGGL(geomjoin_rect_kernel<false>, per_pair, blk, 0, s, a);
      break;
    case kGeomJoinProbeWrite:
      hipLaunchKernelGGL(geomjoin_probe_kernel<true>, per_o, blk, 0, s, a);
      if (a.rect_pairs) hipLaunchKernelGGL(geomjoin_rect_kernel<true>, per_pair, blk, 0, s, a);
      break;
    default:
      if (a.n_lane) hipLaunchKernelGGL(geomjoin_exact_lane_kernel, dim3(geomjoin_blocks(ctx, a.n_lane, kBlock)), blk, 0, s, a);
      if (a.n_wave) hipLaunchKernelGGL(geomjoin_exact_wave_kernel, dim3(geomjoin_blocks(ctx, a.n_wave, kBlock / 64)), blk, 0, s, a);
      break;
  }
  return hipGetLastError();
}

}  // namespace gf
