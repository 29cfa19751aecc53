// geomjoin.cpp -- the geometry-stream joins: a prepared polygon / linestring window (gf_geom_prepare) joined
// with a point window or with a second prepared geometry window (include/geoflink_hip.h, "geometry-stream
// joins").  The joiner owns the grow-only scratch of a run -- the five lists, the tile CSR, the candidate
// list -- and is reused across windows; the cell arithmetic is gf_geomjoin_plan.hpp's, the kernels are
// k_geomjoin.hip's.  A run is synchronous: it reads the class stage's counters (they size the CSR's query
// column and the rectangle pass), the count pass's (they size the candidate list) and the totals.
#define GF_TU_NAME geomjoin_cpp
#include "gf_buildtag.hpp"  // first: records this unit's command-line defines

#include <hip/hip_runtime.h>

#include <cstring>

#include "gf_geom_index.hpp"
#include "gf_geomjoin_plan.hpp"

using namespace gf;

struct gf_geom_join {
  gf_ctx* ctx = nullptr;
  int32_t tile_side = 0;   // 0: the default of join_tile_shift
  int64_t long_tiles = kJoinLongTiles;
  int brute = 0;
  DevArr<uint32_t> short_o, long_o, short_q, long_q, act_q, tile_cnt, tile_off, tile_cur, tile_q, cand, scan_tmp;
  DevArr<int32_t> pcells;
  DevArr<unsigned long long> ctr;
  unsigned long long last[kGeomJoinCtrs] = {};  // the counters of the last run
};

extern "C" int gf_geom_join_create(gf_ctx* ctx, gf_geom_join** out) {
  if (!ctx || !out) return GF_ERR_ARG;
  gf_geom_join* J = new gf_geom_join();
  J->ctx = ctx;
  *out = J;
  return GF_OK;
}

extern "C" void gf_geom_join_destroy(gf_geom_join* J) {
  if (!J) return;
  hipSetDevice(J->ctx->device);
  hipStreamSynchronize(J->ctx->stream);
  delete J;
}

extern "C" int gf_geom_join_set_tuning(gf_geom_join* J, int32_t tile_side, int64_t long_tiles, int brute) {
  if (!J || tile_side < 0 || long_tiles < 0 || (brute != 0 && brute != 1)) return GF_ERR_ARG;
  J->tile_side = tile_side;
  J->long_tiles = long_tiles == 0 ? kJoinLongTiles : long_tiles;
  J->brute = brute;
  return GF_OK;
}

extern "C" int gf_geom_join_info(const gf_geom_join* J, int64_t* candidates, int64_t* box_dropped, int64_t* tested,
                                 int64_t* wave_path, int64_t* long_objects, int64_t* long_queries) {
  if (!J) return GF_ERR_ARG;
  const unsigned long long* c = J->last;
  if (candidates) *candidates = (int64_t)c[kGeomJoinCtrCand];
  if (box_dropped) *box_dropped = (int64_t)c[kGeomJoinCtrFar];
  if (tested) *tested = (int64_t)(c[kGeomJoinCtrLane] + c[kGeomJoinCtrWave]);
  if (wave_path) *wave_path = (int64_t)c[kGeomJoinCtrWave];
  if (long_objects) *long_objects = (int64_t)c[kGeomJoinCtrLongO];
  if (long_queries) *long_queries = (int64_t)c[kGeomJoinCtrLongQ];
  return GF_OK;
}

static void index_side(const gf_geom_index* X, GeomJoinSide& s) {
  const gf_geoms& G = X->geoms;
  s.kind = G.kind;
  s.wide_vertices = X->wide_vertices;
  s.n = G.nobj;
  s.ring_off = G.kind == GF_GEOM_POLYGON ? G.ring_off : nullptr;
  s.vert_off = G.vert_off; s.vx = G.vx; s.vy = G.vy;
  s.ring_env = X->ring_env.p; s.env = X->env.p; s.cells = X->cells.p; s.valid = X->valid.p; s.nvert = X->nvert.p;
}

static int read_counters(gf_geom_join* J, unsigned long long* out) {
  gf_ctx* ctx = J->ctx;
  int st = GF_OK;
  unsigned long long* h = (unsigned long long*)ctx_pinned(ctx, kGeomJoinCtrs * sizeof(unsigned long long), &st);
  if (!h) return st;
  GF_HIP_CHECK(ctx, hipMemcpyAsync(h, J->ctr.p, kGeomJoinCtrs * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
  GF_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  std::memcpy(out, h, kGeomJoinCtrs * sizeof(unsigned long long));
  return GF_OK;
}

// a filled in: the two sides, the query grid, r and the modes
static int join_run(gf_geom_join* J, GeomJoinArgs& a, uint32_t* pairs, int64_t cap, int64_t* npairs, int64_t* nrep) {
  gf_ctx* ctx = J->ctx;
  std::memset(J->last, 0, sizeof(J->last));
  *npairs = 0;
  *nrep = 0;
  if (a.o.n == 0 || a.q.n == 0) return GF_OK;
  int st = bind(ctx);
  if (st) return st;
  a.shift = join_tile_shift(a.n, a.c, J->tile_side);
  a.nt = join_tiles_side(a.n, a.shift);
  a.long_tiles = J->long_tiles;
  a.brute = J->brute;
  a.pairs = pairs;
  a.cap = pairs ? cap : 0;
  const size_t no = (size_t)a.o.n, nq = (size_t)a.q.n, ntiles = (size_t)(a.nt * a.nt);
  if ((st = J->short_o.reserve(ctx, no)) || (st = J->long_o.reserve(ctx, no)) || (st = J->short_q.reserve(ctx, nq)) ||
      (st = J->long_q.reserve(ctx, nq)) || (st = J->act_q.reserve(ctx, nq)) || (st = J->tile_cnt.reserve(ctx, ntiles)) ||
      (st = J->tile_cur.reserve(ctx, ntiles)) || (st = J->tile_off.reserve(ctx, ntiles + 1)) ||
      (st = J->scan_tmp.reserve(ctx, scan_tmp_elems((int64_t)ntiles))) || (st = J->ctr.reserve(ctx, kGeomJoinCtrs)) ||
      (a.q.kind == 0 && (st = J->pcells.reserve(ctx, 4 * nq))))
    return st;
  a.short_o = J->short_o.p; a.long_o = J->long_o.p; a.short_q = J->short_q.p; a.long_q = J->long_q.p; a.act_q = J->act_q.p;
  a.tile_cnt = J->tile_cnt.p; a.tile_cur = J->tile_cur.p; a.tile_off = J->tile_off.p; a.ctr = J->ctr.p;
  if (a.q.kind == 0) {
    a.pcells = J->pcells.p;
    a.q.cells = J->pcells.p;
  }
  GF_HIP_CHECK(ctx, hipMemsetAsync(J->ctr.p, 0, kGeomJoinCtrs * sizeof(unsigned long long), ctx->stream));
  GF_HIP_CHECK(ctx, hipMemsetAsync(J->tile_cnt.p, 0, ntiles * sizeof(uint32_t), ctx->stream));
  GF_HIP_CHECK(ctx, hipMemsetAsync(J->tile_cur.p, 0, ntiles * sizeof(uint32_t), ctx->stream));
  // bin
  if (a.q.kind == 0) GF_HIP_CHECK(ctx, launch_geomjoin(ctx, kGeomJoinPointCells, a));
  GF_HIP_CHECK(ctx, launch_geomjoin(ctx, kGeomJoinClass, a));
  {
    KTimer timer(ctx, GF_K_JOIN_BUCKET);
    GF_HIP_CHECK(ctx, launch_exclusive_scan(ctx->stream, J->tile_cnt.p, (int64_t)ntiles, J->tile_off.p, J->scan_tmp.p));
  }
  unsigned long long c[kGeomJoinCtrs];
  if ((st = read_counters(J, c))) return st;
  const unsigned long long entries = c[kGeomJoinCtrEntries];
  if (entries > (unsigned long long)UINT32_MAX)
    return set_err(ctx, GF_ERR_NOMEM, "gf_geom_join: more than 2^32 - 1 (tile, query) entries; lower long_tiles");
  if (entries) {
    if ((st = J->tile_q.reserve(ctx, (size_t)entries))) return st;
    a.tile_q = J->tile_q.p;
    GF_HIP_CHECK(ctx, launch_geomjoin(ctx, kGeomJoinScatter, a));
  }
  // probe: count, then write
  a.rect_pairs = c[kGeomJoinCtrLongO] * c[kGeomJoinCtrActQ] + c[kGeomJoinCtrShortO] * c[kGeomJoinCtrLongQ];
  GF_HIP_CHECK(ctx, launch_geomjoin(ctx, kGeomJoinProbeCount, a));
  if ((st = read_counters(J, c))) return st;
  if (!a.approx) {
    a.n_lane = c[kGeomJoinCtrLane];
    a.n_wave = c[kGeomJoinCtrWave];
    if (a.n_lane + a.n_wave > 0) {
      if ((st = J->cand.reserve(ctx, 3 * (size_t)(a.n_lane + a.n_wave)))) return st;
      a.cand = J->cand.p;
      GF_HIP_CHECK(ctx, launch_geomjoin(ctx, kGeomJoinProbeWrite, a));
      GF_HIP_CHECK(ctx, launch_geomjoin(ctx, kGeomJoinExact, a));
      if ((st = read_counters(J, c))) return st;
    }
  } else if (a.cap > 0 && c[kGeomJoinCtrHits] > 0) {
    GF_HIP_CHECK(ctx, launch_geomjoin(ctx, kGeomJoinProbeWrite, a));
    GF_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  }
  std::memcpy(J->last, c, sizeof(J->last));
  *npairs = (int64_t)c[kGeomJoinCtrHits];
  *nrep = (int64_t)c[kGeomJoinCtrRep];
  return *npairs > a.cap ? GF_ERR_CAPACITY : GF_OK;
}

extern "C" int gf_geom_join_run(gf_geom_join* J, gf_geom_index* ix_ord, gf_geom_index* ix_qry, double r, int approximate,
                                int metric, int first_is_ordinary, uint32_t* pairs, int64_t cap, int64_t* npairs,
                                int64_t* nrep) {
  if (!J || !ix_ord || !ix_qry || !npairs || !nrep) return GF_ERR_ARG;
  gf_ctx* ctx = J->ctx;
  if (ix_ord->ctx != ctx || ix_qry->ctx != ctx)
    return set_err(ctx, GF_ERR_ARG, "gf_geom_join_run: the joiner and the two indexes must belong to one context");
  if ((metric != 0 && metric != 1) || cap < 0 || (cap > 0 && !pairs) ||
      (first_is_ordinary && !(ix_ord->geoms.kind == GF_GEOM_POLYGON && ix_qry->geoms.kind == GF_GEOM_LINESTRING)))
    return set_err(ctx, GF_ERR_ARG, "gf_geom_join_run: bad argument (a metric, cap >= 0, first_is_ordinary only for "
                                    "polygons joined with linestrings)");
  GeomJoinArgs a{};
  index_side(ix_ord, a.o);
  index_side(ix_qry, a.q);
  const gf_grid& g = ix_qry->grid;
  a.qminX = g.minX; a.qminY = g.minY; a.qcl = g.cellLength; a.n = g.n;
  // getReplicated{Polygon,LineString}QueryStream: no getNeighboringCells, so c <= 0 is an empty K and no error
  a.c = candidate_layers(g.cellLength, r);
  a.out_members = a.c > 0 && guaranteed_layers(g.cellLength, r) == 0;
  a.r = r; a.approx = approximate != 0; a.metric = metric; a.first_is_ordinary = first_is_ordinary != 0;
  return join_run(J, a, pairs, cap, npairs, nrep);
}

extern "C" int gf_geom_join_run_points(gf_geom_join* J, gf_geom_index* ix_ord, const gf_grid* qgrid, const gf_points* q,
                                       double r, int approximate, int metric, uint32_t* pairs, int64_t cap,
                                       int64_t* npairs, int64_t* nrep) {
  if (!J || !ix_ord || !q || !npairs || !nrep) return GF_ERR_ARG;
  gf_ctx* ctx = J->ctx;
  if (ix_ord->ctx != ctx)
    return set_err(ctx, GF_ERR_ARG, "gf_geom_join_run_points: the joiner and the index must belong to one context");
  if (!grid_ok(qgrid) || (metric != 0 && metric != 1) || cap < 0 || (cap > 0 && !pairs))
    return set_err(ctx, GF_ERR_ARG, "gf_geom_join_run_points: bad argument (a grid, a metric, cap >= 0)");
  if (int st = check_points(ctx, q)) return st;
  GeomJoinArgs a{};
  index_side(ix_ord, a.o);
  a.q.kind = 0;
  a.q.n = q->n;
  a.px = q->x; a.py = q->y;
  a.qminX = qgrid->minX; a.qminY = qgrid->minY; a.qcl = qgrid->cellLength; a.n = qgrid->n;
  // getNeighboringCells: r == 0 is every valid cell; otherwise the candidate layers must be positive
  a.c = candidate_layers(qgrid->cellLength, r);
  a.whole = r == 0.0;
  if (!a.whole && a.c <= 0) return set_err(ctx, GF_ERR_LAYERS, "candidateNeighboringLayers cannot be 0 or less");
  a.r = r; a.approx = approximate != 0; a.metric = metric;
  return join_run(J, a, pairs, cap, npairs, nrep);
}
