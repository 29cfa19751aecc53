// trange.cpp -- tRange entry points of the C ABI (tRange/PointPolygonTRangeQuery.java): the plan built
// once per continuous query (its pure host part is gf_trange_plan.hpp's), gf_trange_points (RealTime:
// the contained points' bitmap, enqueued) and gf_trange_run (WindowBased: the trajectories with a
// contained point, each whole; the CSR is traj.cpp's traj_emit, shared with gf_traj_select and
// gf_tfilter_run).  The kernels are in k_trange.hip.  The plan's device tables and the wave path's
// worklist (grow-only) are gf_group.hpp's typed device arrays, freed by its destructor.
#define GF_TU_NAME trange_cpp
#include "gf_buildtag.hpp"  // first: records this unit's command-line defines

#include <hip/hip_runtime.h>

#include "gf_group.hpp"
#include "gf_trange_plan.hpp"

using namespace gf;

struct gf_trange_plan {
  gf_ctx* ctx = nullptr;
  gf_grid grid{};
  TrangeTables tab;  // host: the stats, max_ring for set_thresholds
  int32_t wide_ring = kTrangeWideRing;
  int64_t wide_polygons = 0;
  int64_t max_wide = 0;  // the most wide candidates any one point can have
  int64_t cell_points = 0, inside_points = 0;
  int wave_path = 0;  // the last gf_trange_points / gf_trange_run tested its wide polygons by waves
  DevArr<uint8_t> cls, wide;
  DevArr<int32_t> cand_off, cand_list, extra, ring_off, vert_off;
  DevArr<double> vx, vy, ring_env;
  DevArr<unsigned long long> ctr;
  DevArr<uint2> work;
};

// the worklist never outgrows this: a window whose bound is larger tests every polygon by its lane
// (identical results)
static constexpr size_t kTrangeMaxWorkBytes = (size_t)1 << 30;

// which polygons take the wave path, and the most of them one point can meet
static int trange_apply_wide(gf_trange_plan* P) {
  const TrangeTables& T = P->tab;
  std::vector<uint8_t> w((size_t)std::max(T.npoly, 1), 0);
  P->wide_polygons = 0;
  for (int32_t p = 0; p < T.npoly; ++p) {
    w[p] = T.max_ring[p] >= P->wide_ring;
    P->wide_polygons += w[p];
  }
  int64_t mx = 0;
  const int64_t cells = (int64_t)T.n * T.n;
  for (int64_t c = 0; c < cells && P->wide_polygons; ++c) {
    int64_t k = 0;
    for (int32_t e = T.cand_off[c]; e < T.cand_off[c + 1]; ++e) k += w[T.cand_list[e]];
    mx = std::max(mx, k);
  }
  int64_t ex = 0;  // (an outside cell meets at most every extra polygon)
  for (size_t e = 0; e < T.extra.size(); e += 5) ex += w[T.extra[e]];
  P->max_wide = std::max(mx, ex);
  GF_HIP_CHECK(P->ctx, hipStreamSynchronize(P->ctx->stream));  // queued work may still read the flags
  GF_HIP_CHECK(P->ctx, hipMemcpy(P->wide.p, w.data(), w.size(), hipMemcpyHostToDevice));
  return GF_OK;
}

extern "C" void gf_trange_plan_destroy(gf_trange_plan* P) {
  if (!P) return;
  hipSetDevice(P->ctx->device);
  hipStreamSynchronize(P->ctx->stream);
  delete P;
}

extern "C" int gf_trange_plan_create(gf_ctx* ctx, const gf_grid* g, const gf_polygons* polys, gf_trange_plan** out) {
  if (!ctx || !out || !grid_ok(g) || !polys || polys->npoly < 0 ||
      (polys->npoly > 0 && (!polys->ring_off || !polys->vert_off || !polys->vx || !polys->vy)))
    return set_err(ctx, GF_ERR_ARG, "gf_trange_plan_create: bad argument");
  *out = nullptr;
  gf_trange_plan* P = new gf_trange_plan();
  P->ctx = ctx;
  P->grid = *g;
  static const char* const why[] = {"", "polygon without a shell", "ring must be closed with >= 4 vertices",
                                    "grid too large for a cell table", "cell lists too large"};
  const int bad = trange_build_tables(*g, *polys, P->tab);
  if (bad) {
    delete P;
    return set_err(ctx, bad == 4 ? GF_ERR_NOMEM : GF_ERR_ARG, std::string("gf_trange_plan_create: ") + why[bad]);
  }
  int st = bind(ctx);
  if (st) { delete P; return st; }
  const TrangeTables& T = P->tab;
  const int32_t np = T.npoly, nverts = T.nrings > 0 ? polys->vert_off[T.nrings] : 0;
  std::vector<int32_t> ro(1, 0), vo(1, 0);
  if (np > 0) {
    ro.assign(polys->ring_off, polys->ring_off + np + 1);
    vo.assign(polys->vert_off, polys->vert_off + T.nrings + 1);
  }
  std::vector<double> vx(polys->vx, polys->vx + nverts), vy(polys->vy, polys->vy + nverts);
  std::vector<uint8_t> w((size_t)std::max(np, 1), 0);
  std::vector<unsigned long long> zero(4, 0);
  if ((st = upload(ctx, P->cls, T.cls)) || (st = upload(ctx, P->cand_off, T.cand_off)) ||
      (st = upload(ctx, P->cand_list, T.cand_list)) || (st = upload(ctx, P->extra, T.extra)) ||
      (st = upload(ctx, P->ring_off, ro)) || (st = upload(ctx, P->vert_off, vo)) || (st = upload(ctx, P->vx, vx)) ||
      (st = upload(ctx, P->vy, vy)) || (st = upload(ctx, P->ring_env, T.ring_env)) || (st = upload(ctx, P->wide, w)) ||
      (st = upload(ctx, P->ctr, zero)) || (st = trange_apply_wide(P))) {
    gf_trange_plan_destroy(P);
    return st;
  }
  *out = P;
  return GF_OK;
}

extern "C" int gf_trange_plan_stats(const gf_trange_plan* P, int64_t* none_cells, int64_t* test_cells, int64_t* inside_cells,
                                    int64_t* list_entries, int64_t* wide_polygons) {
  if (!P) return GF_ERR_ARG;
  if (none_cells) *none_cells = P->tab.cells[kTrNone];
  if (test_cells) *test_cells = P->tab.cells[kTrTest];
  if (inside_cells) *inside_cells = P->tab.cells[kTrInside];
  if (list_entries) *list_entries = (int64_t)P->tab.cand_list.size();
  if (wide_polygons) *wide_polygons = P->wide_polygons;
  return GF_OK;
}

extern "C" int gf_trange_plan_set_thresholds(gf_trange_plan* P, int32_t wide_ring) {
  if (!P || wide_ring < 0) return GF_ERR_ARG;
  int st = bind(P->ctx);
  if (st) return st;
  P->wide_ring = wide_ring == 0 ? kTrangeWideRing : wide_ring;
  return trange_apply_wide(P);
}

extern "C" int gf_trange_info(const gf_trange_plan* P, int64_t* cell_points, int64_t* inside_points, int64_t* wide_ring,
                              int64_t* wave_path) {
  if (!P) return GF_ERR_ARG;
  if (cell_points) *cell_points = P->cell_points;
  if (inside_points) *inside_points = P->inside_points;
  if (wide_ring) *wide_ring = P->wide_ring;
  if (wave_path) *wave_path = P->wave_path;
  return GF_OK;
}

// the arguments of one window; the worklist sized for it (or the wave path off), the counters zeroed
static int trange_args(gf_trange_plan* P, const gf_points* pts, TrangeArgs& a) {
  gf_ctx* ctx = P->ctx;
  a.x = pts->x; a.y = pts->y; a.n = pts->n;
  a.grid_n = P->grid.n; a.minX = P->grid.minX; a.minY = P->grid.minY; a.cl = P->grid.cellLength;
  a.cls = P->cls.p; a.cand_off = P->cand_off.p; a.cand_list = P->cand_list.p;
  a.extra = P->extra.p; a.n_extra = (int32_t)(P->tab.extra.size() / 5);
  a.poly.ring_off = P->ring_off.p; a.poly.vert_off = P->vert_off.p; a.poly.vx = P->vx.p; a.poly.vy = P->vy.p;
  a.poly.ring_env = P->ring_env.p; a.poly.metric = 0; a.poly.rect = nullptr;
  a.ctr = P->ctr.p;
  a.wide = nullptr;
  a.work = nullptr;
  a.work_cap = 0;
  P->wave_path = 0;
  if (P->max_wide > 0 && (size_t)P->max_wide <= kTrangeMaxWorkBytes / sizeof(uint2) / (size_t)pts->n) {
    const size_t cap = (size_t)P->max_wide * (size_t)pts->n;
    if (int st = P->work.reserve(ctx, cap)) return st;
    a.wide = P->wide.p;
    a.work = P->work.p;
    a.work_cap = (uint32_t)cap;
    P->wave_path = 1;
  }
  GF_HIP_CHECK(ctx, hipMemsetAsync(a.ctr, 0, 4 * sizeof(unsigned long long), ctx->stream));
  return GF_OK;
}

extern "C" int gf_trange_points(gf_trange_plan* P, const gf_points* pts, uint64_t* bitmap, int64_t* count) {
  if (!P) return GF_ERR_ARG;
  gf_ctx* ctx = P->ctx;
  if (!pts || pts->n < 0 || pts->n > (int64_t)UINT32_MAX || (pts->n > 0 && (!pts->x || !pts->y || !bitmap)))
    return set_err(ctx, GF_ERR_ARG, "gf_trange_points: bad argument");
  int st = bind(ctx);
  if (st) return st;
  if (pts->n == 0) {
    if (count) GF_HIP_CHECK(ctx, hipMemsetAsync(count, 0, sizeof(int64_t), ctx->stream));
    return GF_OK;
  }
  TrangeArgs a{};
  if ((st = trange_args(P, pts, a))) return st;
  a.bitmap = bitmap;
  a.count = count;
  GF_HIP_CHECK(ctx, launch_trange(ctx, kTrangeMark, a));
  if (a.wide) GF_HIP_CHECK(ctx, launch_trange(ctx, kTrangeWaves, a));
  if (count) GF_HIP_CHECK(ctx, launch_trange(ctx, kTrangeCount, a));
  return GF_OK;
}

extern "C" int gf_trange_run(gf_trange_plan* P, gf_traj_groups* G, const gf_points* pts, int64_t* keys, int64_t* off,
                             int64_t cap_traj, double* x, double* y, int64_t* ts, uint32_t* idx, int64_t cap_pts,
                             int64_t* ntraj_out, int64_t* npts_out) {
  if (!P || !G || !G->ctx) return GF_ERR_ARG;
  gf_ctx* ctx = G->ctx;
  if (P->ctx != ctx) return set_err(ctx, GF_ERR_ARG, "gf_trange_run: plan and groups of different contexts");
  if (!ntraj_out || !npts_out || cap_traj < 0 || cap_pts < 0) return set_err(ctx, GF_ERR_ARG, "gf_trange_run: bad argument");
  int st = traj_check_points(G, pts, "gf_trange_run");
  if (st) return st;
  *ntraj_out = 0;
  *npts_out = 0;
  if (off) off[0] = 0;
  P->cell_points = P->inside_points = 0;
  if (G->ntraj == 0) return GF_OK;
  if ((st = bind(ctx)) || (st = traj_hit_clear(G))) return st;
  TrangeArgs a{};
  if ((st = trange_args(P, pts, a))) return st;
  a.did = G->did.p;
  a.hit = G->hit.p;
  GF_HIP_CHECK(ctx, launch_trange(ctx, kTrangeMark, a));
  if (a.wide) GF_HIP_CHECK(ctx, launch_trange(ctx, kTrangeWaves, a));
  // the counters ride to pinned staging behind the kernels; the emit's synchronisation completes the copy
  unsigned long long* c = (unsigned long long*)ctx_pinned(ctx, 4 * sizeof(unsigned long long), &st);
  if (!c) return st;
  GF_HIP_CHECK(ctx, hipMemcpyAsync(c, a.ctr, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
  if ((st = traj_emit(G, pts, keys, off, cap_traj, x, y, ts, idx, cap_pts, ntraj_out, npts_out))) return st;
  P->cell_points = (int64_t)c[1];
  P->inside_points = (int64_t)c[2];
  return GF_OK;
}
