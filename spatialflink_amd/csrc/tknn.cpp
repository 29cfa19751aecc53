// tknn.cpp -- tKnn entry points of the C ABI (tKnn/PointPointTKNNQuery.java windowBased /
// windowBasedNaive, TKNNQuery.java:50-101): gf_tknn_run over a window already grouped by objID
// (gf_traj_group), the read and the testing hook.  The kernels are in k_tknn.hip; the groupings by
// cell and by (cell, trajectory), the sort of the pairs by cell and the multi-word sorts are
// gf_group.hpp's (traj.cpp), run on k_points.hip's radix passes.  The object is made of gf_group.hpp's
// typed device arrays (grow-only, freed by its destructor) and is reused across windows.
#define GF_TU_NAME tknn_cpp
#include "gf_buildtag.hpp"  // first: records this unit's command-line defines

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "gf_group.hpp"

using namespace gf;

struct gf_tknn {
  gf_ctx* ctx = nullptr;
  int64_t rows = 0, npts = 0, in_cells = 0, npairs = 0, records = 0;
  int64_t big_cell = kTknnBigCell;
  KeyGroups cells, pairs;  // dense ids of the entries' packed cells and of their (cell, trajectory) keys
  KeyGroups bycell;        // the pairs sorted by cell id (sort only)
  KeyGroups srt;           // the multi-word sorts' radix workspace
  DevArr<int64_t> e_ckey, comp, o_key, o_ts;
  DevArr<unsigned long long> e_d, p_d, tr_D;
  DevArr<uint32_t> e_t, e_i, counters, p_first, p_cell, p_rec, wkey, sp[2], tr_cells, surv, srank, slist, o_traj, o_len,
      o_off, o_idx;
  DevArr<double> o_dist, o_x, o_y;
  DevArr<int32_t> o_cells;
};

static int tknn_window(gf_tknn* T, gf_traj_groups* G, const gf_grid* grid, const gf_points* pts, double qx, double qy,
                       int32_t xlo, int32_t xhi, int32_t ylo, int32_t yhi, int32_t k, int naive) {
  gf_ctx* ctx = T->ctx;
  int st = GF_OK;
  const int64_t n = G->n, nt = G->ntraj;
  const size_t np = (size_t)n, ntz = (size_t)nt;
  if ((st = T->e_ckey.reserve(ctx, np)) || (st = T->e_t.reserve(ctx, np)) || (st = T->e_d.reserve(ctx, np)) ||
      (st = T->e_i.reserve(ctx, np)) || (st = T->counters.reserve(ctx, kCounterWords)))
    return st;
  TknnArgs a{};
  a.x = pts->x; a.y = pts->y; a.ts = pts->ts;
  a.did = G->did.p;
  a.n = n;
  a.minX = grid->minX; a.minY = grid->minY; a.cl = grid->cellLength;
  a.qx = qx; a.qy = qy;
  a.xlo = xlo; a.xhi = xhi; a.ylo = ylo; a.yhi = yhi;
  a.naive = naive;
  a.k = k;
  a.e_ckey = T->e_ckey.p; a.e_t = T->e_t.p; a.e_d = T->e_d.p; a.e_i = T->e_i.p; a.counters = T->counters.p;
  GF_HIP_CHECK(ctx, hipMemsetAsync(a.counters, 0, kCounterWords * sizeof(uint32_t), ctx->stream));
  GF_HIP_CHECK(ctx, launch_tknn(ctx, kTknnScanWindow, a));
  uint32_t m32 = 0;
  if ((st = read_scalar_sync(ctx, a.counters, &m32))) return st;
  const int64_t m = m32;
  if (m > n) return set_err(ctx, GF_ERR_HIP, "gf_tknn_run: inconsistent entry count");
  T->in_cells = m;
  if (m == 0) return GF_OK;
  a.m = m;
  // the entries' cells and (cell, trajectory) pairs
  if ((st = group_dense_ids(ctx, T->cells, a.e_ckey, m, "gf_tknn_run"))) return st;
  if ((st = T->comp.reserve(ctx, (size_t)m))) return st;
  a.cid = T->cells.did.p;
  a.comp = T->comp.p;
  GF_HIP_CHECK(ctx, launch_tknn(ctx, kTknnCompose, a));
  if ((st = group_dense_ids(ctx, T->pairs, a.comp, m, "gf_tknn_run"))) return st;
  const int64_t npairs = T->pairs.ngroups, ncells = T->cells.ngroups;
  T->npairs = npairs;
  const size_t nq = (size_t)npairs;
  if ((st = T->p_first.reserve(ctx, nq)) || (st = T->p_d.reserve(ctx, nq)) || (st = T->p_cell.reserve(ctx, nq)) ||
      (st = T->p_rec.reserve(ctx, nq)) || (st = T->tr_D.reserve(ctx, ntz)) || (st = T->tr_cells.reserve(ctx, ntz)) ||
      (st = T->surv.reserve(ctx, ntz + 1)) || (st = T->srank.reserve(ctx, ntz + 1)) || (st = T->slist.reserve(ctx, ntz)))
    return st;
  a.pid = T->pairs.did.p;
  a.npairs = npairs;
  a.pkeys = T->pairs.keys.p;
  a.p_first = T->p_first.p; a.p_d = T->p_d.p; a.p_cell = T->p_cell.p; a.p_rec = T->p_rec.p;
  GF_HIP_CHECK(ctx, launch_tknn(ctx, kTknnPairMin, a));
  // the cells' lists: pairs sorted stably by cell id (every cell has a pair)
  if ((st = group_sort_ids(ctx, T->bycell, a.p_cell, npairs, (uint32_t)ncells))) return st;
  a.gperm = T->bycell.perm.p;
  a.gcell = T->bycell.kbuf[T->bycell.sorted_in].p;
  a.cell_off = T->bycell.seg_off.p;
  a.big_cell = (uint32_t)T->big_cell;
  GF_HIP_CHECK(ctx, launch_tknn(ctx, kTknnRankSmall, a));
  uint32_t nbig = 0;
  if ((st = read_scalar_sync(ctx, a.counters + 1, &nbig))) return st;
  if (nbig > 0) {
    const unsigned long long* pk = (const unsigned long long*)a.pkeys;
    const SortWord words[4] = {{pk, nullptr, 0, key_bits((uint64_t)nt)},
                               {a.p_d, nullptr, 0, 32},
                               {a.p_d, nullptr, 32, 32},
                               {pk, nullptr, 32, key_bits((uint64_t)ncells)}};
    if ((st = group_sort_words(ctx, T->srt, T->wkey, T->sp, words, 4, npairs, nullptr, &a.sperm))) return st;
    GF_HIP_CHECK(ctx, launch_tknn(ctx, kTknnRankBig, a));
  }
  // per trajectory: D_t, cells_t, the size rule
  a.ntraj = nt;
  a.seg_off = G->seg_off.p;
  a.tr_D = T->tr_D.p; a.tr_cells = T->tr_cells.p; a.surv = T->surv.p; a.srank = T->srank.p; a.slist = T->slist.p;
  GF_HIP_CHECK(ctx, launch_tknn(ctx, kTknnCombine, a));
  if ((st = group_scan_u32(ctx, T->srt, a.surv, nt, T->srank.p))) return st;
  GF_HIP_CHECK(ctx, launch_tknn(ctx, kTknnSurvivors, a));
  uint32_t tot[4] = {0, 0, 0, 0};  // survivors, -, records
  GF_HIP_CHECK(ctx, hipMemcpyAsync(&tot[0], a.srank + nt, sizeof tot[0], hipMemcpyDeviceToHost, ctx->stream));
  GF_HIP_CHECK(ctx, hipMemcpyAsync(&tot[2], a.counters + 2, sizeof tot[2], hipMemcpyDeviceToHost, ctx->stream));
  GF_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  T->records = tot[2];
  const int64_t nsurv = tot[0];
  if (nsurv > nt) return set_err(ctx, GF_ERR_HIP, "gf_tknn_run: inconsistent survivor count");
  if (nsurv == 0) return GF_OK;
  // the survivors (ascending t) sorted stably by D_t = by (D_t, t); the first k are the rows
  const SortWord dw[2] = {{a.tr_D, a.slist, 0, 32}, {a.tr_D, a.slist, 32, 32}};
  if ((st = group_sort_words(ctx, T->srt, T->wkey, T->sp, dw, 2, nsurv, nullptr, &a.order))) return st;
  const int64_t rows = std::min<int64_t>(nsurv, k);
  const size_t nr = (size_t)rows;
  if ((st = T->o_key.reserve(ctx, nr)) || (st = T->o_dist.reserve(ctx, nr)) || (st = T->o_cells.reserve(ctx, nr)) ||
      (st = T->o_traj.reserve(ctx, nr)) || (st = T->o_len.reserve(ctx, nr + 1)) || (st = T->o_off.reserve(ctx, nr + 1)))
    return st;
  a.rows = rows;
  a.tkeys = G->keys.p;
  a.perm = G->perm.p;
  a.o_key = T->o_key.p; a.o_dist = T->o_dist.p; a.o_cells = T->o_cells.p; a.o_traj = T->o_traj.p; a.o_len = T->o_len.p;
  a.o_off = T->o_off.p;
  GF_HIP_CHECK(ctx, launch_tknn(ctx, kTknnRows, a));
  if ((st = group_scan_u32(ctx, T->srt, a.o_len, rows, T->o_off.p))) return st;
  uint32_t npts = 0;
  if ((st = read_scalar_sync(ctx, a.o_off + rows, &npts))) return st;
  if ((int64_t)npts > n) return set_err(ctx, GF_ERR_HIP, "gf_tknn_run: inconsistent point count");
  const size_t no = (size_t)npts;
  if ((st = T->o_x.reserve(ctx, no)) || (st = T->o_y.reserve(ctx, no)) || (st = T->o_ts.reserve(ctx, no)) ||
      (st = T->o_idx.reserve(ctx, no)))
    return st;
  a.npts = npts;
  a.o_x = T->o_x.p; a.o_y = T->o_y.p; a.o_ts = T->o_ts.p; a.o_idx = T->o_idx.p;
  GF_HIP_CHECK(ctx, launch_tknn(ctx, kTknnGather, a));
  GF_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  T->rows = rows;
  T->npts = npts;
  return GF_OK;
}

extern "C" int gf_tknn_run(gf_traj_groups* G, const gf_grid* grid, const gf_points* pts, double qx, double qy, double r,
                           int32_t k, int mode, gf_tknn** out) {
  if (!G || !G->ctx) return GF_ERR_ARG;
  gf_ctx* ctx = G->ctx;
  if (!out || !grid || !pts) return set_err(ctx, GF_ERR_ARG, "gf_tknn_run: null argument");
  if (!grid_ok(grid)) return set_err(ctx, GF_ERR_ARG, "gf_tknn_run: invalid grid");
  if (k < 1) return set_err(ctx, GF_ERR_ARG, "gf_tknn_run: k < 1");
  if (mode != GF_TKNN_GRID && mode != GF_TKNN_NAIVE) return set_err(ctx, GF_ERR_ARG, "gf_tknn_run: unknown mode");
  if (std::isnan(qx) || std::isnan(qy) || std::isnan(r) || r < 0.0)
    return set_err(ctx, GF_ERR_ARG, "gf_tknn_run: NaN query coordinate or NaN / negative radius");
  if (pts->n != G->n) return set_err(ctx, GF_ERR_ARG, "gf_tknn_run: pts is not the grouped window");
  if (pts->n > 0 && (!pts->x || !pts->y || !pts->objID || !pts->ts))
    return set_err(ctx, GF_ERR_ARG, "gf_tknn_run: null x / y / objID / ts");
  if (*out && (*out)->ctx != ctx) return set_err(ctx, GF_ERR_ARG, "gf_tknn_run: object of another context");
  // N as a rectangle of cells (UniformGrid.java:261-293: within L layers of the query cell and validKey)
  int64_t xlo = 0, xhi = (int64_t)grid->n - 1, ylo = 0, yhi = (int64_t)grid->n - 1;
  if (mode == GF_TKNN_GRID && r != 0.0) {
    const int32_t L = candidate_layers(grid->cellLength, r);
    if (L <= 0) return set_err(ctx, GF_ERR_LAYERS, "candidateNeighboringLayers cannot be 0 or less");
    const int64_t qcx = cell_index(qx, grid->minX, grid->cellLength), qcy = cell_index(qy, grid->minY, grid->cellLength);
    xlo = std::max<int64_t>(qcx - L, xlo); xhi = std::min<int64_t>(qcx + L, xhi);
    ylo = std::max<int64_t>(qcy - L, ylo); yhi = std::min<int64_t>(qcy + L, yhi);
  }
  const bool empty_n = mode == GF_TKNN_GRID && (xlo > xhi || ylo > yhi);
  int st = bind(ctx);
  if (st) return st;
  const bool fresh = *out == nullptr;
  gf_tknn* T = fresh ? new gf_tknn() : *out;
  T->ctx = ctx;
  T->rows = T->npts = T->in_cells = T->npairs = T->records = 0;
  if (G->n > 0 && !empty_n)
    st = tknn_window(T, G, grid, pts, qx, qy, (int32_t)xlo, (int32_t)xhi, (int32_t)ylo, (int32_t)yhi, k,
                     mode == GF_TKNN_NAIVE ? 1 : 0);
  if (st) {
    if (fresh) gf_tknn_destroy(T);
    else T->rows = T->npts = 0;
    return st;
  }
  *out = T;
  return GF_OK;
}

extern "C" void gf_tknn_destroy(gf_tknn* T) {
  if (!T) return;
  if (T->ctx) {
    hipSetDevice(T->ctx->device);
    hipStreamSynchronize(T->ctx->stream);
  }
  delete T;
}

extern "C" int gf_tknn_info(const gf_tknn* T, int64_t* rows, int64_t* npts, int64_t* in_cells, int64_t* pairs,
                            int64_t* records) {
  if (!T) return GF_ERR_ARG;
  if (rows) *rows = T->rows;
  if (npts) *npts = T->npts;
  if (in_cells) *in_cells = T->in_cells;
  if (pairs) *pairs = T->npairs;
  if (records) *records = T->records;
  return GF_OK;
}

extern "C" int gf_tknn_set_thresholds(gf_tknn* T, int64_t big_cell) {
  if (!T || big_cell < 0 || big_cell > (int64_t)UINT32_MAX) return GF_ERR_ARG;
  T->big_cell = big_cell == 0 ? kTknnBigCell : big_cell;
  return GF_OK;
}

extern "C" int gf_tknn_read(gf_tknn* T, int64_t* keys, double* dist, int32_t* cells, int64_t* off, int64_t cap_rows,
                            double* x, double* y, int64_t* ts, uint32_t* idx, int64_t cap_pts) {
  if (!T || !T->ctx) return GF_ERR_ARG;
  gf_ctx* ctx = T->ctx;
  if (cap_rows < 0 || cap_pts < 0) return set_err(ctx, GF_ERR_ARG, "gf_tknn_read: bad argument");
  if (off) off[0] = 0;
  if (T->rows == 0) return GF_OK;
  int st = bind(ctx);
  if (st) return st;
  const size_t wr = (size_t)std::min(T->rows, cap_rows), wp = (size_t)std::min(T->npts, cap_pts);
  OffsetRead ho;
  if ((st = read_back(ctx, keys, T->o_key.p, wr)) || (st = read_back(ctx, dist, T->o_dist.p, wr)) ||
      (st = read_back(ctx, cells, T->o_cells.p, wr)) || (st = read_offsets(ctx, ho, off, T->o_off.p, wr + 1)) ||
      (st = read_back(ctx, x, T->o_x.p, wp)) || (st = read_back(ctx, y, T->o_y.p, wp)) ||
      (st = read_back(ctx, ts, T->o_ts.p, wp)) || (st = read_back(ctx, idx, T->o_idx.p, wp)))
    return st;
  GF_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  ho.widen();
  return GF_OK;
}
