// tknn.cpp -- tKnn entry points of the C ABI (tKnn/PointPointTKNNQuery.java windowBased /
// windowBasedNaive, TKNNQuery.java:50-101): gf_tknn_run over a window already grouped by objID
// (gf_traj_group), the read and the testing hook.  The kernels are in k_tknn.hip; the groupings by
// cell and by (cell, trajectory), the sort of the pairs by cell and the multi-word sorts are
// gf_group.hpp's (traj.cpp), run on k_points.hip's radix passes.  The object owns its device workspace (grow-only)
// and is reused across windows.
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
  DevBuf e_ckey, e_t, e_d, e_i, comp, counters, p_first, p_d, p_cell, p_rec, wkey, sp[2], tr_D, tr_cells, surv, srank,
      slist, o_key, o_dist, o_cells, o_traj, o_len, o_off, o_x, o_y, o_ts, o_idx;
  DevBuf* all[30] = {&e_ckey, &e_t, &e_d, &e_i, &comp, &counters, &p_first, &p_d, &p_cell, &p_rec, &wkey, &sp[0], &sp[1],
                     &tr_D, &tr_cells, &surv, &srank, &slist, &o_key, &o_dist, &o_cells, &o_traj, &o_len, &o_off, &o_x,
                     &o_y, &o_ts, &o_idx, nullptr, nullptr};
};

template <class T>
static int read_back(gf_ctx* ctx, T* host, const void* dev, size_t count) {
  if (!host || count == 0) return GF_OK;
  GF_HIP_CHECK(ctx, hipMemcpyAsync(host, dev, count * sizeof(T), hipMemcpyDeviceToHost, ctx->stream));
  return GF_OK;
}

static int key_bits(uint64_t nids) {
  int bits = 1;
  while (((uint64_t)1 << bits) < nids) ++bits;
  return bits;
}

static int tknn_window(gf_tknn* T, gf_traj_groups* G, const gf_grid* grid, const gf_points* pts, double qx, double qy,
                       int32_t xlo, int32_t xhi, int32_t ylo, int32_t yhi, int32_t k, int naive) {
  gf_ctx* ctx = T->ctx;
  int st = GF_OK;
  const int64_t n = G->n, nt = G->ntraj;
  const size_t np = (size_t)n, ntz = (size_t)nt;
  if ((st = T->e_ckey.reserve(ctx, np * 8)) || (st = T->e_t.reserve(ctx, np * 4)) || (st = T->e_d.reserve(ctx, np * 8)) ||
      (st = T->e_i.reserve(ctx, np * 4)) || (st = T->counters.reserve(ctx, 16)))
    return st;
  TknnArgs a{};
  a.x = pts->x; a.y = pts->y; a.ts = pts->ts;
  a.did = G->did.as<uint32_t>();
  a.n = n;
  a.minX = grid->minX; a.minY = grid->minY; a.cl = grid->cellLength;
  a.qx = qx; a.qy = qy;
  a.xlo = xlo; a.xhi = xhi; a.ylo = ylo; a.yhi = yhi;
  a.naive = naive;
  a.k = k;
  a.e_ckey = T->e_ckey.as<int64_t>(); a.e_t = T->e_t.as<uint32_t>();
  a.e_d = T->e_d.as<unsigned long long>(); a.e_i = T->e_i.as<uint32_t>();
  a.counters = T->counters.as<uint32_t>();
  GF_HIP_CHECK(ctx, hipMemsetAsync(a.counters, 0, 16, ctx->stream));
  GF_HIP_CHECK(ctx, launch_tknn(ctx, 0, a));
  uint32_t m32 = 0;
  if ((st = read_scalar_sync(ctx, a.counters, &m32))) return st;
  const int64_t m = m32;
  if (m > n) return set_err(ctx, GF_ERR_HIP, "gf_tknn_run: inconsistent entry count");
  T->in_cells = m;
  if (m == 0) return GF_OK;
  a.m = m;
  // the entries' cells and (cell, trajectory) pairs
  if ((st = group_dense_ids(ctx, T->cells, a.e_ckey, m, "gf_tknn_run"))) return st;
  if ((st = T->comp.reserve(ctx, (size_t)m * 8))) return st;
  a.cid = T->cells.did.as<uint32_t>();
  a.comp = T->comp.as<int64_t>();
  GF_HIP_CHECK(ctx, launch_tknn(ctx, 1, a));
  if ((st = group_dense_ids(ctx, T->pairs, a.comp, m, "gf_tknn_run"))) return st;
  const int64_t npairs = T->pairs.ngroups, ncells = T->cells.ngroups;
  T->npairs = npairs;
  const size_t nq = (size_t)npairs;
  if ((st = T->p_first.reserve(ctx, nq * 4)) || (st = T->p_d.reserve(ctx, nq * 8)) || (st = T->p_cell.reserve(ctx, nq * 4)) ||
      (st = T->p_rec.reserve(ctx, nq * 4)) || (st = T->tr_D.reserve(ctx, ntz * 8)) ||
      (st = T->tr_cells.reserve(ctx, ntz * 4)) || (st = T->surv.reserve(ctx, (ntz + 1) * 4)) ||
      (st = T->srank.reserve(ctx, (ntz + 1) * 4)) || (st = T->slist.reserve(ctx, ntz * 4)))
    return st;
  a.pid = T->pairs.did.as<uint32_t>();
  a.npairs = npairs;
  a.pkeys = T->pairs.keys.as<int64_t>();
  a.p_first = T->p_first.as<uint32_t>(); a.p_d = T->p_d.as<unsigned long long>();
  a.p_cell = T->p_cell.as<uint32_t>(); a.p_rec = T->p_rec.as<uint32_t>();
  GF_HIP_CHECK(ctx, launch_tknn(ctx, 2, a));
  // the cells' lists: pairs sorted stably by cell id (every cell has a pair)
  if ((st = group_sort_ids(ctx, T->bycell, a.p_cell, npairs, (uint32_t)ncells))) return st;
  a.gperm = T->bycell.perm.as<uint32_t>();
  a.gcell = T->bycell.kbuf[T->bycell.sorted_in].as<uint32_t>();
  a.cell_off = T->bycell.seg_off.as<uint32_t>();
  a.big_cell = (uint32_t)T->big_cell;
  GF_HIP_CHECK(ctx, launch_tknn(ctx, 3, a));
  uint32_t nbig = 0;
  if ((st = read_scalar_sync(ctx, a.counters + 1, &nbig))) return st;
  if (nbig > 0) {
    const unsigned long long* pk = (const unsigned long long*)a.pkeys;
    const SortWord words[4] = {{pk, nullptr, 0, key_bits((uint64_t)nt)},
                               {a.p_d, nullptr, 0, 32},
                               {a.p_d, nullptr, 32, 32},
                               {pk, nullptr, 32, key_bits((uint64_t)ncells)}};
    if ((st = group_sort_words(ctx, T->srt, T->wkey, T->sp, words, 4, npairs, nullptr, &a.sperm))) return st;
    GF_HIP_CHECK(ctx, launch_tknn(ctx, 4, a));
  }
  // per trajectory: D_t, cells_t, the size rule
  a.ntraj = nt;
  a.seg_off = G->seg_off.as<uint32_t>();
  a.tr_D = T->tr_D.as<unsigned long long>(); a.tr_cells = T->tr_cells.as<uint32_t>();
  a.surv = T->surv.as<uint32_t>(); a.srank = T->srank.as<uint32_t>(); a.slist = T->slist.as<uint32_t>();
  GF_HIP_CHECK(ctx, launch_tknn(ctx, 5, a));
  if ((st = group_scan_u32(ctx, T->srt, a.surv, nt, T->srank.as<uint32_t>()))) return st;
  GF_HIP_CHECK(ctx, launch_tknn(ctx, 6, a));
  uint32_t tot[4] = {0, 0, 0, 0};  // survivors, -, records
  GF_HIP_CHECK(ctx, hipMemcpyAsync(&tot[0], a.srank + nt, 4, hipMemcpyDeviceToHost, ctx->stream));
  GF_HIP_CHECK(ctx, hipMemcpyAsync(&tot[2], a.counters + 2, 4, hipMemcpyDeviceToHost, ctx->stream));
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
  if ((st = T->o_key.reserve(ctx, nr * 8)) || (st = T->o_dist.reserve(ctx, nr * 8)) || (st = T->o_cells.reserve(ctx, nr * 4)) ||
      (st = T->o_traj.reserve(ctx, nr * 4)) || (st = T->o_len.reserve(ctx, (nr + 1) * 4)) ||
      (st = T->o_off.reserve(ctx, (nr + 1) * 4)))
    return st;
  a.rows = rows;
  a.tkeys = G->keys.as<int64_t>();
  a.perm = G->perm.as<uint32_t>();
  a.o_key = T->o_key.as<int64_t>(); a.o_dist = T->o_dist.as<double>(); a.o_cells = T->o_cells.as<int32_t>();
  a.o_traj = T->o_traj.as<uint32_t>(); a.o_len = T->o_len.as<uint32_t>(); a.o_off = T->o_off.as<uint32_t>();
  GF_HIP_CHECK(ctx, launch_tknn(ctx, 7, a));
  if ((st = group_scan_u32(ctx, T->srt, a.o_len, rows, T->o_off.as<uint32_t>()))) return st;
  uint32_t npts = 0;
  if ((st = read_scalar_sync(ctx, a.o_off + rows, &npts))) return st;
  if ((int64_t)npts > n) return set_err(ctx, GF_ERR_HIP, "gf_tknn_run: inconsistent point count");
  const size_t no = (size_t)npts;
  if ((st = T->o_x.reserve(ctx, no * 8)) || (st = T->o_y.reserve(ctx, no * 8)) || (st = T->o_ts.reserve(ctx, no * 8)) ||
      (st = T->o_idx.reserve(ctx, no * 4)))
    return st;
  a.npts = npts;
  a.o_x = T->o_x.as<double>(); a.o_y = T->o_y.as<double>(); a.o_ts = T->o_ts.as<int64_t>(); a.o_idx = T->o_idx.as<uint32_t>();
  GF_HIP_CHECK(ctx, launch_tknn(ctx, 8, a));
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
  T->cells.release_groups();
  T->pairs.release_groups();
  T->bycell.release_groups();
  T->srt.release_groups();
  for (DevBuf** b = T->all; *b; ++b) (*b)->release();
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
  std::vector<uint32_t> ho;
  if (off) ho.resize(wr + 1);
  if ((st = read_back(ctx, keys, T->o_key.p, wr)) || (st = read_back(ctx, dist, T->o_dist.p, wr)) ||
      (st = read_back(ctx, cells, T->o_cells.p, wr)) || (st = read_back(ctx, off ? ho.data() : nullptr, T->o_off.p, ho.size())) ||
      (st = read_back(ctx, x, T->o_x.p, wp)) || (st = read_back(ctx, y, T->o_y.p, wp)) ||
      (st = read_back(ctx, ts, T->o_ts.p, wp)) || (st = read_back(ctx, idx, T->o_idx.p, wp)))
    return st;
  GF_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  for (size_t i = 0; i < ho.size(); ++i) off[i] = (int64_t)ho[i];
  return GF_OK;
}
