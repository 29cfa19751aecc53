// range.cpp -- range plans, built once per continuous query (the reference computes its guaranteed /
// candidate cell sets once per operator, PointPointRangeQuery.java:119-125), their per-window entry
// points, the point-polygon join (it runs on a range plan) and the bitmap -> index list expansion.
#define GF_TU_NAME range_cpp
#include "gf_buildtag.hpp"  // first: records this unit's command-line defines

#include <hip/hip_runtime.h>

#include <array>
#include <limits>
#include <unordered_map>

#include "gf_chain_plan.hpp"
#include "gf_host.hpp"

using namespace gf;

// ---------------------------------------------------------------------------------------
// range plans
// ---------------------------------------------------------------------------------------
namespace {

struct Rect { int64_t x0, x1, y0, y1; };

void add_rect(std::vector<int32_t>& diff, int64_t n, Rect r) {
  r.x0 = std::max<int64_t>(r.x0, 0); r.y0 = std::max<int64_t>(r.y0, 0);
  r.x1 = std::min<int64_t>(r.x1, n - 1); r.y1 = std::min<int64_t>(r.y1, n - 1);
  if (r.x0 > r.x1 || r.y0 > r.y1) return;
  const int64_t W = n + 1;
  diff[r.y0 * W + r.x0] += 1;
  diff[r.y0 * W + r.x1 + 1] -= 1;
  diff[(r.y1 + 1) * W + r.x0] -= 1;
  diff[(r.y1 + 1) * W + r.x1 + 1] += 1;
}

void prefix2d(std::vector<int32_t>& d, int64_t n) {
  const int64_t W = n + 1;
  for (int64_t y = 0; y <= n; ++y)
    for (int64_t x = 1; x <= n; ++x) d[y * W + x] += d[y * W + x - 1];
  for (int64_t y = 1; y <= n; ++y)
    for (int64_t x = 0; x <= n; ++x) d[y * W + x] += d[(y - 1) * W + x];
}

Rect expand(Rect b, int64_t e) { return {b.x0 - e, b.x1 + e, b.y0 - e, b.y1 + e}; }

// Candidate cells covered by closed regions at distance 0 from each of their points (axis-
// aligned rectangle polygons; every bbox in approximate mode) become kInside (3) and are
// accepted untested.  A cell's exact coordinate range is the closed box
// [X_c, prev(X_{c+1})] x [Y_c, prev(Y_{c+1})] (X_c = first_at_least(c)).  Cells inside one
// region are marked directly; a cell the regions only partly overlap is split at the regions'
// edges into closed sub-boxes, and is covered iff every sub-box lies in some region -- so
// cells straddling the shared edge of two adjacent squares count too.
void mark_inside(gf_range_plan* P, std::vector<uint8_t>& table, const std::vector<std::array<double, 4>>& regs) {
  const gf_grid& g = P->grid;
  const int64_t n = g.n;
  std::vector<double> XT(n + 1), YT(n + 1);
  for (int64_t c = 0; c <= n; ++c) {
    XT[c] = first_at_least(c, g.minX, g.cellLength);
    YT[c] = first_at_least(c, g.minY, g.cellLength);
  }
  auto hi = [](const std::vector<double>& T, int64_t c) {  // largest double of cell c
    return std::isnan(T[c + 1]) ? INFINITY : std::nextafter(T[c + 1], -INFINITY);
  };
  // cells of [lo, hi] (overlapping: o0..o1; wholly inside: i0..i1)
  auto span = [&](const std::vector<double>& T, double lo, double up, double mn, int64_t& o0, int64_t& o1,
                  int64_t& i0, int64_t& i1) {
    o0 = std::max<int64_t>(cell_index(lo, mn, g.cellLength), 0);
    o1 = std::min<int64_t>(cell_index(up, mn, g.cellLength), n - 1);
    i0 = o0;
    i1 = o1;
    while (i0 <= i1 && !(T[i0] >= lo)) ++i0;
    while (i1 >= i0 && !(hi(T, i1) <= up)) --i1;
  };
  std::unordered_map<int64_t, std::vector<int32_t>> partial;
  for (size_t k = 0; k < regs.size(); ++k) {
    const auto& b = regs[k];
    int64_t ox0, ox1, ix0, ix1, oy0, oy1, iy0, iy1;
    span(XT, b[0], b[2], g.minX, ox0, ox1, ix0, ix1);
    span(YT, b[1], b[3], g.minY, oy0, oy1, iy0, iy1);
    for (int64_t y = oy0; y <= oy1; ++y)
      for (int64_t x = ox0; x <= ox1; ++x) {
        const int64_t cell = y * n + x;
        if (table[cell] != 1) continue;
        const bool in = x >= ix0 && x <= ix1 && y >= iy0 && y <= iy1;
        if (in) table[cell] = 3;
        else partial[cell].push_back((int32_t)k);
      }
  }
  for (auto& kv : partial) {
    const int64_t cell = kv.first;
    if (table[cell] != 1 || kv.second.size() < 2) continue;  // one partial region never covers
    const int64_t cx = cell % n, cy = cell / n;
    const double x0 = XT[cx], x1 = hi(XT, cx), y0 = YT[cy], y1 = hi(YT, cy);
    std::vector<double> xs{x0, x1}, ys{y0, y1};
    for (int32_t k : kv.second) {
      const auto& b = regs[k];
      if (b[0] > x0 && b[0] < x1) xs.push_back(b[0]);
      if (b[2] > x0 && b[2] < x1) xs.push_back(b[2]);
      if (b[1] > y0 && b[1] < y1) ys.push_back(b[1]);
      if (b[3] > y0 && b[3] < y1) ys.push_back(b[3]);
    }
    std::sort(xs.begin(), xs.end());
    xs.erase(std::unique(xs.begin(), xs.end()), xs.end());
    std::sort(ys.begin(), ys.end());
    ys.erase(std::unique(ys.begin(), ys.end()), ys.end());
    bool covered = true;
    for (size_t i = 0; covered && i + 1 < xs.size(); ++i)
      for (size_t j = 0; covered && j + 1 < ys.size(); ++j) {
        bool any = false;
        for (int32_t k : kv.second) {
          const auto& b = regs[k];
          if (b[0] <= xs[i] && xs[i + 1] <= b[2] && b[1] <= ys[j] && ys[j + 1] <= b[3]) { any = true; break; }
        }
        covered = any;
      }
    if (covered) table[cell] = 3;
  }
}

// Cell classes and candidate lists for a set of query objects with base cell rects B_o
// (a query point's cell, or every cell under a polygon's bbox -- Polygon.java:62).
int build_table(gf_range_plan* P, const std::vector<Rect>& base, bool need_lists,
                const std::vector<std::array<double, 4>>* inside = nullptr, bool lists_all = false) {
  gf_ctx* ctx = P->ctx;
  const int64_t n = P->grid.n;
  const int32_t g = P->g_layers, c = P->c_layers;
  if (n * n > (int64_t)1 << 30 || n > 16384) return set_err(ctx, GF_ERR_ARG, "grid too large for a cell table");
  std::vector<int32_t> dG((n + 1) * (n + 1), 0), dC((n + 1) * (n + 1), 0);
  std::vector<int32_t> extra;
  for (const Rect& b : base) {
    if (g > 0) add_rect(dG, n, expand(b, g));
    else if (g == 0) {
      add_rect(dG, n, b);
      if (b.x0 < 0 || b.y0 < 0 || b.x1 >= n || b.y1 >= n) {  // out-of-grid guaranteed cells
        auto cl32 = [](int64_t v) { return (int32_t)std::min<int64_t>(std::max<int64_t>(v, INT32_MIN), INT32_MAX); };
        extra.push_back(cl32(b.x0)); extra.push_back(cl32(b.x1));
        extra.push_back(cl32(b.y0)); extra.push_back(cl32(b.y1));
      }
    }
    if (c > 0) add_rect(dC, n, expand(b, c));
  }
  prefix2d(dG, n);
  prefix2d(dC, n);
  std::vector<uint8_t> table(n * n);
  for (int64_t y = 0; y < n; ++y)
    for (int64_t x = 0; x < n; ++x) {
      const int64_t i = y * (n + 1) + x;
      table[y * n + x] = dG[i] > 0 ? 2 : (dC[i] > 0 ? 1 : 0);
    }
  if (inside && P->r >= 0.0)
    mark_inside(P, table, *inside);
  for (uint8_t v : table) P->cls_cells[v & 3]++;
  std::vector<uint32_t> rows(n);
  for (int64_t y = 0; y < n; ++y) {
    int64_t lo = n, hi = -1;
    for (int64_t x = 0; x < n; ++x)
      if (table[y * n + x]) { lo = std::min(lo, x); hi = std::max(hi, x); }
    rows[y] = hi < 0 ? 0xffffu : (uint32_t)lo | ((uint32_t)hi << 16);  // empty: lo 65535 > hi 0
  }
  std::vector<uint32_t> rowoff(n);
  std::vector<uint8_t> spans;
  for (int64_t y = 0; y < n; ++y) {
    rowoff[y] = (uint32_t)spans.size();
    const int64_t lo = rows[y] & 0xffffu, hi = rows[y] >> 16;
    for (int64_t x = lo; x <= hi; ++x) spans.push_back(table[y * n + x]);
  }
  P->span_bytes = (int64_t)spans.size();
  while (spans.size() % 4) spans.push_back(0);
  if (spans.empty()) spans.assign(4, 0);
  int st;
  if ((st = upload(ctx, &P->table, table)) || (st = upload(ctx, &P->rows, rows)) ||
      (st = upload(ctx, &P->rowoff, rowoff)) || (st = upload(ctx, &P->spans, spans)))
    return st;
  if (n <= 2048) {  // division-free cells in the scan (thresholds staged in LDS)
    std::vector<double> xt(n + 1), yt(n + 1);
    for (int64_t c = 0; c <= n; ++c) {
      xt[c] = first_at_least(c, P->grid.minX, P->grid.cellLength);
      yt[c] = first_at_least(c, P->grid.minY, P->grid.cellLength);
    }
    P->x_lo = xt[0]; P->x_hi = xt[n]; P->y_lo = yt[0]; P->y_hi = yt[n];
    int64_t clo = n, chi = -1;  // union of the row spans (columns holding any class)
    for (int64_t y = 0; y < n; ++y)
      if ((rows[y] & 0xffffu) <= (rows[y] >> 16)) {
        clo = std::min<int64_t>(clo, rows[y] & 0xffffu);
        chi = std::max<int64_t>(chi, rows[y] >> 16);
      }
    P->sx_lo = chi < 0 ? xt[n] : xt[clo];  // empty: sx_lo == sx_hi, every x fails
    P->sx_hi = chi < 0 ? xt[n] : xt[chi + 1];
    int64_t rlo = n, rhi = -1;  // rows holding any class
    for (int64_t y = 0; y < n; ++y)
      if ((rows[y] & 0xffffu) <= (rows[y] >> 16)) {
        rlo = std::min<int64_t>(rlo, y);
        rhi = std::max<int64_t>(rhi, y);
      }
    P->sy_lo = rhi < 0 ? yt[n] : yt[rlo];
    P->sy_hi = rhi < 0 ? yt[n] : yt[rhi + 1];
    P->span_frac = chi < 0 ? 0.0 : (double)(chi - clo + 1) * (double)(rhi - rlo + 1) / ((double)n * (double)n);
    if ((st = upload(ctx, &P->xt, xt)) || (st = upload(ctx, &P->yt, yt))) return st;
  }

  P->n_extra = (int32_t)(extra.size() / 4);
  if ((st = upload(ctx, &P->extra, extra))) return st;
  if (!need_lists) return GF_OK;
  // candidate lists over a (c + 2)-cell reach (superset of every object within r)
  const int64_t reach = (int64_t)std::max(c, 0) + 2;
  double area = 0;
  for (const Rect& b : base) {
    Rect r = expand(b, reach);
    r.x0 = std::max<int64_t>(r.x0, 0); r.y0 = std::max<int64_t>(r.y0, 0);
    r.x1 = std::min<int64_t>(r.x1, n - 1); r.y1 = std::min<int64_t>(r.y1, n - 1);
    if (r.x0 <= r.x1 && r.y0 <= r.y1) area += double(r.x1 - r.x0 + 1) * double(r.y1 - r.y0 + 1);
  }
  if (area > 6.4e7) return GF_OK;  // too large: every candidate-cell point tests every object
  std::vector<int32_t> off(n * n + 1, 0);
  for (int pass = 0; pass < 2; ++pass) {
    std::vector<int32_t> cur;
    std::vector<int32_t> lst;
    if (pass == 1) {
      for (int64_t i = 0; i < n * n; ++i) off[i + 1] += off[i];
      cur.assign(off.begin(), off.end() - 1);
      lst.resize(off[n * n]);
    }
    for (size_t o = 0; o < base.size(); ++o) {
      Rect r = expand(base[o], reach);
      r.x0 = std::max<int64_t>(r.x0, 0); r.y0 = std::max<int64_t>(r.y0, 0);
      r.x1 = std::min<int64_t>(r.x1, n - 1); r.y1 = std::min<int64_t>(r.y1, n - 1);
      for (int64_t y = r.y0; y <= r.y1; ++y)
        for (int64_t x = r.x0; x <= r.x1; ++x) {
          const int64_t cell = y * n + x;
          if (lists_all ? table[cell] == 0 : (table[cell] != 1 && table[cell] != 3)) continue;
          if (pass == 0) off[cell + 1]++;
          else lst[cur[cell]++] = (int32_t)o;
        }
    }
    if (pass == 1) {
      if ((st = upload(ctx, &P->cand_off, off))) return st;
      if (lst.empty()) lst.push_back(0);
      if ((st = upload(ctx, &P->cand_list, lst))) return st;
    }
  }
  return GF_OK;
}

// row-span class tables up to this size are staged in LDS by every scan block
constexpr int64_t kSpanLdsBytes = 32768;

// scan blocks (<= 8 per CU) + deferred-test blocks (8 per CU) of per-block partial counts
int finish_plan(gf_range_plan* P) {
  // partials of <= kRangeMaxParts blocks (scan <= 8 per CU + deferred tests), then the ticket
  if (P->ctx->num_cus * 16 > gf::kRangeMaxParts) return set_err(P->ctx, GF_ERR_ARG, "too many CUs for the partials");
  GF_HIP_CHECK(P->ctx, hipMalloc(&P->partials, sizeof(uint64_t) * (gf::kRangeTicketSlot + 1)));
  GF_HIP_CHECK(P->ctx, hipMemset(P->partials + gf::kRangeTicketSlot, 0, sizeof(uint64_t)));
  GF_HIP_CHECK(P->ctx, hipMalloc(&P->queue_count, sizeof(uint32_t) * (size_t)P->ctx->num_cus * 8));
  return GF_OK;
}

}  // namespace

extern "C" void gf_range_plan_destroy(gf_range_plan* P) {
  if (!P) return;
  hipSetDevice(P->ctx->device);
  hipStreamSynchronize(P->ctx->stream);
  void* bufs[] = {P->table, P->extra, P->cand_off, P->cand_list, P->qx, P->qy, P->ring_off, P->vert_off,
                  P->vx, P->vy, P->bbox, P->ring_env, P->partials, P->queue, P->queue_count, P->queue_xy, P->rows, P->xt, P->yt,
                  P->rowoff, P->spans, P->brect, P->rect, P->jecnt, P->jecand, P->jbtot, P->jtotal,
                  P->batch_partials, P->run_off, P->run_env};
  for (void* b : bufs)
    if (b) hipFree(b);
  delete P;
}

extern "C" int gf_range_pp_plan_create(gf_ctx* ctx, const gf_grid* g, const double* qx, const double* qy,
                                       int32_t nq, double r, int approximate, int metric, gf_range_plan** out) {
  if (!ctx || !out || !grid_ok(g) || nq < 0 || (nq > 0 && (!qx || !qy)) || (metric != 0 && metric != 1))
    return set_err(ctx, GF_ERR_ARG, "gf_range_pp_plan_create: bad argument");
  *out = nullptr;
  int st = bind(ctx);
  if (st) return st;
  gf_range_plan* P = new gf_range_plan();
  P->ctx = ctx;
  P->grid = *g;
  P->r = r;
  P->approx = approximate != 0;
  P->metric = metric;
  P->nq = nq;
  P->g_layers = guaranteed_layers(g->cellLength, r);
  P->c_layers = candidate_layers(g->cellLength, r);
  const double nan = std::numeric_limits<double>::quiet_NaN();
  if (nq == 0) {  // nothing is ever guaranteed or candidate
    P->table_mode = 0;
    P->qr.cgx = P->qr.cgy = P->qr.gx = P->qr.gy = {nan, nan};
    P->qr.g_any = 0;
  } else if (nq == 1) {
    P->table_mode = 0;
    const int32_t qcx = cell_index(qx[0], g->minX, g->cellLength), qcy = cell_index(qy[0], g->minY, g->cellLength);
    P->qr = make_qrect(*g, qcx, qcy, P->g_layers, P->c_layers);
    P->qx0 = qx[0];
    P->qy0 = qy[0];
  } else {
    P->table_mode = 1;
    std::vector<Rect> base(nq);
    for (int32_t q = 0; q < nq; ++q) {
      const int64_t cx = cell_index(qx[q], g->minX, g->cellLength), cy = cell_index(qy[q], g->minY, g->cellLength);
      base[q] = {cx, cx, cy, cy};
    }
    if ((st = build_table(P, base, !P->approx))) { gf_range_plan_destroy(P); return st; }
    std::vector<double> vqx(qx, qx + nq), vqy(qy, qy + nq);
    if ((st = upload(ctx, &P->qx, vqx)) || (st = upload(ctx, &P->qy, vqy))) { gf_range_plan_destroy(P); return st; }
  }
  if ((st = finish_plan(P))) { gf_range_plan_destroy(P); return st; }
  *out = P;
  return GF_OK;
}

namespace {
// join != 0: a point-polygon join plan -- cell lists for every non-none cell (guaranteed ones
// too: the join tests every co-located pair), no inside-cell marking, per-polygon bbox cells.
int ppoly_plan_create(gf_ctx* ctx, const gf_grid* g, const gf_polygons* polys, double r, int approximate, int metric,
                      int join, gf_range_plan** out) {
  if (!ctx || !out || !grid_ok(g) || !polys || polys->npoly < 0 || (metric != 0 && metric != 1))
    return set_err(ctx, GF_ERR_ARG, join ? "gf_join_ppoly_plan_create: bad argument"
                                         : "gf_range_ppoly_plan_create: bad argument");
  *out = nullptr;
  int st = bind(ctx);
  if (st) return st;
  const int32_t np = polys->npoly;
  const int32_t nrings = np > 0 ? polys->ring_off[np] : 0;
  // validate rings: >= 4 vertices, closed (Polygon.createPolygon / JTS LinearRing)
  for (int32_t p = 0; p < np; ++p)
    if (polys->ring_off[p + 1] <= polys->ring_off[p]) return set_err(ctx, GF_ERR_ARG, "polygon without a shell");
  for (int32_t j = 0; j < nrings; ++j) {
    const int32_t v0 = polys->vert_off[j], v1 = polys->vert_off[j + 1];
    if (v1 - v0 < 4 || polys->vx[v0] != polys->vx[v1 - 1] || polys->vy[v0] != polys->vy[v1 - 1])
      return set_err(ctx, GF_ERR_ARG, "ring must be closed with >= 4 vertices");
  }
  gf_range_plan* P = new gf_range_plan();
  P->ctx = ctx;
  P->grid = *g;
  P->r = r;
  P->approx = approximate != 0;
  P->metric = metric;
  P->poly = 1;
  P->table_mode = 1;
  P->npoly = np;
  P->nq = np;
  P->g_layers = guaranteed_layers(g->cellLength, r);
  P->c_layers = candidate_layers(g->cellLength, r);
  std::vector<double> bbox(4 * (size_t)std::max(np, 1)), renv(4 * (size_t)std::max(nrings, 1));
  for (int32_t j = 0; j < nrings; ++j) {
    const int32_t v0 = polys->vert_off[j], v1 = polys->vert_off[j + 1];
    double mnx = polys->vx[v0], mxx = mnx, mny = polys->vy[v0], mxy = mny;
    for (int32_t v = v0 + 1; v < v1; ++v) {
      mnx = std::min(mnx, polys->vx[v]); mxx = std::max(mxx, polys->vx[v]);
      mny = std::min(mny, polys->vy[v]); mxy = std::max(mxy, polys->vy[v]);
    }
    renv[4 * j] = mnx; renv[4 * j + 1] = mxx; renv[4 * j + 2] = mny; renv[4 * j + 3] = mxy;
  }
  std::vector<Rect> base(np);
  for (int32_t p = 0; p < np; ++p) {
    const int32_t sh = polys->ring_off[p];  // shell envelope = Polygon.getEnvelopeInternal
    const double x1 = renv[4 * sh], x2 = renv[4 * sh + 1], y1 = renv[4 * sh + 2], y2 = renv[4 * sh + 3];
    bbox[4 * p] = x1; bbox[4 * p + 1] = y1; bbox[4 * p + 2] = x2; bbox[4 * p + 3] = y2;
    base[p] = {cell_index(x1, g->minX, g->cellLength), cell_index(x2, g->minX, g->cellLength),
               cell_index(y1, g->minY, g->cellLength), cell_index(y2, g->minY, g->cellLength)};
  }
  // regions at distance 0 from each of their points: approximate mode -> every bbox;
  // exact mode -> shells that are axis-aligned rectangles without holes
  std::vector<std::array<double, 4>> inside;
  std::vector<uint8_t> rectf((size_t)std::max(np, 1), 0);
  for (int32_t p = 0; p < np; ++p) {
    const double x1 = bbox[4 * p], y1 = bbox[4 * p + 1], x2 = bbox[4 * p + 2], y2 = bbox[4 * p + 3];
    if (!(x1 < x2 && y1 < y2)) continue;
    bool rect = false;
    if (polys->ring_off[p + 1] - polys->ring_off[p] == 1) {
      const int32_t v0 = polys->vert_off[polys->ring_off[p]], v1 = polys->vert_off[polys->ring_off[p] + 1];
      int corners = 0;
      rect = (v1 - v0 == 5);
      for (int32_t v = v0; rect && v < v1; ++v) {
        const double X = polys->vx[v], Y = polys->vy[v];
        rect = (X == x1 || X == x2) && (Y == y1 || Y == y2);
        if (rect && v > v0) rect = (X == polys->vx[v - 1]) != (Y == polys->vy[v - 1]);  // one axis moves
        if (rect && v < v1 - 1) corners |= 1 << ((X == x2) + 2 * (Y == y2));
      }
      rect = rect && corners == 15;
    }
    rectf[p] = rect;
    if (rect || P->approx) inside.push_back({x1, y1, x2, y2});
  }
  P->join = join;
  if ((st = build_table(P, base, true, join ? nullptr : &inside, join != 0))) { gf_range_plan_destroy(P); return st; }
  if (join) {
    std::vector<int32_t> br(4 * (size_t)std::max(np, 1), 0);
    auto cl32 = [](int64_t v) { return (int32_t)std::min<int64_t>(std::max<int64_t>(v, INT32_MIN), INT32_MAX); };
    for (int32_t p = 0; p < np; ++p) {
      br[4 * p] = cl32(base[p].x0); br[4 * p + 1] = cl32(base[p].x1);
      br[4 * p + 2] = cl32(base[p].y0); br[4 * p + 3] = cl32(base[p].y1);
    }
    if ((st = upload(ctx, &P->brect, br))) { gf_range_plan_destroy(P); return st; }
    GF_HIP_CHECK(ctx, hipMalloc(&P->jbtot, sizeof(uint32_t) * (size_t)ctx->num_cus * 8));
    GF_HIP_CHECK(ctx, hipMalloc(&P->jtotal, sizeof(unsigned long long)));
  }
  const int32_t nverts = nrings > 0 ? polys->vert_off[nrings] : 0;
  std::vector<int32_t> ro(polys->ring_off, polys->ring_off + np + 1), vo(polys->vert_off, polys->vert_off + nrings + 1);
  std::vector<double> vx(polys->vx, polys->vx + nverts), vy(polys->vy, polys->vy + nverts);
  if ((st = upload(ctx, &P->ring_off, ro)) || (st = upload(ctx, &P->vert_off, vo)) || (st = upload(ctx, &P->vx, vx)) ||
      (st = upload(ctx, &P->vy, vy)) || (st = upload(ctx, &P->bbox, bbox)) || (st = upload(ctx, &P->ring_env, renv)) ||
      (st = upload(ctx, &P->rect, rectf))) {
    gf_range_plan_destroy(P);
    return st;
  }
  if ((st = finish_plan(P))) { gf_range_plan_destroy(P); return st; }
  *out = P;
  return GF_OK;
}
}  // namespace

namespace {
// A linestring plan (PointLineStringRangeQuery.java:100-172; join != 0: PointLineStringJoinQuery.java's
// replicated query side, JoinQuery.java:117-137) is a polygon plan with one "ring" per object and
// poly == 2, which selects the open-chain distance in the kernels.  The polygon shortcuts that assume a
// closed region are off: no rectangle detection (rect stays null), and in exact mode no inside cells --
// a cell under a closed chain is still at its distance to the nearest segment, so every candidate cell
// is tested.  In approximate mode the bbox distance is 0 inside the bbox for lines too, and the bboxes
// of positive area mark inside cells as they do for polygons.  Base cells: the cells under the vertex
// envelope (LineString.java: HelperClass.assignGridCellID(bbox)) -- a zero-width or zero-height
// bbox has x1 == x2 or y1 == y2 and yields the one column / row of cells its ordinate lies in.
int pls_plan_create(gf_ctx* ctx, const gf_grid* g, const gf_linestrings* lines, double r, int approximate, int metric,
                    int join, gf_range_plan** out) {
  if (!ctx || !out || !grid_ok(g) || !chain_valid(lines) || (metric != 0 && metric != 1))
    return set_err(ctx, GF_ERR_ARG, join ? "gf_join_pls_plan_create: bad argument (lines of >= 2 vertices)"
                                         : "gf_range_pls_plan_create: bad argument (lines of >= 2 vertices)");
  *out = nullptr;
  int st = bind(ctx);
  if (st) return st;
  const int32_t nl = lines->nline;
  ChainTables T;
  chain_build(*lines, kChainRun, T);
  gf_range_plan* P = new gf_range_plan();
  P->ctx = ctx;
  P->grid = *g;
  P->r = r;
  P->approx = approximate != 0;
  P->metric = metric;
  P->poly = 2;
  P->table_mode = 1;
  P->npoly = nl;
  P->nq = nl;
  P->g_layers = guaranteed_layers(g->cellLength, r);
  P->c_layers = candidate_layers(g->cellLength, r);
  P->join = join;
  std::vector<Rect> base(nl);
  std::vector<std::array<double, 4>> inside;
  for (int32_t l = 0; l < nl; ++l) {
    const double x1 = T.bbox[4 * l], y1 = T.bbox[4 * l + 1], x2 = T.bbox[4 * l + 2], y2 = T.bbox[4 * l + 3];
    base[l] = {cell_index(x1, g->minX, g->cellLength), cell_index(x2, g->minX, g->cellLength),
               cell_index(y1, g->minY, g->cellLength), cell_index(y2, g->minY, g->cellLength)};
    if (P->approx && x1 < x2 && y1 < y2) inside.push_back({x1, y1, x2, y2});
  }
  if ((st = build_table(P, base, true, join ? nullptr : &inside, join != 0))) { gf_range_plan_destroy(P); return st; }
  if (join) {
    std::vector<int32_t> br(4 * (size_t)std::max(nl, 1), 0);
    auto cl32 = [](int64_t v) { return (int32_t)std::min<int64_t>(std::max<int64_t>(v, INT32_MIN), INT32_MAX); };
    for (int32_t l = 0; l < nl; ++l) {
      br[4 * l] = cl32(base[l].x0); br[4 * l + 1] = cl32(base[l].x1);
      br[4 * l + 2] = cl32(base[l].y0); br[4 * l + 3] = cl32(base[l].y1);
    }
    if ((st = upload(ctx, &P->brect, br))) { gf_range_plan_destroy(P); return st; }
    GF_HIP_CHECK(ctx, hipMalloc(&P->jbtot, sizeof(uint32_t) * (size_t)ctx->num_cus * 8));
    GF_HIP_CHECK(ctx, hipMalloc(&P->jtotal, sizeof(unsigned long long)));
  }
  if ((st = upload(ctx, &P->vert_off, T.vert_off)) || (st = upload(ctx, &P->vx, T.vx)) || (st = upload(ctx, &P->vy, T.vy)) ||
      (st = upload(ctx, &P->bbox, T.bbox)) || (st = upload(ctx, &P->run_off, T.run_off)) ||
      (st = upload(ctx, &P->run_env, T.run_env))) {
    gf_range_plan_destroy(P);
    return st;
  }
  if ((st = finish_plan(P))) { gf_range_plan_destroy(P); return st; }
  *out = P;
  return GF_OK;
}
}  // namespace

extern "C" int gf_range_pls_plan_create(gf_ctx* ctx, const gf_grid* g, const gf_linestrings* lines, double r,
                                        int approximate, int metric, gf_range_plan** out) {
  return pls_plan_create(ctx, g, lines, r, approximate, metric, 0, out);
}

extern "C" int gf_join_pls_plan_create(gf_ctx* ctx, const gf_grid* qgrid, const gf_linestrings* lines, double r,
                                       int approximate, int metric, gf_range_plan** out) {
  return pls_plan_create(ctx, qgrid, lines, r, approximate, metric, 1, out);
}

extern "C" int gf_range_plan_set_chain_mode(gf_range_plan* P, int mode) {
  if (!P || P->poly != 2 || (mode != 0 && mode != 1)) return GF_ERR_ARG;
  P->chain_mode = mode;
  return GF_OK;
}

extern "C" int gf_range_ppoly_plan_create(gf_ctx* ctx, const gf_grid* g, const gf_polygons* polys, double r,
                                          int approximate, int metric, gf_range_plan** out) {
  return ppoly_plan_create(ctx, g, polys, r, approximate, metric, 0, out);
}

extern "C" int gf_join_ppoly_plan_create(gf_ctx* ctx, const gf_grid* qgrid, const gf_polygons* polys, double r,
                                         int approximate, int metric, gf_range_plan** out) {
  return ppoly_plan_create(ctx, qgrid, polys, r, approximate, metric, 1, out);
}

namespace {
RangeArgs range_args(const gf_range_plan* P, const gf_points* pts, uint64_t* bitmap, uint64_t* multi) {
  RangeArgs a{};
  a.x = pts->x; a.y = pts->y; a.n = pts->n;
  a.bitmap = bitmap; a.multi = multi; a.partials = P->partials;
  a.nq = P->nq;
  a.qr = P->qr;
  a.grid_n = P->grid.n; a.minX = P->grid.minX; a.minY = P->grid.minY; a.cl = P->grid.cellLength;
  a.table = P->table; a.rows = P->rows; a.extra = P->extra; a.n_extra = P->n_extra;
  a.rowoff = P->rowoff; a.spans = P->spans; a.span_bytes = (int32_t)std::min<int64_t>(P->span_bytes, INT32_MAX);
  a.span_lds = P->span_bytes <= kSpanLdsBytes;
  a.xt = P->xt; a.yt = P->yt; a.x_lo = P->x_lo; a.x_hi = P->x_hi; a.y_lo = P->y_lo; a.y_hi = P->y_hi;
  a.sx_lo = P->sx_lo; a.sx_hi = P->sx_hi;
  a.sy_lo = P->sy_lo; a.sy_hi = P->sy_hi;
  a.inv_cl = 1.0 / P->grid.cellLength;
  a.cand_off = P->cand_off; a.cand_list = P->cand_list;
  a.approx = P->approx; a.metric = P->metric; a.r = P->r; a.s_r = s_prefilter(P->r, 0);
  a.thr = P->metric == 0 ? a.s_r : a.r;
  a.qx0 = P->qx0; a.qy0 = P->qy0;
  a.qx = P->qx; a.qy = P->qy;
  a.npoly = P->npoly; a.ring_off = P->ring_off; a.vert_off = P->vert_off; a.vx = P->vx; a.vy = P->vy;
  a.bbox = P->bbox; a.ring_env = P->ring_env; a.rect = P->rect;
  if (P->poly == 2) {  // a linestring plan: the runs travel in the ring fields (ChainView); mode 1: no runs
    a.ring_off = P->chain_mode == 1 ? nullptr : P->run_off;
    a.ring_env = P->run_env;
  }
  a.brect = P->brect; a.g_layers = P->g_layers; a.c_layers = P->c_layers;
  return a;
}

// the deferred-test queue: one segment per scan block, each large enough for every point the
// block visits (a scan block visits at most 2 points per thread per grid sweep)
int ensure_queue(gf_range_plan* P, RangeArgs& a, int blocks, bool with_counts) {
  gf_ctx* ctx = P->ctx;
  const int64_t tstride = (int64_t)blocks * kBlock * 2;
  a.seg_cap = 2 * kBlock * ((a.n + tstride - 1) / tstride);
  a.drain_lanes = P->drain_lanes;
  const int64_t need = a.seg_cap * blocks;
  if (P->queue_cap < need || (with_counts && !P->jecnt)) {
    GF_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    void* old[] = {P->queue, P->queue_xy, P->jecnt, P->jecand};
    for (void* b : old)
      if (b) GF_HIP_CHECK(ctx, hipFree(b));
    P->queue = nullptr;
    P->queue_xy = nullptr;
    P->jecnt = nullptr;
    P->jecand = nullptr;
    P->queue_cap = 0;
    const int64_t cap = need;
    GF_HIP_CHECK(ctx, hipMalloc(&P->queue, sizeof(uint32_t) * (size_t)cap));
    GF_HIP_CHECK(ctx, hipMalloc(&P->queue_xy, 2 * sizeof(double) * (size_t)cap));
    if (with_counts) {
      GF_HIP_CHECK(ctx, hipMalloc(&P->jecnt, sizeof(uint32_t) * (size_t)cap));
      GF_HIP_CHECK(ctx, hipMalloc(&P->jecand, 4 * sizeof(uint32_t) * (size_t)cap));  // kJoinKeep
    }
    P->queue_cap = cap;
  }
  a.queue = P->queue;
  a.queue_xy = P->queue_xy;
  a.queue_count = P->queue_count;
  return GF_OK;
}

int scan_blocks_range(const gf_range_plan* P, int64_t n, bool span = false) {
  // every wave should run >= 2 pipeline stages of kRangeU tiles (range_kernel); at most 4
  // blocks per CU (the sweep in tools/bench_workloads.py: 1024 blocks best at 10M points), 2
  // for the span prefilter (C3, three windows in flight: 48.9 us per window at 512 blocks,
  // 51.5 at 1024; tools/gpu_r03_c3blocks.sh)
  int blocks = (int)std::min<int64_t>(std::max<int64_t>(n / (4 * 128 * 2 * 2), 1),
                                      (int64_t)P->ctx->num_cus * (span ? 2 : 4));
  if (P->scan_blocks > 0) blocks = P->scan_blocks;
  return std::min(blocks, 2048);  // queue segments / partial slots per window
}
}  // namespace

extern "C" int gf_range_run(gf_range_plan* P, const gf_points* pts, uint64_t* bitmap, uint64_t* multi,
                            int64_t* counts) {
  if (!P || !bitmap) return GF_ERR_ARG;
  if (P->join) return set_err(P->ctx, GF_ERR_ARG, "gf_range_run: a join plan (use gf_join_ppoly_run)");
  gf_ctx* ctx = P->ctx;
  int st = bind(ctx);
  if (st) return st;
  if ((st = check_points(ctx, pts))) return st;
  if (pts->n == 0) {
    if (counts) GF_HIP_CHECK(ctx, hipMemsetAsync(counts, 0, 2 * sizeof(int64_t), ctx->stream));
    return GF_OK;
  }
  RangeArgs a = range_args(P, pts, bitmap, multi);
  // Deferred tests pay a second launch; inline tests stall the waves holding candidate lanes.
  // Auto: defer while candidate cells are more than 5% of the non-none cells.
  const int64_t live = P->cls_cells[1] + P->cls_cells[2] + P->cls_cells[3];
  const bool can_defer = P->table_mode && (P->poly || !P->approx);
  const bool defer = can_defer && (P->defer_mode >= 2 || (P->defer_mode == 0 && P->cls_cells[1] * 20 > live));
  // span prefilter when the class spans cover at most a quarter of the grid (defer_mode 3
  // forces it): the stream skips the table, the block's queued points are classified after it
  // (the span prefilter's classification rounds read the span table from LDS only: it must fit)
  const bool span = defer && P->xt && P->span_bytes <= kSpanLdsBytes &&
                    (P->defer_mode == 3 || (P->defer_mode != 2 && P->span_frac <= 0.25));
  const int blocks = scan_blocks_range(P, pts->n, span);
  if (defer) {
    if ((st = ensure_queue(P, a, blocks, false))) return st;
    a.span_mode = span;
  }
  // the counts are summed by the last block of the window's last kernel (no finalize launch)
  a.counts = counts;
  GF_HIP_CHECK(ctx, launch_range(ctx, a, P->table_mode, P->poly, blocks));
  return GF_OK;
}

extern "C" int gf_range_run_batch(gf_range_plan* P, int32_t nwin, const gf_points* pts, uint64_t* const* bitmaps,
                                  int64_t* const* counts, uint32_t* const* idx, const int64_t* idx_cap,
                                  int64_t* const* idx_count) {
  if (!P || nwin < 1 || nwin > kRangeBatchMax || !pts || !bitmaps || !counts)
    return set_err(P ? P->ctx : nullptr, GF_ERR_ARG, "gf_range_run_batch: 1 <= nwin <= 16, pts / bitmaps / counts");
  if (P->join) return set_err(P->ctx, GF_ERR_ARG, "gf_range_run_batch: a join plan");
  gf_ctx* ctx = P->ctx;
  int st = bind(ctx);
  if (st) return st;
  int64_t nmax = 0;
  for (int32_t w = 0; w < nwin; ++w) {
    if ((st = check_points(ctx, &pts[w]))) return st;
    if (!bitmaps[w] || !counts[w]) return set_err(ctx, GF_ERR_ARG, "gf_range_run_batch: null bitmap / counts");
    if (idx && (pts[w].n > (int64_t)UINT32_MAX || !idx_cap || !idx_count || !idx_count[w] || idx_cap[w] < 0 ||
                (idx_cap[w] > 0 && !idx[w])))
      return set_err(ctx, GF_ERR_ARG, "gf_range_run_batch: index lists need idx, idx_cap, idx_count per window");
    nmax = std::max(nmax, pts[w].n);
  }
  if (!P->batch_partials) {  // tickets start at 0 and every finalising block resets its own
    GF_HIP_CHECK(ctx, hipMalloc(&P->batch_partials, sizeof(uint64_t) * (size_t)kRangeBatchMax * (kRangeTicketSlot + 1)));
    GF_HIP_CHECK(ctx, hipMemsetAsync(P->batch_partials, 0,
                                     sizeof(uint64_t) * (size_t)kRangeBatchMax * (kRangeTicketSlot + 1), ctx->stream));
  }
  RangeArgs a = range_args(P, &pts[0], bitmaps[0], nullptr);
  RangeBatch b{};
  for (int32_t w = 0; w < nwin; ++w)
    b.w[w] = RangeWin{pts[w].x, pts[w].y, pts[w].n, bitmaps[w], nullptr,
                      P->batch_partials + (size_t)w * (kRangeTicketSlot + 1), counts[w]};
  // blocks per window from the largest window (an empty window's blocks exit after the partials),
  // the whole launch held to ~4 blocks per CU as for one large window (r05 sweep, 16 windows of
  // 1M points: 488 blocks per window 3.7 us per window, 256: 3.4, 128: 3.3, 64: 3.25)
  int blocks = scan_blocks_range(P, nmax);
  if (P->scan_blocks == 0) blocks = std::max(1, std::min(blocks, (ctx->num_cus * 4 + nwin - 1) / nwin));
  GF_HIP_CHECK(ctx, launch_range_batch(ctx, a, b, nwin, P->table_mode, P->poly, blocks));
  if (!idx) return GF_OK;
  ExpandBatch e{};
  e.nwin = nwin;
  int64_t tiles = 0;
  for (int32_t w = 0; w < nwin; ++w) {
    e.bm[w] = bitmaps[w];
    e.n[w] = pts[w].n;
    e.idx[w] = idx[w];
    e.cap[w] = idx_cap[w];
    e.count[w] = idx_count[w];
    e.tile0[w] = (int32_t)tiles;
    tiles += std::max<int64_t>(expand_blocks((pts[w].n + 63) / 64), 1);  // >= 1: its block writes the count
  }
  e.tile0[nwin] = (int32_t)tiles;
  return lookback_launch(ctx, tiles, tiles, "launch_expand_batch",
                         [&](const ExpandState& es) { return launch_expand_batch(ctx->stream, e, es); });
}

extern "C" int gf_join_ppoly_run(gf_range_plan* P, const gf_grid* ugrid, const gf_points* pts, uint32_t* pairs,
                                 int64_t cap, int64_t* npairs) {
  if (!P || !npairs || cap < 0 || !grid_ok(ugrid)) return GF_ERR_ARG;
  gf_ctx* ctx = P->ctx;
  if (!P->join) return set_err(ctx, GF_ERR_ARG, "gf_join_ppoly_run: not a join plan (gf_join_ppoly_plan_create)");
  const gf_grid& q = P->grid;
  if (ugrid->n != q.n || ugrid->minX != q.minX || ugrid->maxX != q.maxX || ugrid->minY != q.minY ||
      ugrid->maxY != q.maxY || ugrid->cellLength != q.cellLength)
    return set_err(ctx, GF_ERR_ARG, "gf_join_ppoly_run: the point grid must equal the polygon grid");
  int st = bind(ctx);
  if (st) return st;
  if ((st = check_points(ctx, pts))) return st;
  *npairs = 0;
  if (pts->n == 0 || P->npoly == 0) return GF_OK;
  if (pts->n > (int64_t)UINT32_MAX) return set_err(ctx, GF_ERR_ARG, "gf_join_ppoly_run: window too large");
  RangeArgs a = range_args(P, pts, nullptr, nullptr);
  const int blocks = scan_blocks_range(P, pts->n);
  if ((st = ensure_queue(P, a, blocks, true))) return st;
  const int jblocks = blocks;  // one count/write block per scan block (its queue segment)
  GF_HIP_CHECK(ctx, launch_join_ppoly(ctx, a, blocks, jblocks, P->jecnt, P->jecand, P->jbtot, P->jtotal, pairs,
                                      pairs ? cap : 0, pairs && ((uintptr_t)pairs % 8 == 0), P->poly));
  unsigned long long total = 0;
  if ((st = read_scalar_sync(ctx, P->jtotal, &total))) return st;
  *npairs = (int64_t)total;
  if ((int64_t)total > cap || (total > 0 && !pairs)) return GF_ERR_CAPACITY;
  return GF_OK;
}

extern "C" int gf_join_ppoly(gf_ctx* ctx, const gf_grid* ugrid, const gf_grid* qgrid, const gf_points* pts,
                             const gf_polygons* polys, double r, int approximate, int metric, uint32_t* pairs,
                             int64_t cap, int64_t* npairs) {
  gf_range_plan* P = nullptr;
  int st = gf_join_ppoly_plan_create(ctx, qgrid, polys, r, approximate, metric, &P);
  if (st) return st;
  st = gf_join_ppoly_run(P, ugrid, pts, pairs, cap, npairs);
  gf_range_plan_destroy(P);
  return st;
}

extern "C" int gf_join_pls(gf_ctx* ctx, const gf_grid* ugrid, const gf_grid* qgrid, const gf_points* pts,
                           const gf_linestrings* lines, double r, int approximate, int metric, uint32_t* pairs,
                           int64_t cap, int64_t* npairs) {
  gf_range_plan* P = nullptr;
  int st = gf_join_pls_plan_create(ctx, qgrid, lines, r, approximate, metric, &P);
  if (st) return st;
  st = gf_join_ppoly_run(P, ugrid, pts, pairs, cap, npairs);
  gf_range_plan_destroy(P);
  return st;
}

extern "C" int gf_range_plan_stats(const gf_range_plan* P, int64_t* none_cells, int64_t* candidate_cells,
                                   int64_t* guaranteed_cells, int64_t* inside_cells) {
  if (!P) return GF_ERR_ARG;
  if (none_cells) *none_cells = P->cls_cells[0];
  if (candidate_cells) *candidate_cells = P->cls_cells[1];
  if (guaranteed_cells) *guaranteed_cells = P->cls_cells[2];
  if (inside_cells) *inside_cells = P->cls_cells[3];
  return GF_OK;
}

extern "C" int gf_range_plan_set_tuning(gf_range_plan* P, int32_t scan_blocks, int32_t defer_mode) {
  if (!P || scan_blocks < 0 || scan_blocks > P->ctx->num_cus * 8 || defer_mode < 0 || defer_mode > 3)
    return GF_ERR_ARG;
  P->scan_blocks = scan_blocks;
  P->defer_mode = defer_mode;
  return GF_OK;
}

extern "C" int gf_range_plan_set_drain_lanes(gf_range_plan* P, int32_t lanes) {
  if (!P || lanes < 0 || lanes > 64) return GF_ERR_ARG;
  P->drain_lanes = lanes;
  return GF_OK;
}

extern "C" int gf_bitmap_to_indices(gf_ctx* ctx, const uint64_t* bitmap, int64_t n, uint32_t* idx, int64_t cap,
                                    int64_t* count) {
  if (!ctx || !bitmap || n < 0 || !count) return set_err(ctx, GF_ERR_ARG, "gf_bitmap_to_indices: bad argument");
  int st = bind(ctx);
  if (st) return st;
  const int64_t words = (n + 63) / 64;
  Arena ar;
  uint32_t *pc, *off, *tmp;
  ar.take(pc, words + 1);
  ar.take(off, words + 1);
  ar.take(tmp, scan_tmp_elems(words));
  if ((st = ar.alloc(ctx))) return st;
  GF_HIP_CHECK(ctx, launch_word_popcounts(ctx->stream, bitmap, words, pc));
  GF_HIP_CHECK(ctx, launch_exclusive_scan(ctx->stream, pc, words, off, tmp));
  uint32_t total = 0;
  if (int e = read_scalar_sync(ctx, off + words, &total)) return e;
  *count = total;
  if ((int64_t)total > cap) return GF_ERR_CAPACITY;
  if (total) {
    if (!idx) return GF_ERR_ARG;
    GF_HIP_CHECK(ctx, launch_expand_bitmap(ctx->stream, bitmap, words, n, off, idx, cap));
    GF_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  }
  return GF_OK;
}

extern "C" int gf_bitmap_to_indices_async(gf_ctx* ctx, const uint64_t* bitmap, int64_t n, uint32_t* idx, int64_t cap,
                                          int64_t* count) {
  if (!ctx || !bitmap || n < 0 || n > (int64_t)UINT32_MAX || !count || cap < 0 || (cap > 0 && !idx))
    return set_err(ctx, GF_ERR_ARG, "gf_bitmap_to_indices_async: bad argument");
  int st = bind(ctx);
  if (st) return st;
  const int64_t words = (n + 63) / 64, blocks = expand_blocks(words);
  // (an empty bitmap only zeroes the count: no kernel, no ticket taken)
  return lookback_launch(ctx, blocks, words > 0 ? blocks : 0, "launch_expand_bitmap_async", [&](const ExpandState& es) {
    return launch_expand_bitmap_async(ctx->stream, bitmap, words, n, idx, cap, count, es);
  });
}

