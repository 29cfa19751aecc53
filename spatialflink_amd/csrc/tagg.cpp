// tagg.cpp -- tAggregate entry points of the C ABI (PointTAggregateQuery.java, TAggregateQuery.java:
// 498-613): gf_tagg_group (a window grouped by (cell, objID)), gf_tagg_run (per-group and per-cell
// statistics), the reads and the pure-host row rules (gf_tagg_rows).  The kernels are in k_tagg.hip;
// the three groupings and the sort of the groups by cell are gf_group.hpp's (traj.cpp).  The object
// is made of gf_group.hpp's typed device arrays (grow-only, freed by its destructor) and is reused
// across windows.
#define GF_TU_NAME tagg_cpp
#include "gf_buildtag.hpp"  // first: records this unit's command-line defines

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "gf_group.hpp"

using namespace gf;

struct gf_tagg {
  gf_ctx* ctx = nullptr;
  int64_t n = 0, ncells = 0, ngroups = 0;
  int64_t long_len = kTaggLongLen, big_cell = kTaggBigCell;
  bool ran = false;
  KeyGroups cells, objs, pairs;  // dense ids of pack(cx, cy), of objID, and the grouping of their pair
  KeyGroups bycell;              // the groups sorted by cell id (sort only)
  DevArr<int64_t> ckey, comp;
  DevArr<uint32_t> g_cell, g_m, g_f, g_s, list, counters;
  DevArr<int64_t> g_key, g_L, g_e;
  DevArr<int32_t> c_cx, c_cy;
  DevArr<int64_t> c_count, c_multi, c_sum, c_minLen, c_minKey, c_maxLen, c_maxKey, all_key, all_len;
};

extern "C" int gf_tagg_group(gf_ctx* ctx, const gf_grid* grid, const gf_points* pts, gf_tagg** out) {
  if (!ctx || !out || !pts || !grid) return set_err(ctx, GF_ERR_ARG, "gf_tagg_group: null argument");
  if (!grid_ok(grid)) return set_err(ctx, GF_ERR_ARG, "gf_tagg_group: invalid grid");
  if (pts->n < 0 || pts->n > (int64_t)UINT32_MAX) return set_err(ctx, GF_ERR_ARG, "gf_tagg_group: need 0 <= n < 2^32");
  if (pts->n > 0 && (!pts->x || !pts->y || !pts->objID)) return set_err(ctx, GF_ERR_ARG, "gf_tagg_group: null x / y / objID");
  if (*out && (*out)->ctx != ctx) return set_err(ctx, GF_ERR_ARG, "gf_tagg_group: object of another context");
  int st = bind(ctx);
  if (st) return st;
  const bool fresh = *out == nullptr;
  gf_tagg* G = fresh ? new gf_tagg() : *out;
  G->ctx = ctx;
  auto fail = [&](int code) {
    if (fresh) gf_tagg_destroy(G);
    else G->n = G->ncells = G->ngroups = 0;
    return code;
  };
  const int64_t n = pts->n;
  G->n = n;
  G->ncells = G->ngroups = 0;
  G->ran = false;
  if (n == 0) {
    *out = G;
    return GF_OK;
  }
  if ((st = G->ckey.reserve(ctx, (size_t)n)) || (st = G->comp.reserve(ctx, (size_t)n))) return fail(st);
  TaggArgs a{};
  a.x = pts->x; a.y = pts->y; a.n = n;
  a.minX = grid->minX; a.minY = grid->minY; a.cl = grid->cellLength;
  a.ckey = G->ckey.p;
  a.comp = G->comp.p;
  hipError_t e = launch_tagg(ctx, kTaggCellKeys, a);
  if (e != hipSuccess) return fail(hip_err(ctx, e, "tagg cell keys"));
  if ((st = group_dense_ids(ctx, G->cells, a.ckey, n, "gf_tagg_group")) ||
      (st = group_dense_ids(ctx, G->objs, pts->objID, n, "gf_tagg_group")))
    return fail(st);
  a.cid = G->cells.did.p;
  a.oid = G->objs.did.p;
  if ((e = launch_tagg(ctx, kTaggPairKeys, a)) != hipSuccess) return fail(hip_err(ctx, e, "tagg pair keys"));
  if ((st = group_dense_ids(ctx, G->pairs, a.comp, n, "gf_tagg_group")) ||
      (st = group_sort_ids(ctx, G->pairs, G->pairs.did.p, n, (uint32_t)G->pairs.ngroups)))
    return fail(st);
  if ((e = hipStreamSynchronize(ctx->stream)) != hipSuccess) return fail(hip_err(ctx, e, "gf_tagg_group"));
  G->ncells = G->cells.ngroups;
  G->ngroups = G->pairs.ngroups;
  *out = G;
  return GF_OK;
}

extern "C" int gf_tagg_run(gf_tagg* G, const gf_points* pts) {
  if (!G || !G->ctx) return GF_ERR_ARG;
  gf_ctx* ctx = G->ctx;
  if (!pts || pts->n != G->n) return set_err(ctx, GF_ERR_ARG, "gf_tagg_run: pts is not the grouped window");
  if (pts->n > 0 && !pts->ts) return set_err(ctx, GF_ERR_ARG, "gf_tagg_run: null ts");
  G->ran = false;
  if (G->n == 0) {
    G->ran = true;
    return GF_OK;
  }
  int st = bind(ctx);
  if (st) return st;
  const size_t ng = (size_t)G->ngroups, nc = (size_t)G->ncells;
  if ((st = G->g_cell.reserve(ctx, ng)) || (st = G->g_m.reserve(ctx, ng)) || (st = G->g_key.reserve(ctx, ng)) ||
      (st = G->g_L.reserve(ctx, ng)) || (st = G->g_e.reserve(ctx, ng)) || (st = G->g_f.reserve(ctx, ng)) ||
      (st = G->g_s.reserve(ctx, ng)) || (st = G->list.reserve(ctx, nc)) || (st = G->counters.reserve(ctx, kCounterWords)) ||
      (st = G->c_cx.reserve(ctx, nc)) || (st = G->c_cy.reserve(ctx, nc)) || (st = G->c_count.reserve(ctx, nc)) ||
      (st = G->c_multi.reserve(ctx, nc)) || (st = G->c_sum.reserve(ctx, nc)) || (st = G->c_minLen.reserve(ctx, nc)) ||
      (st = G->c_minKey.reserve(ctx, nc)) || (st = G->c_maxLen.reserve(ctx, nc)) || (st = G->c_maxKey.reserve(ctx, nc)) ||
      (st = G->all_key.reserve(ctx, ng)) || (st = G->all_len.reserve(ctx, ng)))
    return st;
  TaggArgs a{};
  a.n = G->n;
  a.ts = pts->ts;
  a.perm = G->pairs.perm.p;
  a.seg_off = G->pairs.seg_off.p;
  a.sorted = G->pairs.kbuf[G->pairs.sorted_in].p;
  a.gkeys = G->pairs.keys.p;
  a.okeys = G->objs.keys.p;
  a.ngroups = G->ngroups;
  a.long_len = (uint32_t)G->long_len;
  a.g_cell = G->g_cell.p; a.g_m = G->g_m.p; a.g_key = G->g_key.p; a.g_L = G->g_L.p; a.g_e = G->g_e.p;
  a.g_f = G->g_f.p; a.g_s = G->g_s.p; a.list = G->list.p;
  a.list_count = G->counters.p;
  GF_HIP_CHECK(ctx, hipMemsetAsync(G->counters.p, 0, kCounterWords * sizeof(uint32_t), ctx->stream));
  GF_HIP_CHECK(ctx, launch_tagg(ctx, kTaggGroupStats, a));
  // the groups sorted stably by cell id (every cell has a group): a cell's groups stay in first-occurrence order
  if ((st = group_sort_ids(ctx, G->bycell, a.g_cell, G->ngroups, (uint32_t)G->ncells))) return st;
  a.gperm = G->bycell.perm.p;
  a.cell_off = G->bycell.seg_off.p;
  a.ckeys = G->cells.keys.p;
  a.ncells = G->ncells;
  a.big_cell = (uint32_t)G->big_cell;
  a.list_count = G->counters.p + 1;
  a.c_cx = G->c_cx.p; a.c_cy = G->c_cy.p; a.c_count = G->c_count.p; a.c_multi = G->c_multi.p; a.c_sum = G->c_sum.p;
  a.c_minLen = G->c_minLen.p; a.c_minKey = G->c_minKey.p; a.c_maxLen = G->c_maxLen.p; a.c_maxKey = G->c_maxKey.p;
  a.all_key = G->all_key.p; a.all_len = G->all_len.p;
  GF_HIP_CHECK(ctx, launch_tagg(ctx, kTaggCells, a));
  GF_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  G->ran = true;
  return GF_OK;
}

extern "C" void gf_tagg_destroy(gf_tagg* G) {
  if (!G) return;
  if (G->ctx) {
    hipSetDevice(G->ctx->device);
    hipStreamSynchronize(G->ctx->stream);
  }
  delete G;
}

extern "C" int gf_tagg_info(const gf_tagg* G, int64_t* cells, int64_t* groups, int64_t* n) {
  if (!G) return GF_ERR_ARG;
  if (cells) *cells = G->ncells;
  if (groups) *groups = G->ngroups;
  if (n) *n = G->n;
  return GF_OK;
}

extern "C" int gf_tagg_set_thresholds(gf_tagg* G, int64_t long_group, int64_t big_cell) {
  if (!G || long_group < 0 || long_group > (int64_t)UINT32_MAX || big_cell < 0 || big_cell > (int64_t)UINT32_MAX)
    return GF_ERR_ARG;
  G->long_len = long_group == 0 ? kTaggLongLen : long_group;
  G->big_cell = big_cell == 0 ? kTaggBigCell : big_cell;
  return GF_OK;
}

extern "C" int gf_tagg_read_cells(gf_tagg* G, int32_t* cx, int32_t* cy, int64_t* count, int64_t* multi, int64_t* sum,
                                  int64_t* minLen, int64_t* minKey, int64_t* maxLen, int64_t* maxKey, int64_t cap,
                                  int64_t* cells) {
  if (!G || !G->ctx) return GF_ERR_ARG;
  gf_ctx* ctx = G->ctx;
  if (!cells || cap < 0) return set_err(ctx, GF_ERR_ARG, "gf_tagg_read_cells: bad argument");
  if (!G->ran) return set_err(ctx, GF_ERR_ARG, "gf_tagg_read_cells: no gf_tagg_run since the last grouping");
  *cells = G->ncells;
  const size_t w = (size_t)std::min(G->ncells, cap);
  if (w == 0) return GF_OK;
  int st = bind(ctx);
  if (st) return st;
  if ((st = read_back(ctx, cx, G->c_cx.p, w)) || (st = read_back(ctx, cy, G->c_cy.p, w)) ||
      (st = read_back(ctx, count, G->c_count.p, w)) || (st = read_back(ctx, multi, G->c_multi.p, w)) ||
      (st = read_back(ctx, sum, G->c_sum.p, w)) || (st = read_back(ctx, minLen, G->c_minLen.p, w)) ||
      (st = read_back(ctx, minKey, G->c_minKey.p, w)) || (st = read_back(ctx, maxLen, G->c_maxLen.p, w)) ||
      (st = read_back(ctx, maxKey, G->c_maxKey.p, w)))
    return st;
  GF_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  return GF_OK;
}

extern "C" int gf_tagg_read_all(gf_tagg* G, int64_t* off, int64_t* keys, int64_t* len, int64_t cap_cells,
                                int64_t cap_groups, int64_t* cells, int64_t* groups) {
  if (!G || !G->ctx) return GF_ERR_ARG;
  gf_ctx* ctx = G->ctx;
  if (!cells || !groups || cap_cells < 0 || cap_groups < 0) return set_err(ctx, GF_ERR_ARG, "gf_tagg_read_all: bad argument");
  if (!G->ran) return set_err(ctx, GF_ERR_ARG, "gf_tagg_read_all: no gf_tagg_run since the last grouping");
  *cells = G->ncells;
  *groups = G->ngroups;
  if (off) off[0] = 0;
  if (G->ncells == 0) return GF_OK;
  int st = bind(ctx);
  if (st) return st;
  const size_t wc = (size_t)std::min(G->ncells, cap_cells), wg = (size_t)std::min(G->ngroups, cap_groups);
  OffsetRead ho;
  if ((st = read_offsets(ctx, ho, off, G->bycell.seg_off.p, wc + 1)) || (st = read_back(ctx, keys, G->all_key.p, wg)) ||
      (st = read_back(ctx, len, G->all_len.p, wg)))
    return st;
  GF_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  ho.widen();
  return GF_OK;
}

// Math.round(double): floor(x + 1/2) of the exact x (round half up), as a long with Java's saturation
static int64_t java_round(double q) {
  if (std::isnan(q)) return 0;
  const double f = std::floor(q);
  const double r = q - f >= 0.5 ? f + 1.0 : f;  // q - f is exact; past 2^52 every q is an integer
  if (r >= 9223372036854775808.0) return INT64_MAX;
  if (r <= -9223372036854775808.0) return INT64_MIN;
  return (int64_t)r;
}

static bool equals_ignore_case(const char* a, const char* b) {
  for (; *a && *b; ++a, ++b) {
    const char x = *a >= 'a' && *a <= 'z' ? (char)(*a - 32) : *a, y = *b >= 'a' && *b <= 'z' ? (char)(*b - 32) : *b;
    if (x != y) return false;
  }
  return *a == *b;
}

extern "C" int gf_tagg_rows(const char* function, int64_t cells, const int64_t* count, const int64_t* multi,
                            const int64_t* sum, const int64_t* minLen, const int64_t* minKey, const int64_t* maxLen,
                            const int64_t* maxKey, uint8_t* emit, int64_t* value, int64_t* key, int32_t* kind) {
  if (!function || cells < 0 || !emit || !value || !key) return GF_ERR_ARG;
  int k = 0;  // ALL, and the reference's final else: any other name
  if (equals_ignore_case(function, "SUM")) k = 1;
  else if (equals_ignore_case(function, "AVG")) k = 2;
  else if (equals_ignore_case(function, "MIN")) k = 3;
  else if (equals_ignore_case(function, "MAX")) k = 4;
  if (kind) *kind = k;
  if (cells > 0) {
    if (k <= 2 && !sum) return GF_ERR_ARG;
    if (k == 2 && !count) return GF_ERR_ARG;
    if (k == 3 && (!multi || !minLen || !minKey)) return GF_ERR_ARG;
    if (k == 4 && (!multi || !maxLen || !maxKey)) return GF_ERR_ARG;
  }
  for (int64_t c = 0; c < cells; ++c) {
    bool e = true;
    int64_t v = 0, o = 0;
    switch (k) {
      case 0: v = sum[c]; break;
      case 1: e = sum[c] > 0; v = sum[c]; break;
      case 2: e = sum[c] > 0; v = java_round((double)sum[c] / (double)count[c]); break;
      case 3: e = multi[c] > 0; v = minLen[c]; o = minKey[c]; break;
      default: e = multi[c] > 0; v = maxLen[c]; o = maxKey[c]; break;
    }
    emit[c] = e ? 1 : 0;
    value[c] = e ? v : 0;
    key[c] = e ? o : 0;
  }
  return GF_OK;
}
