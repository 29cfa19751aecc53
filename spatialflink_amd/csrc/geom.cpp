// geom.cpp -- polygon / linestring windows against query points: the index of one window
// (gf_geom_prepare; prepared again for the next window, its arrays reused), the query built once per continuous query (its pure host part is
// gf_geom_plan.hpp's), gf_geom_range_run and gf_geom_knn_enqueue.  A query is a point set or, through
// gf_geom_query_create_polygons / _linestrings, a set of polygons or linestrings; the same run calls take
// either.  The kernels are in k_geom.hip (point queries) and k_geompair.hip (geometry queries); the
// kNN record comes from the library's own selection (launch_knn_select for k <= kMaxK, the sorted path
// knn_sorted_record above it).  Everything is enqueued on the context stream; only the calls marked
// sync in the header wait.  The objects' device arrays are gf_group.hpp's typed holders (grow-only).
#define GF_TU_NAME geom_cpp
#include "gf_buildtag.hpp"  // first: records this unit's command-line defines

#include <hip/hip_runtime.h>

#include <cstring>

#include "gf_chain_plan.hpp"
#include "gf_geom_index.hpp"  // struct gf_geom_index: geomjoin.cpp reads it too

using namespace gf;

namespace {
constexpr size_t kIndexCounters = 4;  // GeomArgs::ictr
constexpr size_t kQueryCounters = 8;  // GeomArgs::qctr (5 used)
}  // namespace

struct gf_geom_query {
  gf_ctx* ctx = nullptr;
  gf_grid grid{};
  int32_t nq = 0;
  double r = 0;
  int approx = 0, metric = 0;
  GeomTables tab;  // host copy: the sets' sizes
  DevArr<int32_t> satN, satG;
  DevArr<double> qx, qy;
  // a polygon / linestring query set (qkind != 0; the kernels of k_geompair.hip): CSR, envelopes, runs
  int32_t qkind = 0;
  int plain = 0;        // gf_geom_query_set_chain_mode: 1 = no run envelope is consulted
  int32_t corner = 0;   // guaranteed layers 0, one query, its rectangle leaves the grid
  int32_t q_rect[4] = {0, 0, 0, 0};
  DevArr<int32_t> q_ring_off, q_vert_off, q_run_off;
  DevArr<double> qvx, qvy, q_ring_env, q_env, q_run_env;
  DevArr<unsigned long long> ctr;  // of the last run
  // kNN candidates (grow-only, sized by the largest window so far)
  DevArr<KnnState> st;
  DevArr<double> cand_d;
  DevArr<uint32_t> cand_i;
  DevArr<int64_t> cand_o;
};

static bool same_grid(const gf_grid& a, const gf_grid& b) {
  return a.n == b.n && a.minX == b.minX && a.maxX == b.maxX && a.minY == b.minY && a.maxY == b.maxY &&
         a.cellLength == b.cellLength;
}

// the index's part of the kernel arguments
static void index_args(const gf_geom_index* X, GeomArgs& a) {
  const gf_geoms& G = X->geoms;
  a.kind = G.kind;
  a.nobj = G.nobj;
  a.nrings = X->nrings;
  a.ring_off = G.kind == GF_GEOM_POLYGON ? G.ring_off : nullptr;
  a.vert_off = G.vert_off; a.vx = G.vx; a.vy = G.vy; a.objID = G.objID;
  a.wide_vertices = X->wide_vertices;
  a.minX = X->grid.minX; a.minY = X->grid.minY; a.cl = X->grid.cellLength;
  a.ring_env = X->ring_env.p; a.ring_ok = X->ring_ok.p; a.ring_wide = X->ring_wide.p;
  a.env = X->env.p; a.cells = X->cells.p; a.valid = X->valid.p; a.nvert = X->nvert.p;
  a.ictr = X->ctr.p;
  a.work_short = X->work_short.p; a.work_wide = X->work_wide.p;
}

// ring envelopes -> objects, with the threshold in force
static int index_launch(gf_geom_index* X) {
  gf_ctx* ctx = X->ctx;
  GF_HIP_CHECK(ctx, hipMemsetAsync(X->ctr.p, 0, kIndexCounters * sizeof(unsigned long long), ctx->stream));
  if (X->geoms.nobj == 0) return GF_OK;
  GeomArgs a{};
  index_args(X, a);
  if (X->nrings > 0) {
    GF_HIP_CHECK(ctx, launch_geom(ctx, kGeomRingEnv, a));
    GF_HIP_CHECK(ctx, launch_geom(ctx, kGeomRingEnvWide, a));
  }
  GF_HIP_CHECK(ctx, launch_geom(ctx, kGeomObjects, a));
  return GF_OK;
}

extern "C" void gf_geom_index_destroy(gf_geom_index* X) {
  if (!X) return;
  hipSetDevice(X->ctx->device);
  hipStreamSynchronize(X->ctx->stream);
  delete X;
}

extern "C" int gf_geom_prepare(gf_ctx* ctx, const gf_grid* g, const gf_geoms* geoms, gf_geom_index** out) {
  if (!ctx || !out || !grid_ok(g) || !geoms || geoms->nobj < 0 || geoms->nobj > (int64_t)INT32_MAX ||
      (geoms->kind != GF_GEOM_POLYGON && geoms->kind != GF_GEOM_LINESTRING) || (geoms->nobj > 0 && !geoms->vert_off) ||
      (geoms->nobj > 0 && geoms->kind == GF_GEOM_POLYGON && (!geoms->ring_off || geoms->nrings < 0)) ||
      (!geoms->vx != !geoms->vy) || (*out && (*out)->ctx != ctx))
    return set_err(ctx, GF_ERR_ARG, "gf_geom_prepare: bad argument");
  int st = bind(ctx);
  if (st) return st;
  gf_geom_index* X = *out ? *out : new gf_geom_index();
  X->ctx = ctx;
  X->grid = *g;
  X->geoms = *geoms;
  const size_t n = (size_t)geoms->nobj;
  X->nrings = geoms->kind == GF_GEOM_POLYGON ? (n > 0 ? geoms->nrings : 0) : geoms->nobj;
  // grow-only: in a continuous query no window after the largest allocates or synchronises
  const size_t nr = (size_t)std::max<int64_t>(X->nrings, 1), no = std::max<size_t>(n, 1);
  if ((st = X->ring_env.reserve(ctx, 4 * nr)) || (st = X->ring_ok.reserve(ctx, nr)) || (st = X->ring_wide.reserve(ctx, nr)) ||
      (st = X->env.reserve(ctx, 4 * no)) || (st = X->cells.reserve(ctx, 4 * no)) || (st = X->valid.reserve(ctx, no)) ||
      (st = X->nvert.reserve(ctx, no)) || (st = X->work_short.reserve(ctx, no)) || (st = X->work_wide.reserve(ctx, no)) ||
      (st = X->ctr.reserve(ctx, kIndexCounters)) || (st = index_launch(X))) {
    if (!*out) gf_geom_index_destroy(X);
    return st;
  }
  *out = X;
  return GF_OK;
}

extern "C" int gf_geom_index_set_thresholds(gf_geom_index* X, int32_t wide_vertices) {
  if (!X || wide_vertices < 0) return GF_ERR_ARG;
  int st = bind(X->ctx);
  if (st) return st;
  X->wide_vertices = wide_vertices == 0 ? kGeomWideVertices : wide_vertices;
  return index_launch(X);  // the envelopes again, by the lanes and waves the new threshold assigns
}

extern "C" int gf_geom_index_info(gf_geom_index* X, int64_t* nobj, int64_t* nvert, int64_t* invalid, int64_t* wide) {
  if (!X) return GF_ERR_ARG;
  gf_ctx* ctx = X->ctx;
  int st = bind(ctx);
  if (st) return st;
  unsigned long long* c = (unsigned long long*)ctx_pinned(ctx, kIndexCounters * sizeof(unsigned long long), &st);
  if (!c) return st;
  GF_HIP_CHECK(ctx, hipMemcpyAsync(c, X->ctr.p, kIndexCounters * sizeof(unsigned long long), hipMemcpyDeviceToHost,
                                   ctx->stream));
  GF_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  if (nobj) *nobj = X->geoms.nobj;
  if (nvert) *nvert = (int64_t)c[1];
  if (invalid) *invalid = (int64_t)c[2];
  if (wide) *wide = (int64_t)c[3];
  return GF_OK;
}

extern "C" int gf_geom_index_read(gf_geom_index* X, double* env, int32_t* cells) {
  if (!X) return GF_ERR_ARG;
  gf_ctx* ctx = X->ctx;
  int st = bind(ctx);
  if (st) return st;
  const size_t n = (size_t)X->geoms.nobj;
  if ((st = read_back(ctx, env, X->env.p, 4 * n)) || (st = read_back(ctx, cells, X->cells.p, 4 * n))) return st;
  GF_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  return GF_OK;
}

extern "C" void gf_geom_query_destroy(gf_geom_query* Q) {
  if (!Q) return;
  hipSetDevice(Q->ctx->device);
  hipStreamSynchronize(Q->ctx->stream);
  delete Q;
}

extern "C" int gf_geom_query_create(gf_ctx* ctx, const gf_grid* g, const double* qx, const double* qy, int32_t nq, double r,
                                    int approximate, int metric, gf_geom_query** out) {
  if (!out || !grid_ok(g) || nq <= 0 || !qx || !qy || (metric != 0 && metric != 1) || g->n > kGeomMaxGrid)
    return set_err(ctx, GF_ERR_ARG, "gf_geom_query_create: bad argument");
  *out = nullptr;
  // getNeighboringCells: r == 0 is every cell; otherwise the candidate layers must be positive
  const int32_t gl = guaranteed_layers(g->cellLength, r), cl = candidate_layers(g->cellLength, r);
  if (r != 0.0 && cl <= 0) return set_err(ctx, GF_ERR_LAYERS, "candidateNeighboringLayers cannot be 0 or less");
  if (!ctx) return GF_ERR_ARG;
  int st = bind(ctx);
  if (st) return st;
  gf_geom_query* Q = new gf_geom_query();
  Q->ctx = ctx;
  Q->grid = *g;
  Q->nq = nq;
  Q->r = r;
  Q->approx = approximate != 0;
  Q->metric = metric;
  std::vector<int32_t> qcx((size_t)nq), qcy((size_t)nq);
  for (int32_t q = 0; q < nq; ++q) {
    qcx[q] = cell_index(qx[q], g->minX, g->cellLength);
    qcy[q] = cell_index(qy[q], g->minY, g->cellLength);
  }
  if (geom_build_tables(g->n, nq, qcx.data(), qcy.data(), gl, cl, r == 0.0, Q->tab)) {
    delete Q;
    return set_err(ctx, GF_ERR_ARG, "gf_geom_query_create: grid too large for the summed-area tables");
  }
  std::vector<double> vqx(qx, qx + nq), vqy(qy, qy + nq);
  std::vector<unsigned long long> zero(kQueryCounters, 0);
  std::vector<KnnState> st0(1);
  std::memset(st0.data(), 0, sizeof(KnnState));
  if ((st = upload(ctx, Q->satN, Q->tab.satN)) || (st = upload(ctx, Q->satG, Q->tab.satG)) || (st = upload(ctx, Q->qx, vqx)) ||
      (st = upload(ctx, Q->qy, vqy)) || (st = upload(ctx, Q->ctr, zero)) || (st = upload(ctx, Q->st, st0))) {
    gf_geom_query_destroy(Q);
    return st;
  }
  Q->tab.satN = std::vector<int32_t>();  // the host keeps the counts only
  Q->tab.satG = std::vector<int32_t>();
  *out = Q;
  return GF_OK;
}

// A query set of polygons (ring_off != null) or linestrings: every ring / chain goes through
// gf_chain_plan.hpp as one line -- its envelope and its runs of kChainRun segments.
static int geom_query_create_set(gf_ctx* ctx, const gf_grid* g, int32_t qkind, int32_t nq, const int32_t* ring_off,
                                 const int32_t* vert_off, const double* vx, const double* vy, double r, int approximate,
                                 int metric, gf_geom_query** out, const char* who) {
  if (!out || !grid_ok(g) || (metric != 0 && metric != 1) || g->n > kGeomMaxGrid ||
      !geom_query_set_valid(nq, ring_off, vert_off, vx, vy))
    return set_err(ctx, GF_ERR_ARG, std::string(who) + ": bad argument (a grid, a metric, >= 1 legal geometries)");
  *out = nullptr;
  if (!ctx) return GF_ERR_ARG;
  // no getNeighboringCells here: candidate layers <= 0 is an empty N, not an error
  const int32_t gl = guaranteed_layers(g->cellLength, r), cl = candidate_layers(g->cellLength, r);
  gf_linestrings rings{ring_off ? ring_off[nq] : nq, vert_off, vx, vy};
  ChainTables T;
  chain_build(rings, kChainRun, T);
  std::vector<int32_t> ro, rects(4 * (size_t)nq);
  std::vector<double> env(4 * (size_t)nq), renv(4 * (size_t)rings.nline);
  for (int32_t j = 0; j < rings.nline; ++j) {  // x1, y1, x2, y2 -> PolyView's minx, maxx, miny, maxy
    const double* b = &T.bbox[4 * (size_t)j];
    double* e = &renv[4 * (size_t)j];
    e[0] = b[0]; e[1] = b[2]; e[2] = b[1]; e[3] = b[3];
  }
  for (int32_t q = 0; q < nq; ++q) {  // boundingBox: the shell's / the chain's; gridIDsSet: its cell rectangle
    const double* b = &T.bbox[4 * (size_t)(ring_off ? ring_off[q] : q)];
    std::memcpy(&env[4 * (size_t)q], b, 4 * sizeof(double));
    int32_t* c = &rects[4 * (size_t)q];
    c[0] = cell_index(b[0], g->minX, g->cellLength);
    c[1] = cell_index(b[1], g->minY, g->cellLength);
    c[2] = cell_index(b[2], g->minX, g->cellLength);
    c[3] = cell_index(b[3], g->minY, g->cellLength);
  }
  gf_geom_query* Q = new gf_geom_query();
  bool leaves = false;
  if (geom_build_tables_rects(g->n, nq, rects.data(), gl, cl, Q->tab, &leaves)) {
    delete Q;
    return set_err(ctx, GF_ERR_ARG, std::string(who) + ": grid too large for the summed-area tables");
  }
  if (leaves && nq > 1) {  // the deviation of contract 2: G outside the grid as a union of rectangles
    delete Q;
    return set_err(ctx, GF_ERR_ARG, std::string(who) + ": guaranteed layers 0 with several queries and a query rectangle "
                                                       "that leaves the grid is not supported");
  }
  int st = bind(ctx);
  if (st) { delete Q; return st; }
  Q->ctx = ctx;
  Q->grid = *g;
  Q->nq = nq;
  Q->r = r;
  Q->approx = approximate != 0;
  Q->metric = metric;
  Q->qkind = qkind;
  Q->corner = leaves;
  std::memcpy(Q->q_rect, rects.data(), sizeof(Q->q_rect));
  if (ring_off) ro.assign(ring_off, ring_off + nq + 1);
  else ro.assign(1, 0);  // (never read: a linestring query has no ring level)
  std::vector<unsigned long long> zero(kQueryCounters, 0);
  std::vector<KnnState> st0(1);
  std::memset(st0.data(), 0, sizeof(KnnState));
  if ((st = upload(ctx, Q->satN, Q->tab.satN)) || (st = upload(ctx, Q->satG, Q->tab.satG)) ||
      (st = upload(ctx, Q->q_ring_off, ro)) || (st = upload(ctx, Q->q_vert_off, T.vert_off)) || (st = upload(ctx, Q->qvx, T.vx)) ||
      (st = upload(ctx, Q->qvy, T.vy)) || (st = upload(ctx, Q->q_ring_env, renv)) || (st = upload(ctx, Q->q_env, env)) ||
      (st = upload(ctx, Q->q_run_off, T.run_off)) || (st = upload(ctx, Q->q_run_env, T.run_env)) ||
      (st = upload(ctx, Q->ctr, zero)) || (st = upload(ctx, Q->st, st0))) {
    gf_geom_query_destroy(Q);
    return st;
  }
  Q->tab.satN = std::vector<int32_t>();  // the host keeps the counts only
  Q->tab.satG = std::vector<int32_t>();
  *out = Q;
  return GF_OK;
}

extern "C" int gf_geom_query_create_polygons(gf_ctx* ctx, const gf_grid* g, const gf_polygons* polys, double r, int approximate,
                                             int metric, gf_geom_query** out) {
  if (!polys || !polys->ring_off) return set_err(ctx, GF_ERR_ARG, "gf_geom_query_create_polygons: bad argument");
  return geom_query_create_set(ctx, g, GF_GEOM_POLYGON, polys->npoly, polys->ring_off, polys->vert_off, polys->vx, polys->vy, r,
                               approximate, metric, out, "gf_geom_query_create_polygons");
}

extern "C" int gf_geom_query_create_linestrings(gf_ctx* ctx, const gf_grid* g, const gf_linestrings* lines, double r,
                                                int approximate, int metric, gf_geom_query** out) {
  if (!lines) return set_err(ctx, GF_ERR_ARG, "gf_geom_query_create_linestrings: bad argument");
  return geom_query_create_set(ctx, g, GF_GEOM_LINESTRING, lines->nline, nullptr, lines->vert_off, lines->vx, lines->vy, r,
                               approximate, metric, out, "gf_geom_query_create_linestrings");
}

extern "C" int gf_geom_query_set_chain_mode(gf_geom_query* Q, int mode) {
  if (!Q || Q->qkind == 0 || (mode != 0 && mode != 1)) return GF_ERR_ARG;
  Q->plain = mode;
  return GF_OK;
}

// a query meets an index: same context, same grid
static int geom_pair_ok(const gf_geom_query* Q, const gf_geom_index* X, const char* who) {
  if (!Q || !X) return GF_ERR_ARG;
  if (Q->ctx != X->ctx || !same_grid(Q->grid, X->grid))
    return set_err(Q->ctx, GF_ERR_ARG, std::string(who) + ": the window was prepared on another grid or context");
  return GF_OK;
}

static void query_args(const gf_geom_query* Q, GeomArgs& a) {
  a.grid_n = Q->grid.n;
  a.satN = Q->satN.p; a.satG = Q->satG.p;
  a.qx = Q->qx.p; a.qy = Q->qy.p; a.nq = Q->nq;
  a.r = Q->r; a.approx = Q->approx; a.metric = Q->metric;
  a.qctr = Q->ctr.p;
}

// classify + the two exact passes of one window
static int geom_passes(gf_geom_query* Q, gf_geom_index* X, GeomArgs& a) {
  gf_ctx* ctx = Q->ctx;
  GF_HIP_CHECK(ctx, hipMemsetAsync(Q->ctr.p, 0, kQueryCounters * sizeof(unsigned long long), ctx->stream));
  if (X->geoms.nobj == 0) return GF_OK;
  if (Q->qkind) {  // a polygon / linestring query: the same three passes with the pair distance (k_geompair.hip)
    GeomPairArgs p{};
    p.g = a;
    p.qkind = Q->qkind;
    p.q_ring_off = Q->qkind == GF_GEOM_POLYGON ? Q->q_ring_off.p : nullptr;
    p.q_vert_off = Q->q_vert_off.p; p.qvx = Q->qvx.p; p.qvy = Q->qvy.p;
    p.q_ring_env = Q->q_ring_env.p; p.q_env = Q->q_env.p;
    p.q_run_off = Q->plain ? nullptr : Q->q_run_off.p;
    p.q_run_env = Q->q_run_env.p;
    p.corner = Q->corner;
    std::memcpy(p.q_rect, Q->q_rect, sizeof(p.q_rect));
    GF_HIP_CHECK(ctx, launch_geompair(ctx, kGeomPairClassify, p));
    GF_HIP_CHECK(ctx, launch_geompair(ctx, kGeomPairShort, p));
    if (!Q->approx) GF_HIP_CHECK(ctx, launch_geompair(ctx, kGeomPairWide, p));
    return GF_OK;
  }
  GF_HIP_CHECK(ctx, launch_geom(ctx, kGeomClassify, a));
  GF_HIP_CHECK(ctx, launch_geom(ctx, kGeomExactShort, a));
  if (!Q->approx) GF_HIP_CHECK(ctx, launch_geom(ctx, kGeomExactWide, a));
  return GF_OK;
}

extern "C" int gf_geom_range_run(gf_geom_query* Q, gf_geom_index* X, uint64_t* bitmap, int64_t* counts) {
  if (int st = geom_pair_ok(Q, X, "gf_geom_range_run")) return st;
  gf_ctx* ctx = Q->ctx;
  if (X->geoms.nobj > 0 && !bitmap) return set_err(ctx, GF_ERR_ARG, "gf_geom_range_run: null bitmap");
  int st = bind(ctx);
  if (st) return st;
  GeomArgs a{};
  index_args(X, a);
  query_args(Q, a);
  a.bitmap = bitmap;
  a.counts = counts;
  if ((st = geom_passes(Q, X, a))) return st;
  if (counts) {
    if (X->geoms.nobj == 0) GF_HIP_CHECK(ctx, hipMemsetAsync(counts, 0, 2 * sizeof(int64_t), ctx->stream));
    else GF_HIP_CHECK(ctx, launch_geom(ctx, kGeomCount, a));
  }
  return GF_OK;
}

extern "C" int gf_geom_knn_enqueue(gf_geom_query* Q, gf_geom_index* X, int32_t k, void* result) {
  if (int st = geom_pair_ok(Q, X, "gf_geom_knn_enqueue")) return st;
  gf_ctx* ctx = Q->ctx;
  if (!result || k < 1 || k > kMaxKLarge || Q->nq != 1 || (X->geoms.nobj > 0 && !X->geoms.objID))
    return set_err(ctx, GF_ERR_ARG, "gf_geom_knn_enqueue: bad argument (one query point or geometry, k >= 1, objID keys)");
  int st = bind(ctx);
  if (st) return st;
  const size_t cap = (size_t)std::max<int64_t>(X->geoms.nobj, 1);
  if ((st = Q->cand_d.reserve(ctx, cap)) || (st = Q->cand_i.reserve(ctx, cap)) || (st = Q->cand_o.reserve(ctx, cap))) return st;
  GeomArgs a{};
  index_args(X, a);
  query_args(Q, a);
  a.knn = 1;
  a.st = Q->st.p;
  a.cand_d = Q->cand_d.p; a.cand_i = Q->cand_i.p; a.cand_o = Q->cand_o.p;
  if ((st = geom_passes(Q, X, a))) return st;
  // at most one candidate per object, so the buffers never overflow and the record is final (status 0)
  if (k <= kMaxK) {
    KnnSelectArgs s{};
    s.st = Q->st.p;
    s.cand_d = Q->cand_d.p; s.cand_i = Q->cand_i.p; s.cand_o = Q->cand_o.p;
    s.cap = Q->cand_d.cap;
    s.use_state = 0; s.T = Q->r; s.r = Q->r; s.k = k; s.write_hint = 0; s.idx_base = 0;
    s.result = result;
    GF_HIP_CHECK(ctx, launch_knn_select(ctx, s));  // (zeroes st->count for the next window)
    return GF_OK;
  }
  return knn_sorted_record(ctx, Q->cand_d.p, Q->cand_o.p, Q->cand_i.p, &Q->st.p->count, &Q->st.p->maybe, X->geoms.nobj, k,
                           Q->r, 0, result);
}

extern "C" int gf_geom_info(const gf_geom_query* Q, int64_t* filtered, int64_t* all_guaranteed, int64_t* tested,
                            int64_t* wave_path) {
  if (!Q) return GF_ERR_ARG;
  gf_ctx* ctx = Q->ctx;
  int st = bind(ctx);
  if (st) return st;
  unsigned long long* c = (unsigned long long*)ctx_pinned(ctx, kQueryCounters * sizeof(unsigned long long), &st);
  if (!c) return st;
  GF_HIP_CHECK(ctx, hipMemcpyAsync(c, Q->ctr.p, kQueryCounters * sizeof(unsigned long long), hipMemcpyDeviceToHost,
                                   ctx->stream));
  GF_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  if (filtered) *filtered = (int64_t)c[2];
  if (all_guaranteed) *all_guaranteed = (int64_t)c[3];
  if (tested) *tested = (int64_t)(c[0] + c[1]);
  if (wave_path) *wave_path = (int64_t)c[1];
  return GF_OK;
}
