// knn.cpp -- kNN plans (point and polygon queries) and their per-window entry points: the staged
// sample / scan / select path, the pipelined fused launches (depth 2 to 4), the sorted path for
// k > kMaxK, record decoding with its exact fallback, and the record merges.
#define GF_TU_NAME knn_cpp
#include "gf_buildtag.hpp"  // first: records this unit's command-line defines

#include <hip/hip_runtime.h>

#include <initializer_list>
#include <iterator>
#include <limits>
#include <unordered_set>

#include "gf_chain_plan.hpp"
#include "gf_host.hpp"

using namespace gf;

// ---------------------------------------------------------------------------------------
// kNN
// ---------------------------------------------------------------------------------------
extern "C" size_t gf_knn_result_bytes(int32_t k) {
  return sizeof(gf_knn_header) + (size_t)(k > 0 ? k : 0) * (sizeof(double) + 2 * sizeof(int64_t));
}

extern "C" void gf_knn_plan_destroy(gf_knn_plan* P) {
  if (!P) return;
  hipSetDevice(P->ctx->device);
  hipStreamSynchronize(P->ctx->stream);
  for (auto& L : P->lane) {
    if (L.st) hipFree(L.st);
    if (L.cand_d) hipFree(L.cand_d);
    if (L.cand_i) hipFree(L.cand_i);
    if (L.cand_o) hipFree(L.cand_o);
  }
  if (P->tmp_result) hipFree(P->tmp_result);
  if (P->host_result) hipHostFree(P->host_result);
  for (void* q : {(void*)P->ring_off, (void*)P->vert_off, (void*)P->vx, (void*)P->vy, (void*)P->ring_env})
    if (q) hipFree(q);
  for (uint32_t* m : P->maybe_i)  // one survivor buffer per stream (depth 4: three)
    if (m) hipFree(m);
  delete P;
}

static int knn_alloc_lane(gf_knn_plan* P, int j, int64_t cap) {
  gf_ctx* ctx = P->ctx;
  gf_knn_plan::Lane& L = P->lane[j];
  if (!L.st) {
    GF_HIP_CHECK(ctx, hipMalloc(&L.st, sizeof(KnnState)));
    GF_HIP_CHECK(ctx, hipMemset(L.st, 0, sizeof(KnnState)));
  }
  if (L.cand_d) hipFree(L.cand_d);
  if (L.cand_i) hipFree(L.cand_i);
  if (L.cand_o) hipFree(L.cand_o);
  L.cand_d = nullptr;
  L.cand_i = nullptr;
  L.cand_o = nullptr;
  GF_HIP_CHECK(ctx, hipMalloc(&L.cand_d, sizeof(double) * (size_t)cap));
  GF_HIP_CHECK(ctx, hipMalloc(&L.cand_i, sizeof(uint32_t) * (size_t)cap));
  GF_HIP_CHECK(ctx, hipMalloc(&L.cand_o, sizeof(int64_t) * (size_t)cap));
  return GF_OK;
}

static int knn_alloc_candidates(gf_knn_plan* P, int64_t cap) {
  int st;
  // queued windows may still read the old buffers (the k > kMaxK path queues without host reads)
  GF_HIP_CHECK(P->ctx, hipStreamSynchronize(P->ctx->stream));
  if (int e = sync_aux(P->ctx)) return e;
  for (int j = 0; j < (int)std::size(P->lane); ++j)  // lanes 1.. only once pipelining allocated them
    if ((j == 0 || P->lane[j].st) && (st = knn_alloc_lane(P, j, cap))) return st;
  P->cap = cap;
  return GF_OK;
}

extern "C" int gf_knn_pp_plan_create(gf_ctx* ctx, const gf_grid* g, double qx, double qy, double r, int32_t k,
                                     int metric, gf_knn_plan** out) {
  if (!ctx || !out || !grid_ok(g) || k < 1 || k > kMaxKLarge || (metric != 0 && metric != 1))
    return set_err(ctx, GF_ERR_ARG, "gf_knn_pp_plan_create: bad argument (k must be in [1, 2^24])");
  *out = nullptr;
  int st = bind(ctx);
  if (st) return st;
  gf_knn_plan* P = new gf_knn_plan();
  P->ctx = ctx;
  P->grid = *g;
  P->qx = qx; P->qy = qy; P->r = r; P->k = k; P->metric = metric;
  const int32_t gl = guaranteed_layers(g->cellLength, r), cl = candidate_layers(g->cellLength, r);
  const int32_t qcx = cell_index(qx, g->minX, g->cellLength), qcy = cell_index(qy, g->minY, g->cellLength);
  P->qr = make_qrect(*g, qcx, qcy, gl, cl);  // PointPointKNNQuery.java:134-135
  auto fail = [&](int s) { gf_knn_plan_destroy(P); return s; };
  hipError_t e;
  if ((st = knn_alloc_candidates(P, (int64_t)1 << 20))) return fail(st);
  if ((e = hipMalloc(&P->tmp_result, gf_knn_result_bytes(k))) != hipSuccess) return fail(hip_err(ctx, e, "hipMalloc"));
  if ((e = hipHostMalloc(&P->host_result, gf_knn_result_bytes(k), hipHostMallocDefault)) != hipSuccess)
    return fail(hip_err(ctx, e, "hipHostMalloc"));
  P->scan_blocks = 0;
  P->large = k > kMaxK;
  *out = P;
  return GF_OK;
}

// C u G of the cells under P->bbox (x1, y1, x2, y2) as one rect pair: valid cells within c of the bbox
// rect; for g == 0 the bbox cells themselves, no validKey.  Shared by the polygon and the linestring
// query (UniformGrid.java:193-222, 399-426: per-bbox-cell unions in both forms).
static void bbox_query_rect(gf_knn_plan* P, const gf_grid* g, double r) {
  const int32_t gl = guaranteed_layers(g->cellLength, r), cl = candidate_layers(g->cellLength, r);
  const int64_t bx0 = cell_index(P->bbox[0], g->minX, g->cellLength), bx1 = cell_index(P->bbox[2], g->minX, g->cellLength);
  const int64_t by0 = cell_index(P->bbox[1], g->minY, g->cellLength), by1 = cell_index(P->bbox[3], g->minY, g->cellLength);
  const double nan = std::numeric_limits<double>::quiet_NaN();
  const int64_t n1 = g->n - 1;
  QueryRect q;
  q.minX = g->minX;
  q.minY = g->minY;
  if (cl > 0) {
    q.cgx = axis_iv(std::max<int64_t>(bx0 - cl, 0), std::min<int64_t>(bx1 + cl, n1), g->minX, g->cellLength);
    q.cgy = axis_iv(std::max<int64_t>(by0 - cl, 0), std::min<int64_t>(by1 + cl, n1), g->minY, g->cellLength);
  } else {
    q.cgx = q.cgy = {nan, nan};
  }
  if (gl > 0) {
    q.gx = axis_iv(std::max<int64_t>(bx0 - gl, 0), std::min<int64_t>(bx1 + gl, n1), g->minX, g->cellLength);
    q.gy = axis_iv(std::max<int64_t>(by0 - gl, 0), std::min<int64_t>(by1 + gl, n1), g->minY, g->cellLength);
  } else if (gl == 0) {  // the bbox cells themselves, without validKey
    q.gx = axis_iv(bx0, bx1, g->minX, g->cellLength);
    q.gy = axis_iv(by0, by1, g->minY, g->cellLength);
  } else {
    q.gx = q.gy = {nan, nan};
  }
  q.g_any = (gl >= 0) && !std::isnan(q.gx.lo) && !std::isnan(q.gy.lo);
  P->qr = q;
}

// PointPolygonKNNQuery.run(stream, queryPolygon, r, k) -- knn/PointPolygonKNNQuery.java:245-317:
// the C u G cells of the polygon's bbox cells (UniformGrid.java:193-206,399-411) as one rect
// pair (valid cells within c of the bbox rect; for g == 0 the bbox cells themselves, no
// validKey), the polygon on the device for the exact JTS distance.
extern "C" int gf_knn_ppoly_plan_create(gf_ctx* ctx, const gf_grid* g, const gf_polygons* poly, double r,
                                        int32_t k, int approximate, int metric, gf_knn_plan** out) {
  if (!ctx || !out || !grid_ok(g) || !poly || poly->npoly != 1 || k < 1 || k > kMaxKLarge || (metric != 0 && metric != 1))
    return set_err(ctx, GF_ERR_ARG, "gf_knn_ppoly_plan_create: bad argument (one polygon, 1 <= k <= 2^24)");
  *out = nullptr;
  const int32_t nrings = poly->ring_off[1] - poly->ring_off[0];
  if (poly->ring_off[0] != 0 || nrings < 1) return set_err(ctx, GF_ERR_ARG, "polygon without a shell");
  for (int32_t j = 0; j < nrings; ++j) {
    const int32_t v0 = poly->vert_off[j], v1 = poly->vert_off[j + 1];
    if (v1 - v0 < 4 || poly->vx[v0] != poly->vx[v1 - 1] || poly->vy[v0] != poly->vy[v1 - 1])
      return set_err(ctx, GF_ERR_ARG, "ring must be closed with >= 4 vertices");
  }
  int st = gf_knn_pp_plan_create(ctx, g, 0.0, 0.0, r, k, metric, out);
  if (st) return st;
  gf_knn_plan* P = *out;
  *out = nullptr;
  P->poly = 1;
  P->approx = approximate != 0;
  std::vector<double> renv(4 * (size_t)nrings);
  for (int32_t j = 0; j < nrings; ++j) {
    const int32_t v0 = poly->vert_off[j], v1 = poly->vert_off[j + 1];
    double mnx = poly->vx[v0], mxx = mnx, mny = poly->vy[v0], mxy = mny;
    for (int32_t v = v0 + 1; v < v1; ++v) {
      mnx = std::min(mnx, poly->vx[v]); mxx = std::max(mxx, poly->vx[v]);
      mny = std::min(mny, poly->vy[v]); mxy = std::max(mxy, poly->vy[v]);
    }
    renv[4 * j] = mnx; renv[4 * j + 1] = mxx; renv[4 * j + 2] = mny; renv[4 * j + 3] = mxy;
  }
  P->bbox[0] = renv[0]; P->bbox[1] = renv[2]; P->bbox[2] = renv[1]; P->bbox[3] = renv[3];  // shell envelope
  bbox_query_rect(P, g, r);
  const int32_t nverts = poly->vert_off[nrings];
  std::vector<int32_t> ro = {0, nrings}, vo(poly->vert_off, poly->vert_off + nrings + 1);
  std::vector<double> vx(poly->vx, poly->vx + nverts), vy(poly->vy, poly->vy + nverts);
  if ((st = upload(ctx, &P->ring_off, ro)) || (st = upload(ctx, &P->vert_off, vo)) || (st = upload(ctx, &P->vx, vx)) ||
      (st = upload(ctx, &P->vy, vy)) || (st = upload(ctx, &P->ring_env, renv))) {
    gf_knn_plan_destroy(P);
    return st;
  }
  *out = P;
  return GF_OK;
}

// PointLineStringKNNQuery.run(stream, queryLineString, r, k) -- knn/PointLineStringKNNQuery.java
// windowBased: the polygon query with the geometry renamed (C u G of the line's bbox cells, the bbox
// distance when approximate) and the open-chain distance (DistanceFunctions.java:38-42) when exact.
// poly == 2; the plan's ring fields carry the chain's runs of kChainRun segments and their envelopes.
extern "C" int gf_knn_pls_plan_create(gf_ctx* ctx, const gf_grid* g, const gf_linestrings* lines, double r,
                                      int32_t k, int approximate, int metric, gf_knn_plan** out) {
  if (!ctx || !out || !grid_ok(g) || !chain_valid(lines) || lines->nline != 1 || k < 1 || k > kMaxKLarge ||
      (metric != 0 && metric != 1))
    return set_err(ctx, GF_ERR_ARG, "gf_knn_pls_plan_create: bad argument (one line of >= 2 vertices, 1 <= k <= 2^24)");
  *out = nullptr;
  int st = gf_knn_pp_plan_create(ctx, g, 0.0, 0.0, r, k, metric, out);
  if (st) return st;
  gf_knn_plan* P = *out;
  *out = nullptr;
  P->poly = 2;
  P->approx = approximate != 0;
  ChainTables T;
  chain_build(*lines, kChainRun, T);
  for (int i = 0; i < 4; ++i) P->bbox[i] = T.bbox[i];
  bbox_query_rect(P, g, r);
  if ((st = upload(ctx, &P->ring_off, T.run_off)) || (st = upload(ctx, &P->vert_off, T.vert_off)) ||
      (st = upload(ctx, &P->vx, T.vx)) || (st = upload(ctx, &P->vy, T.vy)) || (st = upload(ctx, &P->ring_env, T.run_env))) {
    gf_knn_plan_destroy(P);
    return st;
  }
  *out = P;
  return GF_OK;
}

extern "C" int gf_knn_plan_set_chain_mode(gf_knn_plan* P, int mode) {
  if (!P || P->poly != 2 || (mode != 0 && mode != 1)) return GF_ERR_ARG;
  P->chain_mode = mode;
  return GF_OK;
}

extern "C" int gf_knn_plan_set_capacity(gf_knn_plan* P, int64_t cap) {
  if (!P || cap < 2 || cap > (int64_t)1 << 31) return GF_ERR_ARG;
  int st = bind(P->ctx);
  if (st) return st;
  int fs = gf_knn_plan_flush(P);
  if (fs) return fs;
  hipStreamSynchronize(P->ctx->stream);
  return knn_alloc_candidates(P, cap & ~(int64_t)1);
}

extern "C" int gf_knn_plan_set_tuning(gf_knn_plan* P, int32_t scan_blocks, int32_t unroll, int32_t nontemporal) {
  if (!P || scan_blocks < 0 || unroll < 1 || unroll > 8) return GF_ERR_ARG;
  P->scan_blocks = scan_blocks;
  P->scan_unroll = unroll;
  P->scan_nt = nontemporal != 0;
  return GF_OK;
}

extern "C" int gf_knn_plan_set_index_base(gf_knn_plan* P, int64_t base) {
  if (!P || base < 0) return GF_ERR_ARG;
  P->idx_base = base;
  return GF_OK;
}

// streams a plan's windows run on: S = depth - 1 once pipelined (depth 2: the context stream alone)
static int knn_streams(const gf_knn_plan* P) { return P->pipeline >= 2 ? P->pipeline - 1 : 1; }

// stream s of them: 0 = the context stream, then the extra ones
static hipStream_t knn_stream(gf_ctx* ctx, int s) { return s == 0 ? ctx->stream : (s == 1 ? ctx->aux : ctx->aux2); }

static KnnScanArgs scan_args(gf_knn_plan* P, int j, const gf_points* pts, int64_t begin, int64_t end, int use_state) {
  const gf_knn_plan::Lane& L = P->lane[j];
  KnnScanArgs s{};
  s.x = pts->x; s.y = pts->y; s.objID = pts->objID; s.begin = begin; s.end = end;
  s.qx = P->qx; s.qy = P->qy; s.qr = P->qr;
  s.T = P->r; s.s_pre = s_prefilter(P->r, P->metric);
  s.use_state = use_state; s.metric = P->metric; s.st = L.st;
  s.cand_d = L.cand_d; s.cand_i = L.cand_i; s.cand_o = L.cand_o; s.cap = (unsigned long long)P->cap;
  return s;
}

static KnnSelectArgs select_args(gf_knn_plan* P, int j, int use_state, int write_hint, void* result,
                                 int64_t idx_base) {
  const gf_knn_plan::Lane& L = P->lane[j];
  KnnSelectArgs q{};
  q.st = L.st; q.cand_d = L.cand_d; q.cand_i = L.cand_i; q.cand_o = L.cand_o;
  q.cap = (unsigned long long)P->cap;
  q.use_state = use_state; q.T = P->r; q.r = P->r; q.k = P->k; q.result = result;
  q.write_hint = write_hint; q.idx_base = idx_base;
  return q;
}

static KnnPolyArgs poly_args(gf_knn_plan* P, int j, const gf_points* pts, int64_t begin, int64_t end, int use_state,
                             int use_hint) {
  const gf_knn_plan::Lane& L = P->lane[j];
  KnnPolyArgs a{};
  a.x = pts->x; a.y = pts->y; a.objID = pts->objID; a.begin = begin; a.end = end;
  a.qr = P->qr;
  a.poly = PolyView{P->ring_off, P->vert_off, P->vx, P->vy, P->ring_env, P->metric};
  if (P->poly == 2 && P->chain_mode == 1) a.poly.ring_off = nullptr;  // linestring, mode 1: the plain segment loop
  for (int i = 0; i < 4; ++i) a.bbox[i] = P->bbox[i];
  a.approx = P->approx; a.r = P->r; a.k = P->k; a.use_state = use_state; a.use_hint = use_hint;
  a.st = L.st; a.cand_d = L.cand_d; a.cand_i = L.cand_i; a.cand_o = L.cand_o; a.cap = (unsigned long long)P->cap;
  // One survivor buffer per stream: on every path lane j runs on stream j % S (the window with
  // sequence number q uses lane q % 2S, or q % S unfused, on stream q % S; depth 1 and the sorted
  // path use lane 0 on the context stream).  Lanes of one stream may share it -- at depth 2 both
  // do -- because a window's scan, its refine and the next window's scan are stream-ordered: the
  // buffer is consumed before it is written again, and its fill count st->maybe is per lane.
  a.maybe_i = P->maybe_i[j % knn_streams(P)];
  return a;
}

// the polygon scan's prefilter-survivor buffers (cap entries per stream)
static int poly_buffers(gf_knn_plan* P) {
  if (P->maybe_cap >= P->cap) return GF_OK;
  GF_HIP_CHECK(P->ctx, hipStreamSynchronize(P->ctx->stream));
  if (int e = sync_aux(P->ctx)) return e;
  for (auto& m : P->maybe_i) {
    if (m) hipFree(m);
    m = nullptr;
    GF_HIP_CHECK(P->ctx, hipMalloc(&m, sizeof(uint32_t) * (size_t)P->cap));
  }
  P->maybe_cap = P->cap;
  return GF_OK;
}

// ---------------------------------------------------------------------------------------
// Point / polygon dispatch: the launches of one window on lane j, on the current ctx->stream.
// Only these (and plan creation / destruction) look at P->poly.
// ---------------------------------------------------------------------------------------
// grid of a scan over n points: 4 blocks per CU at most (re-measured best for the x-first loop at
// 2 tiles per iteration); the polygon prefilter runs on half the blocks a point scan of n would
static int scan_blocks_for(gf_knn_plan* P, int64_t n) {
  if (P->scan_blocks > 0) return P->scan_blocks;
  const int64_t pairs = ((P->poly ? (n + 1) / 2 : n) + 1) / 2;
  return std::min(stream_blocks(P->ctx, pairs), P->ctx->num_cus * 4);
}

// the window's threshold into the lane's state: its hint (use_hint, when it has one) or a sample
static int launch_sample(gf_knn_plan* P, int j, const gf_points* pts, int use_hint) {
  if (P->poly) {
    GF_HIP_CHECK(P->ctx, launch_knn_poly_sample(P->ctx, poly_args(P, j, pts, 0, pts->n, 1, use_hint), P->poly == 2));
    return GF_OK;
  }
  KnnSampleArgs s{};
  s.x = pts->x; s.y = pts->y; s.n = pts->n; s.qx = P->qx; s.qy = P->qy; s.qr = P->qr;
  s.r = P->r; s.s_r = s_prefilter(P->r, P->metric); s.k = P->k; s.metric = P->metric; s.st = P->lane[j].st;
  s.use_hint = use_hint;
  GF_HIP_CHECK(P->ctx, launch_knn_sample(P->ctx, s));
  return GF_OK;
}

// candidates of points [begin, end) into the lane (polygon: prefilter scan + refine)
static int launch_scan(gf_knn_plan* P, int j, const gf_points* pts, int64_t begin, int64_t end, int use_state) {
  gf_ctx* ctx = P->ctx;
  const int blocks = scan_blocks_for(P, end - begin);
  if (P->poly) {
    if (int st = poly_buffers(P)) return st;
    GF_HIP_CHECK(ctx, launch_knn_poly_scan(ctx, poly_args(P, j, pts, begin, end, use_state, 0), blocks, P->poly == 2));
  } else {
    GF_HIP_CHECK(ctx, launch_knn_scan(ctx, scan_args(P, j, pts, begin, end, use_state), blocks, P->scan_unroll,
                                      P->scan_nt));
  }
  return GF_OK;
}

// the fused launch: the window's scan on lane j (use_state 2: the sample just taken, 1: the
// lane's hint) and, in block 0, the select `prev` (has_prev) and the window merge (nullable);
// polygon: the fused launch is the prefilter scan, the window's refine follows
static int launch_fused(gf_knn_plan* P, int j, const gf_points* pts, int use_state, const KnnSelectArgs& prev,
                        int has_prev, const KnnMergeArgs* merge) {
  gf_ctx* ctx = P->ctx;
  const int blocks = scan_blocks_for(P, pts->n);
  if (P->poly) {
    if (int st = poly_buffers(P)) return st;
    GF_HIP_CHECK(ctx, launch_knn_poly_fused(ctx, poly_args(P, j, pts, 0, pts->n, use_state, 0), prev, has_prev, blocks,
                                           merge, P->poly == 2));
  } else {
    GF_HIP_CHECK(ctx, launch_knn_fused(ctx, scan_args(P, j, pts, 0, pts->n, use_state), prev, has_prev, blocks,
                                       P->scan_unroll, P->scan_nt, merge));
  }
  return GF_OK;
}

// a flagged window's first retry is the sample path with the hint ignored -- point queries only; a
// polygon window goes straight to the exact sorted path
static bool fallback_resamples(const gf_knn_plan* P) { return !P->poly; }

// scan + select of points [begin, end) on lane j, stream-ordered
static int knn_scan_select(gf_knn_plan* P, int j, const gf_points* pts, int64_t begin, int64_t end, int use_state,
                           int write_hint, void* result) {
  if (int st = launch_scan(P, j, pts, begin, end, use_state)) return st;
  GF_HIP_CHECK(P->ctx, launch_knn_select(P->ctx, select_args(P, j, use_state, write_hint, result, P->idx_base)));
  return GF_OK;
}

// k > kMaxK (KNNQuery.java:216 takes any k): every candidate within r (T = r; lane 0's buffers
// hold the whole window, so nothing overflows), then two stable LSD radix sorts of the candidate
// permutation over 32-bit key fields (the K2 bucketing passes): (objID, d, idx) -> the first
// entry of each objID -> those by (d, objID, idx) -> the first k.  Grids and scratch are sized
// by the window (an upper bound of the candidate count) and every kernel reads the counts on
// the device: no host read, so windows queue back to back like the pipelined paths'.
static int knn_large(gf_knn_plan* P, const gf_points* pts, void* result) {
  int st;
  const int64_t n = pts->n;
  if (P->cap < n && (st = knn_alloc_candidates(P, n))) return st;
  if ((st = launch_scan(P, 0, pts, 0, n, 0))) return st;  // T = r
  const gf_knn_plan::Lane& L = P->lane[0];
  return knn_sorted_record(P->ctx, L.cand_d, L.cand_o, L.cand_i, &L.st->count, &L.st->maybe, n, P->k, P->r, P->idx_base,
                           result);
}

int gf::knn_sorted_record(gf_ctx* ctx, const double* cd, const int64_t* co, const uint32_t* ci, unsigned long long* count,
                          unsigned long long* maybe, int64_t m_items, int32_t k, double T, int64_t idx_base,
                          void* result) {
  int st;
  const int64_t mm = std::max<int64_t>(m_items, 1);
  const int nb = radix_blocks(ctx, mm);
  const int64_t mat = (int64_t)256 * nb;  // 8-bit digits
  Arena ar;
  uint32_t *keys[2], *perm[2], *cnt, *m, *ms;
  ar.take(keys[0], mm); ar.take(keys[1], mm);
  ar.take(perm[0], mm); ar.take(perm[1], mm);
  ar.take(cnt, 2); ar.take(m, mat); ar.take(ms, mat + 1);
  if ((st = ar.alloc(ctx))) return st;
  KnnLargeArgs a{};
  a.cd = cd; a.co = co; a.ci = ci; a.k = k; a.T = T; a.idx_base = idx_base;
  a.result = result; a.m = mm; a.cnt = cnt;
  a.lane_count = count; a.lane_maybe = maybe;
  GF_HIP_CHECK(ctx, launch_knn_large(ctx, 5, a));                 // counts
  int cur = 0;  // the permutation lives in perm[cur]
  // stable sort of the first cnt[pass] entries of the permutation by key fields (least
  // significant first)
  auto sort_by = [&](int pass, std::initializer_list<int> fields) -> int {
    for (int f : fields) {
      a.perm = perm[cur]; a.field = f; a.keys = keys[0]; a.pass = pass;
      GF_HIP_CHECK(ctx, launch_knn_large(ctx, 1, a));
      for (int p = 0; p < 4; ++p) {  // 32 bits = 4 passes of 8
        RadixArgs r{};
        r.tile = radix_tile();
        r.n = mm; r.n_dev = a.cnt + pass;
        r.kin = keys[p & 1]; r.vin = perm[cur];
        r.kout = keys[(p + 1) & 1]; r.vout = perm[cur ^ 1];
        r.shift = p * 8; r.bits = 8; r.nblk = nb; r.M = m; r.Ms = ms;
        GF_HIP_CHECK(ctx, launch_radix(ctx, 0, r, nb));
        if (int e = scan1(ctx, m, mat, ms)) return e;
        GF_HIP_CHECK(ctx, launch_radix(ctx, 1, r, nb));
        cur ^= 1;
      }
    }
    return GF_OK;
  };
  a.perm = perm[cur];
  GF_HIP_CHECK(ctx, launch_knn_large(ctx, 0, a));                 // identity permutation
  if ((st = sort_by(0, {0, 1, 2, 3, 4}))) return st;               // (objID, d, idx)
  a.perm = perm[cur]; a.out = perm[cur ^ 1];
  GF_HIP_CHECK(ctx, launch_knn_large(ctx, 2, a));                 // first of each objID -> cnt[1]
  cur ^= 1;
  if ((st = sort_by(1, {0, 3, 4, 1, 2}))) return st;               // (d, objID, idx)
  a.perm = perm[cur];
  GF_HIP_CHECK(ctx, launch_knn_large(ctx, 4, a));
  return GF_OK;
}

extern "C" int gf_knn_enqueue(gf_knn_plan* P, const gf_points* pts, void* result) {
  int merged = 0;
  return gf::knn_enqueue_merge(P, pts, result, nullptr, &merged);
}

int gf::knn_enqueue_merge(gf_knn_plan* P, const gf_points* pts, void* result, const KnnMergeArgs* merge,
                          int* merged) {
  *merged = 0;
  if (!P || !result) return GF_ERR_ARG;
  gf_ctx* ctx = P->ctx;
  int st = bind(ctx);
  if (st) return st;
  if ((st = check_points(ctx, pts))) return st;
  if (pts->n > 0 && !pts->objID) return set_err(ctx, GF_ERR_ARG, "kNN needs objID");
  // k > kMaxK: the sorted path queues without host reads at every depth (its record is complete
  // in stream order, earlier than a pipelined plan promises)
  if (P->large) return knn_large(P, pts, result);
  if (P->pipeline == 1) {
    // threshold: the previous window's hint (continuous query) or the sample; tiny windows
    // scan to r
    const bool staged = pts->n >= kSampleMinN;
    if (staged && (st = launch_sample(P, 0, pts, P->use_hint))) return st;
    return knn_scan_select(P, 0, pts, 0, pts->n, staged ? 1 : 0, staged && P->use_hint, result);
  }
  // Depth d >= 2, S = d - 1 streams (depth 2: the context stream alone).  The window with
  // sequence number q runs on stream q % S; window buffers must be complete when enqueued (no
  // cross-stream wait is inserted).
  const uint64_t S = (uint64_t)knn_streams(P), q = P->seq++;
  StreamScope on(ctx, knn_stream(ctx, (int)(q % S)));
  if (P->k > kFusedSelectMaxK) {
    // k in (256, 512]: the select needs the standalone kernel's sort area, so it is not fused;
    // each window runs [sample] + scan + select on lane q % S, complete in stream order (earlier
    // than the depth promises).  A lane's hint chain stays on one stream and, at S > 1,
    // consecutive windows' kernels overlap.
    const int j = (int)(q % S);
    const bool staged = pts->n >= kSampleMinN;  // the sample kernel takes the lane's hint when it has one
    if (staged && (st = launch_sample(P, j, pts, P->use_hint))) return st;
    return knn_scan_select(P, j, pts, 0, pts->n, staged ? 1 : 0, staged && P->use_hint, result);
  }
  // One fused launch per window: it scans lane q % 2S (threshold = the lane's hint) and selects
  // window q - S -- the previous launch on the SAME stream -- in block 0; this window's select
  // rides the launch of window q + S, or the flush.  Every dependency (window q - S's
  // candidates, the lane's last select in launch q - 2S, its hint) stays stream-ordered, while
  // S consecutive windows' launches overlap (one's ramp-up under the other's tail).
  const int j = (int)(q % (2 * S));
  // a lane's first window (or hints off): sample the threshold instead of guessing r
  const bool sample = pts->n >= kSampleMinN && (!P->use_hint || !P->lane_warm[j]);
  if (sample && (st = launch_sample(P, j, pts, 0))) return st;
  P->lane_warm[j] = 1;
  KnnSelectArgs prev{};
  int has_prev = 0;
  if (P->npq > 0 && P->pq[0].seq + S == q) {
    const gf_knn_plan::Pend e = P->pq[0];
    prev = select_args(P, e.lane, 1, P->use_hint, e.result, e.idx_base);
    has_prev = 1;
    std::copy(P->pq + 1, P->pq + P->npq, P->pq);
    --P->npq;
  }
  // the pane engine's window merge rides block 0 too where its select does (depth 2 only)
  const bool fold = S == 1 && merge && merge->nrec > 0 && has_prev && P->k <= kFusedMergeMaxK;
  if ((st = launch_fused(P, j, pts, sample ? 2 : 1, prev, has_prev, fold ? merge : nullptr))) return st;
  *merged = fold ? 1 : 0;
  P->pq[P->npq++] = gf_knn_plan::Pend{j, result, P->idx_base, q};  // the index base in force at this enqueue
  return GF_OK;
}

bool gf::knn_select_pending(const gf_knn_plan* P) { return P->npq > 0; }

extern "C" int gf_knn_plan_flush(gf_knn_plan* P) {
  if (!P) return GF_ERR_ARG;
  gf_ctx* ctx = P->ctx;
  const int S = knn_streams(P);
  // nothing pending: only the unfused mid-range k at S > 1 has put work on the other streams
  if (P->npq == 0) return S > 1 && P->k > kFusedSelectMaxK ? gf_ctx_join(ctx) : GF_OK;
  int st = bind(ctx);
  if (st) return st;
  for (int e = 0; e < P->npq; ++e) {
    const gf_knn_plan::Pend& w = P->pq[e];
    StreamScope on(ctx, knn_stream(ctx, (int)(w.seq % (uint64_t)S)));
    GF_HIP_CHECK(ctx, launch_knn_select(ctx, select_args(P, w.lane, 1, P->use_hint, w.result, w.idx_base)));
  }
  P->npq = 0;
  // every window of the plan is complete in the context stream's order from here on
  return S > 1 ? gf_ctx_join(ctx) : GF_OK;
}

extern "C" int gf_knn_plan_set_pipeline(gf_knn_plan* P, int depth) {
  if (!P || depth < 1 || depth > 4) return GF_ERR_ARG;
  gf_ctx* ctx = P->ctx;
  int st = bind(ctx);
  if (st || (st = gf_knn_plan_flush(P))) return st;
  GF_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  if (int e = sync_aux(ctx)) return e;
  // k > 512 plans return through knn_large (lane 0, stream-ordered) before any pipelined path:
  // no extra lanes, no second stream
  const int lanes = depth >= 2 ? 2 * (depth - 1) : 1;
  for (int j = 1; !P->large && j < lanes; ++j)
    if (!P->lane[j].st && (st = knn_alloc_lane(P, j, P->cap))) return st;
  if (depth >= 3 && !P->large && !ctx->aux)
    GF_HIP_CHECK(ctx, hipStreamCreateWithFlags(&ctx->aux, hipStreamNonBlocking));
  if (depth >= 4 && !P->large && !ctx->aux2)
    GF_HIP_CHECK(ctx, hipStreamCreateWithFlags(&ctx->aux2, hipStreamNonBlocking));
  P->pipeline = depth;
  P->seq = 0;
  for (int& w : P->lane_warm) w = 0;
  return GF_OK;
}

extern "C" int gf_knn_plan_set_hint(gf_knn_plan* P, int enable) {
  if (!P) return GF_ERR_ARG;
  int st = bind(P->ctx);
  if (st) return st;
  P->use_hint = enable != 0;
  if ((st = gf_knn_plan_flush(P))) return st;
  GF_HIP_CHECK(P->ctx, hipStreamSynchronize(P->ctx->stream));
  for (auto& L : P->lane)
    if (L.st) GF_HIP_CHECK(P->ctx, hipMemset(&L.st->hint_T, 0, sizeof(double)));
  for (int& w : P->lane_warm) w = 0;
  return GF_OK;
}

namespace {
struct Ent { double d; int64_t o, i; };
void merge_lists(int32_t k, std::vector<Ent>& all, int64_t* oo, double* od, int64_t* oi, int32_t* n_out) {
  std::sort(all.begin(), all.end(), [](const Ent& a, const Ent& b) {
    if (a.d != b.d) return a.d < b.d;
    if (a.o != b.o) return a.o < b.o;
    return a.i < b.i;
  });
  std::unordered_set<int64_t> seen;
  int32_t n = 0;
  for (const Ent& e : all) {
    if (n >= k) break;
    if (!seen.insert(e.o).second) continue;
    if (oo) oo[n] = e.o;
    if (od) od[n] = e.d;
    if (oi) oi[n] = e.i;
    ++n;
  }
  *n_out = n;
}
}  // namespace

extern "C" int gf_knn_merge_host(int32_t k, int32_t nlists, const int32_t* counts, const int64_t* objID,
                                 const double* dist, const int64_t* idx, int64_t* oo, double* od, int64_t* oi,
                                 int32_t* n_out) {
  if (k < 1 || nlists < 0 || !n_out || (nlists > 0 && (!counts || !objID || !dist))) return GF_ERR_ARG;
  std::vector<Ent> all;
  int64_t off = 0;
  for (int32_t l = 0; l < nlists; ++l)
    for (int32_t j = 0; j < counts[l]; ++j, ++off) all.push_back({dist[off], objID[off], idx ? idx[off] : 0});
  merge_lists(k, all, oo, od, oi, n_out);
  return GF_OK;
}

// Re-evaluation of a flagged window: first the sample path with the hint ignored; if that is
// still inconclusive, the exact sorted path over every candidate within r (knn_large) -- on the
// device, like every other result.
static int knn_fallback(gf_knn_plan* P, const gf_points* pts, int64_t* oo, double* od, int64_t* oi, int32_t* n_out) {
  gf_ctx* ctx = P->ctx;
  const size_t rb = gf_knn_result_bytes(P->k);
  const gf_knn_header* h = (const gf_knn_header*)P->host_result;
  auto fetch = [&]() -> int {
    GF_HIP_CHECK(ctx, hipMemcpyAsync(P->host_result, P->tmp_result, rb, hipMemcpyDeviceToHost, ctx->stream));
    GF_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return GF_OK;
  };
  int st = gf_knn_plan_flush(P);  // lane 0 is free afterwards
  if (st) return st;
  if (fallback_resamples(P) && pts->n >= kSampleMinN) {
    if ((st = launch_sample(P, 0, pts, 0)) ||
        (st = knn_scan_select(P, 0, pts, 0, pts->n, 1, P->use_hint, P->tmp_result)) || (st = fetch()))
      return st;
    if (h->status == 0) return gf_knn_decode(P, pts, P->host_result, oo, od, oi, n_out);
  }
  if ((st = knn_large(P, pts, P->tmp_result)) || (st = fetch())) return st;
  if (h->status != 0) return set_err(ctx, GF_ERR_HIP, "kNN exact path did not converge");
  return gf_knn_decode(P, pts, P->host_result, oo, od, oi, n_out);
}

extern "C" int gf_knn_decode(gf_knn_plan* P, const gf_points* pts, const void* result_host, int64_t* oo,
                             double* od, int64_t* oi, int32_t* n_out) {
  if (!P || !result_host || !n_out) return GF_ERR_ARG;
  const gf_knn_header* h = (const gf_knn_header*)result_host;
  if (h->status == 0) {
    const double* d = (const double*)(h + 1);
    const int64_t* o = (const int64_t*)(d + h->k);
    const int64_t* i = o + h->k;
    for (int32_t j = 0; j < h->n; ++j) {
      if (oo) oo[j] = o[j];
      if (od) od[j] = d[j];
      if (oi) oi[j] = i[j];
    }
    *n_out = h->n;
    return GF_OK;
  }
  int st = bind(P->ctx);
  if (st) return st;
  if ((st = check_points(P->ctx, pts))) return st;
  return knn_fallback(P, pts, oo, od, oi, n_out);
}

extern "C" int gf_knn_run(gf_knn_plan* P, const gf_points* pts, int64_t* oo, double* od, int64_t* oi,
                          int32_t* n_out) {
  if (!P || !n_out) return GF_ERR_ARG;
  gf_ctx* ctx = P->ctx;
  // the synchronous call may get a window the caller produced on the context stream just now:
  // order the second stream after it (nothing to overlap with in a synchronous call)
  int st = P->pipeline >= 3 ? gf_ctx_fork(ctx) : GF_OK;
  if (st) return st;
  st = gf_knn_enqueue(P, pts, P->tmp_result);
  if (st || (st = gf_knn_plan_flush(P))) return st;
  GF_HIP_CHECK(ctx, hipMemcpyAsync(P->host_result, P->tmp_result, gf_knn_result_bytes(P->k), hipMemcpyDeviceToHost,
                                   ctx->stream));
  GF_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  return gf_knn_decode(P, pts, P->host_result, oo, od, oi, n_out);
}

// k > kMaxK merges rank entries in global scratch (the context's, stream-ordered)
static int merge_scratch(gf_ctx* ctx, int32_t k, int32_t nrec, int32_t nwin, void** out) {
  *out = nullptr;
  if (k <= kMaxK) return GF_OK;
  int st = GF_OK;
  *out = ctx_scratch(ctx, merge_any_bytes(nrec, k) * (size_t)nwin, &st);
  return st;
}

extern "C" int gf_knn_merge_dev(gf_ctx* ctx, int32_t k, const void* records, int32_t nrec, void* result) {
  if (!ctx || k < 1 || k > kMaxKLarge || nrec < 1 || nrec > 64 || !records || !result)
    return set_err(ctx, GF_ERR_ARG, "gf_knn_merge_dev: need 1 <= nrec <= 64 and 1 <= k <= 2^24");
  int st = bind(ctx);
  if (st) return st;
  const size_t rb = gf_knn_result_bytes(k);
  void* scratch;
  if ((st = merge_scratch(ctx, k, nrec, 1, &scratch))) return st;
  GF_HIP_CHECK(ctx, launch_knn_merge(ctx, k, records, nrec, rb, 1, 0, result, 0, 0, scratch));
  return GF_OK;
}

extern "C" int gf_knn_merge_dev_batch(gf_ctx* ctx, int32_t k, const void* records, int32_t nrec, int32_t nwin,
                                      int32_t layout, void* results) {
  const int foreign = (layout & GF_MERGE_FOREIGN_KEYS) != 0;
  layout &= ~GF_MERGE_FOREIGN_KEYS;
  if (!ctx || k < 1 || k > kMaxKLarge || nrec < 1 || nrec > 64 || nwin < 1 || nwin > 65535 || !records || !results ||
      (layout != GF_MERGE_SHARD_MAJOR && layout != GF_MERGE_WINDOW_MAJOR))
    return set_err(ctx, GF_ERR_ARG, "gf_knn_merge_dev_batch: bad argument");
  int st = bind(ctx);
  if (st) return st;
  const size_t rb = gf_knn_result_bytes(k);
  // shard-major = all_gather of each rank's [nwin] records: record (shard s, window w) at (s*nwin + w)*rb
  const size_t rec_stride = layout == GF_MERGE_SHARD_MAJOR ? (size_t)nwin * rb : rb;
  const size_t win_stride = layout == GF_MERGE_SHARD_MAJOR ? rb : (size_t)nrec * rb;
  void* scratch;
  if ((st = merge_scratch(ctx, k, nrec, nwin, &scratch))) return st;
  GF_HIP_CHECK(ctx, launch_knn_merge(ctx, k, records, nrec, rec_stride, nwin, win_stride, results, rb, foreign,
                                     scratch));
  return GF_OK;
}

// the exact record of one window (any k, status 0), stream-ordered on the context stream
int gf::knn_exact_record(gf_knn_plan* P, const gf_points* pts, void* result) {
  int st = gf_knn_plan_flush(P);  // lane 0 is free afterwards
  if (st) return st;
  return knn_large(P, pts, result);
}
