// join.cpp -- the point-point join driver (k_join.hip): one call's path choice and sizing, its
// scratch layout, and the two launch sequences -- the row-bucketed probes (row, band, streaming
// experiment) with their fix-up, and the cell-probe fallback.
#define GF_TU_NAME join_cpp
#include "gf_buildtag.hpp"  // first: records this unit's command-line defines

#include <hip/hip_runtime.h>

#include <cstdlib>

#include "gf_host.hpp"

using namespace gf;

namespace {

// one gf_join_pp / gf_join_pp_async call
struct JoinCall {
  gf_ctx* ctx;
  const gf_grid *ugrid, *qgrid;
  const gf_points *ord, *qry;
  double r;
  int approximate, metric;
  uint32_t* pairs;
  int64_t cap;
  int64_t* npairs;
  // nullptr: synchronous (*npairs from a pinned readback); else asynchronous (the packing kernel
  // writes the count to total_out; *npairs untouched)
  unsigned long long* total_out;
};

// which probe runs, and the grids, chunks, regions and spill it runs with
struct JoinSizing {
  int64_t c;           // candidate layers (-1: every grid cell)
  bool rowpath;        // the row-bucketed path (else the cell-probe fallback)
  int32_t f;           // fine factor (> 1: the fine path)
  bool stream, band;   // fine path: the streaming experiment / the band probe (neither: the row probe)
  int blocks;          // cell-probe grid
  int qblk, sblocks;   // bucketing grids of the query / ordinary side
  int64_t bins, fbins; // query cells with the border / q_off entries (sub-cells on the fine path)
  int64_t qmat, mat;   // row histogram matrices of the query / ordinary side
  int64_t probe_blocks, nwaves, chunk;
  double ppp, t_hint;  // pairs per ordinary point of the last join, and the pair count it predicts
  uint64_t e_lim, spill_cap;
};

JoinSizing join_sizing(const JoinCall& k, int64_t c) {
  gf_ctx* ctx = k.ctx;
  const gf_grid *ugrid = k.ugrid, *qgrid = k.qgrid;
  const int64_t no = k.ord->n, nq = k.qry->n;
  const int64_t qn = qgrid->n, W = qn + 2;
  JoinSizing z{};
  z.c = c;
  z.bins = W * W;
  z.blocks = (int)std::min<int64_t>(std::max<int64_t>((no + kBlock - 1) / kBlock, 1), (int64_t)ctx->num_cus * 8);
  // row-bucketed path (k_join.hip): bucket the ordinary side by cell row, probe per task
  // (pairs carry u32 sorted slots or query indices with the top bit as a flag: nq < 2^31)
  z.rowpath = c >= 0 && 2 * c + 1 <= kJoinMaxRows && qn + 8 <= 8192 && nq < ((int64_t)1 << 31) && !ctx->join_legacy;
  // fine path (k_join.hip): c == 1, exact distances, one grid for both sides
  z.f = 1;
  if (z.rowpath && c == 1 && !k.approximate && !ctx->join_coarse && ugrid->n == qgrid->n &&
      ugrid->minX == qgrid->minX && ugrid->minY == qgrid->minY && ugrid->cellLength == qgrid->cellLength) {
    const double ext = (double)qn * qgrid->cellLength;
    const double maxabs = std::max({std::fabs(qgrid->minX), std::fabs(qgrid->minY), std::fabs(qgrid->minX + ext),
                                    std::fabs(qgrid->minY + ext)});
    z.f = join_fine_factor(qgrid->cellLength, k.r, (int32_t)qn, maxabs);
  }
  z.fbins = (int64_t)z.f * W * z.f * W;
  // bucketing grids: one block per CU in the scatter (its tile buffers fill the LDS), split
  // between the sides by their point counts
  z.qblk = (int)std::max<int64_t>(1, std::min<int64_t>(nq / 8192 + 1, (int64_t)ctx->num_cus * nq / (no + nq)));
  z.sblocks = (int)std::max<int64_t>(1, std::min<int64_t>(no / 8192 + 1, (int64_t)ctx->num_cus - z.qblk));
  // experiment: only the query side bucketed, the ordinary points streamed (fine path)
  z.stream = z.rowpath && z.f > 1 && ctx->join_stream;
  z.qmat = z.rowpath ? W * 2 * z.qblk : 1;  // kHistSplit = 2
  z.mat = z.rowpath && !z.stream ? qn * 2 * z.sblocks : 1;  // (qn ordinary-side rows)
  // output (JoinOut): the persistent probe's waves, one chunk each at a time, sized from the last
  // join's pairs per point so that a window takes ~8 chunks per wave: few atomics, small holes
  // (GF_JOIN_BAND_PER_CU, A/B testing only: band probe blocks per CU -- the product's 160 KB
  // block fills a CU's LDS; an experiment build with an 80 KB block can hold two)
  const char* pcu = std::getenv("GF_JOIN_BAND_PER_CU");
  const int64_t per_cu = pcu && *pcu >= '1' && *pcu <= '4' ? *pcu - '0' : 1;
  z.probe_blocks = std::max(8, ctx->num_cus / 8 * 8) * per_cu;
  z.nwaves = z.probe_blocks * (kJoinThreads / 64);
  // pairs per point of the last join: its exact count (sync) or the fix-up's pinned copy (async)
  z.ppp = ctx->join_ppp > 0 ? ctx->join_ppp : 1.0;
  if (ctx->join_hint && ctx->join_hint_no > 0) {
    const unsigned long long h = *(volatile unsigned long long*)ctx->join_hint;
    if (h > 0) z.ppp = (double)h / (double)ctx->join_hint_no;
  }
  // output: the band probe fills per-block regions (JoinOut.regions); the row probe and the
  // streaming experiment take per-wave chunks (one device atomic each, one hole per wave).
  // fine path: the band probe (k_join.hip) unless the row probe is asked for (A/B testing)
  const char* renv = std::getenv("GF_JOIN_ROWPROBE");
  z.band = z.rowpath && z.f > 1 && !z.stream && !(renv && *renv == '1') && z.probe_blocks <= 1016;
  z.chunk = 256;
  while (z.chunk < 65536 && (double)z.chunk * z.nwaves * 8 < z.ppp * (double)no)
    z.chunk <<= 1;
  if (const char* e = std::getenv("GF_JOIN_CHUNK")) {  // testing / tuning: a fixed chunk (power of 2)
    const int64_t v = std::atoll(e);
    if (v >= 64 && v <= 65536 && (v & (v - 1)) == 0) z.chunk = v;
  }
  // band probe regions: e_lim bounds the regions' total E (hint x 1.125 + 1024 per block; the
  // regions come from the last call's per-block pairs x 1.03 + 256, so they are scaled down only
  // when the history and the hint disagree).  Positions used = E + the overflow area, and the
  // overflow (pairs past their block's region) is at most the pair count T, so every position is
  // below E + T <= e_lim + cap whenever T <= cap: a spill of e_lim past cap backs them all, and a
  // window whose pairs fit is never answered GF_ERR_CAPACITY, whatever the regions' sizing
  // (VERDICT r04 item 6).  The spill is scratch written only by overflowing blocks (HBM capacity,
  // not traffic); r06: e_lim no longer takes max(cap, ...), which made every call reserve a
  // second cap-sized buffer.
  z.t_hint = z.ppp * (double)no;
  const uint64_t ucap = k.pairs ? (uint64_t)std::max<int64_t>(k.cap, 0) : 0;
  z.e_lim = (uint64_t)(1.125 * z.t_hint) + (uint64_t)z.probe_blocks * 1024;
  z.spill_cap = z.band ? (ucap == 0 ? 0 : z.e_lim + std::max<uint64_t>(65536, (uint64_t)(z.t_hint / 16)))
                       : (uint64_t)(z.nwaves * z.chunk);
  return z;
}

// the call's buffers in the context's scratch
struct JoinScratch {
  uint32_t* keys; int32_t *qcx, *qcy;              // cell probe: query keys and cells
  uint32_t *hist, *off, *cur, *tmp;                // query cell histogram, offsets (q_off), cursors, scan scratch
  double *sqx, *sqy; int32_t *sqcx, *sqcy; uint32_t* sqi;  // the query side sorted by (sub-)cell
  uint32_t *cnt, *boff;                            // cell probe: pairs per block and their offsets
  uint32_t *cat, *cats;                            // row histograms of both sides (query first) and their scan
  double* txy; uint32_t* tidx;                     // query side scattered by row
  uint32_t *roff, *toff;                           // ordinary row / task offsets
  unsigned long long* gcnt;                        // -, total
  uint64_t* spill;
  uint64_t *bcnt, *bsl;                            // band probe: per-block counts / slices
  uint64_t* tb; uint32_t* tf;                      // tails: base and fill
  uint64_t *hs, *hp, *ss, *sp; uint32_t* fc;       // fix-up: holes, segments, counts
  double* soxy; uint32_t* soidx;                   // ordinary side scattered by row
};

void join_layout(const JoinCall& k, const JoinSizing& z, Arena& ar, JoinScratch& L) {
  const int64_t no = k.ord->n, nq = k.qry->n, nrows = k.qgrid->n;  // ordinary-side rows
  const int64_t cells = std::max(z.bins, z.fbins);
  ar.take(L.keys, nq); ar.take(L.qcx, nq); ar.take(L.qcy, nq);
  ar.take(L.hist, z.bins); ar.take(L.off, cells + 1); ar.take(L.cur, cells);
  ar.take(L.tmp, std::max(scan_tmp_elems(z.bins), scan_tmp_elems(z.blocks)));
  ar.take(L.sqx, nq); ar.take(L.sqy, nq);
  ar.take(L.sqcx, nq); ar.take(L.sqcy, nq); ar.take(L.sqi, nq);
  ar.take(L.cnt, z.blocks); ar.take(L.boff, z.blocks + 1);
  ar.take(L.cat, z.qmat + z.mat); ar.take(L.cats, z.qmat + z.mat + 1);
  ar.take(L.txy, z.rowpath ? 2 * nq : 1); ar.take(L.tidx, z.rowpath ? nq : 1);
  ar.take(L.roff, nrows + 1); ar.take(L.toff, nrows + 1);
  ar.take(L.gcnt, 2);
  ar.take(L.spill, z.rowpath ? std::max<uint64_t>(z.spill_cap, 1) : 1);
  ar.take(L.bcnt, z.probe_blocks); ar.take(L.bsl, z.probe_blocks);
  ar.take(L.tb, z.nwaves); ar.take(L.tf, z.nwaves);
  ar.take(L.hs, z.nwaves + 1); ar.take(L.hp, z.nwaves + 2);
  ar.take(L.ss, z.nwaves + 2); ar.take(L.sp, z.nwaves + 3); ar.take(L.fc, 2);
  ar.take(L.soxy, z.rowpath ? 2 * no : 1); ar.take(L.soidx, z.rowpath ? no : 1);
}

// the row-bucketed path: both sides bucketed by row, the row / band / streaming probe, the fix-up
int join_rows_path(const JoinCall& k, const JoinSizing& z, const JoinScratch& L) {
  gf_ctx* ctx = k.ctx;
  const gf_grid *ugrid = k.ugrid, *qgrid = k.qgrid;
  const int64_t no = k.ord->n, nq = k.qry->n, qn = qgrid->n;
  hipStream_t s = ctx->stream;
  int st;
  if (!ctx->join_gctr) {  // the output counter (the fix-up resets it) and the size hint
    GF_HIP_CHECK(ctx, hipMalloc(&ctx->join_gctr, sizeof(unsigned long long)));
    GF_HIP_CHECK(ctx, hipMemset(ctx->join_gctr, 0, sizeof(unsigned long long)));
    void* h = nullptr;
    if (gf_pinned_alloc(sizeof(unsigned long long), &h) == GF_OK) {
      ctx->join_hint = (unsigned long long*)h;
      *ctx->join_hint = 0ull;
    }
  }
  ctx->join_hint_no = no;
  JoinQueryArgs q{};
  q.qx = k.qry->x; q.qy = k.qry->y; q.nq = nq;
  q.minX = qgrid->minX; q.minY = qgrid->minY; q.cl = qgrid->cellLength; q.qn = (int32_t)qn;
  q.nblk = z.qblk; q.qmat = L.cat; q.qmat_scan = L.cats;
  q.txy = L.txy; q.tidx = L.tidx; q.q_off = L.off;
  q.sqx = L.sqx; q.sqy = L.sqy; q.sqcx = L.sqcx; q.sqcy = L.sqcy; q.sqidx = L.sqi;
  q.f = z.f; q.fs = (double)z.f / qgrid->cellLength;
  JoinRowArgs j{};
  j.ox = k.ord->x; j.oy = k.ord->y; j.no = no;
  j.u_minX = ugrid->minX; j.u_minY = ugrid->minY; j.u_cl = ugrid->cellLength;
  j.qn = (int32_t)qn; j.c = z.c; j.q_off = L.off;
  j.sqx = L.sqx; j.sqy = L.sqy; j.sqcx = L.sqcx; j.sqcy = L.sqcy; j.sqidx = L.sqi;
  j.approx = k.approximate != 0; j.metric = k.metric; j.r = k.r; j.s_r = s_prefilter(k.r, 0);
  j.nblk = z.stream ? 0 : z.sblocks; j.nrows = z.stream ? 0 : (int32_t)qn;
  j.row_mat = L.cat + z.qmat; j.row_mat_scan = L.cats + z.qmat; j.mat_base = (uint32_t)nq;
  j.row_off_w = L.roff; j.row_off = L.roff; j.task_off_w = L.toff; j.task_off = L.toff;
  j.soxy = L.soxy; j.soidx = L.soidx;
  JoinOut& o = j.out;
  o.pairs = k.pairs;
  o.cap = k.pairs ? (uint64_t)std::max<int64_t>(k.cap, 0) : 0;
  o.aligned = ((uintptr_t)k.pairs & 7) == 0;
  o.chunk = (uint32_t)z.chunk;
  o.spill = (uint2*)L.spill;
  o.spill_cap = z.spill_cap;
  if (z.band) {
    if (!ctx->join_hist) {  // zero: no history (the first call's regions come from ppp)
      GF_HIP_CHECK(ctx, hipMalloc(&ctx->join_hist, sizeof(uint64_t) * (3 * (size_t)z.probe_blocks + 1)));
      GF_HIP_CHECK(ctx, hipMemsetAsync(ctx->join_hist, 0, sizeof(uint64_t) * (3 * (size_t)z.probe_blocks + 1), s));
      GF_HIP_CHECK(ctx, hipMalloc(&ctx->join_ovf, 2 * sizeof(unsigned long long)));  // overflow, ticket
      GF_HIP_CHECK(ctx, hipMemsetAsync(ctx->join_ovf, 0, 2 * sizeof(unsigned long long), s));
    }
    o.regions = 1;
    o.bcount = L.bcnt;
    o.bslice = L.bsl;
    o.hist = ctx->join_hist;
    o.ovf = ctx->join_ovf;
    o.e_lim = z.e_lim;
    o.ppp = z.ppp;
  }
  o.gctr = ctx->join_gctr;
  o.tail_base = L.tb;
  o.tail_fill = L.tf;
  o.nwaves = (uint32_t)(z.band ? z.probe_blocks : z.nwaves);  // tails: the probe's waves, or its blocks / regions
  j.f = z.f; j.fs = (double)z.f / ugrid->cellLength;
  j.lds_budget = join_probe_budget(nq, qn, z.c, z.f);
  // (1) row histograms of both sides, (2) one scan of both matrices, (3) write-combined row
  // scatter of both sides, (4) query rows sorted by (sub-)cell + ordinary row / task offsets,
  // (5) probe (its last block scans the task counts), (6) packing
  GF_HIP_CHECK(ctx, launch_join_rows(ctx, j, q, 0));
  if ((st = scan1(ctx, L.cat, z.qmat + z.mat, L.cats))) return st;
  GF_HIP_CHECK(ctx, launch_join_rows(ctx, j, q, 1));
  GF_HIP_CHECK(ctx, launch_join_rows(ctx, j, q, 2));
  JoinFixup fx{};
  fx.o = j.out;
  fx.total = k.total_out ? k.total_out : L.gcnt + 1;
  fx.hint = ctx->join_hint;
  fx.hole_start = L.hs; fx.hole_pref = L.hp;
  fx.seg_start = L.ss; fx.seg_pref = L.sp;
  fx.counts = L.fc;
  if (z.band) {  // its last block prepares the fix-up (fx)
    j.fx = fx;
    j.ticket = ctx->join_ovf + 1;
    GF_HIP_CHECK(ctx, launch_join_band(ctx, j, (int)z.probe_blocks));
  } else if (z.stream) {
    j.out.nwaves = (uint32_t)z.nwaves;  // the stream grid: kBlock-thread blocks, same wave count
    GF_HIP_CHECK(ctx, launch_join_stream(ctx, j));
  } else {
    GF_HIP_CHECK(ctx, launch_join_rows(ctx, j, q, 3));
  }
  fx.o = j.out;  // (the streaming experiment changed its wave count)
  GF_HIP_CHECK(ctx, launch_join_fixup(ctx, fx));
  if (k.total_out) {  // the caller reads *total_out stream-ordered
    ctx->join_async_done = 1;
    return GF_OK;
  }
  unsigned long long total = 0;
  if (int e = read_scalar_sync(ctx, L.gcnt + 1, &total)) return e;
  *k.npairs = (int64_t)total;
  ctx->join_ppp = (double)total / (double)no;
  if ((int64_t)total > k.cap || (total > 0 && !k.pairs)) return GF_ERR_CAPACITY;
  return GF_OK;
}

// the cell-probe fallback: query side bucketed by cell, a count pass and a write pass (synchronous)
int join_legacy_path(const JoinCall& k, const JoinSizing& z, const JoinScratch& L) {
  gf_ctx* ctx = k.ctx;
  const gf_grid *ugrid = k.ugrid, *qgrid = k.qgrid;
  const gf_points* qry = k.qry;
  const int64_t nq = qry->n;
  const int blocks = z.blocks;
  hipStream_t s = ctx->stream;
  GF_HIP_CHECK(ctx, hipMemsetAsync(L.hist, 0, z.bins * sizeof(uint32_t), s));
  GF_HIP_CHECK(ctx, launch_join_qkeys(s, qry->x, qry->y, nq, qgrid->minX, qgrid->minY, qgrid->cellLength,
                                      qgrid->n, L.keys, L.qcx, L.qcy));
  GF_HIP_CHECK(ctx, launch_histogram(s, L.keys, nq, L.hist));
  GF_HIP_CHECK(ctx, launch_exclusive_scan(s, L.hist, z.bins, L.off, L.tmp));
  GF_HIP_CHECK(ctx, hipMemcpyAsync(L.cur, L.off, z.bins * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
  GF_HIP_CHECK(ctx, launch_join_qscatter(s, qry->x, qry->y, L.qcx, L.qcy, L.keys, nq, L.cur,
                                         L.sqx, L.sqy, L.sqcx, L.sqcy, L.sqi));
  JoinArgs a{};
  a.ox = k.ord->x; a.oy = k.ord->y; a.no = k.ord->n;
  a.u_minX = ugrid->minX; a.u_minY = ugrid->minY; a.u_cl = ugrid->cellLength;
  a.qn = qgrid->n; a.c = z.c; a.q_off = L.off;
  a.sqx = L.sqx; a.sqy = L.sqy; a.sqcx = L.sqcx; a.sqcy = L.sqcy; a.sqidx = L.sqi;
  a.approx = k.approximate != 0; a.metric = k.metric; a.r = k.r;
  a.counts = L.cnt; a.offsets = L.boff; a.pairs = k.pairs;
  GF_HIP_CHECK(ctx, launch_join_probe(ctx, a, 0, blocks));
  GF_HIP_CHECK(ctx, launch_exclusive_scan(s, L.cnt, blocks, L.boff, L.tmp));
  uint32_t total = 0;
  if (int e = read_scalar_sync(ctx, L.boff + blocks, &total)) return e;
  *k.npairs = total;
  if ((int64_t)total > k.cap) return GF_ERR_CAPACITY;
  if (total == 0) return GF_OK;
  if (!k.pairs) return set_err(ctx, GF_ERR_ARG, "null pairs");
  GF_HIP_CHECK(ctx, launch_join_probe(ctx, a, 1, blocks));
  GF_HIP_CHECK(ctx, hipStreamSynchronize(s));
  return GF_OK;
}

int join_pp_impl(const JoinCall& k) {
  gf_ctx* ctx = k.ctx;
  if (!ctx || !grid_ok(k.ugrid) || !grid_ok(k.qgrid) || !k.npairs || (k.metric != 0 && k.metric != 1))
    return set_err(ctx, GF_ERR_ARG, "gf_join_pp: bad argument");
  ctx->join_async_done = 0;
  int st = bind(ctx);
  if (st) return st;
  if ((st = check_points(ctx, k.ord)) || (st = check_points(ctx, k.qry))) return st;
  *k.npairs = 0;
  int64_t c;
  if (k.r == 0) {
    c = -1;  // getNeighboringCells: every grid cell (UniformGrid.java:264-266)
  } else {
    c = candidate_layers(k.qgrid->cellLength, k.r);
    if (c <= 0) return set_err(ctx, GF_ERR_LAYERS, "candidateNeighboringLayers cannot be 0 or less");
  }
  if (k.ord->n == 0 || k.qry->n == 0) return GF_OK;
  const int64_t W = (int64_t)k.qgrid->n + 2;
  if (W * W >= (int64_t)INT32_MAX / 2) return set_err(ctx, GF_ERR_ARG, "query grid too large");
  const JoinSizing z = join_sizing(k, c);
  Arena ar;
  JoinScratch L;
  join_layout(k, z, ar, L);
  if ((st = ar.alloc(ctx))) return st;
  // the two paths share nothing past the scratch
  return z.rowpath ? join_rows_path(k, z, L) : join_legacy_path(k, z, L);
}

}  // namespace

extern "C" int gf_join_pp(gf_ctx* ctx, const gf_grid* ugrid, const gf_grid* qgrid, const gf_points* ord,
                          const gf_points* qry, double r, int approximate, int metric, uint32_t* pairs, int64_t cap,
                          int64_t* npairs) {
  return join_pp_impl({ctx, ugrid, qgrid, ord, qry, r, approximate, metric, pairs, cap, npairs, nullptr});
}

extern "C" int gf_join_pp_async(gf_ctx* ctx, const gf_grid* ugrid, const gf_grid* qgrid, const gf_points* ord,
                                const gf_points* qry, double r, int approximate, int metric, uint32_t* pairs,
                                int64_t cap, unsigned long long* total) {
  if (!total) return set_err(ctx, GF_ERR_ARG, "gf_join_pp_async: null total");
  int64_t n = 0;
  int st = join_pp_impl({ctx, ugrid, qgrid, ord, qry, r, approximate, metric, pairs, cap, &n, total});
  if (st == GF_ERR_CAPACITY) st = GF_OK;  // the count is in *total
  if (st) return st;
  if (!ctx->join_async_done) {  // the synchronous paths (r == 0, empty sides): store the count
    const unsigned long long v = (unsigned long long)n;
    GF_HIP_CHECK(ctx, hipMemcpyAsync(total, &v, sizeof v, hipMemcpyHostToDevice, ctx->stream));
    GF_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  }
  return GF_OK;
}
