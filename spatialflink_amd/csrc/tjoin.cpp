// tjoin.cpp -- tJoin entry points of the C ABI (tJoin/PointPointTJoinQuery.java windowBased /
// commonSingle, TJoinQuery.java): gf_tjoin_run over two windows already grouped by objID
// (gf_traj_group), the reads and the testing hook.  The kernels are in k_tjoin.hip; the multi-word sorts
// are gf_group.hpp's (traj.cpp) on k_points.hip's radix passes, the query side's clamped bucket key is
// k_join.hip's launch_join_qkeys.  The object is made of gf_group.hpp's typed device arrays (grow-only,
// freed by its destructor), the row table included, and is reused across windows; the table's growth
// loop lives here.
#define GF_TU_NAME tjoin_cpp
#include "gf_buildtag.hpp"  // first: records this unit's command-line defines

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "gf_group.hpp"

using namespace gf;

struct gf_tjoin {
  gf_ctx* ctx = nullptr;
  int64_t rows = 0, emitted = 0, m[2] = {0, 0}, npts[2] = {0, 0}, passes = 0;
  int64_t slots = 0;       // the table of the last window (0: none yet)
  int64_t want_slots = 0;  // testing: the next run's first table size (0: slots, or the default)
  KeyGroups srt;           // the sorts' radix workspace and the scans' scratch
  DevArr<uint32_t> wkey, sp[2];
  // the query side in bucket order, the ordinary side's cell keys
  DevArr<uint32_t> bkey, qrank, qord, sqr, flag, fscan, rstart, boff;
  DevArr<int32_t> qcx, qcy;
  DevArr<unsigned long long> its, comp, ocell;
  DevArr<double2> sxy;
  DevArr<int4> smeta;
  // the row table, the rows
  DevArr<unsigned long long> tkey, rkey;
  DevArr<uint32_t> tqr, tpf, tcount, occ, cpos, rqr, rpf, o_pfirst, o_qlatest, o_to, o_tq, counters;
  DevArr<int64_t> o_okey, o_qkey;
  DevArr<uint8_t> o_emit;
  DevArr<int32_t> o_oslot, o_qslot;
  // per side: the emitted trajectories' CSR
  DevArr<uint32_t> mark[2], mrank[2], tlist[2], tlen[2], toff[2], c_idx[2];
  DevArr<int64_t> c_keys[2], c_ts[2];
  DevArr<double> c_x[2], c_y[2];
};

constexpr size_t kTjoinCounterWords = 8;  // TjoinArgs::counters
constexpr size_t kTjoinCountWords = (size_t)kTjoinMaxShards * kTjoinShardStride + 1;  // TjoinTable::count, then the overflow word

static int64_t pow2_at_least(double v) {
  int64_t p = kTjoinMinSlots;
  while ((double)p < v && p < ((int64_t)1 << 31)) p <<= 1;
  return p;
}

// the query side in bucket order: qrank, the (bucket, trajectory, qrank) order, the runs
static int tjoin_query_side(gf_tjoin* T, gf_traj_groups* gq, const gf_points* qpts, const gf_grid* grid, TjoinArgs& a) {
  gf_ctx* ctx = T->ctx;
  int st = GF_OK;
  const int64_t nq = gq->n, ntq = gq->ntraj, W = (int64_t)grid->n + 2;
  const size_t z = (size_t)nq;
  a.nb = W * W;
  if ((st = T->bkey.reserve(ctx, z)) || (st = T->qcx.reserve(ctx, z)) || (st = T->qcy.reserve(ctx, z)) ||
      (st = T->its.reserve(ctx, z)) || (st = T->comp.reserve(ctx, z)) || (st = T->qrank.reserve(ctx, z)) ||
      (st = T->qord.reserve(ctx, z)) || (st = T->sxy.reserve(ctx, z)) || (st = T->smeta.reserve(ctx, z)) ||
      (st = T->sqr.reserve(ctx, z)) || (st = T->flag.reserve(ctx, z + 1)) || (st = T->fscan.reserve(ctx, z + 1)) ||
      (st = T->rstart.reserve(ctx, z + 1)) || (st = T->boff.reserve(ctx, (size_t)a.nb + 1)))
    return st;
  a.qx = qpts->x; a.qy = qpts->y; a.qts = qpts->ts;
  a.qdid = gq->did.p; a.qseg = gq->seg_off.p; a.qperm = gq->perm.p; a.qkeys = gq->keys.p;
  a.nq = nq; a.ntq = ntq;
  a.bkey = T->bkey.p; a.qcx = T->qcx.p; a.qcy = T->qcy.p; a.its = T->its.p; a.comp = T->comp.p;
  a.qrank = T->qrank.p; a.qord = T->qord.p; a.sxy = T->sxy.p; a.smeta = T->smeta.p; a.sqr = T->sqr.p;
  a.flag = T->flag.p; a.fscan = T->fscan.p; a.rstart = T->rstart.p; a.boff = T->boff.p;
  GF_HIP_CHECK(ctx, launch_join_qkeys(ctx->stream, a.qx, a.qy, nq, grid->minX, grid->minY, grid->cellLength, grid->n,
                                      T->bkey.p, T->qcx.p, T->qcy.p));
  GF_HIP_CHECK(ctx, launch_tjoin(ctx, kTjoinQueryKeys, a));
  // (trajectory, ts descending, index): the inverted ts words, then the trajectory, least significant first
  const SortWord w3[3] = {{a.its, nullptr, 0, 32}, {a.its, nullptr, 32, 32}, {a.comp, nullptr, 0, key_bits((uint64_t)ntq)}};
  if ((st = group_sort_words(ctx, T->srt, T->wkey, T->sp, w3, 3, nq, nullptr, &a.ord))) return st;
  GF_HIP_CHECK(ctx, launch_tjoin(ctx, kTjoinQueryRank, a));
  // stably by bucket over that order: every bucket sorted by (trajectory, qrank)
  const SortWord wb[1] = {{a.comp, nullptr, 32, key_bits((uint64_t)a.nb)}};
  if ((st = group_sort_words(ctx, T->srt, T->wkey, T->sp, wb, 1, nq, a.qord, &a.sidx))) return st;
  GF_HIP_CHECK(ctx, launch_tjoin(ctx, kTjoinQueryScatter, a));
  if ((st = group_scan_u32(ctx, T->srt, a.flag, nq, T->fscan.p))) return st;
  GF_HIP_CHECK(ctx, launch_tjoin(ctx, kTjoinRunStarts, a));
  GF_HIP_CHECK(ctx, launch_tjoin(ctx, kTjoinRunEnds, a));
  return GF_OK;
}

// the table of `slots` slots, cleared
static int tjoin_table(gf_tjoin* T, int64_t slots, TjoinArgs& a) {
  gf_ctx* ctx = T->ctx;
  int st = GF_OK;
  const size_t z = (size_t)slots;
  uint32_t shards = 1;
  while (shards < kTjoinMaxShards && (int64_t)shards * 2048 <= slots) shards <<= 1;  // >= 512 rows a shard
  const size_t cwords = (size_t)shards * kTjoinShardStride + 1;  // the counters, then the overflow word
  if ((st = T->tkey.reserve(ctx, z)) || (st = T->tqr.reserve(ctx, z)) || (st = T->tpf.reserve(ctx, z)) ||
      (st = T->tcount.reserve(ctx, kTjoinCountWords)))
    return st;
  a.t.key = T->tkey.p;
  a.t.qrank = T->tqr.p;
  a.t.pfirst = T->tpf.p;
  a.t.mask = (uint64_t)slots - 1;
  a.t.count = T->tcount.p;
  a.t.overflow = a.t.count + (size_t)shards * kTjoinShardStride;
  a.t.shard_shift = (uint32_t)(key_bits((uint64_t)slots) - key_bits((uint64_t)shards));  // (both powers of two; 1 shard: >= the key's bits)
  if (shards == 1) a.t.shard_shift = 63;
  a.t.shard_cap = (uint32_t)(slots / 2 / shards);
  a.slots = slots;
  GF_HIP_CHECK(ctx, hipMemsetAsync(a.t.key, 0xFF, z * sizeof *a.t.key, ctx->stream));
  GF_HIP_CHECK(ctx, hipMemsetAsync(a.t.qrank, 0xFF, z * sizeof *a.t.qrank, ctx->stream));
  GF_HIP_CHECK(ctx, hipMemsetAsync(a.t.pfirst, 0xFF, z * sizeof *a.t.pfirst, ctx->stream));
  GF_HIP_CHECK(ctx, hipMemsetAsync(a.t.count, 0, cwords * sizeof *a.t.count, ctx->stream));
  return GF_OK;
}

// one side's CSR: the emitted trajectories' list, lengths and offsets (enqueued)
static int tjoin_side_lists(gf_tjoin* T, int side, TjoinArgs& a) {
  gf_ctx* ctx = T->ctx;
  int st = GF_OK;
  const int64_t nt = side ? a.ntq : a.nto;
  if ((st = group_scan_u32(ctx, T->srt, a.mark[side], nt, T->mrank[side].p))) return st;
  GF_HIP_CHECK(ctx, hipMemsetAsync(T->tlen[side].p, 0, ((size_t)nt + 1) * sizeof(uint32_t), ctx->stream));
  a.side = side;
  a.nt = nt;
  GF_HIP_CHECK(ctx, launch_tjoin(ctx, kTjoinSideList, a));
  return group_scan_u32(ctx, T->srt, a.tlen[side], nt, T->toff[side].p);
}

static int tjoin_window(gf_tjoin* T, gf_traj_groups* go, const gf_points* opts, gf_traj_groups* gq, const gf_points* qpts,
                        const gf_grid* grid, double r, int64_t c, int single) {
  gf_ctx* ctx = T->ctx;
  int st = GF_OK;
  const int64_t no = go->n, nq = gq->n, nto = go->ntraj, ntq = gq->ntraj;
  TjoinArgs a{};
  if ((st = tjoin_query_side(T, gq, qpts, grid, a))) return st;
  // the ordinary side, sorted by cell for the probe
  a.ox = opts->x; a.oy = opts->y; a.ots = opts->ts;
  a.odid = go->did.p; a.oseg = go->seg_off.p; a.operm = go->perm.p; a.okeys = go->keys.p;
  a.no = no; a.nto = nto;
  a.minX = grid->minX; a.minY = grid->minY; a.cl = grid->cellLength; a.r = r;
  a.qn = grid->n; a.c = c; a.single = single;
  if ((st = T->ocell.reserve(ctx, (size_t)no))) return st;
  a.ocell = T->ocell.p;
  GF_HIP_CHECK(ctx, launch_tjoin(ctx, kTjoinCellKeys, a));
  const SortWord wo[1] = {{a.ocell, nullptr, 0, key_bits((uint64_t)grid->n * (uint64_t)grid->n + 1)}};
  if ((st = group_sort_words(ctx, T->srt, T->wkey, T->sp, wo, 1, no, nullptr, &a.oord))) return st;
  // The probe, again with a table twice the size while it overflows.  No row table is larger than
  // min(n_o x n_q, ntraj_o x ntraj_q) rows; a table of eight times that never overflows a shard.
  const double max_rows = std::min((double)no * (double)nq, (double)nto * (double)ntq);
  const int64_t max_slots = pow2_at_least(8.0 * max_rows);
  int64_t slots = T->want_slots ? T->want_slots : std::max(T->slots, std::max(kTjoinSlots, pow2_at_least(2.0 * (double)(nto + ntq))));
  T->want_slots = 0;
  for (;;) {
    size_t free_b = 0, total_b = 0;
    GF_HIP_CHECK(ctx, hipMemGetInfo(&free_b, &total_b));
    const size_t held = T->tkey.bytes() + T->tqr.bytes() + T->tpf.bytes(), need = (size_t)slots * 16;
    if (need > held && need - held > free_b) return set_err(ctx, GF_ERR_NOMEM, "gf_tjoin_run: the row table does not fit the device memory");
    if ((st = tjoin_table(T, slots, a))) return st;
    GF_HIP_CHECK(ctx, launch_tjoin(ctx, kTjoinProbe, a));
    ++T->passes;
    uint32_t ovf = 0;
    if ((st = read_scalar_sync(ctx, a.t.overflow, &ovf))) return st;
    if (!ovf) break;
    if (slots >= max_slots) return set_err(ctx, GF_ERR_NOMEM, "gf_tjoin_run: the row table outgrew its bound");
    slots <<= 1;
  }
  T->slots = slots;
  // the rows: the occupied slots packed, then sorted by (t_o, t_q)
  if ((st = T->occ.reserve(ctx, (size_t)slots + 1)) || (st = T->cpos.reserve(ctx, (size_t)slots + 1))) return st;
  a.occ = T->occ.p;
  a.cpos = T->cpos.p;
  GF_HIP_CHECK(ctx, launch_tjoin(ctx, kTjoinOccupied, a));
  if ((st = group_scan_u32(ctx, T->srt, a.occ, slots, T->cpos.p))) return st;
  uint32_t rows32 = 0;
  if ((st = read_scalar_sync(ctx, a.cpos + slots, &rows32))) return st;
  const int64_t rows = rows32;
  if (rows > slots / 2) return set_err(ctx, GF_ERR_HIP, "gf_tjoin_run: inconsistent row count");
  T->rows = rows;
  if (rows == 0) return GF_OK;
  const size_t nr = (size_t)rows;
  if ((st = T->rkey.reserve(ctx, nr)) || (st = T->rqr.reserve(ctx, nr)) || (st = T->rpf.reserve(ctx, nr)) ||
      (st = T->o_okey.reserve(ctx, nr)) || (st = T->o_qkey.reserve(ctx, nr)) || (st = T->o_pfirst.reserve(ctx, nr)) ||
      (st = T->o_qlatest.reserve(ctx, nr)) || (st = T->o_emit.reserve(ctx, nr)) || (st = T->o_oslot.reserve(ctx, nr)) ||
      (st = T->o_qslot.reserve(ctx, nr)) || (st = T->o_to.reserve(ctx, nr)) || (st = T->o_tq.reserve(ctx, nr)) ||
      (st = T->counters.reserve(ctx, kTjoinCounterWords)))
    return st;
  const int64_t nts[2] = {nto, ntq};
  for (int s = 0; s < 2; ++s) {
    const size_t w = (size_t)nts[s] + 1;
    if ((st = T->mark[s].reserve(ctx, w)) || (st = T->mrank[s].reserve(ctx, w)) || (st = T->tlist[s].reserve(ctx, w)) ||
        (st = T->tlen[s].reserve(ctx, w)) || (st = T->toff[s].reserve(ctx, w)))
      return st;
    GF_HIP_CHECK(ctx, hipMemsetAsync(T->mark[s].p, 0, w * sizeof(uint32_t), ctx->stream));
    a.mark[s] = T->mark[s].p; a.mrank[s] = T->mrank[s].p; a.tlist[s] = T->tlist[s].p; a.tlen[s] = T->tlen[s].p;
    a.toff[s] = T->toff[s].p;
  }
  a.rows = rows;
  a.rkey = T->rkey.p; a.rqr = T->rqr.p; a.rpf = T->rpf.p; a.o_okey = T->o_okey.p; a.o_qkey = T->o_qkey.p;
  a.o_pfirst = T->o_pfirst.p; a.o_qlatest = T->o_qlatest.p; a.o_emit = T->o_emit.p; a.o_oslot = T->o_oslot.p;
  a.o_qslot = T->o_qslot.p; a.o_to = T->o_to.p; a.o_tq = T->o_tq.p; a.counters = T->counters.p;
  GF_HIP_CHECK(ctx, hipMemsetAsync(a.counters, 0, kTjoinCounterWords * sizeof(uint32_t), ctx->stream));
  GF_HIP_CHECK(ctx, launch_tjoin(ctx, kTjoinCompact, a));
  const SortWord wr[2] = {{a.rkey, nullptr, 0, key_bits((uint64_t)ntq)}, {a.rkey, nullptr, 32, key_bits((uint64_t)nto)}};
  if ((st = group_sort_words(ctx, T->srt, T->wkey, T->sp, wr, 2, rows, nullptr, &a.rorder))) return st;
  GF_HIP_CHECK(ctx, launch_tjoin(ctx, kTjoinRows, a));
  // the emitted rows' trajectories per side, their slots, their CSR
  if ((st = tjoin_side_lists(T, 0, a)) || (st = tjoin_side_lists(T, 1, a))) return st;
  GF_HIP_CHECK(ctx, launch_tjoin(ctx, kTjoinRowSlots, a));
  GF_HIP_CHECK(ctx, launch_tjoin(ctx, kTjoinTotals, a));
  struct Totals { uint32_t v[kTjoinCounterWords]; } tot{};
  if ((st = read_scalar_sync(ctx, a.counters, &tot))) return st;
  T->emitted = tot.v[0];
  T->m[0] = tot.v[1]; T->npts[0] = tot.v[2];
  T->m[1] = tot.v[3]; T->npts[1] = tot.v[4];
  if (T->emitted > rows || T->m[0] > nto || T->npts[0] > no || T->m[1] > ntq || T->npts[1] > nq)
    return set_err(ctx, GF_ERR_HIP, "gf_tjoin_run: inconsistent counts");
  for (int s = 0; s < 2; ++s) {
    if (T->m[s] == 0) continue;
    const size_t zm = (size_t)T->m[s], zp = (size_t)T->npts[s];
    if ((st = T->c_keys[s].reserve(ctx, zm)) || (st = T->c_x[s].reserve(ctx, zp)) || (st = T->c_y[s].reserve(ctx, zp)) ||
        (st = T->c_ts[s].reserve(ctx, zp)) || (st = T->c_idx[s].reserve(ctx, zp)))
      return st;
    a.side = s;
    a.m = T->m[s]; a.npts = T->npts[s];
    a.c_keys = T->c_keys[s].p; a.c_x = T->c_x[s].p; a.c_y = T->c_y[s].p; a.c_ts = T->c_ts[s].p; a.c_idx = T->c_idx[s].p;
    GF_HIP_CHECK(ctx, launch_tjoin(ctx, kTjoinGather, a));
  }
  GF_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  return GF_OK;
}

static bool columns_ok(const gf_points* p) { return p->n == 0 || (p->x && p->y && p->objID && p->ts); }

extern "C" int gf_tjoin_run(gf_traj_groups* go, const gf_points* opts, gf_traj_groups* gq, const gf_points* qpts,
                            const gf_grid* grid, double r, int mode, gf_tjoin** out) {
  if (!go || !go->ctx || !gq || !gq->ctx) return GF_ERR_ARG;
  gf_ctx* ctx = go->ctx;
  if (gq->ctx != ctx) return set_err(ctx, GF_ERR_ARG, "gf_tjoin_run: groups of different contexts");
  if (!out || !grid || !opts || !qpts) return set_err(ctx, GF_ERR_ARG, "gf_tjoin_run: null argument");
  if (!grid_ok(grid)) return set_err(ctx, GF_ERR_ARG, "gf_tjoin_run: invalid grid");
  if (mode != GF_TJOIN_PAIR && mode != GF_TJOIN_SINGLE) return set_err(ctx, GF_ERR_ARG, "gf_tjoin_run: unknown mode");
  if (std::isnan(r)) return set_err(ctx, GF_ERR_ARG, "gf_tjoin_run: NaN r");
  if (opts->n != go->n || qpts->n != gq->n) return set_err(ctx, GF_ERR_ARG, "gf_tjoin_run: pts is not the grouped window");
  if (!columns_ok(opts) || !columns_ok(qpts)) return set_err(ctx, GF_ERR_ARG, "gf_tjoin_run: null x / y / objID / ts");
  if (mode == GF_TJOIN_SINGLE && go != gq) return set_err(ctx, GF_ERR_ARG, "gf_tjoin_run: SINGLE joins one groups object with itself");
  if (*out && (*out)->ctx != ctx) return set_err(ctx, GF_ERR_ARG, "gf_tjoin_run: object of another context");
  const int64_t W = (int64_t)grid->n + 2;
  if (W * W >= (int64_t)INT32_MAX / 2) return set_err(ctx, GF_ERR_ARG, "gf_tjoin_run: grid too large");
  int64_t c = -1;  // r == 0: every valid cell (UniformGrid.java:264-266)
  if (r != 0) {
    c = candidate_layers(grid->cellLength, r);
    if (c <= 0) return set_err(ctx, GF_ERR_LAYERS, "candidateNeighboringLayers cannot be 0 or less");
  }
  int st = bind(ctx);
  if (st) return st;
  const bool fresh = *out == nullptr;
  gf_tjoin* T = fresh ? new gf_tjoin() : *out;
  T->ctx = ctx;
  T->rows = T->emitted = T->m[0] = T->m[1] = T->npts[0] = T->npts[1] = T->passes = 0;
  if (go->n > 0 && gq->n > 0) st = tjoin_window(T, go, opts, gq, qpts, grid, r, c, mode == GF_TJOIN_SINGLE ? 1 : 0);
  if (st) {
    if (fresh) gf_tjoin_destroy(T);
    else T->rows = T->emitted = T->m[0] = T->m[1] = T->npts[0] = T->npts[1] = 0;
    return st;
  }
  *out = T;
  return GF_OK;
}

extern "C" void gf_tjoin_destroy(gf_tjoin* T) {
  if (!T) return;
  if (T->ctx) {
    hipSetDevice(T->ctx->device);
    hipStreamSynchronize(T->ctx->stream);
  }
  delete T;
}

extern "C" int gf_tjoin_info(const gf_tjoin* T, int64_t* rows, int64_t* emitted, int64_t* otraj, int64_t* opoints,
                             int64_t* qtraj, int64_t* qpoints, int64_t* probe_passes) {
  if (!T) return GF_ERR_ARG;
  if (rows) *rows = T->rows;
  if (emitted) *emitted = T->emitted;
  if (otraj) *otraj = T->m[0];
  if (opoints) *opoints = T->npts[0];
  if (qtraj) *qtraj = T->m[1];
  if (qpoints) *qpoints = T->npts[1];
  if (probe_passes) *probe_passes = T->passes;
  return GF_OK;
}

extern "C" int gf_tjoin_set_table_slots(gf_tjoin* T, int64_t slots) {
  if (!T || slots < 0 || slots > ((int64_t)1 << 31) || (slots & (slots - 1)) != 0 || (slots != 0 && slots < kTjoinMinSlots))
    return GF_ERR_ARG;
  T->want_slots = slots;
  if (slots == 0) T->slots = 0;
  return GF_OK;
}

extern "C" int gf_tjoin_read_rows(gf_tjoin* T, int64_t* okey, int64_t* qkey, uint32_t* p_first, uint32_t* q_latest,
                                  uint8_t* emit, int32_t* oslot, int32_t* qslot, int64_t cap) {
  if (!T || !T->ctx) return GF_ERR_ARG;
  gf_ctx* ctx = T->ctx;
  if (cap < 0) return set_err(ctx, GF_ERR_ARG, "gf_tjoin_read_rows: bad argument");
  if (T->rows == 0) return GF_OK;
  int st = bind(ctx);
  if (st) return st;
  const size_t w = (size_t)std::min(T->rows, cap);
  if ((st = read_back(ctx, okey, T->o_okey.p, w)) || (st = read_back(ctx, qkey, T->o_qkey.p, w)) ||
      (st = read_back(ctx, p_first, T->o_pfirst.p, w)) || (st = read_back(ctx, q_latest, T->o_qlatest.p, w)) ||
      (st = read_back(ctx, emit, T->o_emit.p, w)) || (st = read_back(ctx, oslot, T->o_oslot.p, w)) ||
      (st = read_back(ctx, qslot, T->o_qslot.p, w)))
    return st;
  GF_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  return GF_OK;
}

extern "C" int gf_tjoin_read_trajs(gf_tjoin* T, int side, int64_t* keys, int64_t* off, int64_t cap_traj, double* x, double* y,
                                   int64_t* ts, uint32_t* idx, int64_t cap_pts) {
  if (!T || !T->ctx) return GF_ERR_ARG;
  gf_ctx* ctx = T->ctx;
  if ((side != 0 && side != 1) || cap_traj < 0 || cap_pts < 0) return set_err(ctx, GF_ERR_ARG, "gf_tjoin_read_trajs: bad argument");
  if (off) off[0] = 0;
  if (T->m[side] == 0) return GF_OK;
  int st = bind(ctx);
  if (st) return st;
  const size_t wt = (size_t)std::min(T->m[side], cap_traj), wp = (size_t)std::min(T->npts[side], cap_pts);
  OffsetRead ho;
  if ((st = read_back(ctx, keys, T->c_keys[side].p, wt)) || (st = read_offsets(ctx, ho, off, T->toff[side].p, wt + 1)) ||
      (st = read_back(ctx, x, T->c_x[side].p, wp)) || (st = read_back(ctx, y, T->c_y[side].p, wp)) ||
      (st = read_back(ctx, ts, T->c_ts[side].p, wp)) || (st = read_back(ctx, idx, T->c_idx[side].p, wp)))
    return st;
  GF_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  ho.widen();
  return GF_OK;
}
