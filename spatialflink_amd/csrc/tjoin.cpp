// tjoin.cpp -- tJoin entry points of the C ABI (tJoin/PointPointTJoinQuery.java windowBased /
// commonSingle, TJoinQuery.java): gf_tjoin_run over two windows already grouped by objID
// (gf_traj_group), the reads and the testing hook.  The kernels are in k_tjoin.hip; the multi-word sorts
// are gf_group.hpp's (traj.cpp) on k_points.hip's radix passes, the query side's clamped bucket key is
// k_join.hip's launch_join_qkeys.  The object owns its device workspace (grow-only), the row table
// included, and is reused across windows; the table's growth loop lives here.
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
  DevBuf wkey, sp[2];
  DevBuf bkey, qcx, qcy, its, comp, qrank, qord, sxy, smeta, sqr, flag, fscan, rstart, boff, ocell, tkey, tqr, tpf, tcount,
      occ, cpos, rkey, rqr, rpf, o_okey, o_qkey, o_pfirst, o_qlatest, o_emit, o_oslot, o_qslot, o_to, o_tq, counters;
  DevBuf mark[2], mrank[2], tlist[2], tlen[2], toff[2], c_keys[2], c_x[2], c_y[2], c_ts[2], c_idx[2];
  std::vector<DevBuf*> all() {
    std::vector<DevBuf*> v = {&wkey, &sp[0], &sp[1], &bkey, &qcx, &qcy, &its, &comp, &qrank, &qord, &sxy, &smeta, &sqr,
                              &flag, &fscan, &rstart, &boff, &ocell, &tkey, &tqr, &tpf, &tcount, &occ, &cpos, &rkey,
                              &rqr, &rpf, &o_okey, &o_qkey, &o_pfirst, &o_qlatest, &o_emit, &o_oslot, &o_qslot, &o_to,
                              &o_tq, &counters};
    for (int s = 0; s < 2; ++s)
      for (DevBuf* b : {&mark[s], &mrank[s], &tlist[s], &tlen[s], &toff[s], &c_keys[s], &c_x[s], &c_y[s], &c_ts[s], &c_idx[s]})
        v.push_back(b);
    return v;
  }
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
  if ((st = T->bkey.reserve(ctx, z * 4)) || (st = T->qcx.reserve(ctx, z * 4)) || (st = T->qcy.reserve(ctx, z * 4)) ||
      (st = T->its.reserve(ctx, z * 8)) || (st = T->comp.reserve(ctx, z * 8)) || (st = T->qrank.reserve(ctx, z * 4)) ||
      (st = T->qord.reserve(ctx, z * 4)) || (st = T->sxy.reserve(ctx, z * 16)) || (st = T->smeta.reserve(ctx, z * 16)) ||
      (st = T->sqr.reserve(ctx, z * 4)) || (st = T->flag.reserve(ctx, (z + 1) * 4)) ||
      (st = T->fscan.reserve(ctx, (z + 1) * 4)) || (st = T->rstart.reserve(ctx, (z + 1) * 4)) ||
      (st = T->boff.reserve(ctx, ((size_t)a.nb + 1) * 4)))
    return st;
  a.qx = qpts->x; a.qy = qpts->y; a.qts = qpts->ts;
  a.qdid = gq->did.as<uint32_t>(); a.qseg = gq->seg_off.as<uint32_t>(); a.qperm = gq->perm.as<uint32_t>();
  a.qkeys = gq->keys.as<int64_t>();
  a.nq = nq; a.ntq = ntq;
  a.bkey = T->bkey.as<uint32_t>(); a.qcx = T->qcx.as<int32_t>(); a.qcy = T->qcy.as<int32_t>();
  a.its = T->its.as<unsigned long long>(); a.comp = T->comp.as<unsigned long long>();
  a.qrank = T->qrank.as<uint32_t>(); a.qord = T->qord.as<uint32_t>();
  a.sxy = T->sxy.as<double2>(); a.smeta = T->smeta.as<int4>(); a.sqr = T->sqr.as<uint32_t>();
  a.flag = T->flag.as<uint32_t>(); a.fscan = T->fscan.as<uint32_t>(); a.rstart = T->rstart.as<uint32_t>();
  a.boff = T->boff.as<uint32_t>();
  GF_HIP_CHECK(ctx, launch_join_qkeys(ctx->stream, a.qx, a.qy, nq, grid->minX, grid->minY, grid->cellLength, grid->n,
                                      T->bkey.as<uint32_t>(), T->qcx.as<int32_t>(), T->qcy.as<int32_t>()));
  GF_HIP_CHECK(ctx, launch_tjoin(ctx, 0, a));
  // (trajectory, ts descending, index): the inverted ts words, then the trajectory, least significant first
  const SortWord w3[3] = {{a.its, nullptr, 0, 32}, {a.its, nullptr, 32, 32}, {a.comp, nullptr, 0, key_bits((uint64_t)ntq)}};
  if ((st = group_sort_words(ctx, T->srt, T->wkey, T->sp, w3, 3, nq, nullptr, &a.ord))) return st;
  GF_HIP_CHECK(ctx, launch_tjoin(ctx, 1, a));
  // stably by bucket over that order: every bucket sorted by (trajectory, qrank)
  const SortWord wb[1] = {{a.comp, nullptr, 32, key_bits((uint64_t)a.nb)}};
  if ((st = group_sort_words(ctx, T->srt, T->wkey, T->sp, wb, 1, nq, a.qord, &a.sidx))) return st;
  GF_HIP_CHECK(ctx, launch_tjoin(ctx, 2, a));
  if ((st = group_scan_u32(ctx, T->srt, a.flag, nq, T->fscan.as<uint32_t>()))) return st;
  GF_HIP_CHECK(ctx, launch_tjoin(ctx, 3, a));
  GF_HIP_CHECK(ctx, launch_tjoin(ctx, 4, a));
  return GF_OK;
}

// the table of `slots` slots, cleared
static int tjoin_table(gf_tjoin* T, int64_t slots, TjoinArgs& a) {
  gf_ctx* ctx = T->ctx;
  int st = GF_OK;
  const size_t z = (size_t)slots;
  uint32_t shards = 1;
  while (shards < kTjoinMaxShards && (int64_t)shards * 2048 <= slots) shards <<= 1;  // >= 512 rows a shard
  const size_t cbytes = (size_t)shards * kTjoinShardStride * 4 + 4;  // the counters, then the overflow word
  if ((st = T->tkey.reserve(ctx, z * 8)) || (st = T->tqr.reserve(ctx, z * 4)) || (st = T->tpf.reserve(ctx, z * 4)) ||
      (st = T->tcount.reserve(ctx, (size_t)kTjoinMaxShards * kTjoinShardStride * 4 + 4)))
    return st;
  a.t.key = T->tkey.as<unsigned long long>();
  a.t.qrank = T->tqr.as<uint32_t>();
  a.t.pfirst = T->tpf.as<uint32_t>();
  a.t.mask = (uint64_t)slots - 1;
  a.t.count = T->tcount.as<uint32_t>();
  a.t.overflow = a.t.count + (size_t)shards * kTjoinShardStride;
  a.t.shard_shift = (uint32_t)(key_bits((uint64_t)slots) - key_bits((uint64_t)shards));  // (both powers of two; 1 shard: >= the key's bits)
  if (shards == 1) a.t.shard_shift = 63;
  a.t.shard_cap = (uint32_t)(slots / 2 / shards);
  a.slots = slots;
  GF_HIP_CHECK(ctx, hipMemsetAsync(a.t.key, 0xFF, z * 8, ctx->stream));
  GF_HIP_CHECK(ctx, hipMemsetAsync(a.t.qrank, 0xFF, z * 4, ctx->stream));
  GF_HIP_CHECK(ctx, hipMemsetAsync(a.t.pfirst, 0xFF, z * 4, ctx->stream));
  GF_HIP_CHECK(ctx, hipMemsetAsync(a.t.count, 0, cbytes, ctx->stream));
  return GF_OK;
}

// one side's CSR: the emitted trajectories' list, lengths and offsets (enqueued)
static int tjoin_side_lists(gf_tjoin* T, int side, TjoinArgs& a) {
  gf_ctx* ctx = T->ctx;
  int st = GF_OK;
  const int64_t nt = side ? a.ntq : a.nto;
  if ((st = group_scan_u32(ctx, T->srt, a.mark[side], nt, T->mrank[side].as<uint32_t>()))) return st;
  GF_HIP_CHECK(ctx, hipMemsetAsync(T->tlen[side].p, 0, ((size_t)nt + 1) * 4, ctx->stream));
  a.side = side;
  a.nt = nt;
  GF_HIP_CHECK(ctx, launch_tjoin(ctx, 11, a));
  return group_scan_u32(ctx, T->srt, a.tlen[side], nt, T->toff[side].as<uint32_t>());
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
  a.odid = go->did.as<uint32_t>(); a.oseg = go->seg_off.as<uint32_t>(); a.operm = go->perm.as<uint32_t>();
  a.okeys = go->keys.as<int64_t>();
  a.no = no; a.nto = nto;
  a.minX = grid->minX; a.minY = grid->minY; a.cl = grid->cellLength; a.r = r;
  a.qn = grid->n; a.c = c; a.single = single;
  if ((st = T->ocell.reserve(ctx, (size_t)no * 8))) return st;
  a.ocell = T->ocell.as<unsigned long long>();
  GF_HIP_CHECK(ctx, launch_tjoin(ctx, 5, a));
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
    const size_t held = T->tkey.bytes + T->tqr.bytes + T->tpf.bytes, need = (size_t)slots * 16;
    if (need > held && need - held > free_b) return set_err(ctx, GF_ERR_NOMEM, "gf_tjoin_run: the row table does not fit the device memory");
    if ((st = tjoin_table(T, slots, a))) return st;
    GF_HIP_CHECK(ctx, launch_tjoin(ctx, 6, a));
    ++T->passes;
    uint32_t ovf = 0;
    if ((st = read_scalar_sync(ctx, a.t.overflow, &ovf))) return st;
    if (!ovf) break;
    if (slots >= max_slots) return set_err(ctx, GF_ERR_NOMEM, "gf_tjoin_run: the row table outgrew its bound");
    slots <<= 1;
  }
  T->slots = slots;
  // the rows: the occupied slots packed, then sorted by (t_o, t_q)
  if ((st = T->occ.reserve(ctx, ((size_t)slots + 1) * 4)) || (st = T->cpos.reserve(ctx, ((size_t)slots + 1) * 4))) return st;
  a.occ = T->occ.as<uint32_t>();
  a.cpos = T->cpos.as<uint32_t>();
  GF_HIP_CHECK(ctx, launch_tjoin(ctx, 7, a));
  if ((st = group_scan_u32(ctx, T->srt, a.occ, slots, T->cpos.as<uint32_t>()))) return st;
  uint32_t rows32 = 0;
  if ((st = read_scalar_sync(ctx, a.cpos + slots, &rows32))) return st;
  const int64_t rows = rows32;
  if (rows > slots / 2) return set_err(ctx, GF_ERR_HIP, "gf_tjoin_run: inconsistent row count");
  T->rows = rows;
  if (rows == 0) return GF_OK;
  const size_t nr = (size_t)rows;
  if ((st = T->rkey.reserve(ctx, nr * 8)) || (st = T->rqr.reserve(ctx, nr * 4)) || (st = T->rpf.reserve(ctx, nr * 4)) ||
      (st = T->o_okey.reserve(ctx, nr * 8)) || (st = T->o_qkey.reserve(ctx, nr * 8)) || (st = T->o_pfirst.reserve(ctx, nr * 4)) ||
      (st = T->o_qlatest.reserve(ctx, nr * 4)) || (st = T->o_emit.reserve(ctx, nr)) || (st = T->o_oslot.reserve(ctx, nr * 4)) ||
      (st = T->o_qslot.reserve(ctx, nr * 4)) || (st = T->o_to.reserve(ctx, nr * 4)) || (st = T->o_tq.reserve(ctx, nr * 4)) ||
      (st = T->counters.reserve(ctx, 32)))
    return st;
  const int64_t nts[2] = {nto, ntq};
  for (int s = 0; s < 2; ++s) {
    const size_t w = ((size_t)nts[s] + 1) * 4;
    if ((st = T->mark[s].reserve(ctx, w)) || (st = T->mrank[s].reserve(ctx, w)) || (st = T->tlist[s].reserve(ctx, w)) ||
        (st = T->tlen[s].reserve(ctx, w)) || (st = T->toff[s].reserve(ctx, w)))
      return st;
    GF_HIP_CHECK(ctx, hipMemsetAsync(T->mark[s].p, 0, w, ctx->stream));
    a.mark[s] = T->mark[s].as<uint32_t>(); a.mrank[s] = T->mrank[s].as<uint32_t>();
    a.tlist[s] = T->tlist[s].as<uint32_t>(); a.tlen[s] = T->tlen[s].as<uint32_t>(); a.toff[s] = T->toff[s].as<uint32_t>();
  }
  a.rows = rows;
  a.rkey = T->rkey.as<unsigned long long>(); a.rqr = T->rqr.as<uint32_t>(); a.rpf = T->rpf.as<uint32_t>();
  a.o_okey = T->o_okey.as<int64_t>(); a.o_qkey = T->o_qkey.as<int64_t>();
  a.o_pfirst = T->o_pfirst.as<uint32_t>(); a.o_qlatest = T->o_qlatest.as<uint32_t>(); a.o_emit = T->o_emit.as<uint8_t>();
  a.o_oslot = T->o_oslot.as<int32_t>(); a.o_qslot = T->o_qslot.as<int32_t>();
  a.o_to = T->o_to.as<uint32_t>(); a.o_tq = T->o_tq.as<uint32_t>();
  a.counters = T->counters.as<uint32_t>();
  GF_HIP_CHECK(ctx, hipMemsetAsync(a.counters, 0, 32, ctx->stream));
  GF_HIP_CHECK(ctx, launch_tjoin(ctx, 8, a));
  const SortWord wr[2] = {{a.rkey, nullptr, 0, key_bits((uint64_t)ntq)}, {a.rkey, nullptr, 32, key_bits((uint64_t)nto)}};
  if ((st = group_sort_words(ctx, T->srt, T->wkey, T->sp, wr, 2, rows, nullptr, &a.rorder))) return st;
  GF_HIP_CHECK(ctx, launch_tjoin(ctx, 9, a));
  // the emitted rows' trajectories per side, their slots, their CSR
  if ((st = tjoin_side_lists(T, 0, a)) || (st = tjoin_side_lists(T, 1, a))) return st;
  GF_HIP_CHECK(ctx, launch_tjoin(ctx, 10, a));
  GF_HIP_CHECK(ctx, launch_tjoin(ctx, 12, a));
  struct Totals { uint32_t v[8]; } tot{};
  if ((st = read_scalar_sync(ctx, a.counters, &tot))) return st;
  T->emitted = tot.v[0];
  T->m[0] = tot.v[1]; T->npts[0] = tot.v[2];
  T->m[1] = tot.v[3]; T->npts[1] = tot.v[4];
  if (T->emitted > rows || T->m[0] > nto || T->npts[0] > no || T->m[1] > ntq || T->npts[1] > nq)
    return set_err(ctx, GF_ERR_HIP, "gf_tjoin_run: inconsistent counts");
  for (int s = 0; s < 2; ++s) {
    if (T->m[s] == 0) continue;
    const size_t zm = (size_t)T->m[s], zp = (size_t)T->npts[s];
    if ((st = T->c_keys[s].reserve(ctx, zm * 8)) || (st = T->c_x[s].reserve(ctx, zp * 8)) || (st = T->c_y[s].reserve(ctx, zp * 8)) ||
        (st = T->c_ts[s].reserve(ctx, zp * 8)) || (st = T->c_idx[s].reserve(ctx, zp * 4)))
      return st;
    a.side = s;
    a.m = T->m[s]; a.npts = T->npts[s];
    a.c_keys = T->c_keys[s].as<int64_t>(); a.c_x = T->c_x[s].as<double>(); a.c_y = T->c_y[s].as<double>();
    a.c_ts = T->c_ts[s].as<int64_t>(); a.c_idx = T->c_idx[s].as<uint32_t>();
    GF_HIP_CHECK(ctx, launch_tjoin(ctx, 13, a));
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
  T->srt.release_groups();
  for (DevBuf* b : T->all()) b->release();
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
  std::vector<uint32_t> ho;
  if (off) ho.resize(wt + 1);
  if ((st = read_back(ctx, keys, T->c_keys[side].p, wt)) ||
      (st = read_back(ctx, off ? ho.data() : nullptr, T->toff[side].p, ho.size())) ||
      (st = read_back(ctx, x, T->c_x[side].p, wp)) || (st = read_back(ctx, y, T->c_y[side].p, wp)) ||
      (st = read_back(ctx, ts, T->c_ts[side].p, wp)) || (st = read_back(ctx, idx, T->c_idx[side].p, wp)))
    return st;
  GF_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  for (size_t i = 0; i < ho.size(); ++i) off[i] = (int64_t)ho[i];
  return GF_OK;
}
