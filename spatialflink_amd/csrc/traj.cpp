// traj.cpp -- trajectory entry points of the C ABI: gf_traj_group (a window grouped by objID),
// gf_tstats_run (TStatsQuery.java:154-188 per trajectory), gf_traj_select (sub-trajectories of a
// hit bitmap), gf_tfilter_run.  The kernels are in k_traj.hip; the stable sort by dense trajectory id
// reuses the LSD radix passes of k_points.hip (radix_sort below: the one pass loop, also under the
// multi-word sorts).  The groups object is made of gf_group.hpp's typed device arrays (grow-only,
// freed by its destructor) and is reused across windows.  The grouping itself -- dense ids of a device
// int64 key column, then the stable sort by them -- is gf_group.hpp's, shared with tagg.cpp, tknn.cpp
// and tjoin.cpp.
#define GF_TU_NAME traj_cpp
#include "gf_buildtag.hpp"  // first: records this unit's command-line defines

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "gf_group.hpp"

using namespace gf;

// ---- gf_group.hpp: the grouping of a device int64 key column ----------------------------------
int gf::group_scan_u32(gf_ctx* ctx, KeyGroups& K, const uint32_t* in, int64_t L, uint32_t* out) {
  if (int st = K.scan_tmp.reserve(ctx, scan_tmp_elems(L))) return st;
  GF_HIP_CHECK(ctx, launch_exclusive_scan(ctx->stream, in, L, out, K.scan_tmp.p));
  return GF_OK;
}

int gf::group_dense_ids(gf_ctx* ctx, KeyGroups& K, const int64_t* key, int64_t n, const char* who) {
  int st = GF_OK;
  K.n = n;
  K.ngroups = 0;
  uint64_t slots = 64;
  while (slots < 2 * (uint64_t)n) slots <<= 1;
  const size_t w = (size_t)n + 1;
  if ((st = K.tkey.reserve(ctx, slots + 1)) || (st = K.tfirst.reserve(ctx, slots + 1)) || (st = K.kbuf[1].reserve(ctx, w)) ||
      (st = K.vbuf[1].reserve(ctx, w)) || (st = K.did.reserve(ctx, w)))
    return st;
  TrajGroupArgs a{};
  a.t.key = K.tkey.p;
  a.t.first = K.tfirst.p;
  a.t.mask = slots - 1;
  a.objID = key;
  a.n = n;
  a.flag = K.kbuf[1].p;
  a.rank = K.vbuf[1].p;
  a.did = K.did.p;
  hipError_t e = launch_traj_group(ctx, kTrajGroupInsert, a);
  if (e != hipSuccess) return hip_err(ctx, e, "traj insert");
  if ((st = group_scan_u32(ctx, K, a.flag, n, K.vbuf[1].p))) return st;
  // the group count sizes the outputs and the sort's digits: the call's one mid-way host read
  uint32_t ng = 0;
  e = hipMemcpyAsync(&ng, a.rank + n, sizeof ng, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) return hip_err(ctx, e, "traj count");
  if (ng < 1 || (int64_t)ng > n) return set_err(ctx, GF_ERR_HIP, std::string(who) + ": inconsistent trajectory count");
  if ((st = K.keys.reserve(ctx, ng))) return st;
  a.keys = K.keys.p;
  a.ntraj = ng;
  if ((e = launch_traj_group(ctx, kTrajGroupAssign, a)) != hipSuccess) return hip_err(ctx, e, "traj assign");
  K.ngroups = ng;
  return GF_OK;
}

// One stable LSD radix sort in K's workspace: keys[0, n) of `bits` bits with the values vals (null: the
// index is the position), by digits of <= kRadixMaxBits bits.  The sorted values land in vout, the
// sorted keys in K.kbuf[K.sorted_in].  Enqueued.
static int radix_sort(gf_ctx* ctx, KeyGroups& K, const uint32_t* keys, const uint32_t* vals, int bits, int64_t n,
                      uint32_t* vout) {
  int st = GF_OK;
  const int passes = (bits + kRadixMaxBits - 1) / kRadixMaxBits, pbits = (bits + passes - 1) / passes;
  const int blocks = radix_blocks(ctx, n);
  const size_t w = (size_t)n + 1, mat = ((size_t)1 << pbits) * (size_t)blocks;
  if ((st = K.kbuf[0].reserve(ctx, w)) || (st = K.kbuf[1].reserve(ctx, w)) || (st = K.vbuf[0].reserve(ctx, w)) ||
      (st = K.vbuf[1].reserve(ctx, w)) || (st = K.mat.reserve(ctx, mat)) || (st = K.mats.reserve(ctx, mat + 1)))
    return st;
  RadixArgs r{};
  r.tile = radix_tile();
  r.n = n;
  r.bits = pbits;
  r.nblk = blocks;
  r.M = K.mat.p;
  r.Ms = K.mats.p;
  for (int p = 0; p < passes; ++p) {
    r.kin = p == 0 ? keys : K.kbuf[(p - 1) & 1].p;
    r.vin = p == 0 ? vals : K.vbuf[(p - 1) & 1].p;
    r.kout = K.kbuf[p & 1].p;
    r.vout = p == passes - 1 ? vout : K.vbuf[p & 1].p;
    r.shift = p * pbits;
    GF_HIP_CHECK(ctx, launch_radix(ctx, 0, r, blocks));  // histogram
    if ((st = group_scan_u32(ctx, K, r.M, (int64_t)mat, K.mats.p))) return st;
    GF_HIP_CHECK(ctx, launch_radix(ctx, 1, r, blocks));  // scatter
  }
  K.sorted_in = (passes - 1) & 1;
  return GF_OK;
}

int gf::group_sort_ids(gf_ctx* ctx, KeyGroups& K, const uint32_t* ids, int64_t n, uint32_t nids) {
  int st = GF_OK;
  if ((st = K.perm.reserve(ctx, (size_t)n + 1)) || (st = K.seg_off.reserve(ctx, (size_t)nids + 1)) ||
      (st = radix_sort(ctx, K, ids, nullptr, key_bits(nids), n, K.perm.p)))
    return st;
  TrajGroupArgs a{};
  a.n = n;
  a.ntraj = nids;
  a.sorted = K.kbuf[K.sorted_in].p;
  a.seg_off = K.seg_off.p;
  const hipError_t e = launch_traj_group(ctx, kTrajGroupBounds, a);
  return e == hipSuccess ? GF_OK : hip_err(ctx, e, "traj bounds");
}

int gf::group_sort_words(gf_ctx* ctx, KeyGroups& K, DevArr<uint32_t>& wkey, DevArr<uint32_t> sp[2], const SortWord* words,
                         int nwords, int64_t cnt, const uint32_t* start, const uint32_t** out) {
  int st = GF_OK;
  const size_t w = (size_t)cnt + 1;
  if ((st = wkey.reserve(ctx, w)) || (st = sp[0].reserve(ctx, w)) || (st = sp[1].reserve(ctx, w))) return st;
  const uint32_t* cur = start;  // the current order (null: the identity)
  for (int iw = 0; iw < nwords; ++iw) {
    const SortWord& W = words[iw];
    GF_HIP_CHECK(ctx, launch_tknn_word(ctx, W.src, W.index, W.shift, cur, cnt, wkey.p));
    uint32_t* next = sp[iw & 1].p;
    if ((st = radix_sort(ctx, K, wkey.p, cur, W.bits, cnt, next))) return st;
    cur = next;
  }
  *out = cur;
  return GF_OK;
}

extern "C" int gf_traj_group(gf_ctx* ctx, const gf_points* pts, gf_traj_groups** out) {
  if (!ctx || !out || !pts) return set_err(ctx, GF_ERR_ARG, "gf_traj_group: null argument");
  if (pts->n < 0 || pts->n > (int64_t)UINT32_MAX) return set_err(ctx, GF_ERR_ARG, "gf_traj_group: need 0 <= n < 2^32");
  if (pts->n > 0 && !pts->objID) return set_err(ctx, GF_ERR_ARG, "gf_traj_group: null objID");
  if (*out && (*out)->ctx != ctx) return set_err(ctx, GF_ERR_ARG, "gf_traj_group: groups of another context");
  int st = bind(ctx);
  if (st) return st;
  const bool fresh = *out == nullptr;
  gf_traj_groups* G = fresh ? new gf_traj_groups() : *out;
  G->ctx = ctx;
  auto fail = [&](int code) {
    if (fresh) gf_traj_groups_destroy(G);
    else G->n = G->ntraj = G->ngroups = 0;
    return code;
  };
  const int64_t n = pts->n;
  G->n = n;
  G->ntraj = G->ngroups = 0;
  if ((st = G->seg_off.reserve(ctx, 1))) return fail(st);
  if (n == 0) {
    hipError_t e = hipMemsetAsync(G->seg_off.p, 0, sizeof(uint32_t), ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return fail(hip_err(ctx, e, "gf_traj_group"));
    *out = G;
    return GF_OK;
  }
  if ((st = group_dense_ids(ctx, *G, pts->objID, n, "gf_traj_group")) ||
      (st = group_sort_ids(ctx, *G, G->did.p, n, (uint32_t)G->ngroups)))
    return fail(st);
  hipError_t e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) return fail(hip_err(ctx, e, "gf_traj_group"));
  G->ntraj = G->ngroups;
  *out = G;
  return GF_OK;
}

extern "C" void gf_traj_groups_destroy(gf_traj_groups* G) {
  if (!G) return;
  if (G->ctx) {
    hipSetDevice(G->ctx->device);
    hipStreamSynchronize(G->ctx->stream);
  }
  delete G;
}

extern "C" int gf_traj_groups_info(const gf_traj_groups* G, int64_t* ntraj, int64_t* n) {
  if (!G) return GF_ERR_ARG;
  if (ntraj) *ntraj = G->ntraj;
  if (n) *n = G->n;
  return GF_OK;
}

extern "C" int gf_traj_groups_set_long_threshold(gf_traj_groups* G, int64_t len) {
  if (!G || len < 0 || len > (int64_t)UINT32_MAX) return GF_ERR_ARG;
  G->long_len = len == 0 ? kTrajLongLen : len;
  return GF_OK;
}

extern "C" int gf_traj_groups_read(gf_traj_groups* G, int64_t* keys, int64_t* seg_off, uint32_t* perm) {
  if (!G) return GF_ERR_ARG;
  gf_ctx* ctx = G->ctx;
  int st = bind(ctx);
  if (st) return st;
  OffsetRead so;
  if ((st = read_back(ctx, keys, G->keys.p, (size_t)G->ntraj)) ||
      (st = read_offsets(ctx, so, seg_off, G->seg_off.p, (size_t)G->ntraj + 1)) ||
      (st = read_back(ctx, perm, G->perm.p, (size_t)G->n)))
    return st;
  GF_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  so.widen();
  return GF_OK;
}

// the grouped window again, with the columns tStats / the extraction read
int gf::traj_check_points(gf_traj_groups* G, const gf_points* pts, const char* who) {
  gf_ctx* ctx = G->ctx;
  if (!pts || pts->n != G->n) return set_err(ctx, GF_ERR_ARG, std::string(who) + ": pts is not the grouped window");
  if (pts->n > 0 && (!pts->x || !pts->y || !pts->ts)) return set_err(ctx, GF_ERR_ARG, std::string(who) + ": null x / y / ts");
  return GF_OK;
}

// trajIDSet: the sorted distinct ids of id_set[0, nset), nset > 0, in G->set; *count = how many
static int upload_id_set(gf_traj_groups* G, const int64_t* id_set, int64_t nset, int64_t* count) {
  std::vector<int64_t> set(id_set, id_set + nset);
  std::sort(set.begin(), set.end());
  set.erase(std::unique(set.begin(), set.end()), set.end());
  *count = (int64_t)set.size();
  return upload(G->ctx, G->set, set);  // (a pageable source: the copy has left `set` when the call returns)
}

extern "C" int gf_tstats_run(gf_traj_groups* G, const gf_points* pts, const int64_t* id_set, int64_t nset, int64_t* keys,
                             double* spatial, int64_t* temporal, double* speed, int64_t cap, int64_t* count) {
  if (!G || !G->ctx) return GF_ERR_ARG;
  gf_ctx* ctx = G->ctx;
  if (!count || cap < 0 || nset < 0 || (nset > 0 && !id_set)) return set_err(ctx, GF_ERR_ARG, "gf_tstats_run: bad argument");
  int st = traj_check_points(G, pts, "gf_tstats_run");
  if (st) return st;
  *count = 0;
  const int64_t nt = G->ntraj;
  if (nt == 0) return GF_OK;
  if ((st = bind(ctx))) return st;
  const size_t m = (size_t)nt;
  if ((st = G->S.reserve(ctx, m)) || (st = G->T.reserve(ctx, m)) || (st = G->V.reserve(ctx, m)) ||
      (st = G->long_list.reserve(ctx, m)) || (st = G->counters.reserve(ctx, kCounterWords)))
    return st;
  TStatsArgs a{};
  a.x = pts->x; a.y = pts->y; a.ts = pts->ts;
  a.perm = G->perm.p;
  a.seg_off = G->seg_off.p;
  a.ntraj = nt;
  a.long_len = (uint32_t)G->long_len;
  a.S = G->S.p; a.T = G->T.p; a.V = G->V.p;
  a.long_list = G->long_list.p;
  a.long_count = G->counters.p;
  GF_HIP_CHECK(ctx, hipMemsetAsync(a.long_count, 0, kCounterWords * sizeof(uint32_t), ctx->stream));
  GF_HIP_CHECK(ctx, launch_tstats(ctx, a));
  const int64_t* dk = G->keys.p;
  const double *dS = a.S, *dV = a.V;
  const int64_t* dT = a.T;
  int64_t rows = nt;
  if (nset > 0) {  // trajIDSet: the rows whose key is in the set, packed in order
    int64_t ids = 0;
    if ((st = upload_id_set(G, id_set, nset, &ids)) || (st = G->sel.reserve(ctx, m + 1)) ||
        (st = G->srank.reserve(ctx, m + 1)) || (st = G->ck.reserve(ctx, m)) || (st = G->cS.reserve(ctx, m)) ||
        (st = G->cT.reserve(ctx, m)) || (st = G->cV.reserve(ctx, m)))
      return st;
    uint32_t* sel = G->sel.p;
    uint32_t* srank = G->srank.p;
    GF_HIP_CHECK(ctx, launch_tstats_filter(ctx, a, dk, G->set.p, ids, sel, srank, nullptr, nullptr, nullptr, nullptr,
                                           kTStatsFilterMark));
    if ((st = group_scan_u32(ctx, *G, sel, nt, srank))) return st;
    GF_HIP_CHECK(ctx, launch_tstats_filter(ctx, a, dk, nullptr, 0, sel, srank, G->ck.p, G->cS.p, G->cT.p, G->cV.p,
                                           kTStatsFilterPack));
    uint32_t r = 0;
    GF_HIP_CHECK(ctx, hipMemcpyAsync(&r, srank + nt, sizeof r, hipMemcpyDeviceToHost, ctx->stream));
    GF_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    rows = r;
    dk = G->ck.p; dS = G->cS.p; dT = G->cT.p; dV = G->cV.p;
  }
  const size_t wr = (size_t)std::min(rows, cap);
  if ((st = read_back(ctx, keys, dk, wr)) || (st = read_back(ctx, spatial, dS, wr)) ||
      (st = read_back(ctx, temporal, dT, wr)) || (st = read_back(ctx, speed, dV, wr)))
    return st;
  GF_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  *count = rows;
  return GF_OK;
}

int gf::traj_hit_clear(gf_traj_groups* G) {
  gf_ctx* ctx = G->ctx;
  const size_t m = (size_t)G->ntraj;
  if (int st = G->hit.reserve(ctx, m + 1)) return st;
  GF_HIP_CHECK(ctx, hipMemsetAsync(G->hit.p, 0, (m + 1) * sizeof(uint32_t), ctx->stream));
  return GF_OK;
}

// The sub-trajectories of G->hit (one flag per trajectory, entry ntraj zero; ntraj > 0): lengths, the
// two scans, the gather, the read-back.  gf_traj_select, gf_trange_run (trange.cpp) and gf_tfilter_run
// end here.  Sync.
int gf::traj_emit(gf_traj_groups* G, const gf_points* pts, int64_t* keys, int64_t* off, int64_t cap_traj, double* x,
                  double* y, int64_t* ts, uint32_t* idx, int64_t cap_pts, int64_t* ntraj_out, int64_t* npts_out) {
  gf_ctx* ctx = G->ctx;
  int st = GF_OK;
  const int64_t nt = G->ntraj, n = G->n;
  const size_t m = (size_t)nt, np = (size_t)n;
  if ((st = G->hit.reserve(ctx, m + 1)) || (st = G->len.reserve(ctx, m + 1)) || (st = G->row.reserve(ctx, m + 1)) ||
      (st = G->off.reserve(ctx, m + 1)) || (st = G->okeys.reserve(ctx, m)) || (st = G->ooff.reserve(ctx, m + 1)) ||
      (st = G->ox.reserve(ctx, np)) || (st = G->oy.reserve(ctx, np)) || (st = G->ots.reserve(ctx, np)) ||
      (st = G->oidx.reserve(ctx, np)))
    return st;
  TrajSelectArgs a{};
  a.x = pts->x; a.y = pts->y; a.ts = pts->ts;
  a.n = n; a.ntraj = nt;
  a.sorted = G->kbuf[G->sorted_in].p;
  a.perm = G->perm.p;
  a.seg_off = G->seg_off.p;
  a.keys = G->keys.p;
  a.hit = G->hit.p;
  a.len = G->len.p;
  a.row = G->row.p;
  a.off = G->off.p;
  a.okeys = G->okeys.p;
  a.ooff = G->ooff.p;
  a.ox = G->ox.p; a.oy = G->oy.p; a.ots = G->ots.p; a.oidx = G->oidx.p;
  GF_HIP_CHECK(ctx, launch_traj_select(ctx, kTrajSelectLens, a));
  if ((st = group_scan_u32(ctx, *G, a.hit, nt, G->row.p)) || (st = group_scan_u32(ctx, *G, a.len, nt, G->off.p)))
    return st;
  GF_HIP_CHECK(ctx, launch_traj_select(ctx, kTrajSelectGather, a));
  uint32_t tot[2] = {0, 0};
  GF_HIP_CHECK(ctx, hipMemcpyAsync(&tot[0], a.row + nt, sizeof tot[0], hipMemcpyDeviceToHost, ctx->stream));
  GF_HIP_CHECK(ctx, hipMemcpyAsync(&tot[1], a.off + nt, sizeof tot[1], hipMemcpyDeviceToHost, ctx->stream));
  GF_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  const size_t wt = (size_t)std::min<int64_t>(tot[0], cap_traj), wp = (size_t)std::min<int64_t>(tot[1], cap_pts);
  OffsetRead ho;
  if ((st = read_back(ctx, keys, G->okeys.p, wt)) || (st = read_offsets(ctx, ho, off, G->ooff.p, wt + 1)) ||
      (st = read_back(ctx, x, G->ox.p, wp)) || (st = read_back(ctx, y, G->oy.p, wp)) || (st = read_back(ctx, ts, G->ots.p, wp)) ||
      (st = read_back(ctx, idx, G->oidx.p, wp)))
    return st;
  GF_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  ho.widen();
  *ntraj_out = tot[0];
  *npts_out = tot[1];
  return GF_OK;
}

extern "C" int gf_traj_select(gf_traj_groups* G, const gf_points* pts, const uint64_t* bitmap, int64_t* keys, int64_t* off,
                              int64_t cap_traj, double* x, double* y, int64_t* ts, uint32_t* idx, int64_t cap_pts,
                              int64_t* ntraj_out, int64_t* npts_out) {
  if (!G || !G->ctx) return GF_ERR_ARG;
  gf_ctx* ctx = G->ctx;
  if (!ntraj_out || !npts_out || cap_traj < 0 || cap_pts < 0 || (G->n > 0 && !bitmap))
    return set_err(ctx, GF_ERR_ARG, "gf_traj_select: bad argument");
  int st = traj_check_points(G, pts, "gf_traj_select");
  if (st) return st;
  *ntraj_out = 0;
  *npts_out = 0;
  if (off) off[0] = 0;
  if (G->ntraj == 0) return GF_OK;
  if ((st = bind(ctx)) || (st = traj_hit_clear(G))) return st;
  TrajSelectArgs a{};
  a.n = G->n;
  a.bitmap = bitmap;
  a.did = G->did.p;
  a.hit = G->hit.p;
  GF_HIP_CHECK(ctx, launch_traj_select(ctx, kTrajSelectHit, a));
  return traj_emit(G, pts, keys, off, cap_traj, x, y, ts, idx, cap_pts, ntraj_out, npts_out);
}

// tFilter/PointTFilterQuery.java windowBased: the trajectories whose key is in the set, whole; an empty
// set is every trajectory (:92-95).  The membership test is gf_tstats_run's binary search.
extern "C" int gf_tfilter_run(gf_traj_groups* G, const gf_points* pts, const int64_t* id_set, int64_t nset, int64_t* keys,
                              int64_t* off, int64_t cap_traj, double* x, double* y, int64_t* ts, uint32_t* idx,
                              int64_t cap_pts, int64_t* ntraj_out, int64_t* npts_out) {
  if (!G || !G->ctx) return GF_ERR_ARG;
  gf_ctx* ctx = G->ctx;
  if (!ntraj_out || !npts_out || cap_traj < 0 || cap_pts < 0 || nset < 0 || (nset > 0 && !id_set))
    return set_err(ctx, GF_ERR_ARG, "gf_tfilter_run: bad argument");
  int st = traj_check_points(G, pts, "gf_tfilter_run");
  if (st) return st;
  *ntraj_out = 0;
  *npts_out = 0;
  if (off) off[0] = 0;
  const int64_t nt = G->ntraj;
  if (nt == 0) return GF_OK;
  if ((st = bind(ctx)) || (st = traj_hit_clear(G))) return st;
  if (nset == 0) {
    GF_HIP_CHECK(ctx, hipMemsetD32Async((hipDeviceptr_t)G->hit.p, 1, (size_t)nt, ctx->stream));
  } else {
    int64_t ids = 0;
    if ((st = upload_id_set(G, id_set, nset, &ids))) return st;
    TStatsArgs a{};
    a.ntraj = nt;
    GF_HIP_CHECK(ctx, launch_tstats_filter(ctx, a, G->keys.p, G->set.p, ids, G->hit.p, nullptr, nullptr, nullptr, nullptr,
                                           nullptr, kTStatsFilterMark));
  }
  return traj_emit(G, pts, keys, off, cap_traj, x, y, ts, idx, cap_pts, ntraj_out, npts_out);
}
