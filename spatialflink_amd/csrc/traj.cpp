// traj.cpp -- trajectory entry points of the C ABI: gf_traj_group (a window grouped by objID),
// gf_tstats_run (TStatsQuery.java:154-188 per trajectory), gf_traj_select (sub-trajectories of a
// hit bitmap).  The kernels are in k_traj.hip; the stable sort by dense trajectory id reuses the
// LSD radix passes of k_points.hip.  The groups object owns its device workspace (grow-only) and is
// reused across windows.  The grouping itself -- dense ids of a device int64 key column, then the
// stable sort by them -- is gf_group.hpp's, shared with tagg.cpp.
#define GF_TU_NAME traj_cpp
#include "gf_buildtag.hpp"  // first: records this unit's command-line defines

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "gf_group.hpp"

using namespace gf;

static int scan_u32(gf_traj_groups* G, const uint32_t* in, int64_t L, uint32_t* out) {
  return group_scan_u32(G->ctx, *G, in, L, out);
}

// ---- gf_group.hpp: the grouping of a device int64 key column ----------------------------------
int gf::group_scan_u32(gf_ctx* ctx, KeyGroups& K, const uint32_t* in, int64_t L, uint32_t* out) {
  if (int st = K.scan_tmp.reserve(ctx, scan_tmp_elems(L) * sizeof(uint32_t))) return st;
  GF_HIP_CHECK(ctx, launch_exclusive_scan(ctx->stream, in, L, out, K.scan_tmp.as<uint32_t>()));
  return GF_OK;
}

int gf::group_dense_ids(gf_ctx* ctx, KeyGroups& K, const int64_t* key, int64_t n, const char* who) {
  int st = GF_OK;
  K.n = n;
  K.ngroups = 0;
  uint64_t slots = 64;
  while (slots < 2 * (uint64_t)n) slots <<= 1;
  const size_t w = sizeof(uint32_t) * (size_t)(n + 1);
  if ((st = K.tkey.reserve(ctx, (slots + 1) * sizeof(unsigned long long))) ||
      (st = K.tfirst.reserve(ctx, (slots + 1) * sizeof(uint32_t))) || (st = K.kbuf[1].reserve(ctx, w)) ||
      (st = K.vbuf[1].reserve(ctx, w)) || (st = K.did.reserve(ctx, w)))
    return st;
  TrajGroupArgs a{};
  a.t.key = K.tkey.as<unsigned long long>();
  a.t.first = K.tfirst.as<uint32_t>();
  a.t.mask = slots - 1;
  a.objID = key;
  a.n = n;
  a.flag = K.kbuf[1].as<uint32_t>();
  a.rank = K.vbuf[1].as<uint32_t>();
  a.did = K.did.as<uint32_t>();
  hipError_t e = launch_traj_group(ctx, 0, a);
  if (e != hipSuccess) return hip_err(ctx, e, "traj insert");
  if ((st = group_scan_u32(ctx, K, a.flag, n, K.vbuf[1].as<uint32_t>()))) return st;
  // the group count sizes the outputs and the sort's digits: the call's one mid-way host read
  uint32_t ng = 0;
  e = hipMemcpyAsync(&ng, a.rank + n, sizeof ng, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) return hip_err(ctx, e, "traj count");
  if (ng < 1 || (int64_t)ng > n) return set_err(ctx, GF_ERR_HIP, std::string(who) + ": inconsistent trajectory count");
  if ((st = K.keys.reserve(ctx, sizeof(int64_t) * (size_t)ng))) return st;
  a.keys = K.keys.as<int64_t>();
  a.ntraj = ng;
  if ((e = launch_traj_group(ctx, 1, a)) != hipSuccess) return hip_err(ctx, e, "traj assign");
  K.ngroups = ng;
  return GF_OK;
}

int gf::group_sort_ids(gf_ctx* ctx, KeyGroups& K, const uint32_t* ids, int64_t n, uint32_t nids) {
  int st = GF_OK;
  const size_t w = sizeof(uint32_t) * (size_t)(n + 1);
  if ((st = K.kbuf[0].reserve(ctx, w)) || (st = K.kbuf[1].reserve(ctx, w)) || (st = K.vbuf[0].reserve(ctx, w)) ||
      (st = K.vbuf[1].reserve(ctx, w)) || (st = K.perm.reserve(ctx, w)) ||
      (st = K.seg_off.reserve(ctx, sizeof(uint32_t) * ((size_t)nids + 1))))
    return st;
  // stable LSD radix over the dense ids (ids < nids): digits of <= kRadixMaxBits bits
  int bits = 1;
  while (((uint64_t)1 << bits) < (uint64_t)nids) ++bits;
  const int passes = (bits + kRadixMaxBits - 1) / kRadixMaxBits, pbits = (bits + passes - 1) / passes;
  const int blocks = radix_blocks(ctx, n);
  const int64_t mat = ((int64_t)1 << pbits) * blocks;
  if ((st = K.mat.reserve(ctx, sizeof(uint32_t) * (size_t)mat)) ||
      (st = K.mats.reserve(ctx, sizeof(uint32_t) * (size_t)(mat + 1))))
    return st;
  RadixArgs r{};
  r.tile = radix_tile();
  r.n = n;
  r.bits = pbits;
  r.nblk = blocks;
  r.M = K.mat.as<uint32_t>();
  r.Ms = K.mats.as<uint32_t>();
  hipError_t e;
  for (int p = 0; p < passes; ++p) {
    r.kin = p == 0 ? ids : K.kbuf[(p - 1) & 1].as<uint32_t>();
    r.vin = p == 0 ? nullptr : K.vbuf[(p - 1) & 1].as<uint32_t>();  // pass 0: the index is the position
    r.kout = K.kbuf[p & 1].as<uint32_t>();
    r.vout = p == passes - 1 ? K.perm.as<uint32_t>() : K.vbuf[p & 1].as<uint32_t>();
    r.shift = p * pbits;
    if ((e = launch_radix(ctx, 0, r, blocks)) != hipSuccess) return hip_err(ctx, e, "traj radix histogram");
    if ((st = group_scan_u32(ctx, K, r.M, mat, K.mats.as<uint32_t>()))) return st;
    if ((e = launch_radix(ctx, 1, r, blocks)) != hipSuccess) return hip_err(ctx, e, "traj radix scatter");
  }
  K.sorted_in = (passes - 1) & 1;
  TrajGroupArgs a{};
  a.n = n;
  a.ntraj = nids;
  a.sorted = K.kbuf[K.sorted_in].as<uint32_t>();
  a.seg_off = K.seg_off.as<uint32_t>();
  if ((e = launch_traj_group(ctx, 2, a)) != hipSuccess) return hip_err(ctx, e, "traj bounds");
  return GF_OK;
}

int gf::group_sort_words(gf_ctx* ctx, KeyGroups& K, DevBuf& wkey, DevBuf sp[2], const SortWord* words, int nwords,
                         int64_t cnt, const uint32_t* start, const uint32_t** out) {
  int st = GF_OK;
  const size_t w = sizeof(uint32_t) * (size_t)(cnt + 1);
  if ((st = K.kbuf[0].reserve(ctx, w)) || (st = K.kbuf[1].reserve(ctx, w)) || (st = K.vbuf[0].reserve(ctx, w)) ||
      (st = K.vbuf[1].reserve(ctx, w)) || (st = wkey.reserve(ctx, w)) || (st = sp[0].reserve(ctx, w)) ||
      (st = sp[1].reserve(ctx, w)))
    return st;
  const int blocks = radix_blocks(ctx, cnt);
  const uint32_t* cur = start;  // the current order (null: the identity)
  int next = 0;
  for (int iw = 0; iw < nwords; ++iw) {
    const SortWord& W = words[iw];
    const int passes = (W.bits + kRadixMaxBits - 1) / kRadixMaxBits, pbits = (W.bits + passes - 1) / passes;
    const int64_t mat = ((int64_t)1 << pbits) * blocks;
    if ((st = K.mat.reserve(ctx, sizeof(uint32_t) * (size_t)mat)) ||
        (st = K.mats.reserve(ctx, sizeof(uint32_t) * (size_t)(mat + 1))))
      return st;
    GF_HIP_CHECK(ctx, launch_tknn_word(ctx, W.src, W.index, W.shift, cur, cnt, wkey.as<uint32_t>()));
    RadixArgs r{};
    r.tile = radix_tile();
    r.n = cnt;
    r.bits = pbits;
    r.nblk = blocks;
    r.M = K.mat.as<uint32_t>();
    r.Ms = K.mats.as<uint32_t>();
    for (int p = 0; p < passes; ++p) {
      r.kin = p == 0 ? wkey.as<uint32_t>() : K.kbuf[(p - 1) & 1].as<uint32_t>();
      r.vin = p == 0 ? cur : K.vbuf[(p - 1) & 1].as<uint32_t>();  // null: the index is the position
      r.kout = K.kbuf[p & 1].as<uint32_t>();
      r.vout = p == passes - 1 ? sp[next].as<uint32_t>() : K.vbuf[p & 1].as<uint32_t>();
      r.shift = p * pbits;
      GF_HIP_CHECK(ctx, launch_radix(ctx, 0, r, blocks));
      if ((st = group_scan_u32(ctx, K, r.M, mat, K.mats.as<uint32_t>()))) return st;
      GF_HIP_CHECK(ctx, launch_radix(ctx, 1, r, blocks));
    }
    cur = sp[next].as<uint32_t>();
    next ^= 1;
  }
  *out = cur;
  return GF_OK;
}

template <class T>
static int read_back(gf_ctx* ctx, T* host, const void* dev, size_t count) {
  if (!host || count == 0) return GF_OK;
  GF_HIP_CHECK(ctx, hipMemcpyAsync(host, dev, count * sizeof(T), hipMemcpyDeviceToHost, ctx->stream));
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
  if ((st = G->seg_off.reserve(ctx, sizeof(uint32_t)))) return fail(st);
  if (n == 0) {
    hipError_t e = hipMemsetAsync(G->seg_off.p, 0, sizeof(uint32_t), ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return fail(hip_err(ctx, e, "gf_traj_group"));
    *out = G;
    return GF_OK;
  }
  if ((st = group_dense_ids(ctx, *G, pts->objID, n, "gf_traj_group")) ||
      (st = group_sort_ids(ctx, *G, G->did.as<uint32_t>(), n, (uint32_t)G->ngroups)))
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
  G->release_groups();
  for (DevBuf** b = G->all; *b; ++b) (*b)->release();
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
  std::vector<uint32_t> so;
  if (seg_off) so.resize((size_t)G->ntraj + 1);
  if ((st = read_back(ctx, keys, G->keys.p, (size_t)G->ntraj)) ||
      (st = read_back(ctx, seg_off ? so.data() : nullptr, G->seg_off.p, so.size())) ||
      (st = read_back(ctx, perm, G->perm.p, (size_t)G->n)))
    return st;
  GF_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  for (size_t i = 0; i < so.size(); ++i) seg_off[i] = (int64_t)so[i];
  return GF_OK;
}

// the grouped window again, with the columns tStats / the extraction read
static int check_traj_points(gf_traj_groups* G, const gf_points* pts, const char* who) {
  gf_ctx* ctx = G->ctx;
  if (!pts || pts->n != G->n) return set_err(ctx, GF_ERR_ARG, std::string(who) + ": pts is not the grouped window");
  if (pts->n > 0 && (!pts->x || !pts->y || !pts->ts)) return set_err(ctx, GF_ERR_ARG, std::string(who) + ": null x / y / ts");
  return GF_OK;
}

extern "C" int gf_tstats_run(gf_traj_groups* G, const gf_points* pts, const int64_t* id_set, int64_t nset, int64_t* keys,
                             double* spatial, int64_t* temporal, double* speed, int64_t cap, int64_t* count) {
  if (!G || !G->ctx) return GF_ERR_ARG;
  gf_ctx* ctx = G->ctx;
  if (!count || cap < 0 || nset < 0 || (nset > 0 && !id_set)) return set_err(ctx, GF_ERR_ARG, "gf_tstats_run: bad argument");
  int st = check_traj_points(G, pts, "gf_tstats_run");
  if (st) return st;
  *count = 0;
  const int64_t nt = G->ntraj;
  if (nt == 0) return GF_OK;
  if ((st = bind(ctx))) return st;
  const size_t m = (size_t)nt;
  if ((st = G->S.reserve(ctx, m * 8)) || (st = G->T.reserve(ctx, m * 8)) || (st = G->V.reserve(ctx, m * 8)) ||
      (st = G->long_list.reserve(ctx, m * 4)) || (st = G->counters.reserve(ctx, 16)))
    return st;
  TStatsArgs a{};
  a.x = pts->x; a.y = pts->y; a.ts = pts->ts;
  a.perm = G->perm.as<uint32_t>();
  a.seg_off = G->seg_off.as<uint32_t>();
  a.ntraj = nt;
  a.long_len = (uint32_t)G->long_len;
  a.S = G->S.as<double>(); a.T = G->T.as<int64_t>(); a.V = G->V.as<double>();
  a.long_list = G->long_list.as<uint32_t>();
  a.long_count = G->counters.as<uint32_t>();
  GF_HIP_CHECK(ctx, hipMemsetAsync(a.long_count, 0, 16, ctx->stream));
  GF_HIP_CHECK(ctx, launch_tstats(ctx, a));
  const int64_t* dk = G->keys.as<int64_t>();
  const double *dS = a.S, *dV = a.V;
  const int64_t* dT = a.T;
  int64_t rows = nt;
  if (nset > 0) {  // trajIDSet: the rows whose key is in the set, packed in order
    std::vector<int64_t> set(id_set, id_set + nset);
    std::sort(set.begin(), set.end());
    set.erase(std::unique(set.begin(), set.end()), set.end());
    if ((st = G->set.reserve(ctx, set.size() * 8)) || (st = G->sel.reserve(ctx, (m + 1) * 4)) ||
        (st = G->srank.reserve(ctx, (m + 1) * 4)) || (st = G->ck.reserve(ctx, m * 8)) || (st = G->cS.reserve(ctx, m * 8)) ||
        (st = G->cT.reserve(ctx, m * 8)) || (st = G->cV.reserve(ctx, m * 8)))
      return st;
    // (a pageable source: the copy has left `set` when the call returns)
    GF_HIP_CHECK(ctx, hipMemcpy(G->set.p, set.data(), set.size() * 8, hipMemcpyHostToDevice));
    uint32_t* sel = G->sel.as<uint32_t>();
    uint32_t* srank = G->srank.as<uint32_t>();
    GF_HIP_CHECK(ctx, launch_tstats_filter(ctx, a, dk, G->set.as<int64_t>(), (int64_t)set.size(), sel, srank, nullptr,
                                           nullptr, nullptr, nullptr, 0));
    if ((st = scan_u32(G, sel, nt, srank))) return st;
    GF_HIP_CHECK(ctx, launch_tstats_filter(ctx, a, dk, nullptr, 0, sel, srank, G->ck.as<int64_t>(), G->cS.as<double>(),
                                           G->cT.as<int64_t>(), G->cV.as<double>(), 1));
    uint32_t r = 0;
    GF_HIP_CHECK(ctx, hipMemcpyAsync(&r, srank + nt, sizeof r, hipMemcpyDeviceToHost, ctx->stream));
    GF_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    rows = r;
    dk = G->ck.as<int64_t>(); dS = G->cS.as<double>(); dT = G->cT.as<int64_t>(); dV = G->cV.as<double>();
  }
  const size_t wr = (size_t)std::min(rows, cap);
  if ((st = read_back(ctx, keys, dk, wr)) || (st = read_back(ctx, spatial, dS, wr)) ||
      (st = read_back(ctx, temporal, dT, wr)) || (st = read_back(ctx, speed, dV, wr)))
    return st;
  GF_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  *count = rows;
  return GF_OK;
}

int gf::traj_check_points(gf_traj_groups* G, const gf_points* pts, const char* who) { return check_traj_points(G, pts, who); }

int gf::traj_hit_clear(gf_traj_groups* G) {
  gf_ctx* ctx = G->ctx;
  const size_t m = (size_t)G->ntraj;
  if (int st = G->hit.reserve(ctx, (m + 1) * 4)) return st;
  GF_HIP_CHECK(ctx, hipMemsetAsync(G->hit.p, 0, (m + 1) * 4, ctx->stream));
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
  if ((st = G->hit.reserve(ctx, (m + 1) * 4)) || (st = G->len.reserve(ctx, (m + 1) * 4)) ||
      (st = G->row.reserve(ctx, (m + 1) * 4)) || (st = G->off.reserve(ctx, (m + 1) * 4)) ||
      (st = G->okeys.reserve(ctx, m * 8)) || (st = G->ooff.reserve(ctx, (m + 1) * 4)) || (st = G->ox.reserve(ctx, np * 8)) ||
      (st = G->oy.reserve(ctx, np * 8)) || (st = G->ots.reserve(ctx, np * 8)) || (st = G->oidx.reserve(ctx, np * 4)))
    return st;
  TrajSelectArgs a{};
  a.x = pts->x; a.y = pts->y; a.ts = pts->ts;
  a.n = n; a.ntraj = nt;
  a.sorted = G->kbuf[G->sorted_in].as<uint32_t>();
  a.perm = G->perm.as<uint32_t>();
  a.seg_off = G->seg_off.as<uint32_t>();
  a.keys = G->keys.as<int64_t>();
  a.hit = G->hit.as<uint32_t>();
  a.len = G->len.as<uint32_t>();
  a.row = G->row.as<uint32_t>();
  a.off = G->off.as<uint32_t>();
  a.okeys = G->okeys.as<int64_t>();
  a.ooff = G->ooff.as<uint32_t>();
  a.ox = G->ox.as<double>(); a.oy = G->oy.as<double>(); a.ots = G->ots.as<int64_t>(); a.oidx = G->oidx.as<uint32_t>();
  GF_HIP_CHECK(ctx, launch_traj_select(ctx, 2, a));
  if ((st = scan_u32(G, a.hit, nt, G->row.as<uint32_t>())) || (st = scan_u32(G, a.len, nt, G->off.as<uint32_t>())))
    return st;
  GF_HIP_CHECK(ctx, launch_traj_select(ctx, 1, a));
  uint32_t tot[2] = {0, 0};
  GF_HIP_CHECK(ctx, hipMemcpyAsync(&tot[0], a.row + nt, 4, hipMemcpyDeviceToHost, ctx->stream));
  GF_HIP_CHECK(ctx, hipMemcpyAsync(&tot[1], a.off + nt, 4, hipMemcpyDeviceToHost, ctx->stream));
  GF_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  const size_t wt = (size_t)std::min<int64_t>(tot[0], cap_traj), wp = (size_t)std::min<int64_t>(tot[1], cap_pts);
  std::vector<uint32_t> ho;
  if (off) ho.resize(wt + 1);
  if ((st = read_back(ctx, keys, a.okeys, wt)) || (st = read_back(ctx, off ? ho.data() : nullptr, a.ooff, ho.size())) ||
      (st = read_back(ctx, x, a.ox, wp)) || (st = read_back(ctx, y, a.oy, wp)) || (st = read_back(ctx, ts, a.ots, wp)) ||
      (st = read_back(ctx, idx, a.oidx, wp)))
    return st;
  GF_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  for (size_t i = 0; i < ho.size(); ++i) off[i] = (int64_t)ho[i];
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
  int st = check_traj_points(G, pts, "gf_traj_select");
  if (st) return st;
  *ntraj_out = 0;
  *npts_out = 0;
  if (off) off[0] = 0;
  if (G->ntraj == 0) return GF_OK;
  if ((st = bind(ctx)) || (st = traj_hit_clear(G))) return st;
  TrajSelectArgs a{};
  a.n = G->n;
  a.bitmap = bitmap;
  a.did = G->did.as<uint32_t>();
  a.hit = G->hit.as<uint32_t>();
  GF_HIP_CHECK(ctx, launch_traj_select(ctx, 0, a));
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
  int st = check_traj_points(G, pts, "gf_tfilter_run");
  if (st) return st;
  *ntraj_out = 0;
  *npts_out = 0;
  if (off) off[0] = 0;
  const int64_t nt = G->ntraj;
  if (nt == 0) return GF_OK;
  if ((st = bind(ctx)) || (st = traj_hit_clear(G))) return st;
  uint32_t* hit = G->hit.as<uint32_t>();
  if (nset == 0) {
    GF_HIP_CHECK(ctx, hipMemsetD32Async((hipDeviceptr_t)hit, 1, (size_t)nt, ctx->stream));
  } else {
    std::vector<int64_t> set(id_set, id_set + nset);
    std::sort(set.begin(), set.end());
    set.erase(std::unique(set.begin(), set.end()), set.end());
    if ((st = G->set.reserve(ctx, set.size() * 8))) return st;
    // (a pageable source: the copy has left `set` when the call returns)
    GF_HIP_CHECK(ctx, hipMemcpy(G->set.p, set.data(), set.size() * 8, hipMemcpyHostToDevice));
    TStatsArgs a{};
    a.ntraj = nt;
    GF_HIP_CHECK(ctx, launch_tstats_filter(ctx, a, G->keys.as<int64_t>(), G->set.as<int64_t>(), (int64_t)set.size(), hit,
                                           nullptr, nullptr, nullptr, nullptr, nullptr, 0));
  }
  return traj_emit(G, pts, keys, off, cap_traj, x, y, ts, idx, cap_pts, ntraj_out, npts_out);
}
