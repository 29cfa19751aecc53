// gf_group.hpp -- "group a device int64 key column" as the host units share it (traj.cpp holds the
// bodies; the kernels are k_traj.hip's traj_* and k_points.hip's radix passes).  gf_traj_group is
// group_keys over objID; tagg.cpp groups by cell, by objID and by the (cell, objID) pair with it.
#pragma once

#include "gf_host.hpp"

namespace gf {

// a grow-only device buffer
struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  int reserve(gf_ctx* ctx, size_t need) {
    if (need <= bytes) return GF_OK;
    GF_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));  // queued work may still read the old one
    if (p) hipFree(p);
    p = nullptr;
    bytes = 0;
    GF_HIP_CHECK(ctx, hipMalloc(&p, need));
    bytes = need;
    return GF_OK;
  }
  void release() {
    if (p) hipFree(p);
    p = nullptr;
    bytes = 0;
  }
  template <class T>
  T* as() const { return (T*)p; }
};

// The workspace and the result of one grouping: n items, ngroups distinct keys.
//   keys[ngroups]        the distinct keys in first-occurrence order
//   did[n]               dense id per item
//   perm[n], seg_off[ngroups + 1], kbuf[sorted_in] = the sorted ids   (after group_sort_ids)
struct KeyGroups {
  int64_t n = 0, ngroups = 0;
  DevBuf tkey, tfirst;       // the hash table (+ the empty marker's slot)
  DevBuf kbuf[2], vbuf[2];   // radix ping-pong (n + 1 each); kbuf[1] = first-item flags, vbuf[1] = their scan
  DevBuf did, perm, keys, seg_off, mat, mats, scan_tmp;
  int sorted_in = 0;         // kbuf[sorted_in] = dense id per perm position
  void release_groups() {
    DevBuf* all[] = {&tkey, &tfirst, &kbuf[0], &kbuf[1], &vbuf[0], &vbuf[1], &did, &perm, &keys, &seg_off, &mat, &mats,
                     &scan_tmp};
    for (DevBuf* b : all) b->release();
  }
};

int group_scan_u32(gf_ctx* ctx, KeyGroups& K, const uint32_t* in, int64_t L, uint32_t* out);
// Dense ids of key[0, n) (device), 0 < n < 2^32: K.did, K.keys, K.ngroups; one mid-way host read (the
// group count).  Enqueued on the context stream; the outputs are complete after a stream sync.
int group_dense_ids(gf_ctx* ctx, KeyGroups& K, const int64_t* key, int64_t n, const char* who);
// Stable LSD radix of the items by ids[0, n) (device; every id in [0, nids) occurs): K.perm, the sorted
// ids (K.kbuf[K.sorted_in]) and K.seg_off[nids + 1].  Enqueued; ids may be K.did.
int group_sort_ids(gf_ctx* ctx, KeyGroups& K, const uint32_t* ids, int64_t n, uint32_t nids);

// One word of a multi-word key: item q's word = (uint32)(src[index ? index[q] : q] >> shift), `bits` wide.
struct SortWord {
  const unsigned long long* src;
  const uint32_t* index;
  int shift, bits;
};
// Stable LSD radix sort of the items [0, cnt) by the words given, least significant first: *out[p] =
// the item at sorted position p (one of sp[0], sp[1]); `start` = the order to begin from (null: the
// identity; not one of sp).  Every word is read in the order the words before it left (launch_tknn_word
// into wkey), then sorted by digits of <= kRadixMaxBits bits as group_sort_ids does, in K's radix
// workspace.  Enqueued.  tknn.cpp and tjoin.cpp share it.
int group_sort_words(gf_ctx* ctx, KeyGroups& K, DevBuf& wkey, DevBuf sp[2], const SortWord* words, int nwords, int64_t cnt,
                     const uint32_t* start, const uint32_t** out);

}  // namespace gf

// a window grouped by objID (gf_traj_group, traj.cpp): trajectory t = dense id t; tknn.cpp reads did,
// perm, seg_off and keys
struct gf_traj_groups : gf::KeyGroups {
  gf_ctx* ctx = nullptr;
  int64_t ntraj = 0;
  int64_t long_len = gf::kTrajLongLen;
  // tStats
  gf::DevBuf S, T, V, long_list, counters, set, sel, srank, ck, cS, cT, cV;
  // sub-trajectories
  gf::DevBuf hit, len, row, off, okeys, ooff, ox, oy, ots, oidx;
  gf::DevBuf* all[23] = {&S, &T, &V, &long_list, &counters, &set, &sel, &srank, &ck, &cS, &cT, &cV, &hit, &len,
                     &row, &off, &okeys, &ooff, &ox, &oy, &ots, &oidx, nullptr};
};

namespace gf {
// sub-trajectory emission shared by gf_traj_select, gf_trange_run and gf_tfilter_run (traj.cpp)
int traj_check_points(gf_traj_groups* G, const gf_points* pts, const char* who);  // pts is the grouped window, with x / y / ts
int traj_hit_clear(gf_traj_groups* G);  // G->hit[ntraj + 1] = 0 (enqueued)
int traj_emit(gf_traj_groups* G, const gf_points* pts, int64_t* keys, int64_t* off, int64_t cap_traj, double* x, double* y,
              int64_t* ts, uint32_t* idx, int64_t cap_pts, int64_t* ntraj_out, int64_t* npts_out);
}  // namespace gf
