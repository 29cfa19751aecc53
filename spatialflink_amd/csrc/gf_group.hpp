// gf_group.hpp -- what the trajectory host units (traj, tagg, tknn, tjoin, trange) share: the typed
// device array their objects are made of, the reads back to the caller, and "group a device int64
// key column" (traj.cpp holds the bodies; the kernels are k_traj.hip's traj_* and k_points.hip's radix
// passes).  gf_traj_group is group_dense_ids + group_sort_ids over objID; tagg.cpp groups by cell, by
// objID and by the (cell, objID) pair with them.
#pragma once

#include "gf_host.hpp"

namespace gf {

// A grow-only device array of T that frees itself: an object made of these needs no list of its
// buffers, and its destroy is set device, stream sync, delete.
template <class T>
struct DevArr {
  T* p = nullptr;
  size_t cap = 0;  // elements
  DevArr() = default;
  DevArr(const DevArr&) = delete;
  DevArr& operator=(const DevArr&) = delete;
  ~DevArr() { release(); }
  int reserve(gf_ctx* ctx, size_t count) {
    if (count <= cap) return GF_OK;
    GF_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));  // queued work may still read the old one
    release();
    GF_HIP_CHECK(ctx, hipMalloc(&p, count * sizeof(T)));
    cap = count;
    return GF_OK;
  }
  void release() {
    if (p) hipFree(p);
    p = nullptr;
    cap = 0;
  }
  size_t bytes() const { return cap * sizeof(T); }
};

// a plan's host table -> a device array of its own (plan creation: synchronous); an empty table: none
template <class T>
int upload(gf_ctx* ctx, DevArr<T>& dst, const std::vector<T>& src) {
  if (int st = dst.reserve(ctx, src.size())) return st;
  if (!src.empty()) GF_HIP_CHECK(ctx, hipMemcpy(dst.p, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice));
  return GF_OK;
}

// dev[0, count) -> host on the context stream (enqueued); a column the caller does not want is null
template <class T>
int read_back(gf_ctx* ctx, T* host, const T* dev, size_t count) {
  if (!host || count == 0) return GF_OK;
  GF_HIP_CHECK(ctx, hipMemcpyAsync(host, dev, count * sizeof(T), hipMemcpyDeviceToHost, ctx->stream));
  return GF_OK;
}

// CSR offsets are uint32 on the device and int64 for the caller: read_offsets stages and enqueues the
// copy of dev[0, count) (host null: nothing), widen() fills the caller's array after the stream sync.
struct OffsetRead {
  int64_t* host = nullptr;
  std::vector<uint32_t> stage;
  void widen() const {
    for (size_t i = 0; i < stage.size(); ++i) host[i] = (int64_t)stage[i];
  }
};
inline int read_offsets(gf_ctx* ctx, OffsetRead& o, int64_t* host, const uint32_t* dev, size_t count) {
  o.host = host;
  o.stage.resize(host ? count : 0);
  return read_back(ctx, o.stage.data(), dev, o.stage.size());
}

// the device counters of a tStats / tAggregate / tKnn object: uint32 words, zeroed before the first stage
constexpr size_t kCounterWords = 4;

// the bits of an id below nids (at least 1)
inline int key_bits(uint64_t nids) {
  int bits = 1;
  while (((uint64_t)1 << bits) < nids) ++bits;
  return bits;
}

// The workspace and the result of one grouping: n items, ngroups distinct keys.
//   keys[ngroups]        the distinct keys in first-occurrence order
//   did[n]               dense id per item
//   perm[n], seg_off[ngroups + 1], kbuf[sorted_in] = the sorted ids   (after group_sort_ids)
struct KeyGroups {
  int64_t n = 0, ngroups = 0;
  DevArr<unsigned long long> tkey;  // the hash table (+ the empty marker's slot)
  DevArr<uint32_t> tfirst;
  DevArr<uint32_t> kbuf[2], vbuf[2];  // radix ping-pong (n + 1 each); kbuf[1] = first-item flags, vbuf[1] = their scan
  DevArr<uint32_t> did, perm, seg_off, mat, mats, scan_tmp;
  DevArr<int64_t> keys;
  int sorted_in = 0;  // kbuf[sorted_in] = the keys of the last radix sort: dense id per perm position
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
// into wkey), then sorted by the passes group_sort_ids runs, in K's radix workspace.  Enqueued.
// tknn.cpp and tjoin.cpp share it.
int group_sort_words(gf_ctx* ctx, KeyGroups& K, DevArr<uint32_t>& wkey, DevArr<uint32_t> sp[2], const SortWord* words,
                     int nwords, int64_t cnt, const uint32_t* start, const uint32_t** out);

}  // namespace gf

// a window grouped by objID (gf_traj_group, traj.cpp): trajectory t = dense id t; tknn.cpp and
// tjoin.cpp read did, perm, seg_off and keys
struct gf_traj_groups : gf::KeyGroups {
  gf_ctx* ctx = nullptr;
  int64_t ntraj = 0;
  int64_t long_len = gf::kTrajLongLen;
  // tStats
  gf::DevArr<double> S, V, cS, cV;
  gf::DevArr<int64_t> T, set, ck, cT;
  gf::DevArr<uint32_t> long_list, counters, sel, srank;
  // sub-trajectories
  gf::DevArr<uint32_t> hit, len, row, off, ooff, oidx;
  gf::DevArr<int64_t> okeys, ots;
  gf::DevArr<double> ox, oy;
};

namespace gf {
// sub-trajectory emission shared by gf_traj_select, gf_trange_run and gf_tfilter_run (traj.cpp)
int traj_check_points(gf_traj_groups* G, const gf_points* pts, const char* who);  // pts is the grouped window, with x / y / ts
int traj_hit_clear(gf_traj_groups* G);  // G->hit[ntraj + 1] = 0 (enqueued)
int traj_emit(gf_traj_groups* G, const gf_points* pts, int64_t* keys, int64_t* off, int64_t cap_traj, double* x, double* y,
              int64_t* ts, uint32_t* idx, int64_t cap_pts, int64_t* ntraj_out, int64_t* npts_out);
}  // namespace gf
