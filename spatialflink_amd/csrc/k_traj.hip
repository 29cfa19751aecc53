// k_traj.hip -- trajectory operators: a window's points grouped by objID (the reference's
// keyBy(objID) + `for (Point p : input)` of TStatsQuery.java:148-189, PointPolygonTRangeQuery.java:
// 158-176, PointPointTKNNQuery.java:241-270), tStats over the groups, sub-trajectory extraction.
//
// Grouping (gf_traj_group; traj.cpp drives the launches).  Trajectory t is the objID whose first
// point has the t-th smallest index; its points keep their window order:
//   traj_clear    the open-addressing table (>= 2n slots, linear probe): key = kTrajEmpty, first = ~0
//   traj_insert   one lane per point: claim the key's slot with one 64-bit CAS, atomicMin the point
//                 index into it.  Any int64 is a legal key, so the table's empty marker is a key too:
//                 points carrying it own the extra slot past the table (no claim needed).
//   traj_flag     flag[i] = 1 iff i is its slot's minimum (the trajectory's first point)
//   (scan)        rank = exclusive prefix of the flags = the dense id in first-occurrence order
//   traj_assign   first points: keys[rank] = key, the slot's `first` becomes the dense id
//   traj_ids      did[i] = dense id of point i
//   (radix)       stable LSD passes over (did, index) -- k_points.hip's histogram / scatter with
//                 kin / vin -- give perm and the sorted ids
//   traj_bounds   seg_off[t] = first position holding id t (every id occurs), seg_off[ntraj] = n
// The minimum per slot, the scan and the stable sort are all order-free: no output depends on which
// lane wins the CAS (only WHICH slot a key lands in does, and no output names a slot).
#define GF_TU_NAME k_traj_hip
#include "gf_buildtag.hpp"  // first: records this unit's command-line defines

#include "gf_internal.hpp"

namespace gf {

__device__ __forceinline__ uint64_t traj_hash(unsigned long long k) {
  k ^= k >> 33;
  k *= 0xff51afd7ed558ccdull;
  k ^= k >> 33;
  k *= 0xc4ceb9fe1a85ec53ull;
  k ^= k >> 33;
  return k;
}

// block-uniform loop over items [0, n): every lane of a block runs every iteration (the bodies use
// wave shuffles / ballots), `i < n` masks the tail
#define GF_TRAJ_LOOP(i, n)                                                                                      \
  for (int64_t i##0 = (int64_t)blockIdx.x * kBlock, i = i##0 + threadIdx.x; i##0 < (n);                         \
       i##0 += (int64_t)gridDim.x * kBlock, i = i##0 + threadIdx.x)

__global__ __launch_bounds__(kBlock) void traj_clear_kernel(TrajTable t) {
  const uint64_t slots = t.mask + 2;  // the table + the empty marker's own slot
  for (uint64_t s = (uint64_t)blockIdx.x * kBlock + threadIdx.x; s < slots; s += (uint64_t)gridDim.x * kBlock) {
    t.key[s] = kTrajEmpty;
    t.first[s] = 0xFFFFFFFFu;
  }
}

// the slot of a key that traj_insert placed (read-only; later kernels)
__device__ __forceinline__ uint64_t traj_find(const TrajTable& t, unsigned long long k) {
  if (k == kTrajEmpty) return t.mask + 1;
  uint64_t pos = traj_hash(k) & t.mask;
  while (t.key[pos] != k) pos = (pos + 1) & t.mask;
  return pos;
}

__global__ __launch_bounds__(kBlock) void traj_insert_kernel(TrajTable t, const int64_t* __restrict__ objID, int64_t n) {
  const int lane = threadIdx.x & 63;
  GF_TRAJ_LOOP(i, n) {
    const bool valid = i < n;
    uint64_t pos = ~0ull;
    if (valid) {
      const unsigned long long k = (unsigned long long)objID[i];
      if (k == kTrajEmpty) {
        pos = t.mask + 1;
      } else {
        pos = traj_hash(k) & t.mask;
        for (;;) {  // distinct keys <= n < slots / 2: an empty slot always ends the probe
          unsigned long long cur = __hip_atomic_load(&t.key[pos], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          if (cur == kTrajEmpty) cur = atomicCAS(&t.key[pos], kTrajEmpty, k);
          if (cur == kTrajEmpty || cur == k) break;
          pos = (pos + 1) & t.mask;
        }
      }
    }
    // Equal slots aggregated before the atomic: a lane whose lower neighbour holds the same slot
    // cannot be the minimum (the neighbour's index is smaller), and a slot whose minimum is already
    // below this index needs no atomic at all -- a hot objID settles after its first few points.
    const uint64_t prev = __shfl_up(pos, 1, 64);
    if (valid && !(lane > 0 && prev == pos)) {
      if (__hip_atomic_load(&t.first[pos], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > (uint32_t)i)
        atomicMin(&t.first[pos], (uint32_t)i);
    }
  }
}

__global__ __launch_bounds__(kBlock) void traj_flag_kernel(TrajTable t, const int64_t* __restrict__ objID, int64_t n,
                                                           uint32_t* __restrict__ flag) {
  GF_TRAJ_LOOP(i, n) {
    if (i < n) flag[i] = t.first[traj_find(t, (unsigned long long)objID[i])] == (uint32_t)i ? 1u : 0u;
  }
}

// (reads flag / rank only: the slots' `first` words are rewritten here as dense ids)
__global__ __launch_bounds__(kBlock) void traj_assign_kernel(TrajTable t, const int64_t* __restrict__ objID, int64_t n,
                                                             const uint32_t* __restrict__ flag,
                                                             const uint32_t* __restrict__ rank, int64_t* __restrict__ keys) {
  GF_TRAJ_LOOP(i, n) {
    if (i < n && flag[i]) {
      const int64_t k = objID[i];
      t.first[traj_find(t, (unsigned long long)k)] = rank[i];
      keys[rank[i]] = k;
    }
  }
}

__global__ __launch_bounds__(kBlock) void traj_ids_kernel(TrajTable t, const int64_t* __restrict__ objID, int64_t n,
                                                          uint32_t* __restrict__ did) {
  GF_TRAJ_LOOP(i, n) {
    if (i < n) did[i] = t.first[traj_find(t, (unsigned long long)objID[i])];
  }
}

__global__ __launch_bounds__(kBlock) void traj_bounds_kernel(const uint32_t* __restrict__ sorted, int64_t n,
                                                             uint32_t ntraj, uint32_t* __restrict__ seg_off) {
  GF_TRAJ_LOOP(p, n) {
    if (p < n) {
      const uint32_t d = sorted[p];
      if (p == 0 || sorted[p - 1] != d) seg_off[d] = (uint32_t)p;
      if (p == n - 1) seg_off[ntraj] = (uint32_t)n;
    }
  }
}

static unsigned traj_blocks(gf_ctx* ctx, uint64_t items) {
  const uint64_t b = (items + kBlock - 1) / kBlock, cap = (uint64_t)ctx->num_cus * 8;
  return (unsigned)(b < 1 ? 1 : (b > cap ? cap : b));
}

hipError_t launch_traj_group(gf_ctx* ctx, int stage, const TrajGroupArgs& a) {
  hipStream_t s = ctx->stream;
  KTimer timer(ctx, GF_K_TRAJ_GROUP);
  const unsigned g = traj_blocks(ctx, (uint64_t)a.n);
  switch (stage) {
    case kTrajGroupInsert:
      hipLaunchKernelGGL(traj_clear_kernel, dim3(traj_blocks(ctx, a.t.mask + 2)), dim3(kBlock), 0, s, a.t);
      hipLaunchKernelGGL(traj_insert_kernel, dim3(g), dim3(kBlock), 0, s, a.t, a.objID, a.n);
      hipLaunchKernelGGL(traj_flag_kernel, dim3(g), dim3(kBlock), 0, s, a.t, a.objID, a.n, a.flag);
      break;
    case kTrajGroupAssign:
      hipLaunchKernelGGL(traj_assign_kernel, dim3(g), dim3(kBlock), 0, s, a.t, a.objID, a.n, a.flag, a.rank, a.keys);
      hipLaunchKernelGGL(traj_ids_kernel, dim3(g), dim3(kBlock), 0, s, a.t, a.objID, a.n, a.did);
      break;
    default:  // kTrajGroupBounds
      hipLaunchKernelGGL(traj_bounds_kernel, dim3(g), dim3(kBlock), 0, s, a.sorted, a.n, a.ntraj, a.seg_off);
      break;
  }
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------
// tStats -- TStatsQuery.TStatsQueryWFunction.apply (TStatsQuery.java:154-188) per trajectory, its
// points in perm order.  S is the sequential left-to-right fp64 sum on both paths (no FMA: the
// build's -ffp-contract=off; no tree).
//   tstats_walk_kernel  one lane per trajectory shorter than long_len walks its segment with the
//                       reference's state machine; longer ones are appended to a list
//   tstats_long_kernel  one block per listed trajectory, 256 points per tile (ts >= 0, the header's
//                       contract: a point counts iff ts > max(0, every earlier ts)): block prefix-max
//                       of ts -> counted flags; every counted point finds the counted point before it
//                       (this tile's ballots, else the carry) and computes its step distance; the
//                       steps, compacted in order in LDS, are added to S by ONE lane in order while
//                       the other lanes already load the next tile.  T = last - first counted ts (the
//                       telescoped integer sum).
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void tstats_walk_kernel(TStatsArgs a) {
  const int lane = threadIdx.x & 63;
  GF_TRAJ_LOOP(t, a.ntraj) {
    bool is_long = false;
    if (t < a.ntraj) {
      const uint32_t b = a.seg_off[t], e = a.seg_off[t + 1];
      if (e - b >= a.long_len) {
        is_long = true;
      } else {
        int64_t last = 0, T = 0;
        double S = 0.0, X = 0.0, Y = 0.0;
        for (uint32_t p = b; p < e; ++p) {
          const uint32_t i = a.perm[p];
          const int64_t ts = a.ts[i];
          if (last == 0) {  // the reference's first-point test: lastTimestamp.equals(0L)
            last = ts; X = a.x[i]; Y = a.y[i]; S = 0.0; T = 0;
          } else if (ts > last) {
            const double px = a.x[i], py = a.y[i];
            S += sqrt((py - Y) * (py - Y) + (px - X) * (px - X));  // DistanceFunctions.java:60-63
            T += ts - last;
            last = ts; X = px; Y = py;
          }
        }
        a.S[t] = S;
        a.T[t] = T;
        a.V[t] = S / (double)T;  // Java 0.0 / 0 = NaN for fewer than two counted points
      }
    }
    const uint64_t m = __ballot(is_long);
    if (m) {  // wave-uniform: one atomic per wave (the list's order carries no meaning)
      uint32_t base = 0;
      if (lane == 0) base = atomicAdd(a.long_count, (uint32_t)__popcll(m));
      base = __shfl(base, 0, 64);
      if (is_long) a.long_list[base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = (uint32_t)t;
    }
  }
}

__global__ __launch_bounds__(kBlock) void tstats_long_kernel(TStatsArgs a) {
  constexpr int W = kBlock / 64;
  __shared__ double sd[kBlock], sx[kBlock], sy[kBlock];
  __shared__ unsigned long long cm[W];
  __shared__ long long wmax[W];
  __shared__ double cX, cY;      // the last counted point so far
  __shared__ long long cFirst;   // the first counted ts
  __shared__ int cHave;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const uint64_t below = (1ull << lane) - 1ull;
  const uint32_t nlong = *a.long_count;
  for (uint32_t j = blockIdx.x; j < nlong; j += gridDim.x) {  // block-uniform
    const uint32_t t = a.long_list[j];
    const uint32_t b = a.seg_off[t], e = a.seg_off[t + 1];
    __syncthreads();  // the previous trajectory's carry has been read
    if (threadIdx.x == 0) { cHave = 0; cFirst = 0; cX = 0.0; cY = 0.0; }
    long long last = 0;  // max(0, every ts so far), block-uniform
    double S = 0.0;      // thread 0's
    for (uint32_t p0 = b; p0 < e; p0 += kBlock) {  // block-uniform (e - b < 2^32: p0 cannot wrap past e
      const uint32_t left = e - p0;                //  unless e > 2^32 - kBlock, handled by `left`)
      const bool valid = (uint32_t)threadIdx.x < left;
      long long ts = 0;
      double px = 0.0, py = 0.0;
      if (valid) {
        const uint32_t i = a.perm[p0 + threadIdx.x];
        ts = a.ts[i]; px = a.x[i]; py = a.y[i];
      }
      long long inc = ts;  // inclusive prefix max inside the wave
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const long long u = __shfl_up(inc, o, 64);
        if (lane >= o && u > inc) inc = u;
      }
      long long excl = __shfl_up(inc, 1, 64);
      if (lane == 0) excl = 0;
      if (lane == 63) wmax[w] = inc;
      __syncthreads();  // A
      long long before = last, all = last;
#pragma unroll
      for (int q = 0; q < W; ++q) {
        const long long v = wmax[q];
        if (q < w && v > before) before = v;
        if (v > all) all = v;
      }
      if (excl > before) before = excl;
      const bool counted = valid && ts > before;
      const uint64_t bal = __ballot(counted);
      if (lane == 0) cm[w] = bal;
      sx[threadIdx.x] = px;
      sy[threadIdx.x] = py;
      __syncthreads();  // B
      const int have = cHave;
      uint32_t rank = 0, c = 0;
      int pi = -1;  // the counted point before this one, in the tile
#pragma unroll
      for (int q = 0; q < W; ++q) {
        const unsigned long long mq = cm[q];
        c += (uint32_t)__popcll(mq);
        if (q < w) {
          rank += (uint32_t)__popcll(mq);
          if (mq) pi = q * 64 + 63 - __clzll((long long)mq);
        }
      }
      if (bal & below) pi = w * 64 + 63 - __clzll((long long)(bal & below));
      rank += (uint32_t)__popcll(bal & below);
      if (counted) {
        double d = 0.0;  // the trajectory's first counted point adds 0.0 to S == 0.0
        if (pi >= 0 || have) {
          const double X = pi >= 0 ? sx[pi] : cX, Y = pi >= 0 ? sy[pi] : cY;
          d = sqrt((py - Y) * (py - Y) + (px - X) * (px - X));
        }
        sd[rank] = d;
      }
      __syncthreads();  // C: the steps are in sd[0, c); cX / cY / cHave have been read
      if (counted && rank == c - 1) { cX = px; cY = py; }
      if (counted && rank == 0 && !have) { cFirst = ts; cHave = 1; }
      if (threadIdx.x == 0)
        for (uint32_t q = 0; q < c; ++q) S += sd[q];  // the ordered add (serial by contract)
      last = all;
      if (left <= (uint32_t)kBlock) break;  // the last tile (keeps p0 from wrapping)
      // no barrier here: the next tile writes wmax before its barrier A (read above by all, before
      // B), sx / sy / cm after A and sd after B -- thread 0 reads only sd and reaches A itself
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      const long long T = cHave ? last - cFirst : 0;
      a.S[t] = S;
      a.T[t] = T;
      a.V[t] = S / (double)T;
    }
  }
}

// trajIDSet filter: sel[t] = 1 iff keys[t] is in the sorted, distinct set
__global__ __launch_bounds__(kBlock) void tstats_filter_kernel(const int64_t* __restrict__ keys, int64_t ntraj,
                                                               const int64_t* __restrict__ set, int64_t nset,
                                                               uint32_t* __restrict__ sel) {
  GF_TRAJ_LOOP(t, ntraj) {
    if (t < ntraj) {
      const int64_t k = keys[t];
      int64_t lo = 0, hi = nset;
      while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (set[mid] < k) lo = mid + 1; else hi = mid;
      }
      sel[t] = lo < nset && set[lo] == k ? 1u : 0u;
    }
  }
}

__global__ __launch_bounds__(kBlock) void tstats_compact_kernel(TStatsArgs a, const uint32_t* __restrict__ sel,
                                                                const uint32_t* __restrict__ rank,
                                                                const int64_t* __restrict__ keys, int64_t* __restrict__ ok,
                                                                double* __restrict__ oS, int64_t* __restrict__ oT,
                                                                double* __restrict__ oV) {
  GF_TRAJ_LOOP(t, a.ntraj) {
    if (t < a.ntraj && sel[t]) {
      const uint32_t r = rank[t];
      ok[r] = keys[t]; oS[r] = a.S[t]; oT[r] = a.T[t]; oV[r] = a.V[t];
    }
  }
}

hipError_t launch_tstats(gf_ctx* ctx, const TStatsArgs& a) {
  KTimer timer(ctx, GF_K_TSTATS);
  hipLaunchKernelGGL(tstats_walk_kernel, dim3(traj_blocks(ctx, (uint64_t)a.ntraj)), dim3(kBlock), 0, ctx->stream, a);
  hipLaunchKernelGGL(tstats_long_kernel, dim3((unsigned)ctx->num_cus * 4), dim3(kBlock), 0, ctx->stream, a);
  return hipGetLastError();
}

hipError_t launch_tstats_filter(gf_ctx* ctx, const TStatsArgs& a, const int64_t* keys, const int64_t* set, int64_t nset,
                                uint32_t* sel, const uint32_t* rank, int64_t* ok, double* oS, int64_t* oT, double* oV,
                                int stage) {
  KTimer timer(ctx, GF_K_TSTATS);
  const unsigned g = traj_blocks(ctx, (uint64_t)a.ntraj);
  if (stage == kTStatsFilterMark)
    hipLaunchKernelGGL(tstats_filter_kernel, dim3(g), dim3(kBlock), 0, ctx->stream, keys, a.ntraj, set, nset, sel);
  else
    hipLaunchKernelGGL(tstats_compact_kernel, dim3(g), dim3(kBlock), 0, ctx->stream, a, sel, rank, keys, ok, oS, oT, oV);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------
// Sub-trajectories: every trajectory with a flagged point, whole, as CSR (the second half of the
// window-based tRange / tKnn / tJoin: PointPolygonTRangeQuery.java:158-176).
//   traj_hit     point i flagged -> hit[did[i]] = 1 (every writer stores the same 1)
//   traj_lens    len[t] = hit[t] ? the segment's length : 0
//   (scans)      of hit -> output row, of len -> output offset
//   traj_gather  rows: keys / offsets; positions of hit trajectories: x, y, ts, idx in perm order
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void traj_hit_kernel(const uint64_t* __restrict__ bitmap,
                                                          const uint32_t* __restrict__ did, int64_t n,
                                                          uint32_t* __restrict__ hit) {
  GF_TRAJ_LOOP(i, n) {
    if (i < n && ((bitmap[i >> 6] >> (i & 63)) & 1ull)) hit[did[i]] = 1u;
  }
}

__global__ __launch_bounds__(kBlock) void traj_lens_kernel(const uint32_t* __restrict__ hit,
                                                           const uint32_t* __restrict__ seg_off, int64_t ntraj,
                                                           uint32_t* __restrict__ len) {
  GF_TRAJ_LOOP(t, ntraj) {
    if (t < ntraj) len[t] = hit[t] ? seg_off[t + 1] - seg_off[t] : 0u;
  }
}

__global__ __launch_bounds__(kBlock) void traj_gather_kernel(TrajSelectArgs a) {
  GF_TRAJ_LOOP(t, a.ntraj) {
    if (t < a.ntraj && a.hit[t]) {
      const uint32_t r = a.row[t];
      a.okeys[r] = a.keys[t];
      a.ooff[r] = a.off[t];
    }
    if (t == 0) a.ooff[a.row[a.ntraj]] = a.off[a.ntraj];
  }
  GF_TRAJ_LOOP(p, a.n) {
    if (p < a.n) {
      const uint32_t t = a.sorted[p];
      if (a.hit[t]) {
        const uint32_t dst = a.off[t] + ((uint32_t)p - a.seg_off[t]), i = a.perm[p];
        a.ox[dst] = a.x[i];
        a.oy[dst] = a.y[i];
        a.ots[dst] = a.ts[i];
        a.oidx[dst] = i;
      }
    }
  }
}

hipError_t launch_traj_select(gf_ctx* ctx, int stage, const TrajSelectArgs& a) {
  KTimer timer(ctx, GF_K_TRAJ_SELECT);
  hipStream_t s = ctx->stream;
  if (stage == kTrajSelectHit) {
    hipLaunchKernelGGL(traj_hit_kernel, dim3(traj_blocks(ctx, (uint64_t)a.n)), dim3(kBlock), 0, s, a.bitmap, a.did, a.n,
                       a.hit);
  } else if (stage == kTrajSelectLens) {
    hipLaunchKernelGGL(traj_lens_kernel, dim3(traj_blocks(ctx, (uint64_t)a.ntraj)), dim3(kBlock), 0, s, a.hit, a.seg_off,
                       a.ntraj, a.len);
  } else {
    hipLaunchKernelGGL(traj_gather_kernel, dim3(traj_blocks(ctx, (uint64_t)a.n)), dim3(kBlock), 0, s, a);
  }
  return hipGetLastError();
}

}  // namespace gf
