// k_tagg.hip -- tAggregate, the windowed heatmap (PointTAggregateQuery.java, TAggregateQuery.java:
// 498-613 TimeWindowProcessFunction.process): per grid cell of a window the distinct objIDs, how long
// each stayed there (max ts - min ts of its points in the cell) and the cell's SUM / AVG / MIN / MAX
// of those stays.  The group-by key is the pair (cell, objID); tagg.cpp drives the launches.
//
//   tagg_cellkey   ckey[i] = pack(cx, cy), K1's cell of point i (HelperClass.assignGridCellID)
//   (group)        dense cell id and dense objID id per point, both in first-occurrence order
//                  (traj.cpp's group_dense_ids: k_traj.hip's table kernels)
//   tagg_compose   comp[i] = cell id << 32 | objID id
//   (group)        dense ids of comp, then the stable sort: group g = the g-th (cell, objID) pair in
//                  first-occurrence order, its points in window order
//   tagg_gstats    per group: m, L = max ts - min ts, e = |t2 - t1|, s = the index of the second
//                  point, f = the largest of s, the first index at min ts, the first index at max ts
//                  (the point at which the reference's running max - min first equals L).  One lane
//                  walks a short group; groups of >= long_len points are left to
//   tagg_glong     every position of the sorted window in parallel (a hot group can hold a fifth of
//                  the window: one block per group measured 7.8 ms there): integer atomicMin / Max of
//                  ts per long group, then atomicMin of the indices holding them.  Min and max of a
//                  set: the final words do not depend on the order of the atomics.
//   tagg_glong_rows  the long groups' rows from those words
//   (radix)        the groups sorted stably by cell id -> gperm, cell_off: a cell's groups keep
//                  first-occurrence order = its objIDs in the order of their first point in the cell
//   tagg_cell      per cell: count, multi, sum, (minLen, minKey) = the lexicographic min of (e, s),
//                  (maxLen, maxKey) = the max L with the smallest f, over the groups with m >= 2.
//                  One lane walks a small cell; cells of >= big_cell groups are listed and
//   tagg_cbig      one block reduces each listed cell (int64 sums: associative; s and f are window
//                  indices, distinct between groups: the lexicographic winners are unique).
//   tagg_all       the ALL rows in cell order: all_key[q], all_len[q] of group gperm[q]
// Determinism: the grouping's argument (k_traj.hip:18-19) holds for each of the three groupings; the
// cell list's order carries no meaning (every listed cell writes its own row); no float anywhere.
#define GF_TU_NAME k_tagg_hip
#include "gf_buildtag.hpp"  // first: records this unit's command-line defines

#include "gf_internal.hpp"

namespace gf {

// block-uniform loop over items [0, n): every lane of a block runs every iteration (the bodies use
// wave ballots), `i < n` masks the tail
#define GF_TAGG_LOOP(i, n)                                                                                      \
  for (int64_t i##0 = (int64_t)blockIdx.x * kBlock, i = i##0 + threadIdx.x; i##0 < (n);                         \
       i##0 += (int64_t)gridDim.x * kBlock, i = i##0 + threadIdx.x)

__global__ __launch_bounds__(kBlock) void tagg_cellkey_kernel(TaggArgs a) {
  GF_TAGG_LOOP(i, a.n) {
    if (i < a.n) {
      const uint32_t cx = (uint32_t)cell_index(a.x[i], a.minX, a.cl), cy = (uint32_t)cell_index(a.y[i], a.minY, a.cl);
      a.ckey[i] = (int64_t)(((uint64_t)cx << 32) | cy);
    }
  }
}

__global__ __launch_bounds__(kBlock) void tagg_compose_kernel(TaggArgs a) {
  GF_TAGG_LOOP(i, a.n) {
    if (i < a.n) a.comp[i] = (int64_t)(((uint64_t)a.cid[i] << 32) | a.oid[i]);
  }
}

// (ts, index) candidates of a group's min and max: on equal ts the smaller index wins both
struct TaggExt {
  long long mn, mx;
  uint32_t imn, imx;
};

// the row of group g, its first two points (i0, t1), (i1, t2) and its extremes known
__device__ __forceinline__ void tagg_group_row(const TaggArgs& a, int64_t g, uint32_t m, uint32_t i1, long long t1,
                                               long long t2, const TaggExt& r) {
  const uint64_t ck = (uint64_t)a.gkeys[g];
  a.g_cell[g] = (uint32_t)(ck >> 32);
  a.g_key[g] = a.okeys[(uint32_t)ck];
  a.g_m[g] = m;
  a.g_L[g] = r.mx - r.mn;
  uint32_t f = r.imn > r.imx ? r.imn : r.imx;
  if (i1 > f) f = i1;
  a.g_e[g] = m >= 2 ? (t2 > t1 ? t2 - t1 : t1 - t2) : 0;
  a.g_f[g] = m >= 2 ? f : 0u;
  a.g_s[g] = m >= 2 ? i1 : 0u;
}

// one wave-aggregated append of the flagged lanes' items to a list
__device__ __forceinline__ void tagg_list_push(bool flag, uint32_t item, uint32_t* list, uint32_t* count) {
  const int lane = threadIdx.x & 63;
  const uint64_t m = __ballot(flag);
  if (m) {  // wave-uniform: one atomic per wave (the list's order carries no meaning)
    uint32_t base = 0;
    if (lane == 0) base = atomicAdd(count, (uint32_t)__popcll(m));
    base = __shfl(base, 0, 64);
    if (flag) list[base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = item;
  }
}

__global__ __launch_bounds__(kBlock) void tagg_gstats_kernel(TaggArgs a) {
  const int lane = threadIdx.x & 63;
  GF_TAGG_LOOP(g, a.ngroups) {
    bool is_long = false;
    if (g < a.ngroups) {
      const uint32_t b = a.seg_off[g], e = a.seg_off[g + 1], m = e - b;
      if (m >= a.long_len) {
        is_long = true;  // the identities of tagg_glong's reductions, in the row's own words
        a.g_L[g] = INT64_MAX; a.g_e[g] = INT64_MIN; a.g_f[g] = 0xFFFFFFFFu; a.g_s[g] = 0xFFFFFFFFu;
      } else {
        const uint32_t i0 = a.perm[b];
        const long long t1 = a.ts[i0];
        TaggExt r{t1, t1, i0, i0};
        uint32_t i1 = 0;
        long long t2 = 0;
        for (uint32_t p = b + 1; p < e; ++p) {  // ascending indices: strict comparisons keep the first
          const uint32_t i = a.perm[p];
          const long long t = a.ts[i];
          if (p == b + 1) { i1 = i; t2 = t; }
          if (t < r.mn) { r.mn = t; r.imn = i; }
          if (t > r.mx) { r.mx = t; r.imx = i; }
        }
        tagg_group_row(a, g, m, i1, t1, t2, r);
      }
    }
    const uint64_t bal = __ballot(is_long);
    if (bal && lane == 0) atomicAdd(a.list_count, (uint32_t)__popcll(bal));  // (a count only: glong returns at once on 0)
  }
}

// Long groups, every position of the sorted window in parallel.  Stage 0: min ts -> g_L, max ts -> g_e;
// stage 1: the smallest index holding the min -> g_f, holding the max -> g_s.  Integer atomicMin /
// atomicMax: the final word is the min / max of a set, whatever the order.  A wave whose 64 positions
// lie in one group (the rule inside a long group) reduces first and sends one atomic; a word that
// already beats the candidate is left alone.
__global__ __launch_bounds__(kBlock) void tagg_glong_kernel(TaggArgs a, int stage) {
  if (*a.list_count == 0) return;
  long long* gmn = (long long*)a.g_L;
  long long* gmx = (long long*)a.g_e;
  GF_TAGG_LOOP(p, a.n) {
    uint32_t g = 0xFFFFFFFFu, i = 0;
    long long t = 0;
    if (p < a.n) {
      const uint32_t gg = a.sorted[p];
      if (a.seg_off[gg + 1] - a.seg_off[gg] >= a.long_len) {
        g = gg;
        i = a.perm[p];
        t = a.ts[i];
      }
    }
    const bool valid = g != 0xFFFFFFFFu;
    if (!__any(valid)) continue;  // wave-uniform
    const bool uniform = __all(g == __shfl(g, 0, 64)) && valid;  // (valid: lane 0's, so every lane's)
    if (stage == 0) {
      long long mn = t, mx = t;
      if (uniform) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
          const long long umn = __shfl_xor(mn, o, 64), umx = __shfl_xor(mx, o, 64);
          if (umn < mn) mn = umn;
          if (umx > mx) mx = umx;
        }
      }
      if (valid && (!uniform || (threadIdx.x & 63) == 0)) {
        if (__hip_atomic_load(&gmn[g], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > mn) atomicMin(&gmn[g], mn);
        if (__hip_atomic_load(&gmx[g], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < mx) atomicMax(&gmx[g], mx);
      }
    } else {
      uint32_t imn = 0xFFFFFFFFu, imx = 0xFFFFFFFFu;
      if (valid) {  // (stage 0 has completed: plain loads)
        if (t == gmn[g]) imn = i;
        if (t == gmx[g]) imx = i;
      }
      if (uniform) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
          const uint32_t umn = __shfl_xor(imn, o, 64), umx = __shfl_xor(imx, o, 64);
          if (umn < imn) imn = umn;
          if (umx < imx) imx = umx;
        }
      }
      if (valid && (!uniform || (threadIdx.x & 63) == 0)) {
        if (imn != 0xFFFFFFFFu && __hip_atomic_load(&a.g_f[g], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > imn)
          atomicMin(&a.g_f[g], imn);
        if (imx != 0xFFFFFFFFu && __hip_atomic_load(&a.g_s[g], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > imx)
          atomicMin(&a.g_s[g], imx);
      }
    }
  }
}

// the rows of the long groups from the reduced words (each row's own lane reads them, then writes the row)
__global__ __launch_bounds__(kBlock) void tagg_glong_rows_kernel(TaggArgs a) {
  if (*a.list_count == 0) return;
  GF_TAGG_LOOP(g, a.ngroups) {
    if (g < a.ngroups) {
      const uint32_t b = a.seg_off[g], e = a.seg_off[g + 1], m = e - b;
      if (m >= a.long_len) {
        const TaggExt r{a.g_L[g], a.g_e[g], a.g_f[g], a.g_s[g]};
        const uint32_t i0 = a.perm[b], i1 = m >= 2 ? a.perm[b + 1] : 0u;
        tagg_group_row(a, g, m, i1, a.ts[i0], m >= 2 ? a.ts[i1] : 0, r);
      }
    }
  }
}

// a cell's running aggregate; add() takes one group, merge() another aggregate
struct TaggCell {
  long long sum, minLen, minKey, maxLen, maxKey;
  uint32_t multi, minS, maxF;
};
__device__ __forceinline__ TaggCell tagg_cell_zero() {
  return TaggCell{0, INT64_MAX, 0, INT64_MIN, 0, 0u, 0xFFFFFFFFu, 0xFFFFFFFFu};
}
__device__ __forceinline__ void tagg_cell_min(TaggCell& c, long long e, uint32_t s, long long key) {
  if (e < c.minLen || (e == c.minLen && s < c.minS)) { c.minLen = e; c.minS = s; c.minKey = key; }
}
__device__ __forceinline__ void tagg_cell_max(TaggCell& c, long long L, uint32_t f, long long key) {
  if (L > c.maxLen || (L == c.maxLen && f < c.maxF)) { c.maxLen = L; c.maxF = f; c.maxKey = key; }
}
__device__ __forceinline__ void tagg_cell_add(const TaggArgs& a, TaggCell& c, uint32_t g) {
  const long long L = a.g_L[g];
  c.sum += L;
  if (a.g_m[g] >= 2) {
    const long long key = a.g_key[g];
    ++c.multi;
    tagg_cell_min(c, a.g_e[g], a.g_s[g], key);
    tagg_cell_max(c, L, a.g_f[g], key);
  }
}
__device__ __forceinline__ void tagg_cell_row(const TaggArgs& a, int64_t c, uint32_t count, const TaggCell& r) {
  const uint64_t ck = (uint64_t)a.ckeys[c];
  a.c_cx[c] = (int32_t)(uint32_t)(ck >> 32);
  a.c_cy[c] = (int32_t)(uint32_t)ck;
  a.c_count[c] = count;
  a.c_multi[c] = r.multi;
  a.c_sum[c] = r.sum;
  a.c_minLen[c] = r.minLen;
  a.c_minKey[c] = r.minKey;
  a.c_maxLen[c] = r.maxLen;
  a.c_maxKey[c] = r.maxKey;
}

__global__ __launch_bounds__(kBlock) void tagg_cell_kernel(TaggArgs a) {
  GF_TAGG_LOOP(c, a.ncells) {
    bool is_big = false;
    if (c < a.ncells) {
      const uint32_t b = a.cell_off[c], e = a.cell_off[c + 1];
      if (e - b >= a.big_cell) {
        is_big = true;
      } else {
        TaggCell r = tagg_cell_zero();
        for (uint32_t q = b; q < e; ++q) tagg_cell_add(a, r, a.gperm[q]);
        tagg_cell_row(a, c, e - b, r);
      }
    }
    tagg_list_push(is_big, (uint32_t)c, a.list, a.list_count);
  }
}

__global__ __launch_bounds__(kBlock) void tagg_cbig_kernel(TaggArgs a) {
  constexpr int W = kBlock / 64;
  __shared__ TaggCell part[W];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const uint32_t nbig = *a.list_count;
  for (uint32_t j = blockIdx.x; j < nbig; j += gridDim.x) {  // block-uniform
    const uint32_t c = a.list[j];
    const uint32_t b = a.cell_off[c], e = a.cell_off[c + 1];
    TaggCell r = tagg_cell_zero();
    for (uint64_t q = (uint64_t)b + threadIdx.x; q < e; q += kBlock) tagg_cell_add(a, r, a.gperm[q]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      TaggCell u;
      u.sum = __shfl_down(r.sum, o, 64);
      u.minLen = __shfl_down(r.minLen, o, 64);
      u.minKey = __shfl_down(r.minKey, o, 64);
      u.maxLen = __shfl_down(r.maxLen, o, 64);
      u.maxKey = __shfl_down(r.maxKey, o, 64);
      u.multi = __shfl_down(r.multi, o, 64);
      u.minS = __shfl_down(r.minS, o, 64);
      u.maxF = __shfl_down(r.maxF, o, 64);
      r.sum += u.sum;
      r.multi += u.multi;
      tagg_cell_min(r, u.minLen, u.minS, u.minKey);
      tagg_cell_max(r, u.maxLen, u.maxF, u.maxKey);
    }
    __syncthreads();  // the previous cell's partials have been read
    if (lane == 0) part[w] = r;
    __syncthreads();
    if (threadIdx.x == 0) {
      TaggCell t = part[0];
      for (int v = 1; v < W; ++v) {
        t.sum += part[v].sum;
        t.multi += part[v].multi;
        tagg_cell_min(t, part[v].minLen, part[v].minS, part[v].minKey);
        tagg_cell_max(t, part[v].maxLen, part[v].maxF, part[v].maxKey);
      }
      tagg_cell_row(a, c, e - b, t);
    }
  }
}

__global__ __launch_bounds__(kBlock) void tagg_all_kernel(TaggArgs a) {
  GF_TAGG_LOOP(q, a.ngroups) {
    if (q < a.ngroups) {
      const uint32_t g = a.gperm[q];
      a.all_key[q] = a.g_key[g];
      a.all_len[q] = a.g_L[g];
    }
  }
}

static unsigned tagg_blocks(gf_ctx* ctx, uint64_t items) {
  const uint64_t b = (items + kBlock - 1) / kBlock, cap = (uint64_t)ctx->num_cus * 8;
  return (unsigned)(b < 1 ? 1 : (b > cap ? cap : b));
}

hipError_t launch_tagg(gf_ctx* ctx, int stage, const TaggArgs& a) {
  hipStream_t s = ctx->stream;
  KTimer timer(ctx, GF_K_TAGG);
  const dim3 blk(kBlock), wide((unsigned)ctx->num_cus * 4);
  switch (stage) {
    case kTaggCellKeys:
      hipLaunchKernelGGL(tagg_cellkey_kernel, dim3(tagg_blocks(ctx, (uint64_t)a.n)), blk, 0, s, a);
      break;
    case kTaggPairKeys:
      hipLaunchKernelGGL(tagg_compose_kernel, dim3(tagg_blocks(ctx, (uint64_t)a.n)), blk, 0, s, a);
      break;
    case kTaggGroupStats:
      hipLaunchKernelGGL(tagg_gstats_kernel, dim3(tagg_blocks(ctx, (uint64_t)a.ngroups)), blk, 0, s, a);
      hipLaunchKernelGGL(tagg_glong_kernel, dim3(tagg_blocks(ctx, (uint64_t)a.n)), blk, 0, s, a, 0);
      hipLaunchKernelGGL(tagg_glong_kernel, dim3(tagg_blocks(ctx, (uint64_t)a.n)), blk, 0, s, a, 1);
      hipLaunchKernelGGL(tagg_glong_rows_kernel, dim3(tagg_blocks(ctx, (uint64_t)a.ngroups)), blk, 0, s, a);
      break;
    default:  // kTaggCells
      hipLaunchKernelGGL(tagg_cell_kernel, dim3(tagg_blocks(ctx, (uint64_t)a.ncells)), blk, 0, s, a);
      hipLaunchKernelGGL(tagg_cbig_kernel, wide, blk, 0, s, a);
      hipLaunchKernelGGL(tagg_all_kernel, dim3(tagg_blocks(ctx, (uint64_t)a.ngroups)), blk, 0, s, a);
      break;
  }
  return hipGetLastError();
}

}  // namespace gf
