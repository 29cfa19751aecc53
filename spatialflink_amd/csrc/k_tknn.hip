// k_tknn.hip -- tKnn, the window-based trajectory kNN (tKnn/PointPointTKNNQuery.java windowBased /
// windowBasedNaive, TKNNQuery.java:50-101 kNNEvaluationWindowed): the k trajectories nearest to a query
// point, a trajectory's distance being that of its nearest point in a cell of N that made the cell's
// own top-k list.  The contract is include/geoflink_hip.h's; tknn.cpp drives the launches.
//
//   tknn_scan       the window's ONE pass (x, y, trajectory id: 20 B per point): K1's cell, the N test
//                   (an integer rectangle, or every cell for NAIVE), the distance; the points in N are
//                   appended as entries (pack(cx, cy), t, distance bits, window index) with one atomic
//                   per block and 1024 points.  The entries' order is whatever the atomics gave: no later
//                   stage reads it.
//   (group)         dense cell id per entry (group_dense_ids over the packed cells)
//   tknn_compose    comp = cell id << 32 | t
//   (group)         dense pair id per entry, the pairs' keys
//   tknn_pair_init / tknn_pair_min / tknn_pair_nan
//                   per pair the smallest window index (atomicMin) and the smallest distance (atomicMin
//                   on the bits: distances are never negative, NaN is one pattern above +inf); then the
//                   entry that IS the pair's first point overwrites the minimum with NaN if its own
//                   distance is NaN (the reference's `new < cur` never replaces a NaN).  A wave whose 64
//                   entries share a pair reduces first and sends one atomic; a word that already beats
//                   the candidate is left alone -- a pair holding most of the window settles at once.
//   (radix)         the pairs sorted stably by cell id -> gperm, cell_off
//   tknn_rank_small cells below big_cell pairs: every pair counts the pairs of its cell that order
//                   before it by (d, t); rank < k puts it on the list
//   (radix)         if some cell is big: all pairs sorted by (cell id, d, t), four key words LSD
//   tknn_rank_big   pairs of big cells: rank = sorted position - the cell's start
//   tknn_traj_init / tknn_combine
//                   listed pairs: atomicMin of the bits into D_t, atomicAdd into cells_t
//   tknn_survive    in a list and >= 2 points in the whole window
//   (scan, radix)   the survivors, ascending t, sorted stably by D_t's two words = by (D_t, t)
//   tknn_rows       the first k of them: key, D_t, cells_t, length
//   tknn_gather     the rows' segments in result order (a binary search of the row per output point)
// Determinism: dense cell and pair ids depend on the entries' order, and nothing else does -- minima
// and counts of sets, a rank among the (d, t) of one cell (t is unique inside a cell), and stable
// sorts of unique keys.  No output names a cell id or a pair id.  No float is ever added.
#define GF_TU_NAME k_tknn_hip
#include "gf_buildtag.hpp"  // first: records this unit's command-line defines

#include "gf_internal.hpp"

namespace gf {

// block-uniform loop over items [0, n): every lane of a block runs every iteration (the bodies use
// wave ballots), `i < n` masks the tail
#define GF_TKNN_LOOP(i, n)                                                                                      \
  for (int64_t i##0 = (int64_t)blockIdx.x * kBlock, i = i##0 + threadIdx.x; i##0 < (n);                         \
       i##0 += (int64_t)gridDim.x * kBlock, i = i##0 + threadIdx.x)

// Four points per lane and iteration (their loads are independent: four in flight per lane), and ONE
// atomic per block and iteration: the blocks' waves add up their ballots in LDS first.  Atomics on one
// address serialise (~10 ns each, measured: a counter bumped once per wave and 64 points cost 1.5 ms per
// 10M points in N); per 1024 points they cost a sixteenth of that.
constexpr int kTknnScanU = 4;
__global__ __launch_bounds__(kBlock) void tknn_scan_kernel(TknnArgs a) {
  constexpr int U = kTknnScanU, W = kBlock / 64;
  __shared__ uint32_t wcnt[2][W];  // by iteration parity: the next iteration writes the other set
  __shared__ uint32_t bbase[2];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const uint64_t below = (1ull << lane) - 1ull;
  int par = 0;
  for (int64_t i0 = (int64_t)blockIdx.x * (kBlock * U); i0 < a.n; i0 += (int64_t)gridDim.x * (kBlock * U), par ^= 1) {
    double px[U], py[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t i = i0 + u * kBlock + threadIdx.x;
      px[u] = i < a.n ? a.x[i] : 0.0;
      py[u] = i < a.n ? a.y[i] : 0.0;
    }
    int32_t cx[U], cy[U];
    uint64_t bal[U];
    uint32_t cnt = 0;  // wave-uniform
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t i = i0 + u * kBlock + threadIdx.x;
      cx[u] = cell_index(px[u], a.minX, a.cl);
      cy[u] = cell_index(py[u], a.minY, a.cl);
      const bool in = i < a.n && (a.naive || (cx[u] >= a.xlo && cx[u] <= a.xhi && cy[u] >= a.ylo && cy[u] <= a.yhi));
      bal[u] = __ballot(in);
      cnt += (uint32_t)__popcll(bal[u]);
    }
    if (lane == 0) wcnt[par][w] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
      uint32_t tot = 0;
#pragma unroll
      for (int q = 0; q < W; ++q) tot += wcnt[par][q];
      bbase[par] = tot ? atomicAdd(&a.counters[0], tot) : 0u;  // (at most n entries: every point appends once)
    }
    __syncthreads();
    uint32_t base = bbase[par];
#pragma unroll
    for (int q = 0; q < W; ++q) base += q < w ? wcnt[par][q] : 0u;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if ((bal[u] >> lane) & 1ull) {
        const int64_t i = i0 + u * kBlock + threadIdx.x;
        const uint32_t pos = base + (uint32_t)__popcll(bal[u] & below);
        const double d = sqrt((a.qy - py[u]) * (a.qy - py[u]) + (a.qx - px[u]) * (a.qx - px[u]));  // DistanceFunctions.java:60-63
        a.e_ckey[pos] = (int64_t)(((uint64_t)(uint32_t)cx[u] << 32) | (uint32_t)cy[u]);
        a.e_t[pos] = a.did[i];
        a.e_d[pos] = d == d ? (unsigned long long)dbits(d) : kTknnNaN;
        a.e_i[pos] = (uint32_t)i;
      }
      base += (uint32_t)__popcll(bal[u]);
    }
  }
}

__global__ __launch_bounds__(kBlock) void tknn_compose_kernel(TknnArgs a) {
  GF_TKNN_LOOP(j, a.m) {
    if (j < a.m) a.comp[j] = (int64_t)(((uint64_t)a.cid[j] << 32) | a.e_t[j]);
  }
}

__global__ __launch_bounds__(kBlock) void tknn_pair_init_kernel(TknnArgs a) {
  GF_TKNN_LOOP(q, a.npairs) {
    if (q < a.npairs) {
      a.p_first[q] = 0xFFFFFFFFu;
      a.p_d[q] = kTknnNone;
      a.p_cell[q] = (uint32_t)((uint64_t)a.pkeys[q] >> 32);
      a.p_rec[q] = 0u;
    }
  }
}

__global__ __launch_bounds__(kBlock) void tknn_pair_min_kernel(TknnArgs a) {
  const int lane = threadIdx.x & 63;
  GF_TKNN_LOOP(j, a.m) {
    const bool valid = j < a.m;
    uint32_t q = 0xFFFFFFFFu, i = 0xFFFFFFFFu;
    unsigned long long d = kTknnNone;
    if (valid) { q = a.pid[j]; i = a.e_i[j]; d = a.e_d[j]; }
    const bool uniform = __all(q == __shfl(q, 0, 64)) && valid;  // (valid: lane 0's, so every lane's)
    if (uniform) {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const uint32_t ui = __shfl_xor(i, o, 64);
        const unsigned long long ud = __shfl_xor(d, o, 64);
        if (ui < i) i = ui;
        if (ud < d) d = ud;
      }
    }
    if (valid && (!uniform || lane == 0)) {
      if (__hip_atomic_load(&a.p_first[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > i) atomicMin(&a.p_first[q], i);
      if (__hip_atomic_load(&a.p_d[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > d) atomicMin(&a.p_d[q], d);
    }
  }
}

// (one writer per pair: window indices are distinct)
__global__ __launch_bounds__(kBlock) void tknn_pair_nan_kernel(TknnArgs a) {
  GF_TKNN_LOOP(j, a.m) {
    if (j < a.m && a.e_d[j] == kTknnNaN) {
      const uint32_t q = a.pid[j];
      if (a.p_first[q] == a.e_i[j]) a.p_d[q] = kTknnNaN;
    }
  }
}

// (d, t) of pair q orders before (d0, t0)
__device__ __forceinline__ bool tknn_before(const TknnArgs& a, uint32_t q, unsigned long long d0, uint32_t t0) {
  const unsigned long long d = a.p_d[q];
  return d < d0 || (d == d0 && (uint32_t)a.pkeys[q] < t0);
}

__global__ __launch_bounds__(kBlock) void tknn_rank_small_kernel(TknnArgs a) {
  const int lane = threadIdx.x & 63;
  uint32_t nbig = 0;  // this lane's pairs of big cells: one atomic per wave at the end (see tknn_scan)
  GF_TKNN_LOOP(s, a.npairs) {
    bool is_big = false;
    if (s < a.npairs) {
      const uint32_t c = a.gcell[s], b = a.cell_off[c], e = a.cell_off[c + 1];
      if (e - b >= a.big_cell) {
        is_big = true;
      } else {
        const uint32_t q = a.gperm[s];
        const unsigned long long d0 = a.p_d[q];
        const uint32_t t0 = (uint32_t)a.pkeys[q];
        uint32_t rank = 0;
        for (uint32_t u = b; u < e; ++u) rank += tknn_before(a, a.gperm[u], d0, t0) ? 1u : 0u;
        a.p_rec[q] = rank < (uint32_t)a.k ? 1u : 0u;
      }
    }
    nbig += is_big ? 1u : 0u;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) nbig += __shfl_xor(nbig, o, 64);
  if (lane == 0 && nbig) atomicAdd(&a.counters[1], nbig);
}

__global__ __launch_bounds__(kBlock) void tknn_rank_big_kernel(TknnArgs a) {
  GF_TKNN_LOOP(s, a.npairs) {
    if (s < a.npairs) {
      const uint32_t q = a.sperm[s], c = a.p_cell[q], b = a.cell_off[c], e = a.cell_off[c + 1];
      if (e - b >= a.big_cell) a.p_rec[q] = (uint32_t)s - b < (uint32_t)a.k ? 1u : 0u;
    }
  }
}

__global__ __launch_bounds__(kBlock) void tknn_traj_init_kernel(TknnArgs a) {
  GF_TKNN_LOOP(t, a.ntraj) {
    if (t < a.ntraj) {
      a.tr_D[t] = kTknnNone;
      a.tr_cells[t] = 0u;
    }
  }
}

__global__ __launch_bounds__(kBlock) void tknn_combine_kernel(TknnArgs a) {
  const int lane = threadIdx.x & 63;
  uint32_t nrec = 0;  // this lane's records: one atomic per wave at the end
  GF_TKNN_LOOP(q, a.npairs) {
    const bool rec = q < a.npairs && a.p_rec[q] != 0u;
    if (rec) {
      const uint32_t t = (uint32_t)a.pkeys[q];
      atomicMin(&a.tr_D[t], a.p_d[q]);
      atomicAdd(&a.tr_cells[t], 1u);
    }
    nrec += rec ? 1u : 0u;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) nrec += __shfl_xor(nrec, o, 64);
  if (lane == 0 && nrec) atomicAdd(&a.counters[2], nrec);
}

__global__ __launch_bounds__(kBlock) void tknn_survive_kernel(TknnArgs a) {
  GF_TKNN_LOOP(t, a.ntraj) {
    if (t < a.ntraj) a.surv[t] = a.tr_cells[t] > 0u && a.seg_off[t + 1] - a.seg_off[t] >= 2u ? 1u : 0u;
  }
}

__global__ __launch_bounds__(kBlock) void tknn_slist_kernel(TknnArgs a) {
  GF_TKNN_LOOP(t, a.ntraj) {
    if (t < a.ntraj && a.surv[t]) a.slist[a.srank[t]] = (uint32_t)t;
  }
}

__global__ __launch_bounds__(kBlock) void tknn_rows_kernel(TknnArgs a) {
  GF_TKNN_LOOP(j, a.rows) {
    if (j < a.rows) {
      const uint32_t t = a.slist[a.order[j]];
      a.o_key[j] = a.tkeys[t];
      a.o_dist[j] = from_bits(a.tr_D[t]);
      a.o_cells[j] = (int32_t)a.tr_cells[t];
      a.o_traj[j] = t;
      a.o_len[j] = a.seg_off[t + 1] - a.seg_off[t];
    }
  }
}

__global__ __launch_bounds__(kBlock) void tknn_gather_kernel(TknnArgs a) {
  GF_TKNN_LOOP(p, a.npts) {
    if (p < a.npts) {
      int64_t lo = 0, hi = a.rows;  // the row j with o_off[j] <= p < o_off[j + 1] (o_off[rows] = npts > p)
      while (hi - lo > 1) {
        const int64_t mid = lo + (hi - lo) / 2;
        if ((int64_t)a.o_off[mid] <= p) lo = mid; else hi = mid;
      }
      const uint32_t t = a.o_traj[lo];
      const uint32_t i = a.perm[a.seg_off[t] + ((uint32_t)p - a.o_off[lo])];
      a.o_x[p] = a.x[i];
      a.o_y[p] = a.y[i];
      a.o_ts[p] = a.ts[i];
      a.o_idx[p] = i;
    }
  }
}

__global__ __launch_bounds__(kBlock) void tknn_word_kernel(const unsigned long long* __restrict__ src,
                                                           const uint32_t* __restrict__ index, int shift,
                                                           const uint32_t* __restrict__ cur, int64_t cnt,
                                                           uint32_t* __restrict__ out) {
  GF_TKNN_LOOP(p, cnt) {
    if (p < cnt) {
      const uint32_t item = cur ? cur[p] : (uint32_t)p;
      out[p] = (uint32_t)(src[index ? index[item] : item] >> shift);
    }
  }
}

static unsigned tknn_blocks(gf_ctx* ctx, uint64_t items) {
  const uint64_t b = (items + kBlock - 1) / kBlock, cap = (uint64_t)ctx->num_cus * 8;
  return (unsigned)(b < 1 ? 1 : (b > cap ? cap : b));
}

hipError_t launch_tknn(gf_ctx* ctx, int stage, const TknnArgs& a) {
  hipStream_t s = ctx->stream;
  KTimer timer(ctx, GF_K_TKNN);
  const dim3 blk(kBlock);
  const dim3 gn(tknn_blocks(ctx, (uint64_t)a.n)), gm(tknn_blocks(ctx, (uint64_t)a.m)),
      gp(tknn_blocks(ctx, (uint64_t)a.npairs)), gt(tknn_blocks(ctx, (uint64_t)a.ntraj));
  switch (stage) {
    case kTknnScanWindow:
      hipLaunchKernelGGL(tknn_scan_kernel, dim3(tknn_blocks(ctx, ((uint64_t)a.n + kTknnScanU - 1) / kTknnScanU)), blk, 0, s, a);
      break;
    case kTknnCompose: hipLaunchKernelGGL(tknn_compose_kernel, gm, blk, 0, s, a); break;
    case kTknnPairMin:
      hipLaunchKernelGGL(tknn_pair_init_kernel, gp, blk, 0, s, a);
      hipLaunchKernelGGL(tknn_pair_min_kernel, gm, blk, 0, s, a);
      hipLaunchKernelGGL(tknn_pair_nan_kernel, gm, blk, 0, s, a);
      break;
    case kTknnRankSmall: hipLaunchKernelGGL(tknn_rank_small_kernel, gp, blk, 0, s, a); break;
    case kTknnRankBig: hipLaunchKernelGGL(tknn_rank_big_kernel, gp, blk, 0, s, a); break;
    case kTknnCombine:
      hipLaunchKernelGGL(tknn_traj_init_kernel, gt, blk, 0, s, a);
      hipLaunchKernelGGL(tknn_combine_kernel, gp, blk, 0, s, a);
      hipLaunchKernelGGL(tknn_survive_kernel, gt, blk, 0, s, a);
      break;
    case kTknnSurvivors: hipLaunchKernelGGL(tknn_slist_kernel, gt, blk, 0, s, a); break;
    case kTknnRows: hipLaunchKernelGGL(tknn_rows_kernel, dim3(tknn_blocks(ctx, (uint64_t)a.rows)), blk, 0, s, a); break;
    default:  // kTknnGather
      hipLaunchKernelGGL(tknn_gather_kernel, dim3(tknn_blocks(ctx, (uint64_t)a.npts)), blk, 0, s, a);
      break;
  }
  return hipGetLastError();
}

hipError_t launch_tknn_word(gf_ctx* ctx, const unsigned long long* src, const uint32_t* index, int shift,
                            const uint32_t* cur, int64_t cnt, uint32_t* out) {
  KTimer timer(ctx, GF_K_TKNN);
  hipLaunchKernelGGL(tknn_word_kernel, dim3(tknn_blocks(ctx, (uint64_t)cnt)), dim3(kBlock), 0, ctx->stream, src, index,
                     shift, cur, cnt, out);
  return hipGetLastError();
}

}  // namespace gf
