// k_tjoin.hip -- tJoin, the window-based trajectory join (tJoin/PointPointTJoinQuery.java windowBased /
// commonSingle, TJoinQuery.java): the distinct pairs of trajectories (t_o of the ordinary window, t_q of
// the query window) with a point of one within r of a point of the other, per pair the latest matching
// query point and the first matching ordinary point.  The contract is include/geoflink_hip.h's;
// tjoin.cpp drives the launches.  The point pairs are those of gf_join_pp (k_join.hip's cell probe is
// the model: the query side bucketed by its clamped cell, every ordinary point of a valid cell walking
// the bucket rows within c layers of its cell), but no pair is ever written.
//
//   tjoin_qprep     per query point: ~ts (ascending = ts descending) and bucket key << 32 | trajectory
//   (radix)         the query points sorted by (trajectory, ts descending, index) -> ord
//   tjoin_qrank     qrank = the point's position among its trajectory's points in that order; a copy of
//                   ord turns (trajectory, qrank) back into a window index
//   (radix)         that order sorted stably by bucket key: every bucket sorted by (trajectory, qrank)
//   tjoin_qscatter  the bucket-order arrays (x, y | real cell, trajectory | qrank) and the run flags: a
//                   RUN is the points of one trajectory in one bucket, best qrank first
//   (scan) tjoin_runs / tjoin_runend
//                   run starts, bucket offsets, and per element run_end = the position after its run
//   tjoin_ocell     per ordinary point its cell key (outside the grid: one key past the cells)
//   (radix)         the ordinary points sorted by cell: a wave's lanes then walk the same bucket rows
//   tjoin_probe     one lane per ordinary point of a valid cell: the Chebyshev test on the real cells,
//                   the distance test; inside a run the FIRST match is the run's best qrank, so the lane
//                   inserts it and jumps to run_end.  Insert: the row's slot in an open-addressing table
//                   is claimed by one 64-bit compare-and-swap of t_o << 32 | t_q, then atomicMin of the
//                   qrank and of the ordinary index -- integer minima of sets, so the table's CONTENT
//                   does not depend on arrival order (which slot a key lands in does; no output names a
//                   slot).  A lane keeps its last key's slot to skip the search.  Rows are counted per
//                   shard of home slots; a shard past its share of half the table sets the overflow
//                   word, every lane stops, and the host doubles the table and probes again.
//   tjoin_occupied (scan) tjoin_compact
//                   the occupied slots packed
//   (radix)         sorted by (t_o, t_q): unique keys, so the order is the keys' own
//   tjoin_rows      the row table: keys, p_first, q_latest from qrank, emit from the two seg_off tables,
//                   marks of the emitted rows' trajectories per side
//   (scans) tjoin_slots / tjoin_tlist (scans) tjoin_totals / tjoin_gather
//                   the rows' slots, the emitted trajectories per side in ascending rank, their CSR
// No float is ever added and every reduction is an integer minimum or a count: results are identical
// from run to run.
#define GF_TU_NAME k_tjoin_hip
#include "gf_buildtag.hpp"  // first: records this unit's command-line defines

#include <algorithm>

#include "gf_internal.hpp"

namespace gf {

#define GF_TJOIN_LOOP(i, n)                                                                          \
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < (n); i += (int64_t)gridDim.x * kBlock)

__global__ __launch_bounds__(kBlock) void tjoin_qprep_kernel(TjoinArgs a) {
  GF_TJOIN_LOOP(i, a.nq) {
    a.its[i] = ~(unsigned long long)a.qts[i];
    a.comp[i] = ((unsigned long long)a.bkey[i] << 32) | a.qdid[i];
  }
}

__global__ __launch_bounds__(kBlock) void tjoin_qrank_kernel(TjoinArgs a) {
  GF_TJOIN_LOOP(p, a.nq) {
    const uint32_t i = a.ord[p];
    a.qrank[i] = (uint32_t)p - a.qseg[a.qdid[i]];  // (ord lists the trajectories in rank order, as gq's perm does)
    a.qord[p] = i;
  }
}

__global__ __launch_bounds__(kBlock) void tjoin_qscatter_kernel(TjoinArgs a) {
  GF_TJOIN_LOOP(s, a.nq) {
    const uint32_t i = a.sidx[s];
    a.sxy[s] = make_double2(a.qx[i], a.qy[i]);
    a.smeta[s] = make_int4(a.qcx[i], a.qcy[i], (int32_t)a.qdid[i], 0);
    a.sqr[s] = a.qrank[i];
    a.flag[s] = s == 0 || a.comp[i] != a.comp[a.sidx[s - 1]] ? 1u : 0u;
  }
}

// (after the scan of the flags) run starts and bucket offsets: the element that opens a bucket fills
// the offsets of the empty buckets before it too, the last element those after it
__global__ __launch_bounds__(kBlock) void tjoin_runs_kernel(TjoinArgs a) {
  GF_TJOIN_LOOP(s, a.nq) {
    if (a.flag[s]) a.rstart[a.fscan[s]] = (uint32_t)s;
    const int64_t b = (int64_t)(a.comp[a.sidx[s]] >> 32);
    const int64_t prev = s == 0 ? -1 : (int64_t)(a.comp[a.sidx[s - 1]] >> 32);
    for (int64_t k = prev + 1; k <= b; ++k) a.boff[k] = (uint32_t)s;
    if (s == a.nq - 1) {
      a.rstart[a.fscan[a.nq]] = (uint32_t)a.nq;
      for (int64_t k = b + 1; k <= a.nb; ++k) a.boff[k] = (uint32_t)a.nq;
    }
  }
}

__global__ __launch_bounds__(kBlock) void tjoin_runend_kernel(TjoinArgs a) {
  GF_TJOIN_LOOP(s, a.nq) {
    a.smeta[s].w = (int32_t)a.rstart[a.fscan[s] + a.flag[s]];  // run id = fscan + flag - 1; the next run's start
  }
}

__global__ __launch_bounds__(kBlock) void tjoin_ocell_kernel(TjoinArgs a) {
  GF_TJOIN_LOOP(p, a.no) {
    const int32_t cx = cell_index(a.ox[p], a.minX, a.cl), cy = cell_index(a.oy[p], a.minY, a.cl);
    const bool in = cx >= 0 && cy >= 0 && cx < a.qn && cy < a.qn;
    a.ocell[p] = in ? (unsigned long long)cy * (unsigned long long)a.qn + (unsigned long long)cx
                    : (unsigned long long)a.qn * (unsigned long long)a.qn;
  }
}

__device__ __forceinline__ uint64_t tjoin_hash(uint64_t k) {
  k ^= k >> 33;
  k *= 0xff51afd7ed558ccdull;
  k ^= k >> 33;
  k *= 0xc4ceb9fe1a85ec53ull;
  k ^= k >> 33;
  return k;
}

__device__ __forceinline__ uint32_t tjoin_peek(const uint32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The row (t_o, t_q) takes qrank qr and ordinary index p.  false: the pass is void (overflow), stop.
__device__ __forceinline__ bool tjoin_insert(const TjoinTable& T, unsigned long long key, uint32_t qr, uint32_t p,
                                             unsigned long long& last_key, uint64_t& last_slot) {
  uint64_t h = last_slot;
  if (key != last_key) {
    const uint64_t home = tjoin_hash(key) & T.mask;
    h = home;
    for (uint64_t step = 0;; ++step) {
      if (step > T.mask) {  // every slot seen and none free (rows claimed before the overflow word was seen)
        atomicExch(T.overflow, 1u);
        return false;
      }
      unsigned long long cur = __hip_atomic_load(&T.key[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (cur == kTjoinEmpty) {
        if (tjoin_peek(T.overflow)) return false;
        cur = atomicCAS(&T.key[h], kTjoinEmpty, key);
        if (cur == kTjoinEmpty) {  // a new row, claimed by this lane alone: count it once
          if (atomicAdd(&T.count[(home >> T.shard_shift) * kTjoinShardStride], 1u) >= T.shard_cap) {
            atomicExch(T.overflow, 1u);
            return false;
          }
          break;
        }
      }
      if (cur == key) break;
      h = (h + 1) & T.mask;
    }
    last_key = key;
    last_slot = h;
  }
  // (the minima start at 0xFFFFFFFF from the clear before the launch: no order with the claim is needed)
  if (tjoin_peek(&T.qrank[h]) > qr) atomicMin(&T.qrank[h], qr);
  if (tjoin_peek(&T.pfirst[h]) > p) atomicMin(&T.pfirst[h], p);
  return true;
}

__global__ __launch_bounds__(kBlock) void tjoin_probe_kernel(TjoinArgs a) {
  const int64_t W = (int64_t)a.qn + 2, qn = a.qn, c = a.c;
  unsigned long long last_key = kTjoinEmpty;
  uint64_t last_slot = 0;
  GF_TJOIN_LOOP(j, a.no) {
    if (tjoin_peek(a.t.overflow)) return;
    const uint32_t p = a.oord[j];
    const double px = a.ox[p], py = a.oy[p];
    const int32_t cx = cell_index(px, a.minX, a.cl), cy = cell_index(py, a.minY, a.cl);
    if (!(cx >= 0 && cy >= 0 && cx < a.qn && cy < a.qn)) continue;  // p.gridID must be a replicated key
    const uint32_t to = a.odid[p];
    int64_t x0, x1, y0, y1;
    if (c < 0) {
      x0 = -1; x1 = qn; y0 = -1; y1 = qn;
    } else {
      x0 = cx - c < -1 ? -1 : cx - c; x1 = cx + c > qn ? qn : cx + c;
      y0 = cy - c < -1 ? -1 : cy - c; y1 = cy + c > qn ? qn : cy + c;
    }
    for (int64_t ry = y0; ry <= y1; ++ry) {
      const int64_t row = (ry + 1) * W;
      const uint32_t b = a.boff[row + x0 + 1], e = a.boff[row + x1 + 2];
      if (b >= e) continue;
      // one element ahead: the loads of s + 1 are in flight while s is tested (a match jumps to run_end and
      // fetches anew)
      uint32_t s = b;
      int4 m = a.smeta[s];
      double2 q = a.sxy[s];
      for (;;) {
        const uint32_t s1 = s + 1;
        int4 m1 = m;
        double2 q1 = q;
        if (s1 < e) {
          m1 = a.smeta[s1];
          q1 = a.sxy[s1];
        }
        uint32_t next = s1;
        const uint32_t run_end = (uint32_t)m.w > s ? (uint32_t)m.w : s1;  // (> s by construction)
        if (a.single && (uint32_t)m.z == to) {  // the whole run is p's own trajectory
          next = run_end;
        } else {
          bool ok = true;
          if (c >= 0) {
            const int64_t ddx = (int64_t)m.x - cx, ddy = (int64_t)m.y - cy;
            ok = !(ddx > c || ddx < -c || ddy > c || ddy < -c);
          }
          if (ok && distance(px, py, q.x, q.y, 0) <= a.r) {
            if (!tjoin_insert(a.t, ((unsigned long long)to << 32) | (uint32_t)m.z, a.sqr[s], p, last_key, last_slot)) return;
            next = run_end;
          }
        }
        if (next >= e) break;
        if (next == s1) {
          m = m1;
          q = q1;
        } else {
          m = a.smeta[next];
          q = a.sxy[next];
        }
        s = next;
      }
    }
  }
}

__global__ __launch_bounds__(kBlock) void tjoin_occupied_kernel(TjoinArgs a) {
  GF_TJOIN_LOOP(h, a.slots) { a.occ[h] = a.t.key[h] != kTjoinEmpty ? 1u : 0u; }
}

__global__ __launch_bounds__(kBlock) void tjoin_compact_kernel(TjoinArgs a) {
  GF_TJOIN_LOOP(h, a.slots) {
    const unsigned long long k = a.t.key[h];
    if (k != kTjoinEmpty) {
      const uint32_t c = a.cpos[h];
      a.rkey[c] = k;
      a.rqr[c] = a.t.qrank[h];
      a.rpf[c] = a.t.pfirst[h];
    }
  }
}

__global__ __launch_bounds__(kBlock) void tjoin_rows_kernel(TjoinArgs a) {
  const int lane = threadIdx.x & 63;
  for (int64_t j0 = (int64_t)blockIdx.x * kBlock, j = j0 + threadIdx.x; j0 < a.rows;
       j0 += (int64_t)gridDim.x * kBlock, j = j0 + threadIdx.x) {
    bool emit = false;
    if (j < a.rows) {
      const uint32_t cpt = a.rorder[j];
      const unsigned long long k = a.rkey[cpt];
      const uint32_t to = (uint32_t)(k >> 32), tq = (uint32_t)k;
      emit = a.oseg[to + 1] - a.oseg[to] >= 2u && a.qseg[tq + 1] - a.qseg[tq] >= 2u;
      a.o_okey[j] = a.okeys[to];
      a.o_qkey[j] = a.qkeys[tq];
      a.o_pfirst[j] = a.rpf[cpt];
      a.o_qlatest[j] = a.qord[a.qseg[tq] + a.rqr[cpt]];
      a.o_emit[j] = emit ? 1 : 0;
      a.o_to[j] = to;
      a.o_tq[j] = tq;
      if (emit) {  // (every writer stores the same 1)
        a.mark[0][to] = 1u;
        a.mark[1][tq] = 1u;
      }
    }
    const uint32_t cnt = (uint32_t)__popcll(__ballot(emit));
    if (lane == 0 && cnt) atomicAdd(&a.counters[0], cnt);
  }
}

__global__ __launch_bounds__(kBlock) void tjoin_slots_kernel(TjoinArgs a) {
  GF_TJOIN_LOOP(j, a.rows) {
    const bool emit = a.o_emit[j] != 0;
    a.o_oslot[j] = emit ? (int32_t)a.mrank[0][a.o_to[j]] : -1;
    a.o_qslot[j] = emit ? (int32_t)a.mrank[1][a.o_tq[j]] : -1;
  }
}

// one side: the emitted trajectories in ascending rank and their lengths (tlen zeroed before)
__global__ __launch_bounds__(kBlock) void tjoin_tlist_kernel(TjoinArgs a) {
  const uint32_t* seg = a.side ? a.qseg : a.oseg;
  GF_TJOIN_LOOP(t, a.nt) {
    if (a.mark[a.side][t]) {
      const uint32_t s = a.mrank[a.side][t];
      a.tlist[a.side][s] = (uint32_t)t;
      a.tlen[a.side][s] = seg[t + 1] - seg[t];
    }
  }
}

__global__ void tjoin_totals_kernel(TjoinArgs a) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    a.counters[1] = a.mrank[0][a.nto];
    a.counters[2] = a.toff[0][a.nto];
    a.counters[3] = a.mrank[1][a.ntq];
    a.counters[4] = a.toff[1][a.ntq];
  }
}

// one side's CSR: the pattern of tknn_gather_kernel (a binary search of the trajectory per output point)
__global__ __launch_bounds__(kBlock) void tjoin_gather_kernel(TjoinArgs a) {
  const int sd = a.side;
  const uint32_t *seg = sd ? a.qseg : a.oseg, *perm = sd ? a.qperm : a.operm, *off = a.toff[sd];
  const double *x = sd ? a.qx : a.ox, *y = sd ? a.qy : a.oy;
  const int64_t *ts = sd ? a.qts : a.ots, *keys = sd ? a.qkeys : a.okeys;
  GF_TJOIN_LOOP(u, a.m) { a.c_keys[u] = keys[a.tlist[sd][u]]; }
  GF_TJOIN_LOOP(p, a.npts) {
    int64_t lo = 0, hi = a.m;  // the trajectory u with off[u] <= p < off[u + 1] (off[m] = npts > p)
    while (hi - lo > 1) {
      const int64_t mid = lo + (hi - lo) / 2;
      if ((int64_t)off[mid] <= p) lo = mid; else hi = mid;
    }
    const uint32_t t = a.tlist[sd][lo];
    const uint32_t i = perm[seg[t] + ((uint32_t)p - off[lo])];
    a.c_x[p] = x[i];
    a.c_y[p] = y[i];
    a.c_ts[p] = ts[i];
    a.c_idx[p] = i;
  }
}

static unsigned tjoin_blocks(gf_ctx* ctx, uint64_t items) {
  const uint64_t b = (items + kBlock - 1) / kBlock, cap = (uint64_t)ctx->num_cus * 8;
  return (unsigned)(b < 1 ? 1 : (b > cap ? cap : b));
}

hipError_t launch_tjoin(gf_ctx* ctx, int stage, const TjoinArgs& a) {
  hipStream_t s = ctx->stream;
  KTimer timer(ctx, GF_K_TJOIN);
  const dim3 blk(kBlock);
  const dim3 gq(tjoin_blocks(ctx, (uint64_t)a.nq)), go(tjoin_blocks(ctx, (uint64_t)a.no)),
      gs(tjoin_blocks(ctx, (uint64_t)a.slots)), gr(tjoin_blocks(ctx, (uint64_t)a.rows));
  switch (stage) {
    case kTjoinQueryKeys: hipLaunchKernelGGL(tjoin_qprep_kernel, gq, blk, 0, s, a); break;
    case kTjoinQueryRank: hipLaunchKernelGGL(tjoin_qrank_kernel, gq, blk, 0, s, a); break;
    case kTjoinQueryScatter: hipLaunchKernelGGL(tjoin_qscatter_kernel, gq, blk, 0, s, a); break;
    case kTjoinRunStarts: hipLaunchKernelGGL(tjoin_runs_kernel, gq, blk, 0, s, a); break;
    case kTjoinRunEnds: hipLaunchKernelGGL(tjoin_runend_kernel, gq, blk, 0, s, a); break;
    case kTjoinCellKeys: hipLaunchKernelGGL(tjoin_ocell_kernel, go, blk, 0, s, a); break;
    case kTjoinProbe: {
      // every lane walks its own bucket rows: as many blocks as there are points, so that the points of
      // one crowded cell (neighbours in the probe's order) spread over the CUs
      const uint64_t b = ((uint64_t)a.no + kBlock - 1) / kBlock;
      hipLaunchKernelGGL(tjoin_probe_kernel, dim3((unsigned)(b < 1 ? 1 : (b > (1u << 20) ? (1u << 20) : b))), blk, 0, s, a);
      break;
    }
    case kTjoinOccupied: hipLaunchKernelGGL(tjoin_occupied_kernel, gs, blk, 0, s, a); break;
    case kTjoinCompact: hipLaunchKernelGGL(tjoin_compact_kernel, gs, blk, 0, s, a); break;
    case kTjoinRows: hipLaunchKernelGGL(tjoin_rows_kernel, gr, blk, 0, s, a); break;
    case kTjoinRowSlots: hipLaunchKernelGGL(tjoin_slots_kernel, gr, blk, 0, s, a); break;
    case kTjoinSideList: hipLaunchKernelGGL(tjoin_tlist_kernel, dim3(tjoin_blocks(ctx, (uint64_t)a.nt)), blk, 0, s, a); break;
    case kTjoinTotals: hipLaunchKernelGGL(tjoin_totals_kernel, dim3(1), dim3(64), 0, s, a); break;
    default:  // kTjoinGather
      hipLaunchKernelGGL(tjoin_gather_kernel, dim3(tjoin_blocks(ctx, (uint64_t)std::max(a.npts, a.m))), blk, 0, s, a);
      break;
  }
  return hipGetLastError();
}

}  // namespace gf
