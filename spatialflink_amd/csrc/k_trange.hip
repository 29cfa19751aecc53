// k_trange.hip -- tRange: which points of a window a polygon set contains (JTS contains: located
// INTERIOR -- include/geoflink_hip.h, "tRange / tFilter"), as a bitmap per point (RealTime,
// PointPolygonTRangeQuery.java:53-87) or as one flag per trajectory (WindowBased, :89-176).
//
//   trange_mark   one lane per point in window order, grid-stride.  The loads of an iteration (x, y,
//                 the dense trajectory id, the cell class from a clamped address) are issued before any
//                 branch that consumes them.  A point in a `none` cell is done; in trajectory mode a
//                 point whose trajectory's flag is already set is done too; an `inside` cell accepts a
//                 non-NaN point untested; otherwise the lane walks its cell's polygon list (a point
//                 outside the grid: the polygons whose bbox cells leave the grid and hold its cell) with
//                 contains_lane.  Polygons flagged wide are not walked by the lane: if no narrow one
//                 contained the point, the lane appends (point, polygon) per wide candidate to the
//                 worklist -- slots reserved per wave with a ballot and one atomic per round.
//   trange_wide   one wave per worklist entry (a block takes four): the ring's edges striped over the 64
//                 lanes, each lane running RayCrossingCounter's edge step on its edges; the boundary
//                 verdict is OR-reduced by ballot (boundary is absorbing), the crossing parity
//                 XOR-reduced as the popcount of the ballot of odd lanes.  Holes follow the shell on the
//                 same wave.  Parity and OR are order-free, so the verdict equals contains_lane's.
//   trange_count  point mode: the bitmap's set bits (the wide path ORs its bits in after the mark).
//
// The trajectory flag hit[t] only ever goes 0 -> 1 and every writer stores the same 1 (a plain store,
// no atomic).  A lane that reads a stale 0 merely repeats a test whose outcome can only set the flag
// again: the race decides how much work is skipped, never a result.  The two counters of gf_trange_info
// are taken before the flag is read, so they do not depend on it either.
#define GF_TU_NAME k_trange_hip
#include "gf_buildtag.hpp"  // first: records this unit's command-line defines

#include "gf_geom.hpp"
#include "gf_trange_plan.hpp"  // the cell classes kTr*

namespace gf {

// Geometry.contains(point): the shell envelope holds p (NaN and infinite coordinates fail), p is
// located INTERIOR of the shell and neither INTERIOR nor BOUNDARY of any hole
static __device__ __forceinline__ bool contains_lane(double px, double py, const PolyView& a, int p) {
  const int r0 = a.ring_off[p], r1 = a.ring_off[p + 1];
  const double* e = a.ring_env + 4 * r0;
  if (!(px >= e[0] && px <= e[1] && py >= e[2] && py <= e[3])) return false;
  const int v0 = a.vert_off[r0], nv = a.vert_off[r0 + 1] - v0;
  if (locate_in_ring(px, py, a.vx + v0, a.vy + v0, nv, e) != kLocInterior) return false;
  for (int h = r0 + 1; h < r1; ++h) {
    const int hv0 = a.vert_off[h], hnv = a.vert_off[h + 1] - hv0;
    if (locate_in_ring(px, py, a.vx + hv0, a.vy + hv0, hnv, a.ring_env + 4 * h) != kLocExterior) return false;
  }
  return true;
}

static __device__ __forceinline__ bool contains_wave(double px, double py, const PolyView& a, int p, int lane) {
  const int r0 = a.ring_off[p], r1 = a.ring_off[p + 1];
  const double* e = a.ring_env + 4 * r0;
  if (!(px >= e[0] && px <= e[1] && py >= e[2] && py <= e[3])) return false;
  const int v0 = a.vert_off[r0], nv = a.vert_off[r0 + 1] - v0;
  if (locate_in_ring_wave(px, py, a.vx + v0, a.vy + v0, nv, e, lane) != kLocInterior) return false;
  for (int h = r0 + 1; h < r1; ++h) {
    const int hv0 = a.vert_off[h], hnv = a.vert_off[h + 1] - hv0;
    if (locate_in_ring_wave(px, py, a.vx + hv0, a.vy + hv0, hnv, a.ring_env + 4 * h, lane) != kLocExterior) return false;
  }
  return true;
}

// the lane's candidate polygons: its cell's list, or (outside the grid) the extra ranges holding its cell
struct TrCursor {
  int cur, end;
  bool extras;
  int cx, cy;
};
static __device__ __forceinline__ int next_candidate(const TrangeArgs& a, TrCursor& c) {
  if (!c.extras) return c.cur < c.end ? a.cand_list[c.cur++] : -1;
  while (c.cur < c.end) {
    const int32_t* e = a.extra + 5 * (size_t)c.cur++;
    if (c.cx >= e[1] && c.cx <= e[2] && c.cy >= e[3] && c.cy <= e[4]) return e[0];
  }
  return -1;
}

template <bool kTraj>
__global__ __launch_bounds__(kBlock) void trange_mark_kernel(TrangeArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t gn = a.grid_n;
  unsigned long long n_cell = 0, n_inside = 0;  // this wave's (lane 0 keeps them)
  for (int64_t i0 = (int64_t)blockIdx.x * kBlock; i0 < a.n; i0 += (int64_t)gridDim.x * kBlock) {
    const int64_t i = i0 + threadIdx.x;
    const bool valid = i < a.n;
    const int64_t il = valid ? i : a.n - 1;  // clamped: the loads never branch
    const double px = a.x[il], py = a.y[il];
    uint32_t t = 0;
    if (kTraj) t = a.did[il];
    const int32_t cx = cell_index(px, a.minX, a.cl), cy = cell_index(py, a.minY, a.cl);
    const bool ingrid = cx >= 0 && cx < gn && cy >= 0 && cy < gn;
    const int64_t cell = ingrid ? (int64_t)cy * gn + cx : 0;
    const uint8_t c0 = a.cls[cell];
    TrCursor cur;
    cur.extras = !ingrid;
    cur.cx = cx; cur.cy = cy;
    uint8_t cls = kTrNone;
    if (valid) {
      if (ingrid) {
        cls = c0;
        cur.cur = a.cand_off[cell];
        cur.end = a.cand_off[cell + 1];
      } else {
        cur.cur = 0;
        cur.end = a.n_extra;
        TrCursor probe = cur;
        if (next_candidate(a, probe) >= 0) cls = kTrTest;
      }
    }
    const bool fast = cls == kTrInside && px == px && py == py;
    const unsigned long long m_cell = __ballot(cls != kTrNone), m_in = __ballot(fast);
    n_cell += __popcll(m_cell);
    n_inside += __popcll(m_in);
    bool need = cls != kTrNone;
    if (kTraj && need && a.hit[t]) need = false;
    bool verdict = false;
    int nwide = 0;
    const TrCursor start = cur;
    if (need) {
      if (fast) {
        verdict = true;
      } else if (cls == kTrTest) {
        for (int p = next_candidate(a, cur); p >= 0; p = next_candidate(a, cur)) {
          if (a.wide && a.wide[p]) { ++nwide; continue; }
          if (contains_lane(px, py, a.poly, p)) { verdict = true; break; }
        }
      }
    }
    if (kTraj) {
      if (verdict) a.hit[t] = 1u;
    } else {
      const unsigned long long bits = __ballot(verdict);
      if (lane == 0 && i < a.n) a.bitmap[i >> 6] = bits;
    }
    // the wide candidates of the points no narrow polygon contained: one worklist slot each
    bool more = need && !verdict && nwide > 0;
    cur = start;
    while (__ballot(more)) {  // wave-uniform: every lane of the wave takes every round
      int p = -1;
      if (more) {
        for (int q = next_candidate(a, cur); q >= 0; q = next_candidate(a, cur))
          if (a.wide[q]) { p = q; break; }
        if (p < 0) more = false;
      }
      const unsigned long long m = __ballot(p >= 0);
      if (!m) break;
      const int leader = __ffsll((long long)m) - 1;
      unsigned long long base = 0;
      if (lane == leader) base = atomicAdd(a.ctr, (unsigned long long)__popcll(m));
      base = __shfl(base, leader);
      const unsigned long long slot = base + __popcll(m & ((1ull << lane) - 1ull));
      if (p >= 0 && slot < a.work_cap) a.work[slot] = make_uint2((uint32_t)i, (uint32_t)p);
    }
  }
  if (kTraj && lane == 0) {
    if (n_cell) atomicAdd(a.ctr + 1, n_cell);
    if (n_inside) atomicAdd(a.ctr + 2, n_inside);
  }
}

template <bool kTraj>
__global__ __launch_bounds__(kBlock) void trange_wide_kernel(TrangeArgs a) {
  const int lane = threadIdx.x & 63;
  unsigned long long cnt = a.ctr[0];
  if (cnt > a.work_cap) cnt = a.work_cap;
  const int64_t waves = (int64_t)gridDim.x * (kBlock / 64);
  for (int64_t e = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6); e < (int64_t)cnt; e += waves) {
    const uint2 w = a.work[e];  // wave-uniform
    const uint32_t i = w.x;
    uint32_t t = 0;
    if (kTraj) {
      t = a.did[i];
      if (__ballot(a.hit[t] != 0)) continue;  // its trajectory got hit meanwhile
    }
    const bool in = contains_wave(a.x[i], a.y[i], a.poly, (int)w.y, lane);
    if (in && lane == 0) {
      if (kTraj) a.hit[t] = 1u;
      else atomicOr((unsigned long long*)a.bitmap + (i >> 6), 1ull << (i & 63));
    }
  }
}

__global__ __launch_bounds__(kBlock) void trange_count_kernel(TrangeArgs a) {
  const int64_t words = (a.n + 63) >> 6;
  unsigned long long c = 0;
  for (int64_t w = (int64_t)blockIdx.x * kBlock + threadIdx.x; w < words; w += (int64_t)gridDim.x * kBlock)
    c += __popcll(a.bitmap[w]);
  for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o);
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(a.ctr + 3, c);
}
__global__ void trange_count_store_kernel(TrangeArgs a) { *a.count = (int64_t)a.ctr[3]; }

static unsigned trange_blocks(gf_ctx* ctx, uint64_t items) {
  const uint64_t b = (items + kBlock - 1) / kBlock, cap = (uint64_t)ctx->num_cus * 8;
  return (unsigned)(b < 1 ? 1 : (b > cap ? cap : b));
}

hipError_t launch_trange(gf_ctx* ctx, int stage, const TrangeArgs& a) {
  KTimer timer(ctx, GF_K_TRANGE);
  hipStream_t s = ctx->stream;
  const dim3 blk(kBlock);
  const bool traj = a.did != nullptr;
  if (stage == kTrangeMark) {
    const dim3 g(trange_blocks(ctx, (uint64_t)a.n));
    if (traj) hipLaunchKernelGGL(trange_mark_kernel<true>, g, blk, 0, s, a);
    else hipLaunchKernelGGL(trange_mark_kernel<false>, g, blk, 0, s, a);
  } else if (stage == kTrangeWaves) {
    const dim3 g((unsigned)ctx->num_cus * 8);
    if (traj) hipLaunchKernelGGL(trange_wide_kernel<true>, g, blk, 0, s, a);
    else hipLaunchKernelGGL(trange_wide_kernel<false>, g, blk, 0, s, a);
  } else {
    hipLaunchKernelGGL(trange_count_kernel, dim3(trange_blocks(ctx, (uint64_t)((a.n + 63) >> 6))), blk, 0, s, a);
    hipLaunchKernelGGL(trange_count_store_kernel, dim3(1), dim3(1), 0, s, a);
  }
  return hipGetLastError();
}

}  // namespace gf
