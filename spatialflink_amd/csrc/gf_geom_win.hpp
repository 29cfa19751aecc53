// gf_geom_win.hpp -- what the geometry-window kernels of k_geom.hip (point queries), k_geompair.hip
// (polygon / linestring queries) and k_geomjoin.hip (the joins) share: slot reservation by wave ballot, the
// wave sum, the point-to-geometry distances by one wave, the emission of a hit into the bitmap or the kNN
// candidates, and the body of the classify pass.
#pragma once

#include "gf_geom.hpp"
#include "gf_geom_plan.hpp"

namespace gf {

// one slot per lane with c set: a ballot and one atomic per wave (every lane of the wave calls it)
template <class Store>
static __device__ __forceinline__ void geom_reserve(unsigned long long* ctr, bool c, Store&& store) {
  const unsigned long long m = __ballot(c);
  if (m == 0) return;
  const int lane = threadIdx.x & 63;
  const int leader = __ffsll((long long)m) - 1;
  unsigned long long base = 0;
  if (lane == leader) base = atomicAdd(ctr, (unsigned long long)__popcll(m));
  base = __shfl(base, leader, 64);
  if (c) store(base + (unsigned long long)__popcll(m & ((1ull << lane) - 1ull)));
}

static __device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;  // lane 0 holds the sum
}

// polygon_distance by one whole wave (every lane calls it with the same arguments; the same value in
// every lane): the wave passes of k_geom.hip and k_geomjoin.hip
static __device__ __forceinline__ double polygon_distance_wave(double px, double py, const PolyView& a, int p, int lane) {
  const int r0 = a.ring_off[p], r1 = a.ring_off[p + 1];
  if (px == px) {  // NaN x: containment skipped, as polygon_distance
    const int v0 = a.vert_off[r0], nv = a.vert_off[r0 + 1] - v0;
    const int loc = locate_in_ring_wave(px, py, a.vx + v0, a.vy + v0, nv, a.ring_env + 4 * r0, lane);
    if (loc == kLocBoundary) return 0.0;
    if (loc == kLocInterior) {
      bool inside = true;
      for (int h = r0 + 1; h < r1; ++h) {
        const int hv0 = a.vert_off[h], hnv = a.vert_off[h + 1] - hv0;
        const int hl = locate_in_ring_wave(px, py, a.vx + hv0, a.vy + hv0, hnv, a.ring_env + 4 * h, lane);
        if (hl == kLocInterior) { inside = false; break; }
        if (hl == kLocBoundary) return 0.0;
      }
      if (inside) return 0.0;
    }
  }
  double md = 1.7976931348623157e308;
  for (int rg = r0; rg < r1; ++rg) {
    const int v0 = a.vert_off[rg], nv = a.vert_off[rg + 1] - v0;
    if (env_point_distance(a.ring_env + 4 * rg, px, py) > md) continue;  // md is the wave's: the serial skip
    double l = md;
    for (int i = lane; i < nv - 1; i += 64) {
      const double d = point_to_segment(px, py, a.vx[v0 + i], a.vy[v0 + i], a.vx[v0 + i + 1], a.vy[v0 + i + 1], a.metric);
      if (d < l) l = d;
    }
    md = wave_min(l);
    if (md <= 0.0) return md;
  }
  return md;
}
static __device__ __forceinline__ double chain_distance_wave(double px, double py, const ChainView& a, int l, int lane) {
  const int v0 = a.vert_off[l], nseg = a.vert_off[l + 1] - v0 - 1;
  double md = 1.7976931348623157e308;
  for (int i = lane; i < nseg; i += 64) {
    const double d = point_to_segment(px, py, a.vx[v0 + i], a.vy[v0 + i], a.vx[v0 + i + 1], a.vy[v0 + i + 1], a.metric);
    if (d < md) md = d;
  }
  return wave_min(md);
}

// a hit of object i at distance d: its bit, or its candidate (every lane of the wave calls it)
static __device__ __forceinline__ void geom_emit(const GeomArgs& a, bool hit, uint32_t i, double d) {
  if (a.knn) {
    geom_reserve(&a.st->count, hit, [&](unsigned long long pos) {
      a.cand_d[pos] = d;  // pos < the objects tested <= the buffers' nobj entries
      a.cand_i[pos] = i;
      a.cand_o[pos] = a.objID[i];
    });
  } else if (hit) {
    atomicOr((unsigned long long*)a.bitmap + (i >> 6), 1ull << (i & 63));
  }
}

// The classify pass, one lane per object: "some cell in N" and "every cell in G" as rectangle sums over the
// query's summed-area tables; range: the all-G objects go straight into the bitmap (one ballot word per
// wave, every word written); the objects to test go to the two worklists.  `corner(c)` returns what the
// in-grid tables cannot hold about the cell rectangle c (k_geompair.hip: the out-of-grid members of G and N):
// bit 0 = some cell in N, bit 1 = every cell in G; the point queries pass a functor that returns 0.
template <class Corner>
static __device__ __forceinline__ void geom_classify_body(const GeomArgs& a, Corner&& corner) {
  const int lane = threadIdx.x & 63;
  unsigned long long n_filt = 0, n_allg = 0;  // this wave's (lane 0 keeps them)
  for (int64_t i0 = (int64_t)blockIdx.x * kBlock; i0 < a.nobj; i0 += (int64_t)gridDim.x * kBlock) {  // wave-uniform
    const int64_t i = i0 + threadIdx.x;
    const bool in = i < a.nobj;
    const int64_t il = in ? i : a.nobj - 1;  // clamped: the loads never branch
    const int4 c = reinterpret_cast<const int4*>(a.cells)[il];
    const bool ok = in && a.valid[il];
    const int32_t nv = a.nvert[il];
    const unsigned extra = corner(c);  // bit 0: a cell in N outside the tables; bit 1: every cell in G by them
    const bool filt = ok && (geom_rect_count(a.satN, a.grid_n, c.x, c.y, c.z, c.w) > 0 || (extra & 1u));
    bool allg = false;
    if (filt && !a.knn)
      allg = geom_rect_count(a.satG, a.grid_n, c.x, c.y, c.z, c.w) == geom_rect_area(c.x, c.y, c.z, c.w) || (extra & 2u);
    const unsigned long long m_allg = __ballot(allg);
    n_filt += __popcll(__ballot(filt));
    n_allg += __popcll(m_allg);
    if (!a.knn && lane == 0 && in) a.bitmap[i >> 6] = m_allg;
    const bool test = filt && !allg;
    const bool wide = test && !a.approx && nv >= a.wide_vertices;  // (the bbox distance walks nothing)
    geom_reserve(a.qctr, test && !wide, [&](unsigned long long pos) { a.work_short[pos] = (uint32_t)i; });
    geom_reserve(a.qctr + 1, wide, [&](unsigned long long pos) { a.work_wide[pos] = (uint32_t)i; });
  }
  if (lane == 0) {
    if (n_filt) atomicAdd(a.qctr + 2, n_filt);
    if (n_allg) atomicAdd(a.qctr + 3, n_allg);
  }
}

}  // namespace gf
