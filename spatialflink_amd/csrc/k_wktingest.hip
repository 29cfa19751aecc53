// k_wktingest.hip -- GPU WKT ingest of point, polygon and linestring streams
// (Deserialization.WKTTo[T]Spatial, WKTTo[T]SpatialPolygon, WKTTo[T]SpatialLineString,
// Deserialization.java:214-288, 461-586, 748-835).  The geometry streams keep the shape of
// k_geomingest.hip; after the newline index (k_csv.hip csv_nlindex):
//
//   wkt_pass_a    one lane per line: gf_wkt_geom.hpp wkt_line_eval -- the fields of a T variant
//                 (objID, ts), the tag, the canonical grammar with every number token checked --
//                 and per line the taken object's ring and position counts, its type and the byte
//                 position of the geometry's first '('
//   (scans)       the exclusive scans of the two counts (the look-back scan, k_points.hip)
//   wkt_head      totals, the first bad line and -- by one lane -- its kind, for the host
//   wkt_pass_b    one lane per line: ring closure (the one rule that needs values), then the
//                 positions parsed into vx / vy at the line's offsets, rings in createPolygon order
//
// A block takes 64 consecutive lines (one wave) and stages their bytes in LDS with 16-B loads when
// they fit the staging area (sized from the mean line); a block whose lines do not fit reads global
// memory byte by byte.  The point stream is one pass (wkt_points): one lane per line, 192 lines per
// block staged the same way, x, y, objID (null), ts (0) and the cell written at once.
#define GF_TU_NAME k_wktingest_hip
#include "gf_buildtag.hpp"  // first: records this unit's command-line defines

#include "k_wktingest.hpp"

namespace gf {

static __device__ const uint64_t kPow5Wkt[] = {GF_POW5_TABLE};

// the text's line counts from the device (csv_nlindex's total)
template <class Args>
__device__ __forceinline__ void wkt_counts(const Args& a, int64_t& newlines, int64_t& lines) {
  newlines = (int64_t)*a.nl_total;
  lines = newlines + (a.text[a.len - 1] != '\n' ? 1 : 0);
}
// line j's bytes [b, e), '\r' dropped; 0, or the error of an empty line
template <class Args, class Src>
__device__ __forceinline__ int wkt_bounds(const Args& a, const Src& s, int64_t j, int64_t newlines, int64_t& b, int64_t& e) {
  b = j == 0 ? 0 : a.nl[j - 1] + 1;
  e = j < newlines ? a.nl[j] : a.len;
  if (e > b && s(e - 1) == '\r') --e;
  return e <= b ? kCsvEmptyLine : kCsvOk;
}
// The block's lines [L0, L1) into lds (text position a0 at lds[0]); false: they do not fit.
// (block-uniform; a barrier inside)
template <int NL, class Args>
__device__ __forceinline__ bool wkt_stage(const Args& a, char* lds, int64_t L0, int64_t L1, int64_t newlines, int64_t& a0) {
  const int64_t b0 = L0 == 0 ? 0 : a.nl[L0 - 1] + 1;
  const int64_t b1 = L1 - 1 < newlines ? a.nl[L1 - 1] : a.len;  // the last line's '\n' (or the end)
  a0 = b0 & ~(int64_t)15;
  if (b1 - a0 > a.lds_cap) return false;
  for (int64_t off = a0 + 16 * threadIdx.x; off < b1; off += 16 * NL) {
    if (off + 16 <= a.len) {
      *reinterpret_cast<uint4*>(lds + (off - a0)) = *reinterpret_cast<const uint4*>(a.text + off);
    } else {
      for (int k = 0; k < 16 && off + k < a.len; ++k) lds[off - a0 + k] = a.text[off + k];
    }
  }
  __syncthreads();
  return true;
}

template <class Src>
__device__ __forceinline__ int wkt_eval_line(const WktIngestArgs& a, const Src& s, int64_t j, int64_t newlines, bool values,
                                             GeomNote* n, LineOut* o) {
  int64_t b = 0, e = 0;
  const int bs = wkt_bounds(a, s, j, newlines, b, e);
  if (bs) return bs;
  return wkt_line_eval(WktProps{a.kind, (char)a.delim, a.date_fmt, a.tz_off_ms, kPow5Wkt}, s, b, e, values, n, o);
}
// pass A of line j; true when its objID needs the dictionary (*w filled)
template <class Src>
__device__ __forceinline__ bool wkt_a_line(const WktIngestArgs& a, const Src& s, int64_t j, int64_t newlines, DictWork* w) {
  GeomNote n{0, 0, 0, 0};
  LineOut o{0, 0, 0.0, 0.0, false, {0, 0}};
  const int st = wkt_eval_line(a, s, j, newlines, false, &n, &o);
  if (st != kCsvOk) {
    atomicMin(&a.err->line, (unsigned long long)j);
    a.cnt_r[j] = 0u;
    a.cnt_v[j] = 0u;
    return false;
  }
  a.cnt_r[j] = (uint32_t)n.nrings;
  a.cnt_v[j] = (uint32_t)n.nverts;
  a.gpos[j] = n.cpos;
  a.tcode[j] = n.tcode;
  a.ts_s[j] = o.ts;
  a.obj_s[j] = o.dict ? 0 : o.obj;
  if (o.dict) *w = DictWork{o.f_obj.b, (int32_t)(o.f_obj.e - o.f_obj.b), (uint32_t)j};
  return o.dict;
}

__global__ __launch_bounds__(kGeomLines) void wkt_pass_a_kernel(WktIngestArgs a) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  int64_t newlines, lines;
  wkt_counts(a, newlines, lines);
  // false: the index was cut (more newlines than nl_cap: the host regrows and re-runs)
  const bool ok = newlines <= a.nl_cap && lines <= a.grid_lines;
  const int64_t L0 = (int64_t)blockIdx.x * kGeomLines;
  const int64_t j = L0 + threadIdx.x;
  if (!ok || L0 >= lines) {  // block-uniform: slots past the text's lines count nothing
    if (j < a.grid_lines) {
      a.cnt_r[j] = 0u;
      a.cnt_v[j] = 0u;
    }
    return;
  }
  const int64_t L1 = L0 + kGeomLines < lines ? L0 + kGeomLines : lines;  // exclusive
  DictWork w{0, 0, 0};
  bool need = false;
  int64_t a0 = 0;
  if (wkt_stage<kGeomLines>(a, lds, L0, L1, newlines, a0)) {
    if (j < L1) need = wkt_a_line(a, LBytes{(GF_LDS_PTR(char))lds, a0}, j, newlines, &w);
  } else if (j < L1) {
    need = wkt_a_line(a, GBytes{a.text}, j, newlines, &w);
  }
  if (j >= L1 && j < a.grid_lines) {
    a.cnt_r[j] = 0u;
    a.cnt_v[j] = 0u;
  }
  // the wave's dictionary objIDs into the queue (one atomic per wave; the order is free)
  const uint64_t m = __ballot(need);
  if (m) {
    const int lane = threadIdx.x & 63;
    unsigned long long nb = need ? (unsigned long long)w.n : 0ull;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) nb += __shfl_xor(nb, o, 64);
    uint32_t base = 0;
    if (lane == 0) {
      base = atomicAdd(a.dict_n, (uint32_t)__popcll(m));
      atomicAdd(a.dict_bytes, nb);
    }
    base = __shfl(base, 0, 64);
    if (need) a.dict_work[base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = w;
  }
}

// The head: counts and totals, the first bad line, and its kind re-derived by one lane with the
// whole contract (ring closure included) over that line.
__global__ void wkt_head_kernel(WktIngestArgs a) {
  if (threadIdx.x != 0) return;
  int64_t newlines, lines;
  wkt_counts(a, newlines, lines);
  const bool ok = newlines <= a.nl_cap && lines <= a.grid_lines;
  const unsigned long long j = a.err->line;
  if (ok && j != ~0ull) {
    GeomNote n{0, 0, 0, 0};
    LineOut o{0, 0, 0.0, 0.0, false, {0, 0}};
    a.err->kind = wkt_eval_line(a, GBytes{a.text}, (int64_t)j, newlines, true, &n, &o);
  }
  a.head->newlines = (unsigned long long)newlines;
  a.head->lines = (unsigned long long)lines;
  a.head->nrings = ok ? a.off_r[a.grid_lines] : 0ull;
  a.head->nverts = ok ? a.off_v[a.grid_lines] : 0ull;
  a.head->dict_n = *a.dict_n;
  a.head->dict_bytes = *a.dict_bytes;
  a.head->err = *a.err;
}

template <class Src>
__device__ __forceinline__ void wkt_b_line(const WktIngestArgs& a, const Src& s, int64_t j, int64_t newlines, int64_t lines) {
  const int64_t e0 = j < newlines ? a.nl[j] : a.len;
  const int64_t b = j == 0 ? 0 : a.nl[j - 1] + 1;
  const int64_t e = e0 > b && s(e0 - 1) == '\r' ? e0 - 1 : e0;
  const GeomNote n{a.tcode[j], (int32_t)a.cnt_r[j], (int32_t)a.cnt_v[j], a.gpos[j]};
  const bool closed = wkt_closed(s, n.cpos, e, n.tcode, kPow5Wkt);
  if (!closed) atomicMin(&a.err->line, (unsigned long long)j);
  if (!a.fill) return;
  const int32_t r0 = (int32_t)a.off_r[j], v0 = (int32_t)a.off_v[j];
  const bool poly = a.kind == GF_GEOM_POLYGON;
  if (poly) a.ring_off[j] = r0;
  else a.vert_off[j] = v0;
  a.ts[j] = a.ts_s[j];
  a.objID[j] = a.obj_s[j];
  if (j == lines - 1) {  // the closing offsets
    const int32_t nr = (int32_t)a.off_r[a.grid_lines], nv = (int32_t)a.off_v[a.grid_lines];
    if (poly) {
      a.ring_off[lines] = nr;
      a.vert_off[nr] = nv;
    } else {
      a.vert_off[lines] = nv;
    }
  }
  if (!closed) return;
  const RingTmp t{a.tmp.area + r0, a.tmp.start + r0, a.tmp.count + r0, a.tmp.order + r0};
  wkt_fill(s, e, n, kPow5Wkt, v0, poly ? a.vert_off + r0 : (int32_t*)nullptr, t, a.vx, a.vy);
}

__global__ __launch_bounds__(kGeomLines) void wkt_pass_b_kernel(WktIngestArgs a) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  int64_t newlines, lines;
  wkt_counts(a, newlines, lines);  // (the host launches pass B only after a pass A that fitted)
  const int64_t L0 = (int64_t)blockIdx.x * kGeomLines;
  if (L0 >= a.limit) return;  // block-uniform
  const int64_t L1 = L0 + kGeomLines < a.limit ? L0 + kGeomLines : a.limit;  // exclusive
  const int64_t j = L0 + threadIdx.x;
  int64_t a0 = 0;
  if (wkt_stage<kGeomLines>(a, lds, L0, L1, newlines, a0)) {
    if (j < L1) wkt_b_line(a, LBytes{(GF_LDS_PTR(char))lds, a0}, j, newlines, lines);
  } else if (j < L1) {
    wkt_b_line(a, GBytes{a.text}, j, newlines, lines);
  }
}

// ---- the point stream: one pass ---------------------------------------------------------------------
// Both point maps build Point(x, y, uGrid): objID null, ts 0 (the T variant never reads its fields).
template <class Src>
__device__ __forceinline__ int wkt_point_eval(const WktPointArgs& a, const Src& s, int64_t j, int64_t newlines, LineOut* o) {
  int64_t b = 0, e = 0;
  const int bs = wkt_bounds(a, s, j, newlines, b, e);
  if (bs) return bs;
  GeomNote n{0, 0, 0, 0};
  return wkt_line_eval(WktProps{kWktPoints, (char)0, 0, 0, kPow5Wkt}, s, b, e, false, &n, o);
}
template <class Src>
__device__ __forceinline__ void wkt_point_line(const WktPointArgs& a, const Src& s, int64_t j, int64_t newlines) {
  LineOut o{0, 0, 0.0, 0.0, false, {0, 0}};
  if (wkt_point_eval(a, s, j, newlines, &o) != kCsvOk) {
    atomicMin(&a.err->line, (unsigned long long)j);
    return;
  }
  a.x[j] = o.x;
  a.y[j] = o.y;
  a.objID[j] = GF_OBJID_NULL;
  a.ts[j] = 0;
  if (a.cx) {
    a.cx[j] = cell_index(o.x, a.minX, a.cl);
    a.cy[j] = cell_index(o.y, a.minY, a.cl);
  }
}
// false when nothing may be written: the index was cut, or more lines than the caller's capacity
__device__ __forceinline__ bool wkt_point_counts(const WktPointArgs& a, int64_t& newlines, int64_t& lines) {
  wkt_counts(a, newlines, lines);
  return newlines <= a.nl_cap && lines <= a.cap && lines <= a.grid_lines;
}
__global__ __launch_bounds__(kWktPointLines) void wkt_points_kernel(WktPointArgs a) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  int64_t newlines, lines;
  const bool ok = wkt_point_counts(a, newlines, lines);
  const int64_t L0 = (int64_t)blockIdx.x * kWktPointLines;
  if (!ok || L0 >= lines) return;  // block-uniform
  const int64_t L1 = L0 + kWktPointLines < lines ? L0 + kWktPointLines : lines;  // exclusive
  const int64_t j = L0 + threadIdx.x;
  int64_t a0 = 0;
  if (wkt_stage<kWktPointLines>(a, lds, L0, L1, newlines, a0)) {
    if (j < L1) wkt_point_line(a, LBytes{(GF_LDS_PTR(char))lds, a0}, j, newlines);
  } else if (j < L1) {
    wkt_point_line(a, GBytes{a.text}, j, newlines);
  }
}
__global__ void wkt_points_head_kernel(WktPointArgs a) {
  if (threadIdx.x != 0) return;
  int64_t newlines, lines;
  const bool ok = wkt_point_counts(a, newlines, lines);
  const unsigned long long j = a.err->line;
  if (ok && j != ~0ull) {
    LineOut o{0, 0, 0.0, 0.0, false, {0, 0}};
    a.err->kind = wkt_point_eval(a, GBytes{a.text}, (int64_t)j, newlines, &o);
  }
  a.head->newlines = (unsigned long long)newlines;
  a.head->lines = (unsigned long long)lines;
  a.head->nrings = a.head->nverts = a.head->dict_n = a.head->dict_bytes = 0ull;
  a.head->err = *a.err;
}

hipError_t launch_wktingest_a(gf_ctx* ctx, const WktIngestArgs& a) {
  const unsigned blocks = (unsigned)((a.grid_lines + kGeomLines - 1) / kGeomLines);
  hipLaunchKernelGGL(wkt_pass_a_kernel, dim3(blocks), dim3(kGeomLines), (size_t)a.lds_cap, ctx->stream, a);
  return hipGetLastError();
}
hipError_t launch_wktingest_head(gf_ctx* ctx, const WktIngestArgs& a) {
  hipLaunchKernelGGL(wkt_head_kernel, dim3(1), dim3(64), 0, ctx->stream, a);
  return hipGetLastError();
}
hipError_t launch_wktingest_b(gf_ctx* ctx, const WktIngestArgs& a) {
  if (a.limit <= 0) return hipSuccess;
  const unsigned blocks = (unsigned)((a.limit + kGeomLines - 1) / kGeomLines);
  hipLaunchKernelGGL(wkt_pass_b_kernel, dim3(blocks), dim3(kGeomLines), (size_t)a.lds_cap, ctx->stream, a);
  return hipGetLastError();
}
hipError_t launch_wkt_points(gf_ctx* ctx, const WktPointArgs& a) {
  if (a.grid_lines > 0) {
    const unsigned blocks = (unsigned)((a.grid_lines + kWktPointLines - 1) / kWktPointLines);
    hipLaunchKernelGGL(wkt_points_kernel, dim3(blocks), dim3(kWktPointLines), (size_t)a.lds_cap, ctx->stream, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(wkt_points_head_kernel, dim3(1), dim3(64), 0, ctx->stream, a);
  return hipGetLastError();
}

}  // namespace gf
