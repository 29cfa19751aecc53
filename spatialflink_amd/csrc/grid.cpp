// grid.cpp -- the uniform grid on the host: the exact cell thresholds the kernels compare against,
// cell ids, and the drivers of K1 (cells), K2 (bucketing by cell) and the column-band shard pass.
#define GF_TU_NAME grid_cpp
#include "gf_buildtag.hpp"  // first: records this unit's command-line defines

#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>

#include "gf_host.hpp"

using namespace gf;

// ---------------------------------------------------------------------------------------
// Exact cell thresholds.  cell(x) = jint(floor((x - mn)/cl)) is monotone non-decreasing in x
// over the non-NaN doubles (every step is a monotone rounding), so for any integer A the set
// {x : cell(x) >= A} is an up-set of the double order: a bisection over the ordered bit
// patterns finds its first element exactly.  The kernels then compare coordinates with
// these doubles instead of dividing.
// ---------------------------------------------------------------------------------------
static uint64_t okey_of(double d) {
  uint64_t b = dbits(d);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
static double of_okey(uint64_t k) {
  uint64_t b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  return from_bits(b);
}

double gf::first_at_least(int64_t A, double mn, double cl) {
  const double nan = std::numeric_limits<double>::quiet_NaN();
  if (A <= (int64_t)INT32_MIN) return -INFINITY;
  if (A > (int64_t)INT32_MAX) return nan;
  if (cell_index(INFINITY, mn, cl) < A) return nan;
  if (cell_index(-INFINITY, mn, cl) >= A) return -INFINITY;
  uint64_t lo = okey_of(-INFINITY), hi = okey_of(INFINITY);  // cell(lo) < A <= cell(hi)
  while (hi - lo > 1) {
    uint64_t mid = lo + (hi - lo) / 2;
    if (cell_index(of_okey(mid), mn, cl) >= A) hi = mid; else lo = mid;
  }
  return of_okey(hi);
}

// doubles whose cell index lies in [a, b]
AxisIv gf::axis_iv(int64_t a, int64_t b, double mn, double cl) {
  const double nan = std::numeric_limits<double>::quiet_NaN();
  if (a > b) return {nan, nan};
  AxisIv iv;
  iv.lo = first_at_least(a, mn, cl);
  iv.hi_excl = first_at_least(b + 1, mn, cl);
  return iv;
}

QueryRect gf::make_qrect(const gf_grid& g, int32_t qcx, int32_t qcy, int32_t gl, int32_t cl) {
  QueryRect q;
  const double nan = std::numeric_limits<double>::quiet_NaN();
  q.minX = g.minX;
  q.minY = g.minY;
  const int64_t n1 = g.n - 1;
  if (cl > 0) {
    q.cgx = axis_iv(std::max<int64_t>((int64_t)qcx - cl, 0), std::min<int64_t>((int64_t)qcx + cl, n1), g.minX, g.cellLength);
    q.cgy = axis_iv(std::max<int64_t>((int64_t)qcy - cl, 0), std::min<int64_t>((int64_t)qcy + cl, n1), g.minY, g.cellLength);
  } else {
    q.cgx = q.cgy = {nan, nan};
  }
  if (gl > 0) {
    q.gx = axis_iv(std::max<int64_t>((int64_t)qcx - gl, 0), std::min<int64_t>((int64_t)qcx + gl, n1), g.minX, g.cellLength);
    q.gy = axis_iv(std::max<int64_t>((int64_t)qcy - gl, 0), std::min<int64_t>((int64_t)qcy + gl, n1), g.minY, g.cellLength);
  } else if (gl == 0) {  // getGuaranteedNeighboringCells adds the query cell itself, no validKey
    q.gx = axis_iv(qcx, qcx, g.minX, g.cellLength);
    q.gy = axis_iv(qcy, qcy, g.minY, g.cellLength);
  } else {
    q.gx = q.gy = {nan, nan};
  }
  q.g_any = (gl >= 0) && !std::isnan(q.gx.lo) && !std::isnan(q.gy.lo);
  return q;
}

// ---------------------------------------------------------------------------------------
// grid / cell IDs
// ---------------------------------------------------------------------------------------
extern "C" int gf_grid_make(int32_t n, double minX, double maxX, double minY, double maxY, gf_grid* out) {
  if (!out || n <= 0) return GF_ERR_ARG;
  out->n = n;
  out->reserved = 0;
  out->minX = minX; out->maxX = maxX; out->minY = minY; out->maxY = maxY;
  out->cellLength = (maxX - minX) / n;  // UniformGrid.java:83
  return grid_ok(out) ? GF_OK : GF_ERR_ARG;
}

extern "C" int gf_grid_layers(const gf_grid* g, double r, int32_t* gl, int32_t* cl) {
  if (!g) return GF_ERR_ARG;
  if (gl) *gl = guaranteed_layers(g->cellLength, r);
  if (cl) *cl = candidate_layers(g->cellLength, r);
  return GF_OK;
}

extern "C" int gf_cell_of(const gf_grid* g, double x, double y, int32_t* cx, int32_t* cy) {
  if (!g || !cx || !cy) return GF_ERR_ARG;
  *cx = cell_index(x, g->minX, g->cellLength);
  *cy = cell_index(y, g->minY, g->cellLength);
  return GF_OK;
}

extern "C" int gf_format_cell_id(int32_t cx, int32_t cy, char* buf, int32_t cap) {
  if (!buf || cap <= 0) return GF_ERR_ARG;
  int w = snprintf(buf, (size_t)cap, "%05d%05d", cx, cy);
  return (w >= 0 && w < cap) ? GF_OK : GF_ERR_CAPACITY;
}

static int32_t parse_java_int(const char* s, size_t len) {
  size_t i = 0;
  while (i + 1 < len && s[i] == '0') i++;  // replaceFirst("^0+(?!$)", "")
  bool neg = false;
  long long v = 0;
  if (i < len && (s[i] == '-' || s[i] == '+')) { neg = s[i] == '-'; i++; }
  for (; i < len; i++) v = v * 10 + (s[i] - '0');
  return (int32_t)(neg ? -v : v);
}

extern "C" int gf_parse_cell_id(const char* id, int32_t* cx, int32_t* cy) {
  if (!id || !cx || !cy) return GF_ERR_ARG;
  size_t len = strlen(id);
  if (len < 6) return GF_ERR_ARG;
  *cx = parse_java_int(id, 5);
  *cy = parse_java_int(id + 5, len - 5);
  return GF_OK;
}

// ---------------------------------------------------------------------------------------
// K1 / K2
// ---------------------------------------------------------------------------------------
extern "C" int gf_assign_cells(gf_ctx* ctx, const gf_grid* g, const gf_points* pts, int32_t* cx, int32_t* cy) {
  if (!ctx || !grid_ok(g) || !cx || !cy) return set_err(ctx, GF_ERR_ARG, "gf_assign_cells: bad argument");
  int st = bind(ctx);
  if (st) return st;
  if ((st = check_points(ctx, pts))) return st;
  if (((uintptr_t)cx | (uintptr_t)cy) & 7) return set_err(ctx, GF_ERR_ALIGN, "cx/cy must be 8-byte aligned");
  GF_HIP_CHECK(ctx, launch_assign(ctx, g, pts, cx, cy));
  return GF_OK;
}

// the radix passes' arguments every K2 / shard driver starts from: the window and its grid
static RadixArgs radix_args(const gf_grid* g, const gf_points* pts) {
  RadixArgs a{};
  a.tile = radix_tile();
  a.x = pts->x; a.y = pts->y; a.n = pts->n;
  a.minX = g->minX; a.minY = g->minY; a.cl = g->cellLength; a.gn = g->n;
  return a;
}

// K2 in row mode (grids up to 511 x 511, where the LSD sort takes two 9-bit passes): pass A
// sorts stably by row (the keys' high digit, as the LSD's last pass would), pass B sorts every
// row stably by column -- over row SEGMENTS, so each block's output lies inside its row's range
// (row-local writes instead of 512 runs spread over the whole output), only the permutation is
// written, and the cells' starts come from pass B's own scan (no key read-back, no bounds pass).
constexpr int kRowSeg = 32768;  // points per row segment (a uniform 10M-point window on 500 x 500: one per row,
                                // sorted whole by radix_row_sort_kernel, whose capacity this is)
static int bucket_rows(gf_ctx* ctx, const gf_grid* g, const gf_points* pts, uint32_t* perm, uint32_t* cell_start,
                       int blocks) {
  const int64_t n = pts->n;
  const int64_t D = kRadixMaxDigits, matA = D * blocks;
  const int64_t ub = n / kRowSeg + g->n + 2;  // segments <= sum over rows of (size / seg + 1)
  const int64_t matB = D * ub;
  Arena ar;
  uint32_t *k0, *v1, *ma, *msa, *mb, *msb, *flag;
  uint16_t* k1;
  ar.take(k0, n); ar.take(k1, n); ar.take(v1, n);
  ar.take(ma, matA); ar.take(msa, matA + 1);
  ar.take(mb, matB); ar.take(msb, matB + 1);
  ar.take(flag, 1);
  int st = ar.alloc(ctx);
  if (st) return st;
  RadixArgs a = radix_args(g, pts);
  a.bits = kRadixMaxBits; a.nblk = blocks; a.rowmode = 1;
  // (GF_K2_SELFCOUNT=1, A/B only: a one-segment row's scatter block counts its own columns instead
  // of the histogram kernel -- r06 A/B 0.2028 / 0.1997 vs 0.1988 / 0.1991 ms, profiles/r06_k2b_ab.jsonl)
  const char* sce = std::getenv("GF_K2_SELFCOUNT");
  const bool self_count = sce && *sce == '1';
  // r06: one-segment rows sorted whole, each by one block with its output staged in LDS
  // (radix_row_sort_kernel); GF_K2_ROWSORT=0 (A/B only) leaves them to the segment path
  const char* rse = std::getenv("GF_K2_ROWSORT");
  const bool rowsort = !(rse && *rse == '0') && !self_count && kRowSeg <= radix_row_sort_cap();
  a.multiseg = rowsort ? flag : nullptr;  // zeroed by pass A's histogram
  // pass A: row keys -> k0 with the histogram of rows, scan, stable scatter by row
  a.kout = k0;
  a.shift = kRadixMaxBits;
  a.M = ma;
  a.Ms = msa;
  GF_HIP_CHECK(ctx, launch_radix(ctx, 0, a, blocks));
  if ((st = scan1(ctx, ma, matA, msa))) return st;
  a.kin = k0;
  a.vin = nullptr;
  a.kout = nullptr;
  a.kout16 = k1;  // the columns (u16): the row is the position's
  a.vout = v1;
  GF_HIP_CHECK(ctx, launch_radix(ctx, 1, a, blocks));
  // pass B: per row segment column histograms (one-segment rows count their own columns in the
  // scatter), one scan, stable scatter by column (perm only)
  RadixArgs b = a;
  b.kin = nullptr;
  b.kin16 = k1;
  b.kout16 = nullptr;
  b.vin = v1;
  b.kout = nullptr;
  b.vout = perm;
  b.shift = 0;
  b.seg = kRowSeg;
  b.MsA = msa;
  b.nblkA = blocks;
  b.M = mb;
  b.Ms = msb;
  b.cstart = cell_start;
  b.self_count = self_count;
  b.rowsort = rowsort;
  if (b.rowsort) {
    // the rows sorted whole (blocks 0 .. gn) and the multi-segment rows' column histograms --
    // in one launch (the blocks past the rows) or, GF_K2_MERGE=0 (A/B), a histogram launch of their
    // own; the multi-segment rows' scatter blocks scan their own row's counts (no scan launch)
    const char* me = std::getenv("GF_K2_MERGE");
    const bool merge = !(me && *me == '0');
    GF_HIP_CHECK(ctx, launch_radix(ctx, 4, b, g->n + 1 + (merge ? (int)ub : 0)));
    if (!merge) GF_HIP_CHECK(ctx, launch_radix(ctx, 3, b, (int)ub));
  } else {
    GF_HIP_CHECK(ctx, launch_radix(ctx, 3, b, (int)ub));
    if ((st = scan1(ctx, mb, matB, msb))) return st;
  }
  GF_HIP_CHECK(ctx, launch_radix(ctx, 1, b, (int)ub));
  return GF_OK;
}

extern "C" int gf_bucket_by_cell(gf_ctx* ctx, const gf_grid* g, const gf_points* pts, uint32_t* perm,
                                 uint32_t* cell_start) {
  if (!ctx || !grid_ok(g) || !perm || !cell_start) return set_err(ctx, GF_ERR_ARG, "gf_bucket_by_cell: bad argument");
  int st = bind(ctx);
  if (st) return st;
  if ((st = check_points(ctx, pts))) return st;
  const int64_t bins = (int64_t)g->n * g->n + 1;
  if (bins >= (int64_t)INT32_MAX) return set_err(ctx, GF_ERR_ARG, "grid too large for bucketing");
  const int64_t n = pts->n;
  if (n == 0) {
    GF_HIP_CHECK(ctx, hipMemsetAsync(cell_start, 0, sizeof(uint32_t) * (size_t)(bins + 1), ctx->stream));
    return GF_OK;
  }
  int bits = 1;
  while (((int64_t)1 << bits) < bins) ++bits;
  const int passes = (bits + kBucketBits - 1) / kBucketBits, pbits = (bits + passes - 1) / passes;
  const int blocks = radix_blocks(ctx, n);
  if (passes >= 2 && g->n + 1 <= kRadixMaxDigits && !std::getenv("GF_K2_LSD"))
    return bucket_rows(ctx, g, pts, perm, cell_start, blocks);
  const int64_t mat = ((int64_t)1 << pbits) * blocks;
  Arena ar;
  uint32_t *k[2], *v[2], *k0, *m, *ms;
  ar.take(k[0], n); ar.take(k[1], n);
  ar.take(v[0], n); ar.take(v[1], n);
  ar.take(k0, n);  // pass 0's keys (stored by its histogram)
  ar.take(m, mat); ar.take(ms, mat + 1);
  if ((st = ar.alloc(ctx))) return st;
  RadixArgs a = radix_args(g, pts);
  a.bits = pbits; a.nblk = blocks;
  for (int p = 0; p < passes; ++p) {
    a.kin = p == 0 ? nullptr : k[(p - 1) & 1];
    a.vin = p == 0 ? nullptr : v[(p - 1) & 1];
    a.kout = p == 0 ? k0 : k[p & 1];
    a.shift = p * pbits;
    a.M = m;
    a.Ms = ms;
    GF_HIP_CHECK(ctx, launch_radix(ctx, 0, a, blocks));  // pass 0: keys -> k0
    if ((st = scan1(ctx, m, mat, ms))) return st;
    if (p == 0) a.kin = k0;  // the scatter reads the stored keys, index = position
    a.kout = k[p & 1];
    a.vout = p == passes - 1 ? perm : v[p & 1];
    GF_HIP_CHECK(ctx, launch_radix(ctx, 1, a, blocks));
  }
  // cell_start[0 .. bins] from the sorted keys' run boundaries (one kernel, every entry written once)
  a.M = cell_start;
  GF_HIP_CHECK(ctx, launch_radix(ctx, 2, a, blocks));
  return GF_OK;
}

// A window's points partitioned by owning GPU (multi-GPU sharding by cell-column bands, the
// keyBy(gridID) shuffle of PointPointRangeQuery.java:144-148 across ranks): one stable radix pass
// over the band keys (K1's column + the band search, fused into the histogram), so every shard
// lists its points in arrival order -- identical to sharding.shard_order.
extern "C" int gf_shard_by_columns(gf_ctx* ctx, const gf_grid* g, const gf_points* pts, int32_t nbands,
                                   const int32_t* band_lo, uint32_t* perm, uint32_t* offsets) {
  if (!ctx || !grid_ok(g) || !perm || !offsets || !band_lo || nbands < 1 || nbands > kMaxShardBands)
    return set_err(ctx, GF_ERR_ARG, "gf_shard_by_columns: bad argument");
  for (int j = 1; j < nbands; ++j)
    if (band_lo[j] < band_lo[j - 1]) return set_err(ctx, GF_ERR_ARG, "gf_shard_by_columns: band starts must ascend");
  int st = bind(ctx);
  if (st) return st;
  if ((st = check_points(ctx, pts))) return st;
  const int64_t n = pts->n;
  if (n == 0) {
    GF_HIP_CHECK(ctx, hipMemsetAsync(offsets, 0, sizeof(uint32_t) * (size_t)(nbands + 1), ctx->stream));
    return GF_OK;
  }
  if (n > (int64_t)UINT32_MAX) return set_err(ctx, GF_ERR_ARG, "gf_shard_by_columns: window too large");
  int bits = 1;
  while ((1 << bits) < nbands) ++bits;
  const int blocks = radix_blocks(ctx, n);
  const int64_t mat = ((int64_t)1 << bits) * blocks;
  Arena ar;
  uint32_t *k0, *k, *m, *ms;
  ar.take(k0, n); ar.take(k, n);
  ar.take(m, mat); ar.take(ms, mat + 1);
  if ((st = ar.alloc(ctx))) return st;
  RadixArgs a = radix_args(g, pts);
  a.bits = bits; a.nblk = blocks; a.shift = 0;
  a.nbands = nbands;
  for (int j = 0; j < nbands; ++j) a.band_lo[j] = band_lo[j];
  a.kin = nullptr; a.vin = nullptr; a.kout = k0; a.M = m; a.Ms = ms;
  GF_HIP_CHECK(ctx, launch_radix(ctx, 0, a, blocks));  // band keys -> k0, histograms
  if ((st = scan1(ctx, m, mat, ms))) return st;
  a.kin = k0; a.kout = k; a.vout = perm;
  GF_HIP_CHECK(ctx, launch_radix(ctx, 1, a, blocks));  // stable scatter: perm
  a.M = offsets; a.bins = (uint32_t)nbands;
  GF_HIP_CHECK(ctx, launch_radix(ctx, 2, a, blocks));  // offsets[0 .. nbands]
  return GF_OK;
}

extern "C" int gf_gather_points(gf_ctx* ctx, const gf_points* pts, const uint32_t* perm, int64_t begin, int64_t end,
                                double* x, double* y, int64_t* objID, int64_t* ts) {
  if (!ctx || !pts || !perm || begin < 0 || end < begin || end > pts->n || (objID && !pts->objID) ||
      (ts && !pts->ts))
    return set_err(ctx, GF_ERR_ARG, "gf_gather_points: bad argument (need 0 <= begin <= end <= n)");
  int st = check_points(ctx, pts);
  if (st) return st;
  if ((st = bind(ctx))) return st;
  GF_HIP_CHECK(ctx, launch_gather_points(ctx->stream, *pts, perm, begin, end - begin, x, y, objID, ts));
  return GF_OK;
}

